/* duck_fleet.h — C ABI of the batched deployment loop (sim2sim.FleetInfer; libduck.so and every
 * model's own library).
 *
 * The reference decides whether an exported policy goes on the robot by running it in its deployment
 * control loop (playground/open_duck_mini_v2/mujoco_infer.py:156-241 on mujoco_infer_base.py), which is
 * not the training env: +1.3 on the accelerometer's x, a motor-speed limit, no latency, noise or
 * pushes. One control period of that loop for N robots is four launches on one stream:
 *
 *   duck_physics_step   mj_step x decimation (mujoco_infer.py:170-174), 10 substeps, with `aux`
 *   duck_fleet_observe  the phase advance and get_obs (mujoco_infer.py:175-197, :67-103), plus the
 *                       per-robot bookkeeping of an evaluation (brax EvalWrapper's rule, as
 *                       duck_episode_accumulate(EVAL) applies it)
 *   duck_policy_act     self.policy.infer(obs) (mujoco_infer.py:203; duck_ppo.h)
 *   duck_fleet_actuate  the action history, motor targets, speed limit and ctrl (mujoco_infer.py:208-231)
 *
 * and, only when the caller disturbs the loop as the training env does (noise, changing commands, pushes),
 * duck_fleet_disturb between duck_fleet_observe and duck_policy_act; and, only when the caller keeps a flight
 * recorder, duck_fleet_record after duck_fleet_actuate; and, only when the caller configures a latency,
 * duck_fleet_actuate_delayed in duck_fleet_actuate's place and, when an IMU delay is among it,
 * duck_fleet_sense_delay right after duck_fleet_observe -- or, when a joint-encoder delay is among it,
 * duck_fleet_sensor_delay in that place, which delays the IMU and the encoder columns in one launch; and, only
 * when the caller asks how the robots walk and load their servos, duck_fleet_gait after the actuation. A period's
 * order, optional launches in brackets:
 *
 *   physics, observe, [sense_delay or sensor_delay], [disturb], policy or follow, actuate or actuate_delayed, [record]
 *
 * and, with the gait record kept, duck_fleet_gait between the actuation and the recorder:
 *
 *   ..., policy or follow, actuate or actuate_delayed, [gait], [record]
 *
 * (duck_fleet_follow, in duck_policy_act's place, when the robots follow a recorded log instead of a policy.)
 *
 * The entries are model-agnostic: a host descriptor filled from the compiled model tells them where
 * the sensors, the actuated joints and the foot contacts are. Conventions are duck.h's: DEVICE
 * pointers, float32, no allocation, no synchronisation, work ordered on `stream`, negative codes with
 * duck_last_error(), DUCK_EINVAL on null pointers and bad sizes.
 *
 * Arithmetic: every value written is one fp32 operation on loaded words (no contraction into fma), so a
 * float32 restatement reproduces it bit for bit. The library runs with fp32 denormals flushed to zero.
 */
#ifndef DUCK_FLEET_H_
#define DUCK_FLEET_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DUCK_FLEET_MAX_NU 16

typedef struct {
  int nq, nv, nu;        /* nu <= DUCK_FLEET_MAX_NU */
  int naux;              /* rows of the aux record (duck_aux_size) */
  int sens_off, con_off; /* first aux row of sensordata and of con_dist (write_aux's order:
                            qacc, qacc_smooth, qvel, qfrc_smooth [nv each], actuator_force [nu], sensordata, con_dist) */
  int gyro, accelerometer, upvector, local_linvel; /* sensor_adr of each (3 values) inside sensordata */
  int act_qpos[DUCK_FLEET_MAX_NU];      /* jnt_qposadr of each actuator's joint */
  int act_dof[DUCK_FLEET_MAX_NU];       /* jnt_dofadr of each actuator's joint */
  float act_default[DUCK_FLEET_MAX_NU]; /* the home keyframe's ctrl (default_actuator, mujoco_infer_base.py) */
  int foot_con[2];        /* first of the 4 con_dist slots of the (floor, left foot) and (floor, right foot) pairs */
  float dof_vel_scale;    /* 0.05  (mujoco_infer.py:30) */
  float action_scale;     /* 0.25  (mujoco_infer.py:31) */
  float accel_x_offset;   /* 1.3   (mujoco_infer.py:74) */
  float target_step;      /* float32(5.24 * 0.002 * 10): max_motor_velocity * sim_dt * decimation (mujoco_infer.py:58, :216-225) */
  int nb_steps_in_period; /* PolyReferenceMotion.nb_steps_in_period (>= 1 unless standing) */
  int standing;           /* mujoco_infer.py:175: the phase is not advanced */
  int speed_limits;       /* USE_MOTOR_SPEED_LIMITS (mujoco_infer.py:14) */
} duck_fleet_desc;

/* Per-robot control record ctl [N][C], row-major, C = DUCK_FLEET_CTL_SIZE(nu) floats:
 *   [0, nu)        last_action
 *   [nu, 2nu)      last_last_action
 *   [2nu, 3nu)     last_last_last_action
 *   [3nu, 4nu)     motor_targets
 *   [4nu, 5nu)     prev_motor_targets
 *   [5nu, 5nu+7)   command (lin_vel_x, lin_vel_y, ang_vel, neck_pitch, head_pitch, head_yaw, head_roll)
 *   5nu+7          imitation_i
 *   5nu+8          phase_frequency_factor
 *   5nu+9, 5nu+10  imitation_phase (cos, sin)
 * The reference starts with zero actions, both targets at default_actuator, a zero command, imitation_i 0,
 * factor 1 and phase (0, 0) (mujoco_infer.py:49-60).
 * The first word of each field (each macro in its own arguments only, as the sizes are): */
#define DUCK_FLEET_CTL_ACTION(nu, d) ((d) * (nu)) /* history entry d = 0, 1, 2: last_action, last_last_action, ... */
#define DUCK_FLEET_CTL_MOTOR_TARGETS(nu) (3 * (nu))
#define DUCK_FLEET_CTL_PREV_MOTOR_TARGETS(nu) (4 * (nu))
#define DUCK_FLEET_CTL_COMMAND(nu) (5 * (nu))
#define DUCK_FLEET_CTL_IMITATION_I(nu) (5 * (nu) + 7)
#define DUCK_FLEET_CTL_PHASE_FREQUENCY_FACTOR(nu) (5 * (nu) + 8)
#define DUCK_FLEET_CTL_IMITATION_PHASE(nu) (5 * (nu) + 9)
#define DUCK_FLEET_CTL_SIZE(nu) (5 * (nu) + 11)
/* obs [N][DUCK_FLEET_OBS_SIZE(nu)] row-major; acc [N][DUCK_FLEET_ACC_SIZE] row-major */
#define DUCK_FLEET_OBS_SIZE(nu) (17 + 6 * (nu))
#define DUCK_FLEET_ACC_SIZE 6

/* mujoco_infer.py:175-197 and :67-103 after a control period's physics. qpos [nq][N], qvel [nv][N] and
 * aux [naux][N] are duck_physics_step's SoA buffers (aux of the period's last substep).
 *
 * Phase (unless desc.standing), fp32: i = fmodf(i + factor, nb); a = (i / nb) * float32(2 pi), the
 * division correctly rounded; imitation_phase = (cosf(a), sinf(a)) with the accurate functions.
 *
 * obs row, the reference's order: gyro[3], accelerometer[3] (x + accel_x_offset), command[7],
 * qpos[act_qpos[a]] - act_default[a], dof_vel_scale * qvel[act_dof[a]], last_action, last_last_action,
 * last_last_last_action, motor_targets, the two foot contacts, imitation_phase. A foot contact is 1.0
 * when any of the foot's four con_dist values is < 0, else 0.0 (NaN and +-0 are no contact;
 * mujoco_infer_base.py:259-282).
 *
 * Bookkeeping. A robot is fallen when upvector[2] < 0 or any of its qpos or qvel is NaN (the training
 * env's termination on the same sensor, joystick.py:483-485). While alive[e] != 0: if fallen, alive[e] = 0;
 * otherwise acc[e][.] += {1, vx, vy, wz, (vx-cx)*(vx-cx) + (vy-cy)*(vy-cy), (wz-cz)*(wz-cz)} with
 * v = local_linvel, w = gyro, c = command: plain fp32 adds in period order, every product and sum rounded
 * on its own. A fallen robot is still observed and controlled (the reference loop never stops); only its
 * accumulators stop. alive [N] float32, set to 1 by the caller. */
int duck_fleet_observe(const duck_fleet_desc* desc, int N, const float* qpos, const float* qvel, const float* aux,
                       float* ctl, float* obs, float* acc, float* alive, void* stream);

/* mujoco_infer.py:208-231. action [N][nu] row-major (duck_policy_act's output). Shifts the three-deep
 * action history, motor_targets = act_default + action * action_scale (product, then sum); when
 * desc.speed_limits: motor_targets = min(max(motor_targets, prev - target_step), prev + target_step) (a NaN
 * target stays NaN, as np.clip leaves it) and prev_motor_targets = motor_targets; then ctrl [nu][N] (SoA,
 * the next duck_physics_step's input) = motor_targets. */
int duck_fleet_actuate(const duck_fleet_desc* desc, int N, const float* action, float* ctl, float* ctrl,
                       void* stream);

/* Disturbances of the deployment loop: sensor noise on the observation the policy is about to see, the
 * command of the next period from a schedule, and a push of the base before the next period's physics
 * (the training env's, joystick.py:492-558, :449-477, :381-400). One more launch, between
 * duck_fleet_observe and duck_policy_act; a loop that configures none of the three does not enqueue it.
 *
 * The period's count lives on the device: tick [N] int32, p = tick[e] the periods robot e completed before
 * this one (0 at the loop's start, set by the caller), so that a captured graph, which freezes every host
 * argument, replays the same launch for every period.
 *
 * Random stream, threefry2x32 (20 rounds): key = threefry2x32((seed low, seed high), (id low,
 * DUCK_FLEET_KEY_TAG ^ id high)) with id = robot_offset + e, the robot's global id (csrc/duck_math.h
 * derive_key); block b of period p is threefry2x32(key, (p, b)), whose two words are the slots 2b and 2b + 1;
 * a slot's uniform is u = (word >> 9) * 2^-23 in [0, 1), exact in float32.
 *   slot 0   u0, the push's magnitude        slot 1   u1, the push's direction
 *   obs column k: slot 2 * (1 + k % 16 + 16 * (k / 32)) + (k / 16) % 2
 * (columns k and k + 16 of an even k / 16 share a block: a lane of the 16-lane group evaluates it once).
 * A robot's draws depend on (seed, id, p) only -- not on N, the launch geometry or graph replay.
 *
 * In this order, for robot e:
 *   noise    for every obs column k < DUCK_FLEET_OBS_SIZE(nu) with noise_scale[k] != 0:
 *            obs[e][k] = obs[e][k] + (2u - 1) * noise_scale[k]; 2u - 1 is exact, the product is rounded,
 *            then the sum. A column of scale 0 is not written (a -0 keeps its bits). The bookkeeping of
 *            duck_fleet_observe has run on the true sensors.
 *   command  when sched != NULL, with t = p + 1: the 7 values of ctl.command =
 *            sched[min(max(sched_id[e], 0), n_sched - 1)][min(t / seg_periods, n_seg - 1)] (the last
 *            segment is held). sched [n_sched][n_seg][7] row-major float32, sched_id [N] int32.
 *   push     when push != NULL: push [N][DUCK_FLEET_PUSH_SIZE] row-major =
 *            {first, interval, mag_lo, mag_hi, theta_lo, theta_hi}, first and interval integer-valued,
 *            0 <= . < 2^24. A push is due at t = p + 1 (it acts before period t's physics) when first >= 1 and
 *            (t == first, or interval > 0 and t > first and (t - first) % interval == 0); first == 0 never
 *            pushes. When due: mag = mag_lo + (mag_hi - mag_lo) * u0, theta = theta_lo + (theta_hi - theta_lo)
 *            * u1 (lo == hi gives lo), qvel[0][e] += cosf(theta) * mag, qvel[1][e] += sinf(theta) * mag with
 *            the accurate functions, every product and sum rounded on its own. No other qvel row is written
 *            (desc.nv >= 2 is required with a push table).
 *   tick     tick[e] = p + 1.
 * desc gives nu (the widths of ctl and obs) and nv. N == 0 launches nothing. */
#define DUCK_FLEET_PUSH_SIZE 6
#define DUCK_FLEET_KEY_TAG 0xF1EEu
typedef struct {
  uint64_t seed;
  int n_sched, n_seg, seg_periods; /* the schedule table's shape; each >= 1 when sched != NULL, else unused */
  float noise_scale[DUCK_FLEET_OBS_SIZE(DUCK_FLEET_MAX_NU)]; /* per obs column, the level folded in; 0: untouched */
} duck_fleet_disturbance;

int duck_fleet_disturb(const duck_fleet_desc* desc, const duck_fleet_disturbance* dis, int N, int64_t robot_offset,
                       int32_t* tick, const float* sched, const int32_t* sched_id, const float* push, float* qvel,
                       float* ctl, float* obs, void* stream);

/* The flight recorder: a ring of the last `depth` control periods per robot that freezes when the robot
 * falls, so that a fall is still there to be looked at after the run (the reference keeps what its loop saw
 * for the same purpose: saved_obs, mujoco_infer.py:202, :241). One more launch, enqueued last in the period,
 * after duck_fleet_actuate; a loop without a recorder does not enqueue it. All of its state is on the device
 * (head, after), so that a captured graph replays it.
 *
 * ring [N][depth][F] row-major float32, F = DUCK_FLEET_FRAME_SIZE(nq, nv, nu): a robot's ring is contiguous
 * and a frame is F consecutive words, in this order:
 *   qpos            nq                       qpos[k][e]
 *   qvel            nv                       qvel[k][e]; a push duck_fleet_disturb applied for the next period
 *                                            is already in it
 *   qacc_warmstart  nv                       warm[k][e]
 *   ctl             DUCK_FLEET_CTL_SIZE(nu)  the control record after duck_fleet_actuate
 *   obs             DUCK_FLEET_OBS_SIZE(nu)  what the policy saw, the noise included
 *   action          nu                       duck_policy_act's output, action [N][nu]
 *   actuator_force  nu                       aux rows 4 nv + a (write_aux's order, see duck_fleet_desc)
 *   sensors         DUCK_FLEET_SENS_SIZE     aux rows sens_off + gyro, accelerometer, upvector, local_linvel
 *                                            (3 each, in this order; raw: no offset, no noise)
 * That is the loop's whole input for the next period (qpos, qvel, qacc_warmstart, ctl; ctrl is not stored:
 * it equals ctl.motor_targets bit for bit) and what the robot sensed and did in this one. Words are copied,
 * never computed: NaN payloads, -0 and denormals keep their bits.
 *
 * For robot e, with dead = (alive[e] == 0): when dead and after[e] >= post + 1 the robot is frozen and
 * nothing of it is written. Otherwise the frame is written at slot head[e] % depth, head[e] += 1, and when
 * dead, after[e] += 1. So a robot that never falls holds its last min(head, depth) periods, oldest at slot
 * head % depth once head >= depth; one that falls holds the periods up to the one in which
 * duck_fleet_observe cleared alive (the fall frame) and `post` more (post = 0: the ring ends at the fall
 * frame); one that was dead before the first call writes post + 1 frames. head, after [N] int32, zeroed by
 * the caller; a frame carries no stamp: the j-th call (from 1) since the counters were zeroed wrote the frame
 * that head counted as its j-th, for every robot not yet frozen.
 *
 * desc gives nq, nv, nu, naux and the sensor addresses; DUCK_EINVAL on depth < 1, post < 0, a sensor address
 * outside the aux record (duck_fleet_observe's checks) or 4 nv + nu > naux. N == 0 launches nothing. */
#define DUCK_FLEET_SENS_SIZE 12
/* nq + 2 nv + CTL(nu) + OBS(nu) + 2 nu + 12, written out so the macro uses its arguments only */
#define DUCK_FLEET_FRAME_SIZE(nq, nv, nu) ((nq) + 2 * (nv) + 13 * (nu) + 40)

int duck_fleet_record(const duck_fleet_desc* desc, int N, int depth, int post, const float* qpos, const float* qvel,
                      const float* warm, const float* aux, const float* ctl, const float* obs, const float* action,
                      const float* alive, int32_t* head, int32_t* after, float* ring, void* stream);

/* Latency of the deployment loop: the action that reaches the motors, the IMU sample and the joint-encoder
 * readings that reach the policy are each 0 to DUCK_FLEET_MAX_DELAY control periods old (the training env's
 * action delay, joystick.py:361-376, and IMU delay, joystick.py:521-530; the encoder delay is the robot's own: its
 * joint positions and velocities are read back from bus servos over a half-duplex serial line, one after
 * another, and the training env does not model that). A delay is a whole number of periods (20 ms each);
 * DUCK_FLEET_MAX_DELAY is the depth of the action history the control record already holds. A loop that
 * configures no latency enqueues none of the three entries.
 *
 * lat [N][DUCK_FLEET_LAT_SIZE] row-major int32 = {act_lo, act_hi, sense_lo, sense_hi}, 0 <= lo <= hi <=
 * DUCK_FLEET_MAX_DELAY, validated by the caller; the kernels clamp lo into [0, MAX_DELAY] and hi into
 * [lo, MAX_DELAY], so that a bad row cannot address outside the robot's history or line. lo == hi is a fixed
 * delay; otherwise the delay is drawn per robot and period, uniformly over lo..hi, both ends included. (The
 * training env's randint(min, max) excludes max: its default action_min_delay = 0, action_max_delay = 3 is
 * (0, 2) here.)
 *
 * The period's count lives on the device, for duck_fleet_disturb's reason: lat_tick [N] int32, p = lat_tick[e]
 * the periods robot e completed since the latency was configured (0 then, set by the caller). It has one
 * writer, duck_fleet_actuate_delayed, as its last store; duck_fleet_sense_delay and duck_fleet_sensor_delay,
 * earlier in the period, read the same p. A negative lat_tick is read as p = 0.
 *
 * Random stream, threefry2x32 (20 rounds), apart from the disturbances': key = derive_key(seed, robot_offset + e,
 * DUCK_FLEET_LAT_TAG) (duck_fleet_disturb's key with the other tag; the latency has its own seed). Block b of
 * period p is threefry2x32(key, (p, b)). Word 0 of block 0 draws the action delay, word 1 of block 0 the IMU
 * delay, word 0 of block 1 the encoder delay (word 1 of block 1 is not used):
 *   d = lo + (((word >> 9) * (uint32_t)(hi - lo + 1)) >> 23)
 * in integers: exact, and never above hi. A robot's draws depend on (seed, id, p) only -- not on N, the launch
 * geometry or graph replay -- and a delay's draws do not depend on whether the other delays are drawn.
 *
 * duck_fleet_sense_delay, after duck_fleet_observe and before duck_fleet_disturb; enqueued only when some robot
 * has sense_hi > 0. line [N][DUCK_FLEET_MAX_DELAY + 1][6] row-major float32 is the robot's delay line of obs
 * columns 0-5 as duck_fleet_observe wrote them (gyro, then the accelerometer with the x offset; no noise yet).
 * For robot e: the six words go to slot p % 3; then, with d the drawn sensor delay and d_eff = min(d, min(p, 2))
 * (a line that is not yet full holds its oldest sample), when d_eff > 0 the six obs columns are overwritten
 * with the words of slot (p - d_eff) % 3; when d_eff == 0 obs is not written. Words are copied as uint32_t:
 * NaN payloads and -0 keep their bits. The noise of duck_fleet_disturb is added after the delay: it is i.i.d.
 * per period, so the sum has the distribution of the training env's noise-then-history order, and the line
 * stays a function of the true sensors. duck_fleet_observe's bookkeeping has run on the true sensors. This entry
 * delays the IMU columns only (the encoder columns: duck_fleet_sensor_delay). lat_tick is not written. desc
 * gives nu.
 *
 * duck_fleet_sensor_delay, in duck_fleet_sense_delay's place (after duck_fleet_observe, before duck_fleet_disturb);
 * enqueued only when some robot has enc_hi > 0, and then instead of duck_fleet_sense_delay: an encoder delay
 * adds no launch to a loop that delays the IMU, and one to a loop that does not.
 * enc [N][DUCK_FLEET_ENC_SIZE] row-major int32 = {enc_lo, enc_hi}, validated and clamped as a pair of lat is.
 * eline [N][DUCK_FLEET_MAX_DELAY + 1][2 nu] row-major float32 is the robot's delay line of the encoder words:
 * obs columns 13 .. 13 + 2 nu - 1 as duck_fleet_observe wrote them, qpos[act_qpos[a]] - act_default[a] for a <
 * nu and then dof_vel_scale * qvel[act_dof[a]] (no noise yet). One delay serves both groups: the position and
 * the velocity of a joint come from one servo read.
 *   IMU      duck_fleet_sense_delay's rule, word for word: obs columns 0-5, line, {sense_lo, sense_hi} of lat,
 *            the draw word 1 of block 0. With enc all zero, obs and line are that entry's bit for bit.
 *   encoder  for robot e: the 2 nu words go to slot p % 3 of eline (for every robot, whatever its row); then, with d
 *            the drawn encoder delay and d_eff = min(d, min(p, 2)), when d_eff > 0 the 2 nu obs columns are
 *            overwritten with the words of slot (p - d_eff) % 3; when d_eff == 0 they are not written.
 * Words are copied as uint32_t: NaN payloads and -0 keep their bits. No other obs column is written; the noise is
 * added after the delay and the bookkeeping has run on the true state, as above. lat_tick is not written. desc
 * gives nu.
 *
 * duck_fleet_actuate_delayed, in duck_fleet_actuate's place. The history shift is duck_fleet_actuate's:
 * last_action etc. hold the policy's undelayed actions (state.info["last_act"] in training). After the shift,
 * the action that forms the motor targets is history entry d, the drawn action delay: entry 0 this period's
 * action, entry 1 last_last_action, entry 2 last_last_last_action. The history starts at zero actions, as the
 * reference loop's and the training env's do, so a young history is not clamped. motor_targets, the
 * speed-limit clip, prev_motor_targets and ctrl are duck_fleet_actuate's fp32 expressions in its order on that
 * action: with d == 0 the result is duck_fleet_actuate's bit for bit. Last, lat_tick[e] = lat_tick[e] + 1.
 *
 * N == 0 launches nothing. */
#define DUCK_FLEET_MAX_DELAY 2
#define DUCK_FLEET_LAT_SIZE 4
#define DUCK_FLEET_LAT_TAG 0x1A7Eu
#define DUCK_FLEET_ENC_SIZE 2

int duck_fleet_sense_delay(const duck_fleet_desc* desc, int N, uint64_t seed, int64_t robot_offset,
                           const int32_t* lat_tick, const int32_t* lat, float* line, float* obs, void* stream);
int duck_fleet_sensor_delay(const duck_fleet_desc* desc, int N, uint64_t seed, int64_t robot_offset,
                            const int32_t* lat_tick, const int32_t* lat, const int32_t* enc,
                            float* line, float* eline, float* obs, void* stream);
int duck_fleet_actuate_delayed(const duck_fleet_desc* desc, int N, uint64_t seed, int64_t robot_offset,
                               int32_t* lat_tick, const int32_t* lat, const float* action, float* ctl,
                               float* ctrl, void* stream);

/* Following a recorded log: the robots are fed the actions a logged robot's policy gave, and every simulated
 * observation is scored against the logged one, per robot and per column (the reference compares the two by eye:
 * its loop and the robot both save what the policy saw, mujoco_infer.py:202, :241, and common/plot_saved_obs.py
 * plots them side by side). In duck_policy_act's place: after duck_fleet_observe, [sense_delay or
 * sensor_delay] and [disturb], before duck_fleet_actuate or duck_fleet_actuate_delayed -- a robot's IMU delay,
 * encoder delay and sensor noise are in the observation that is scored, its action delay acts on the fed action. No launch more than the loop with a
 * policy; a loop without a log does not enqueue it.
 *
 * log [n_log][T][DUCK_FLEET_LOG_SIZE(nu)] row-major float32: row p of a log is the observation the logged
 * robot's policy saw in period p (DUCK_FLEET_OBS_SIZE(nu) words in duck_fleet_observe's order), then the nu
 * actions the policy answered with. log_id [N] int32 names each robot's log, clamped into [0, n_log - 1] as
 * sched_id is. log_tick [N] int32 lives on the device, for tick's and lat_tick's reason: p = log_tick[e], a
 * negative value read as 0 (set to 0 by the caller at the log's start). score [N][DUCK_FLEET_OBS_SIZE(nu)]
 * float32, zeroed by the caller: the sum over the periods so far of the squared difference, per column.
 *
 * In this order, for robot e with row = log[min(max(log_id[e], 0), n_log - 1)]:
 *   score    when p < T, for every obs column k whose log word r = row[p][k] is not a NaN:
 *            d = obs[e][k] - r, q = d * d, score[e][k] = score[e][k] + q, each rounded on its own. A NaN in the
 *            log marks a missing sample: that score word is not written (it keeps its bits). A NaN in the
 *            simulated observation makes the score NaN, the right rank for such a model. alive is not looked at.
 *   action   when p < T: action[e][a] = row[p][OBS + a], copied as uint32_t (NaN payloads and -0 keep their
 *            bits); when p >= T: action[e][a] = +0.0.
 *   command  when p + 1 < T: the 7 words of ctl.command = row[p + 1][6 .. 12], copied; they take effect in the
 *            next period's observation, as a schedule's do. Otherwise the command is kept.
 *   tick     log_tick[e] = min(p + 1, T), the kernel's last store for the robot.
 * obs is read only. desc gives nu (the widths of ctl, obs and a log row). DUCK_EINVAL on n_log < 1 or T < 1.
 * N == 0 launches nothing. */
#define DUCK_FLEET_LOG_SIZE(nu) (17 + 7 * (nu)) /* an obs row, then the action that answered it */

int duck_fleet_follow(const duck_fleet_desc* desc, int N, int n_log, int T, const float* log, const int32_t* log_id,
                      int32_t* log_tick, const float* obs, float* score, float* ctl, float* action, void* stream);

/* Gait and servo load: how a robot that stays up does it -- how hard the servos push and how close to their force
 * and speed limits, how much the actions chatter, how the feet step, slip and clear the ground (the training env
 * prices some of these as costs, joystick.py `torques` and `action_rate`; the deployment loop has none of them).
 * One more launch, after duck_fleet_actuate or duck_fleet_actuate_delayed, so that history entry 0 is this period's
 * action and entry 1 the one before, and before duck_fleet_record, which stays last; a loop that does not ask for
 * it does not enqueue it. It reads this period's aux, qvel, ctl and alive and writes gait only.
 *
 * What is sampled: the period's last substep, 50 Hz. Peaks are peaks of those samples, and work is a 50 Hz
 * sampling of a 500 Hz signal.
 *
 * gait [N][DUCK_FLEET_GAIT_SIZE(nu)] row-major float32, zeroed by the caller; with B = 7 nu:
 *   [0, nu)        force_sq      sum of f^2
 *   [nu, 2nu)      force_max     max |f|
 *   [2nu, 3nu)     force_sat     periods with |f| >= force_sat[a]
 *   [3nu, 4nu)     speed_max     max |w|
 *   [4nu, 5nu)     speed_sat     periods with |w| >= speed_sat
 *   [5nu, 6nu)     work          sum of |f * w|
 *   [6nu, 7nu)     action_rate   sum of (last_action - last_last_action)^2
 *   B              periods       periods accumulated
 *   B + 1          double_support   periods with both feet in contact
 *   B + 2          flight           periods with neither foot in contact
 *   B + 3 + 6 f    foot f = 0 (left), 1 (right): contact, touchdowns, slip, apex_sum, prev (state), apex (state)
 * Counts are float adds of 1, exact below 2^24.
 *
 * For robot e, only while alive[e] != 0 (acc's rule: a dead robot gets no word written, the state words included;
 * duck_fleet_observe has cleared alive in the period of the fall, so that period is not accumulated and periods
 * equals acc[e][0] when both were zeroed together). With first = (gait[e][B] == 0), read before any store of the
 * call:
 *   actuator a < nu   f = aux[4 nv + a][e] (actuator_force, write_aux's order), w = qvel[act_dof[a]][e], af = |f|,
 *            aw = |w|: force_sq += f * f; force_max = af > force_max ? af : force_max (a NaN never enters a
 *            maximum); force_sat += 1 when af >= force_sat[a] (a NaN is not counted); the same two for aw against
 *            speed_sat; work += |f * w|; d = last_action[a] - last_last_action[a], action_rate += d * d.
 *   foot f   c = duck_fleet_observe's contact (any of the four con_dist slots at con_off + foot_con[f] is < 0);
 *            vx, vy = sensordata words foot_linvel[f] + 0, 1; z = word foot_pos[f] + 2.
 *            When c: contact += 1, slip += (vx * vx) + (vy * vy) (two products, their sum, the add).
 *            touchdown = !first && prev == 0 && c; liftoff = !first && prev != 0 && !c.
 *            When !c: apex = (first || liftoff) ? z : (z > apex ? z : apex).
 *            When touchdown: touchdowns += 1, apex_sum += apex - z (the subtraction, then the add): the height of
 *            the swing's highest sample over the landing sample.
 *            Last, prev = c ? 1 : 0.
 *   body     double_support += 1 when both feet are in contact, flight += 1 when neither is; periods += 1, the
 *            robot's last store.
 * Every value written is one fp32 operation on loaded words, each rounded on its own.
 *
 * DUCK_EINVAL on duck_fleet_observe's descriptor checks, 4 nv + nu > naux, or one of the four foot sensor
 * addresses outside the sensordata rows (adr < 0 or sens_off + adr + 3 > con_off). N == 0 launches nothing. */
typedef struct duck_fleet_gait_desc duck_fleet_gait_desc; /* the second host descriptor: its fields are stated in */
#include "duck_fleet_gait.h"                              /* duck_fleet_gait.h, which this header brings along */

/* The first word of each field (each macro in its own arguments only, as the sizes are): */
#define DUCK_FLEET_GAIT_FORCE_SQ(nu) (0 * (nu))
#define DUCK_FLEET_GAIT_FORCE_MAX(nu) (1 * (nu))
#define DUCK_FLEET_GAIT_FORCE_SAT(nu) (2 * (nu))
#define DUCK_FLEET_GAIT_SPEED_MAX(nu) (3 * (nu))
#define DUCK_FLEET_GAIT_SPEED_SAT(nu) (4 * (nu))
#define DUCK_FLEET_GAIT_WORK(nu) (5 * (nu))
#define DUCK_FLEET_GAIT_ACTION_RATE(nu) (6 * (nu))
#define DUCK_FLEET_GAIT_PERIODS(nu) (7 * (nu))
#define DUCK_FLEET_GAIT_DOUBLE_SUPPORT(nu) (7 * (nu) + 1)
#define DUCK_FLEET_GAIT_FLIGHT(nu) (7 * (nu) + 2)
#define DUCK_FLEET_GAIT_FOOT(nu, f) (7 * (nu) + 3 + 6 * (f)) /* foot f = 0, 1; then, inside a foot's six words: */
#define DUCK_FLEET_GAIT_FOOT_CONTACT 0
#define DUCK_FLEET_GAIT_FOOT_TOUCHDOWNS 1
#define DUCK_FLEET_GAIT_FOOT_SLIP 2
#define DUCK_FLEET_GAIT_FOOT_APEX_SUM 3
#define DUCK_FLEET_GAIT_FOOT_PREV 4
#define DUCK_FLEET_GAIT_FOOT_APEX 5
#define DUCK_FLEET_GAIT_FOOT_SIZE 6
#define DUCK_FLEET_GAIT_SIZE(nu) (7 * (nu) + 15)

int duck_fleet_gait(const duck_fleet_desc* desc, const duck_fleet_gait_desc* gait_desc, int N, const float* qvel,
                    const float* aux, const float* ctl, const float* alive, float* gait, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUCK_FLEET_H_ */
