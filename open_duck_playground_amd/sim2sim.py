"""Single-robot 50 Hz control loop with an ONNX policy in the loop (mirror of
playground/open_duck_mini_v2/mujoco_infer.py:16-241 and mujoco_infer_base.py:7-285).

The reference steps CPU MuJoCo (``mujoco.mj_step``) at 500 Hz in a viewer loop and runs the ONNX
policy every ``decimation`` = 10 steps. Here the physics of one control period (10 substeps) is one
``duck_physics_step`` launch of the HIP kernels for a single env, the policy runs on the host
(``onnx_infer.OnnxInfer``), and the viewer / keyboard / wall-clock pacing are replaced by an explicit
``run(n_periods, command)`` (``realtime=True`` sleeps like the reference's loop).

Observation (mujoco_infer.py:67-103), 101 values: gyro, accelerometer with +1.3 added to x (this
script applies it; the training env's obs does not, joystick.py:502), command[7], actuator joint
angles - default, 0.05 * joint velocities, the last three actions, motor targets, foot contacts
(any penetrating contact between a foot and the floor, mujoco_infer_base.py:259-282), imitation
phase (cos, sin) advanced by ``phase_frequency_factor`` per period (:184-205).

``FleetInfer`` is the same loop for N robots, resident on the device (include/duck_fleet.h): the question a
user has of an exported policy -- does it track commands over the whole command box, does it survive the
randomised models -- takes thousands of runs. ``python -m open_duck_playground_amd.sim2sim`` keeps the
reference's flags and adds ``--num_robots``, ``--periods``, ``--command_grid``, ``--randomize``, ``--out``, and the
disturbances the training env has and the reference's deployment loop lacks: ``--push_grid``, ``--push_at``,
``--push_every``, ``--push_magnitude``, ``--recovery_window``, ``--noise``, ``--noise_seed``,
``--resample_commands``; the latency the training env randomises and the joint encoders' (``--delay_grid
NAxNS[xNE]``), ``--delay_jitter``, ``--delay_seed``; and the flight recorder, ``--record_falls``, ``--record_post``, ``--record_out``,
``--record_max``: the last periods of every robot that fell, written to an ``.npz`` (the reference keeps what
its loop saw in ``saved_obs``; the file holds the same observations and the state around them).
``--policies P1 P2 ...`` puts several exported policies (the checkpoints of one training run) into one fleet,
``--num_robots`` / K robots each on the same models, commands, push cells and delays, and ranks them.
``--gait`` (``--gait_force_frac``, ``--gait_speed_frac``) keeps a gait and servo-load record per robot on the device
and adds its summary to the report: for the fleet, per command cell and per policy.
"""

from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import constants
from .cabi import HEADERS, dr_layout
from .joystick import Joystick
from .onnx_infer import OnnxInfer

USE_MOTOR_SPEED_LIMITS = True  # mujoco_infer.py:14
CON_PER_PAIR = HEADERS.consts["DUCK_CON_PER_PAIR"]   # con_dist slots of a collision pair


def aux_fields(m) -> Dict[str, Tuple[int, int]]:
    """(first row, rows) of each field of duck_physics_step's aux record, in write_aux's order
    (csrc/duck_physics.h; duck_aux_size rows in all)."""
    out, o = {}, 0
    for k, n in (("qacc", m.nv), ("qacc_smooth", m.nv), ("qvel", m.nv), ("qfrc_smooth", m.nv),
                 ("actuator_force", m.nu), ("sensordata", m.nsensordata), ("con_dist", CON_PER_PAIR * m.npair)):
        out[k] = (o, n)
        o += n
    return out


def foot_con_slots(m) -> List[int]:
    """The first con_dist slot of the (floor, foot) pair of each foot in constants.FEET_GEOMS; a pair has
    CON_PER_PAIR slots."""
    floor = m.id("geom", "floor")
    pairs = [{int(m.pair_geom1[k]), int(m.pair_geom2[k])} for k in range(m.npair)]
    return [CON_PER_PAIR * pairs.index({floor, m.id("geom", foot)}) for foot in constants.FEET_GEOMS]


class MjInfer:
    """MjInfer(model_path, reference_data, onnx_model_path, standing) on one MI355X env."""

    def __init__(self, model_path: str = "flat_terrain", reference_data: Optional[str] = None,
                 onnx_model_path: Optional[str] = None, standing: bool = False, device="cuda:0", policy=None):
        self.env = Joystick(model_path, num_envs=1, device=device, use_imitation=False)
        m = self.model = self.env.mj_model
        self.device = torch.device(device)
        self.sim_dt = 0.002   # mujoco_infer_base.py:15-18
        self.decimation = 10
        self.standing = standing
        self.head_control_mode = self.standing
        self.dof_vel_scale = 0.05
        self.action_scale = 0.25
        self.max_motor_velocity = 5.24
        self.phase_frequency_factor = 1.0
        self.num_dofs = m.nu
        self.policy = policy if policy is not None else OnnxInfer(onnx_model_path, awd=True)
        if not standing:
            table = np.load(reference_data or constants.POLY_COEFFICIENTS, allow_pickle=False)
            self.nb_steps_in_period = int(table["nb_steps_in_period"])
        self.actuator_qpos_addr = np.array([m.jnt_qposadr[j] for j in m.actuator_trnid])
        self.actuator_qvel_addr = np.array([m.jnt_dofadr[j] for j in m.actuator_trnid])
        names = m.names["sensor"]
        self.gyro_addr = int(m.sensor_adr[names.index("gyro")])
        self.accelerometer_addr = int(m.sensor_adr[names.index("accelerometer")])
        self._foot_slots = [slice(s, s + CON_PER_PAIR) for s in foot_con_slots(m)]
        self._aux_fields = aux_fields(m)
        key = m.names["key"].index("home")
        self.default_actuator = m.key_ctrl[key].copy()
        self.motor_targets = self.default_actuator.copy()
        self.prev_motor_targets = self.default_actuator.copy()
        self.last_action = np.zeros(self.num_dofs)
        self.last_last_action = np.zeros(self.num_dofs)
        self.last_last_last_action = np.zeros(self.num_dofs)
        self.commands = [0.0] * 7
        self.imitation_i = 0.0
        self.imitation_phase = np.array([0.0, 0.0])
        self.saved_obs: List[np.ndarray] = []
        # MJInferBase.__init__: MjData at qpos0 with zero ctrl, one mj_step, then the home keyframe's
        # qpos and ctrl (the velocity of that first step is kept)
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)[:, None], device=self.device)  # noqa: E731
        self.qpos, self.qvel = t(m.qpos0), t(np.zeros(m.nv))
        self.warm, self.ctrl = t(np.zeros(m.nv)), t(np.zeros(m.nu))
        self.aux = torch.zeros(self.env.aux_size(), 1, dtype=torch.float32, device=self.device)
        self.env.physics_step(self.qpos, self.qvel, self.warm, self.ctrl, 1, self.aux)
        self.qpos.copy_(t(m.key_qpos[key]))
        self.ctrl.copy_(t(self.default_actuator))
        self._aux_np = None

    # --- one control period of physics (mj_step x decimation) ---------------------------------
    def _physics(self):
        self.env.physics_step(self.qpos, self.qvel, self.warm, self.ctrl, self.decimation, self.aux)
        torch.cuda.synchronize(self.device)
        self._aux_np = self.aux[:, 0].cpu().numpy().astype(np.float64)

    def _aux(self, name: str) -> np.ndarray:
        o, n = self._aux_fields[name]
        return self._aux_np[o:o + n]

    def get_gyro(self) -> np.ndarray:
        return self._aux("sensordata")[self.gyro_addr:self.gyro_addr + 3].copy()

    def get_accelerometer(self) -> np.ndarray:
        return self._aux("sensordata")[self.accelerometer_addr:self.accelerometer_addr + 3].copy()

    def get_feet_contacts(self):
        d = self._aux("con_dist")
        return tuple(bool((d[s] < 0).any()) for s in self._foot_slots)

    def get_obs(self, command: Sequence[float]) -> np.ndarray:
        """mujoco_infer.py:67-103 (state of the last mj_step of the period, sensors as mj_step left them)."""
        gyro = self.get_gyro()
        accelerometer = self.get_accelerometer()
        accelerometer[0] += 1.3
        qpos = self.qpos[:, 0].cpu().numpy().astype(np.float64)
        qvel = self.qvel[:, 0].cpu().numpy().astype(np.float64)
        joint_angles = qpos[self.actuator_qpos_addr]
        joint_vel = qvel[self.actuator_qvel_addr]
        contacts = np.array(self.get_feet_contacts(), dtype=np.float64)
        return np.concatenate([gyro, accelerometer, np.asarray(command, dtype=np.float64),
                               joint_angles - self.default_actuator, joint_vel * self.dof_vel_scale,
                               self.last_action, self.last_last_action, self.last_last_last_action,
                               self.motor_targets, contacts, self.imitation_phase])

    def control_step(self):
        """One policy period of mujoco_infer.py:175-241: decimation substeps, then obs -> action -> ctrl."""
        self._physics()
        if not self.standing:
            self.imitation_i += 1.0 * self.phase_frequency_factor
            self.imitation_i = self.imitation_i % self.nb_steps_in_period
            ph = self.imitation_i / self.nb_steps_in_period * 2 * np.pi
            self.imitation_phase = np.array([np.cos(ph), np.sin(ph)])
        obs = self.get_obs(self.commands)
        self.saved_obs.append(obs)
        action = np.asarray(self.policy.infer(obs), dtype=np.float64)
        self.last_last_last_action = self.last_last_action.copy()
        self.last_last_action = self.last_action.copy()
        self.last_action = action.copy()
        self.motor_targets = self.default_actuator + action * self.action_scale
        if USE_MOTOR_SPEED_LIMITS:
            lim = self.max_motor_velocity * (self.sim_dt * self.decimation)
            self.motor_targets = np.clip(self.motor_targets, self.prev_motor_targets - lim,
                                         self.prev_motor_targets + lim)
            self.prev_motor_targets = self.motor_targets.copy()
        self.ctrl.copy_(torch.tensor(self.motor_targets.astype(np.float32)[:, None], device=self.device))
        return obs, action

    def run(self, n_periods: int, command: Optional[Sequence[float]] = None, realtime: bool = False):
        if command is not None:
            self.commands = list(command)
        period = self.sim_dt * self.decimation
        for _ in range(n_periods):
            t0 = time.time()
            self.control_step()
            if realtime:
                time.sleep(max(0.0, period - (time.time() - t0)))
        return self.saved_obs


# --- the same loop for N robots, resident on the device ----------------------------------------

COMMANDS_RANGE_X = (-0.15, 0.15)      # mujoco_infer.py:40-42
COMMANDS_RANGE_Y = (-0.2, 0.2)
COMMANDS_RANGE_THETA = (-1.0, 1.0)


def fleet_obs_size(nu: int) -> int:
    """DUCK_FLEET_OBS_SIZE(nu): the width of the deployment loop's observation."""
    return HEADERS.value(f"DUCK_FLEET_OBS_SIZE({int(nu)})")


def ctl_fields(nu: int) -> Dict[str, Tuple[int, int]]:
    """(first column, width) of each field of the per-robot control record (include/duck_fleet.h)."""
    at = lambda field, *d: HEADERS.value(f"DUCK_FLEET_CTL_{field}({', '.join(str(int(v)) for v in (nu, *d))})")  # noqa: E731
    return {"last_action": (at("ACTION", 0), nu), "last_last_action": (at("ACTION", 1), nu),
            "last_last_last_action": (at("ACTION", 2), nu), "motor_targets": (at("MOTOR_TARGETS"), nu),
            "prev_motor_targets": (at("PREV_MOTOR_TARGETS"), nu), "command": (at("COMMAND"), 7),
            "imitation_i": (at("IMITATION_I"), 1), "phase_frequency_factor": (at("PHASE_FREQUENCY_FACTOR"), 1),
            "imitation_phase": (at("IMITATION_PHASE"), 2)}


FRAME_SENSORS = ("gyro", "accelerometer", "upvector", "local_linvel")   # the order inside a frame's "sensors"


def frame_fields(nq: int, nv: int, nu: int) -> Dict[str, Tuple[int, int]]:
    """(first word, width) of each field of a recorded frame, in the frame's order (include/duck_fleet.h
    duck_fleet_record; DUCK_FLEET_FRAME_SIZE(nq, nv, nu) words in all). ``ctl`` is the whole control record
    (``ctl_fields``), ``sensors`` the four raw sensors of ``FRAME_SENSORS``, 3 words each."""
    out, o = {}, 0
    for k, n in (("qpos", nq), ("qvel", nv), ("qacc_warmstart", nv), ("ctl", HEADERS.value(f"DUCK_FLEET_CTL_SIZE({int(nu)})")),
                 ("obs", fleet_obs_size(nu)), ("action", nu), ("actuator_force", nu),
                 ("sensors", HEADERS.consts["DUCK_FLEET_SENS_SIZE"])):
        out[k] = (o, int(n))
        o += int(n)
    assert o == HEADERS.value(f"DUCK_FLEET_FRAME_SIZE({int(nq)},{int(nv)},{int(nu)})")
    return out


def unroll_ring(ring_row, head: int, depth: int, rec_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """One robot's ring in period order. ``ring_row`` [depth][F] (or flat), ``head`` the frames the robot has
    written: the last min(head, depth) of them are held, the j-th written (from 1) at slot (j - 1) % depth.
    Returns (frames [T][F] oldest first, period [T] = rec_base + j)."""
    depth, head = int(depth), int(head)
    ring_row = np.asarray(ring_row).reshape(depth, -1)
    j = np.arange(max(head - depth, 0), head, dtype=np.int64)        # j - 1 of the frames still held
    return ring_row[j % depth], int(rec_base) + j + 1


def fleet_desc(m, naux: int, nb_steps_in_period: int, standing: bool, speed_limits: bool = USE_MOTOR_SPEED_LIMITS):
    """duck_fleet_desc (include/duck_fleet.h) of a compiled model: where the deployment loop's sensors,
    actuated joints and foot contacts are, and the loop's constants (mujoco_infer.py:27-31, :58, :74)."""
    from .native import FLEET_MAX_NU, DuckError, DuckFleetDesc
    if m.nu > FLEET_MAX_NU:
        raise DuckError(f"the fleet kernels take at most {FLEET_MAX_NU} actuators, the model has {m.nu}")
    d = DuckFleetDesc()
    d.nq, d.nv, d.nu, d.naux = int(m.nq), int(m.nv), int(m.nu), int(naux)
    aux = aux_fields(m)
    d.sens_off, d.con_off = aux["sensordata"][0], aux["con_dist"][0]
    names = m.names["sensor"]
    for field, sensor in (("gyro", constants.GYRO_SENSOR), ("accelerometer", constants.ACCELEROMETER_SENSOR),
                          ("upvector", constants.GRAVITY_SENSOR), ("local_linvel", constants.LOCAL_LINVEL_SENSOR)):
        setattr(d, field, int(m.sensor_adr[names.index(sensor)]))
    key = m.names["key"].index("home")
    for a, j in enumerate(m.actuator_trnid):
        d.act_qpos[a], d.act_dof[a] = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        d.act_default[a] = float(m.key_ctrl[key][a])
    d.foot_con[:] = foot_con_slots(m)
    d.dof_vel_scale, d.action_scale, d.accel_x_offset = 0.05, 0.25, 1.3
    d.target_step = float(np.float32(5.24 * 0.002 * 10))
    d.nb_steps_in_period = int(nb_steps_in_period)
    d.standing, d.speed_limits = int(bool(standing)), int(bool(speed_limits))
    return d


MAX_MOTOR_VELOCITY = 5.24     # rad/s, mujoco_infer.py:58
GAIT_ACTUATOR_FIELDS = ("force_sq", "force_max", "force_sat", "speed_max", "speed_sat", "work", "action_rate")
GAIT_FOOT_FIELDS = ("contact", "touchdowns", "slip", "apex_sum", "prev", "apex")
GAIT_FEET = ("left", "right")


def gait_fields(nu: int) -> Dict[str, Tuple[int, int]]:
    """(first column, width) of each field of the per-robot gait record (include/duck_fleet.h duck_fleet_gait;
    DUCK_FLEET_GAIT_SIZE(nu) words in all): the seven per-actuator blocks, ``periods``, ``double_support``,
    ``flight`` and, per foot, ``left_contact`` ... ``right_apex``."""
    nu = int(nu)
    at = lambda field, *f: HEADERS.value(f"DUCK_FLEET_GAIT_{field}({', '.join(str(int(v)) for v in (nu, *f))})")  # noqa: E731
    out = {name: (at(name.upper()), nu) for name in GAIT_ACTUATOR_FIELDS}
    out.update({name: (at(name.upper()), 1) for name in ("periods", "double_support", "flight")})
    for f, foot in enumerate(GAIT_FEET):
        for name in GAIT_FOOT_FIELDS:
            out[f"{foot}_{name}"] = (at("FOOT", f) + HEADERS.consts[f"DUCK_FLEET_GAIT_FOOT_{name.upper()}"], 1)
    assert max(o + w for o, w in out.values()) == HEADERS.value(f"DUCK_FLEET_GAIT_SIZE({nu})")
    return out


def gait_desc(m, force_frac: float = 0.9, speed_frac: float = 1.0):
    """duck_fleet_gait_desc (include/duck_fleet_gait.h) of a compiled model: the feet's velocity and position sensors by
    name, and the saturation thresholds -- ``force_frac`` of each force-limited actuator's largest |forcerange|
    (+inf for one without a limit: never saturated), ``speed_frac`` of the reference loop's max_motor_velocity."""
    from .native import FLEET_MAX_NU, DuckError, DuckFleetGaitDesc
    if m.nu > FLEET_MAX_NU:
        raise DuckError(f"the fleet kernels take at most {FLEET_MAX_NU} actuators, the model has {m.nu}")
    if not (float(force_frac) >= 0 and float(speed_frac) >= 0):
        raise DuckError(f"the gait thresholds are fractions >= 0, got {force_frac!r}, {speed_frac!r}")
    d = DuckFleetGaitDesc()
    names = m.names["sensor"]
    for f, site in enumerate(constants.FEET_SITES):
        d.foot_linvel[f] = int(m.sensor_adr[names.index(f"{site}_global_linvel")])
        d.foot_pos[f] = int(m.sensor_adr[names.index(constants.FEET_POS_SENSOR[f])])
    for a in range(FLEET_MAX_NU):
        limited = a < m.nu and bool(m.actuator_forcelimited[a])
        d.force_sat[a] = float(force_frac) * float(np.abs(m.actuator_forcerange[a]).max()) if limited else float("inf")
    d.speed_sat = float(speed_frac) * MAX_MOTOR_VELOCITY
    return d


class FleetInfer:
    """The deployment loop of ``MjInfer`` for ``num_robots`` robots at once, resident on the device: one
    control period is four launches on one stream -- duck_physics_step (10 substeps, with the aux record),
    duck_fleet_observe, duck_policy_act, duck_fleet_actuate (include/duck_fleet.h) -- with no host round
    trip. The exported ONNX policy is imported as dense layers (onnx_infer.dense_policy); one outside
    duck_policy_act's limits raises DuckError (there is no host fallback).

    Every robot starts as MJInferBase starts its one: a substep from qpos0 with zero ctrl, then the home
    keyframe's qpos and ctrl with that step's velocity kept. ``randomize=seed`` gives each robot its
    duck_randomize(seed) model for the whole run (before that first step); None runs the nominal model.
    Per robot, duck_fleet_observe accumulates the periods survived, the tracked velocity and the squared
    tracking errors until the robot falls (``report()``); fallen robots keep being simulated and controlled.

    The first ``run`` is eager; later ones replay a captured graph of ``CHUNK`` periods (one stream, a
    linear graph) and run the remainder eagerly.

    Disturbances (all off by default; ``set_command_schedule``, ``set_pushes``, ``set_noise`` or the
    keyword arguments of the same names, each the tuple of its setter's arguments): when any is
    configured, a period is physics -> observe -> duck_fleet_disturb -> policy -> actuate, the fifth launch
    adding sensor noise to the observation, writing the next period's command and pushing the base before
    the next period's physics. The period count ``tick`` lives on the device, so a captured graph replays it.
    With none configured the loop is the four launches above, unchanged. ``robot_offset`` is the global id of
    robot 0 in the disturbance stream (a robot's draws depend on the seed, its global id and the period only).

    Latency (off by default; ``set_latency(action, sense, seed, encoder)`` or ``latency=(action, sense, seed[,
    encoder])``): the action that reaches the motors, the IMU sample and the joint-encoder readings that reach the
    policy are 0 to 2 control periods old, fixed per robot or drawn per robot and period (the training env's action
    and IMU delay; the encoder delay is the robot's serial servo bus). With a latency
    set, duck_fleet_actuate_delayed takes duck_fleet_actuate's place (no launch more), and with an IMU delay
    among it duck_fleet_sense_delay runs right after duck_fleet_observe (one launch more); with an encoder delay
    among it duck_fleet_sensor_delay runs in that place and delays both (no launch more than that): physics ->
    observe -> [sense_delay or sensor_delay] -> [disturb] -> policy -> actuate or actuate_delayed -> [record]. The
    latency has its own seed and its own period count ``lat_tick`` on the device. With none set (``latent()``
    False) the loop enqueues exactly the launches above.

    The flight recorder (off by default; ``set_recorder(depth, post)`` or ``recorder=(depth, post)``): one more
    launch at the end of the period, duck_fleet_record, keeps every robot's last ``depth`` periods in a ring on
    the device -- the state the next period starts from, the control record, the observation the policy saw,
    its action, the actuator forces and the raw sensors -- and freezes a robot's ring ``post`` periods after
    the one in which it fell. Its counters live on the device, so it runs inside the captured graph.
    ``recorded(robot)`` returns the frames in period order; ``replay(robot, frame)`` returns a one-robot fleet
    loaded from a recorded frame, whose next periods reproduce the robot's bit for bit.

    Following a log (off by default; ``set_log(log, ids)`` or ``follow=(log, ids)``): duck_fleet_follow takes
    duck_policy_act's place (no launch more): physics -> observe -> [sense_delay or sensor_delay] -> [disturb] ->
    policy or follow -> actuate or actuate_delayed -> [record]. The robots are fed the actions and commands of a recorded robot log,
    and ``scores()`` / ``score_report()`` tell, per robot and observation column, how far the simulated observations
    were from the logged ones: over randomised models and a delay grid, which model the logged robot moves like.
    ``onnx_model_path=None`` is allowed with ``follow``: no policy is loaded. The start state is the loop's own (a log
    that starts elsewhere is the caller's to load with ``load_state``).
    With no log set (``following()`` False) the loop enqueues exactly the launches above.

    Gait and servo load (off by default; ``set_gait(on, force_frac, speed_frac)`` or ``gait=(on, force_frac,
    speed_frac)``): one more launch after the actuation and before the recorder's, duck_fleet_gait: physics -> observe ->
    [sense_delay or sensor_delay] -> [disturb] -> policy or follow -> actuate or actuate_delayed -> [gait] -> [record].
    Per robot and while it is alive it sums, per actuator, the squared force, |force x joint speed| and the squared
    action change, keeps the peak force and joint speed and counts the periods at the force and the speed limit; per
    foot it counts contact periods and touchdowns and sums the slip speed squared and the swing clearance; and it
    counts the periods of double support and of flight (``gait_records()``, ``gait_report``, ``gait_summary``). The
    samples are the period's last substep's (50 Hz). It reads the loop and writes its own record only; with it off
    (``gaited()`` False) the loop enqueues exactly the launches above. A ``replay()`` has it off: a frame does not
    carry the gait state.

    Several policies (``onnx_model_path`` a list or tuple of K paths, at most DUCK_POLICY_MAX_POLICIES, all of one
    architecture and all with or all without a normaliser): the robots are policy-major, segment k --
    ``policy_robots[k]`` robots, by default ``num_robots / K`` each -- is served by file k, and duck_policy_act_multi
    takes duck_policy_act's place (no launch more; a tile of 16 rows never mixes policies). ``num_policies``,
    ``policy_seg`` [K + 1] and ``policy_of`` [N] tell who is served by what. Robot r of segment k computes what a
    single-policy fleet of that segment with ``robot_offset`` + seg[k] computes, bit for bit. A ``str`` path is
    today's loop with today's launches; a list of one path goes through the new entry with K = 1. A list cannot be
    combined with ``follow``.
    Pairing: ``randomize=seed`` with several policies needs equal segments of S robots, draws S models and gives
    every segment the same S columns of the randomisation record; ``tile_over_policies(a)`` repeats an [S, ...]
    per-robot table K times for ``set_commands``, the schedule ids, ``set_pushes`` and ``set_latency``. Robot j of
    every segment then has the same model, commands, push cell and fixed delays, and ``paired_wins`` compares the
    policies scenario by scenario. Pairing does NOT cover the random streams -- the sensor noise, a push drawn from a
    range (lo != hi) and delay jitter: they are keyed by the robot's global id, so they are independent between
    segments and identically distributed, not common random numbers."""

    # control periods per captured graph (200 launches; 50 more with disturbances, 50 more with an IMU or encoder delay, 50 more
    # with the gait record, 50 more with a recorder: 400 at the most)
    CHUNK = 50

    def __init__(self, model_path: str = "flat_terrain", onnx_model_path: Optional[str] = None, num_robots: int = 1,
                 reference_data: Optional[str] = None, standing: bool = False, device="cuda:0",
                 randomize: Optional[int] = None, command_schedule: Optional[tuple] = None,
                 pushes: Optional[tuple] = None, noise: Optional[tuple] = None, recorder: Optional[tuple] = None,
                 robot_offset: int = 0, latency: Optional[tuple] = None, follow: Optional[tuple] = None,
                 policy_robots: Optional[Sequence[int]] = None, gait: Optional[tuple] = None):
        import ctypes as C

        from .native import DuckError, check
        from .onnx_infer import OnnxGraph, dense_policy
        from .ppo import POLICY_ACT_MAX_LAYERS, POLICY_ACT_MAX_WIDTH
        n = self.num_robots = int(num_robots)
        if n < 1:
            raise DuckError("num_robots must be >= 1")
        pol = pols = None
        self.num_policies, self.policy_seg = 1, np.array([0, n], dtype=np.int32)
        if isinstance(onnx_model_path, (list, tuple)):
            onnx_model_path = [str(p) for p in onnx_model_path]
            pols, self.policy_seg = load_policies(onnx_model_path, n, policy_robots, following=follow is not None)
            self.num_policies = len(pols)
            pol, sizes = pols[0], pols[0]["sizes"]
            if randomize is not None and len(set(np.diff(self.policy_seg).tolist())) > 1:
                raise DuckError(f"randomize pairs the policies on the same models: it needs equal segments, got "
                                f"{np.diff(self.policy_seg).tolist()} robots")
        elif policy_robots is not None:
            raise DuckError("policy_robots splits the robots over a list of policies: onnx_model_path is not a list")
        elif onnx_model_path is None:
            if follow is None:
                raise DuckError("a fleet needs a policy (onnx_model_path) or a log to follow (follow=(log, ids))")
        else:
            with open(onnx_model_path, "rb") as f:
                pol = dense_policy(OnnxGraph(f.read()))
            sizes = pol["sizes"]
            if len(pol["W"]) > POLICY_ACT_MAX_LAYERS or max(sizes) > POLICY_ACT_MAX_WIDTH:
                raise DuckError(f"policy layers {sizes} are outside duck_policy_act's limits (at most "
                                f"{POLICY_ACT_MAX_LAYERS} layers, at most {POLICY_ACT_MAX_WIDTH} wide); there is no host fallback")
        self.env = Joystick(model_path, num_envs=n, device=device, use_imitation=False)
        m = self.model = self.env.mj_model
        self.device = dev = torch.device(device)
        self.standing = bool(standing)
        self.decimation = 10
        self._lib, self._sim, self._check = self.env._lib, self.env._sim, check
        nb = 0
        if not standing:
            table = np.load(reference_data or constants.POLY_COEFFICIENTS, allow_pickle=False)
            nb = int(table["nb_steps_in_period"])
        self.nb_steps_in_period = nb
        naux = self.env.aux_size()
        self.desc = fleet_desc(m, naux, nb, standing)
        nu = self.num_dofs = int(m.nu)
        self.obs_size = fleet_obs_size(nu)

        # the policy's dense layers on the device, pointers in host arrays (duck_policy_act's arguments)
        self._policy_args = None        # no policy loaded: the fleet can only follow a log
        self._multi_args = None         # a list of policies: duck_policy_act_multi's (K, seg) in front of them
        self.policy_of = np.repeat(np.arange(self.num_policies), np.diff(self.policy_seg)).astype(np.int32)
        if pol is not None:
            if sizes[0] != self.obs_size or pol["action_size"] != nu:
                raise DuckError(f"policy maps {sizes[0]} -> {pol['action_size']}, the model's loop needs {self.obs_size} -> {nu}")
            up = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
            if pols is not None:   # the K policies' parameters stacked [K][...]
                stack = lambda key, l=None: np.stack([p[key] if l is None else p[key][l] for p in pols])  # noqa: E731
                pol = {"W": [stack("W", l) for l in range(len(sizes) - 1)], "b": [stack("b", l) for l in range(len(sizes) - 1)],
                       "mean": None if pol["mean"] is None else stack("mean"),
                       "istd": None if pol["istd"] is None else stack("istd")}
                self._multi_args = (self.num_policies, (C.c_int * (self.num_policies + 1))(*self.policy_seg.tolist()))
            self._W, self._b = [up(w) for w in pol["W"]], [up(b) for b in pol["b"]]
            self._mean, self._istd = up(pol["mean"]), up(pol["istd"])
            self._policy_args = (len(sizes) - 1, (C.c_int * len(sizes))(*sizes),
                                 (C.c_void_p * len(self._W))(*[w.data_ptr() for w in self._W]),
                                 (C.c_void_p * len(self._b))(*[b.data_ptr() for b in self._b]),
                                 None if self._mean is None else self._mean.data_ptr(),
                                 None if self._istd is None else self._istd.data_ptr())

        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.qpos, self.qvel = z(m.nq, n), z(m.nv, n)
        self.warm, self.ctrl, self.aux = z(m.nv, n), z(nu, n), z(naux, n)
        self.fields = ctl_fields(nu)
        self.ctl, self.obs, self.action = z(n, HEADERS.value(f"DUCK_FLEET_CTL_SIZE({nu})")), z(n, self.obs_size), z(n, nu)
        self.acc, self.alive = z(n, HEADERS.consts["DUCK_FLEET_ACC_SIZE"]), torch.ones(n, dtype=torch.float32, device=dev)
        self.dr = None
        if randomize is not None:
            rows, K = dr_layout(m.nbody, nu)["nfloat"], self.num_policies
            self.dr = z(rows * n)
            s = n // K     # several policies: S models, every segment the same S columns of the record
            draw = self.dr if K == 1 else z(rows * s)
            check(self._lib.duck_randomize(self._sim, s, draw.data_ptr(), int(randomize) & 0xFFFFFFFFFFFFFFFF, 0,
                                           self._stream()), self._lib)
            if K > 1:
                self.dr.view(rows, K, s).copy_(draw.view(rows, 1, s).expand(rows, K, s))
        self.default_actuator = np.asarray(m.key_ctrl[m.names["key"].index("home")], dtype=np.float32)
        self.calls, self.graph = 0, None
        # the disturbances (include/duck_fleet.h duck_fleet_disturb): all off
        from .native import DuckFleetDisturbance
        self.tick = torch.zeros(n, dtype=torch.int32, device=dev)
        self.dis = DuckFleetDisturbance()
        self.sched = self.sched_id = self.push = None
        self.robot_offset = int(robot_offset)
        # the latency (include/duck_fleet.h duck_fleet_sense_delay, duck_fleet_sensor_delay,
        # duck_fleet_actuate_delayed): off
        self.lat = self.lat_tick = self.line = self.enc = self.eline = None
        self.lat_seed = self.lat_base = 0
        self.lat_sense = self.lat_encoder = False
        # following a log (include/duck_fleet.h duck_fleet_follow): off
        self.log = self.log_id = self.log_tick = self.score = None
        self.log_base = 0
        # gait and servo load (include/duck_fleet.h duck_fleet_gait): off
        self.gait_fields = gait_fields(nu)
        self.gait_desc = self.gait_rec = None
        # the flight recorder (include/duck_fleet.h duck_fleet_record): off
        self.frame_fields = frame_fields(int(m.nq), int(m.nv), nu)
        self.ring = self.rec_head = self.rec_after = None
        self.rec_depth = self.rec_post = self.rec_base = self.periods_done = 0
        self._made_from = dict(model_path=model_path, onnx_model_path=onnx_model_path, reference_data=reference_data,
                               standing=standing, device=device)
        self.restart()
        if command_schedule is not None:
            self.set_command_schedule(*command_schedule)
        if pushes is not None:
            self.set_pushes(*pushes)
        if noise is not None:
            self.set_noise(*noise)
        if recorder is not None:
            self.set_recorder(*recorder)
        if latency is not None:
            self.set_latency(*latency)
        if follow is not None:
            self.set_log(*follow)
        if gait is not None:
            self.set_gait(*gait)

    def restart(self) -> None:
        """Every robot back to the loop's start, with the randomisation record ``dr`` as it is now.
        MJInferBase.__init__: MjData at qpos0 with zero ctrl, one mj_step, then the home keyframe's qpos and
        ctrl (the velocity of that first step is kept); mujoco_infer.py:49-60 for the control record. The
        period count goes back to 0, a command schedule to its segment 0, a recorder to no frames, a latency
        to its first period (the delay line fills anew), a followed log to its row 0 with zero scores and the gait
        record to zero."""
        m, n = self.model, self.num_robots
        col = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)[:, None], device=self.device)  # noqa: E731
        key = m.names["key"].index("home")
        self.qpos.copy_(col(m.qpos0).expand(-1, n))
        for t in (self.qvel, self.warm, self.ctrl, self.ctl):
            t.zero_()
        self._physics(1)
        self.qpos.copy_(col(m.key_qpos[key]).expand(-1, n))
        self.ctrl.copy_(col(self.default_actuator).expand(-1, n))
        default = torch.tensor(self.default_actuator, device=self.device)
        self.ctl_field("motor_targets").copy_(default.expand(n, -1))
        self.ctl_field("prev_motor_targets").copy_(default.expand(n, -1))
        self.ctl_field("phase_frequency_factor").fill_(1.0)
        self.tick.zero_()
        self._schedule_command()   # segment 0 of a schedule, if one is set
        self.reset_report()
        self.periods_done = self.rec_base = 0
        if self.ring is not None:
            self.rec_head.zero_()
            self.rec_after.zero_()
        self.lat_base = 0
        if self.lat_tick is not None:
            self.lat_tick.zero_()
        self.log_base = 0
        if self.log is not None:
            self.log_tick.zero_()
            self.score.zero_()
            self._log_command()    # row 0's command

    # --- launches -----------------------------------------------------------------------------
    def _stream(self):
        import ctypes as C
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _physics(self, n_substeps: int):
        L = self._lib
        self._check(L.duck_physics_step(self._sim, self.num_robots, self.qpos.data_ptr(), self.qvel.data_ptr(),
                                        self.warm.data_ptr(), self.ctrl.data_ptr(),
                                        None if self.dr is None else self.dr.data_ptr(), int(n_substeps),
                                        self.aux.data_ptr(), self._stream()), L)

    def _launch(self, name: str, *args, lead=()):
        """A fleet entry of the model's library: the descriptor (then ``lead``) and N in front, tensors as their
        device pointers (None stays NULL), the stream behind."""
        import ctypes as C
        L = self._lib
        ptrs = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in args]
        self._check(getattr(L, name)(C.byref(self.desc), *lead, self.num_robots, *ptrs, self._stream()), L)

    def observe(self):
        """duck_fleet_observe on the current state: phase, observation, bookkeeping."""
        self._launch("duck_fleet_observe", self.qpos, self.qvel, self.aux, self.ctl, self.obs, self.acc, self.alive)

    def policy(self):
        """duck_policy_act on ``obs``; of a fleet made from a list of policies, duck_policy_act_multi."""
        from .native import DuckError, lib
        if self._policy_args is None:
            raise DuckError("no policy is loaded (onnx_model_path=None): the fleet can only follow a log (set_log)")
        P = lib()   # the policy kernel ships with libduck.so only, the rest with the model's library
        if self._multi_args is not None:
            self._check(P.duck_policy_act_multi(self.num_robots, *self._multi_args, *self._policy_args, self.obs.data_ptr(),
                                                None, self.action.data_ptr(), self._stream()), P)
            return
        self._check(P.duck_policy_act(self.num_robots, *self._policy_args, self.obs.data_ptr(), None,
                                      self.action.data_ptr(), self._stream()), P)

    def actuate(self):
        """duck_fleet_actuate: history, motor targets, ctrl."""
        self._launch("duck_fleet_actuate", self.action, self.ctl, self.ctrl)

    def act(self):
        """duck_policy_act on ``obs`` (following a log: duck_fleet_follow in its place), then duck_fleet_actuate,
        or with a latency duck_fleet_actuate_delayed."""
        if self.following():
            self.follow()
        else:
            self.policy()
        if self.latent():
            self.actuate_delayed()
        else:
            self.actuate()

    def latent(self) -> bool:
        """Whether a latency is set (duck_fleet_actuate_delayed in duck_fleet_actuate's place)."""
        return self.lat is not None

    def following(self) -> bool:
        """Whether a log is set (duck_fleet_follow in duck_policy_act's place)."""
        return self.log is not None

    def follow(self):
        """duck_fleet_follow on this period's ``obs``: the score, the log's action, the next period's command, log_tick."""
        self._launch("duck_fleet_follow", int(self.log.shape[0]), int(self.log.shape[1]), self.log, self.log_id,
                     self.log_tick, self.obs, self.score, self.ctl, self.action)

    def sense_delay(self):
        """duck_fleet_sense_delay on this period's ``obs``: the IMU columns into the delay line and, delayed, back."""
        self._launch("duck_fleet_sense_delay", self.lat_seed, self.robot_offset, self.lat_tick, self.lat, self.line, self.obs)

    def sensor_delay(self):
        """duck_fleet_sensor_delay on this period's ``obs``: duck_fleet_sense_delay's IMU columns and, by the same
        rule on their own line, the joint-encoder columns."""
        self._launch("duck_fleet_sensor_delay", self.lat_seed, self.robot_offset, self.lat_tick, self.lat, self.enc,
                     self.line, self.eline, self.obs)

    def actuate_delayed(self):
        """duck_fleet_actuate_delayed: duck_fleet_actuate on the delayed entry of the history, then lat_tick."""
        self._launch("duck_fleet_actuate_delayed", self.lat_seed, self.robot_offset, self.lat_tick, self.lat, self.action,
                     self.ctl, self.ctrl)

    def disturbed(self) -> bool:
        """Whether a schedule, a push table or a non-zero noise is set (the loop's fifth launch)."""
        return self.sched is not None or self.push is not None or any(self.dis.noise_scale)

    def disturb(self):
        """duck_fleet_disturb on this period's ``obs``: noise, the next period's command and push, the tick."""
        import ctypes as C
        self._launch("duck_fleet_disturb", self.robot_offset, self.tick, self.sched, self.sched_id, self.push, self.qvel,
                     self.ctl, self.obs, lead=(C.byref(self.dis),))

    def gaited(self) -> bool:
        """Whether the gait record is kept (duck_fleet_gait after the actuation)."""
        return self.gait_rec is not None

    def gait(self):
        """duck_fleet_gait on this period's aux, qvel, ctl and alive: the servo loads, the action rate, the feet."""
        import ctypes as C
        self._launch("duck_fleet_gait", self.qvel, self.aux, self.ctl, self.alive, self.gait_rec,
                     lead=(C.byref(self.gait_desc),))

    def record(self):
        """duck_fleet_record: this period's frame into the ring of every robot not yet frozen."""
        self._launch("duck_fleet_record", self.rec_depth, self.rec_post, self.qpos, self.qvel, self.warm, self.aux,
                     self.ctl, self.obs, self.action, self.alive, self.rec_head, self.rec_after, self.ring)

    def _periods(self, k: int, rec: Optional[torch.Tensor] = None, t0: int = 0):
        disturbed, recording, gaited = self.disturbed(), self.ring is not None, self.gaited()
        sense = self.latent() and self.lat_sense
        encoder = self.latent() and self.lat_encoder      # the IMU and the encoders in one launch, in sense_delay's place
        for t in range(k):
            self._physics(self.decimation)
            self.observe()
            if encoder:
                self.sensor_delay()
            elif sense:
                self.sense_delay()
            if disturbed:
                self.disturb()
            if rec is not None:
                rec[t0 + t].copy_(self.obs)
            self.act()
            if gaited:
                self.gait()
            if recording:
                self.record()

    @torch.no_grad()
    def run(self, n_periods: int, record: bool = False):
        """``n_periods`` control periods for every robot. ``record=True`` returns the observations
        [T][N][obs] the policy saw (a numpy array; such a run is eager). Following a log of T rows, a run that
        would pass row T raises before anything is enqueued; so does one with neither a policy nor a log."""
        from .native import DuckError
        from .ppo import check_device_error
        n_periods = int(n_periods)
        if self.following():
            done, T = self.periods_done - self.log_base, int(self.log.shape[1])
            if done + n_periods > T:
                raise DuckError(f"the log holds {T} periods and {done} are followed: {n_periods} more would pass its end")
        elif self._policy_args is None:
            raise DuckError("no policy is loaded and no log is set: nothing to run (set_log)")
        rec = torch.empty(n_periods, self.num_robots, self.obs_size, device=self.device) if record else None
        self.calls += 1
        self.periods_done += n_periods
        chunk = max(1, int(self.CHUNK))
        if record or self.calls == 1 or n_periods < chunk:
            self._periods(n_periods, rec)
        else:
            if self.graph is None or self.graph[1] != chunk:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):   # one capture stream: a linear graph
                    self._periods(chunk)
                # (capturing records the launches without running them)
                self.graph = (g, chunk)
            for _ in range(n_periods // chunk):
                self.graph[0].replay()
            self._periods(n_periods % chunk)
        torch.cuda.synchronize(self.device)
        check_device_error(self.env, "fleet run")   # a replayed graph never re-enters duck_physics_step's entry check
        return rec.cpu().numpy() if record else None

    # --- host interface -----------------------------------------------------------------------
    def ctl_field(self, name: str) -> torch.Tensor:
        """A view [N, width] of one field of the control record (``ctl_fields``)."""
        o, w = self.fields[name]
        return self.ctl[:, o:o + w]

    def tile_over_policies(self, a) -> np.ndarray:
        """An [S, ...] per-robot table of one segment repeated for every policy, [K S, ...] (``tile_over_policies``,
        the module's function): robot j of every segment gets row j. Needs equal segments of S robots."""
        from .native import DuckError
        sizes = np.diff(self.policy_seg)
        if len(set(sizes.tolist())) > 1:
            raise DuckError(f"a table is tiled over equal segments, got {sizes.tolist()} robots")
        a = np.asarray(a)
        if a.ndim < 1 or a.shape[0] != int(sizes[0]):
            raise DuckError(f"a per-robot table of a segment is [{int(sizes[0])}, ...], got {tuple(a.shape)}")
        return tile_over_policies(a, self.num_policies)

    def set_commands(self, cmd) -> None:
        """``cmd`` [7] for every robot, or [N][7]."""
        from .native import DuckError
        c = torch.as_tensor(np.asarray(cmd, dtype=np.float32), device=self.device)
        if c.shape not in ((7,), (self.num_robots, 7)):
            raise DuckError(f"commands must be [7] or [{self.num_robots}][7], got {tuple(c.shape)}")
        self.ctl_field("command").copy_(c.expand(self.num_robots, 7))

    # --- disturbances (include/duck_fleet.h duck_fleet_disturb) -------------------------------------
    def _schedule_command(self) -> None:
        """``ctl.command`` = the schedule's segment of the current tick (segment 0 after ``restart``)."""
        if self.sched is None:
            return
        seg = torch.clamp(self.tick.long() // int(self.dis.seg_periods), max=int(self.dis.n_seg) - 1)
        self.ctl_field("command").copy_(self.sched[self.sched_id.long(), seg])

    def set_command_schedule(self, table, ids=None, seg_periods: int = 1) -> None:
        """Commands that change while the robots walk (the reference loop is driven from a keyboard,
        mujoco_infer.py:105-154; the training env resamples every 500 steps, joystick.py:449-477).
        ``table`` [S][K][7]: S schedules of K segments; robot r follows schedule ``ids[r]`` ([N], default
        r mod S), one segment per ``seg_periods`` control periods, the last one held. The command of the
        period now due is written at once. ``table=None`` turns the schedule off (the commands stay)."""
        from .native import DuckError
        n = self.num_robots
        if table is None:
            if self.sched is not None:
                self.sched = self.sched_id = None
                self.graph = None
            return
        if self.log is not None:
            raise DuckError("a log is being followed and writes the command itself: set_log(None) before a schedule")
        tab = np.asarray(table, dtype=np.float32)
        if tab.ndim != 3 or tab.shape[0] < 1 or tab.shape[1] < 1 or tab.shape[2] != 7:
            raise DuckError(f"a command schedule is [S][K][7] with S, K >= 1, got {tuple(tab.shape)}")
        if not np.isfinite(tab).all():
            raise DuckError("a command schedule must be finite")
        idv = np.arange(n) % tab.shape[0] if ids is None else np.asarray(ids)
        if idv.shape != (n,) or not np.issubdtype(idv.dtype, np.integer):
            raise DuckError(f"schedule ids must be [{n}] integers, got {idv.dtype} {tuple(idv.shape)}")
        if idv.min() < 0 or idv.max() >= tab.shape[0]:
            raise DuckError(f"schedule ids must lie in [0, {tab.shape[0]}), got [{idv.min()}, {idv.max()}]")
        if int(seg_periods) != seg_periods or int(seg_periods) < 1 or int(seg_periods) >= 2 ** 31:
            raise DuckError(f"seg_periods must be an integer >= 1, got {seg_periods!r}")
        shape = (int(self.dis.n_sched), int(self.dis.n_seg), int(self.dis.seg_periods))
        new = tab.shape[:2] + (int(seg_periods),)
        if self.sched is None or shape != new:     # new buffers, or a value the captured launch took by value
            self.sched = torch.empty(tab.shape, dtype=torch.float32, device=self.device)
            self.sched_id = torch.empty(n, dtype=torch.int32, device=self.device)
            self.dis.n_sched, self.dis.n_seg, self.dis.seg_periods = new
            self.graph = None
        self.sched.copy_(torch.as_tensor(tab))
        self.sched_id.copy_(torch.as_tensor(idv.astype(np.int32)))
        self._schedule_command()

    def set_pushes(self, first=None, interval=0, magnitude=0.0, theta=0.0) -> None:
        """Pushes of the base (joystick.py:381-400): at the start of period ``first`` (>= 1; 0: never) and,
        with ``interval`` > 0, every ``interval`` periods after it, the base's linear velocity gains
        magnitude * (cos theta, sin theta) in the world frame, just before that period's physics.
        ``first`` and ``interval`` are a scalar or [N] of integers; ``magnitude`` (m/s) and ``theta`` (rad)
        are a scalar, an [N] list or array, or a tuple ``(lo, hi)`` of such, drawn uniformly per push from
        the disturbance stream (``set_noise``'s seed). ``first=None`` turns pushes off."""
        from .native import FLEET_PUSH_SIZE, DuckError
        n = self.num_robots
        if first is None:
            if self.push is not None:
                self.push = None
                self.graph = None
            return
        if self.model.nv < 2:
            raise DuckError("a push needs a base with at least two velocity rows")
        row = np.zeros((n, FLEET_PUSH_SIZE), dtype=np.float32)

        def column(name, v):
            a = np.asarray(v, dtype=np.float64)
            if a.shape not in ((), (n,)):
                raise DuckError(f"{name} must be a scalar or [{n}], got {tuple(a.shape)}")
            if not np.isfinite(a).all():
                raise DuckError(f"{name} must be finite")
            return np.broadcast_to(a, (n,))
        for k, (name, v) in enumerate((("first", first), ("interval", interval))):
            a = column(name, v)
            if (a != np.floor(a)).any() or (a < 0).any() or (a >= 2 ** 24).any():
                raise DuckError(f"{name} must be integers in [0, 2^24)")
            row[:, k] = a
        for k, (name, v) in enumerate((("magnitude", magnitude), ("theta", theta))):
            lo, hi = v if isinstance(v, tuple) else (v, v)
            if isinstance(v, tuple) and len(v) != 2:
                raise DuckError(f"{name} as a tuple is (lo, hi), got {len(v)} values")
            row[:, 2 + 2 * k], row[:, 3 + 2 * k] = column(name, lo), column(name, hi)
        if self.push is None:
            self.push = torch.empty(n, FLEET_PUSH_SIZE, dtype=torch.float32, device=self.device)
            self.graph = None
        self.push.copy_(torch.as_tensor(row))

    def default_noise_scales(self) -> np.ndarray:
        """The training env's noise scales per obs column (config.default_config().noise_config, joystick.py:
        492-558): gyro, accelerometer, the bug-compatible config.qpos_noise_scale on the joint angles and
        joint_vel * dof_vel_scale on the joint velocities; every other column 0."""
        return default_noise_scales(self.num_dofs, float(self.desc.dof_vel_scale))

    def set_noise(self, level: float = 0.0, seed: int = 0, scales=None) -> None:
        """Sensor noise on the observation the policy sees: column k gains U[-1, 1) * level * scales[k], drawn
        per robot and period from the stream of ``seed`` (which also draws the random pushes). ``scales``
        [obs_size] defaults to ``default_noise_scales()``. The training env adds the noise to the raw joint
        velocity and scales by dof_vel_scale afterwards; here it is added to the scaled column, with the scale
        multiplied in. duck_fleet_observe's bookkeeping has run on the true sensors. The noise is added after an
        IMU or encoder delay (``set_latency``). ``level=0`` turns the noise off."""
        from .native import DuckError
        sc = self.default_noise_scales() if scales is None else np.asarray(scales, dtype=np.float64)
        if sc.shape != (self.obs_size,):
            raise DuckError(f"noise scales must be [{self.obs_size}], got {tuple(sc.shape)}")
        if not np.isfinite(level) or not np.isfinite(sc).all():
            raise DuckError("the noise level and scales must be finite")
        eff = (float(level) * sc).astype(np.float32)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        old = np.array(self.dis.noise_scale[:self.obs_size], dtype=np.float32)
        if seed != int(self.dis.seed) or old.tobytes() != eff.tobytes():   # taken by value by a captured launch
            self.graph = None
        self.dis.seed = seed
        for k in range(self.obs_size):
            self.dis.noise_scale[k] = float(eff[k])

    # --- latency (include/duck_fleet.h duck_fleet_sense_delay, duck_fleet_actuate_delayed) ----------------
    def set_latency(self, action=0, sense=0, seed: int = 0, encoder=0) -> None:
        """Latency in whole control periods (20 ms each): ``action`` delays the action that forms the motor targets
        (the training env's action delay, joystick.py:361-376), ``sense`` the gyro and accelerometer columns of the
        observation (its IMU delay, joystick.py:521-530), ``encoder`` the joint-position and joint-velocity columns
        (the robot's bus servos, read back one after another over a serial line; one delay for both groups; the
        training env has no such delay). Each is a scalar, an [N] list or array of integers, or a
        tuple ``(lo, hi)`` of such: drawn per robot and period, uniformly over lo..hi with both ends included, from
        the stream of ``seed`` (the latency's own; the training env's randint excludes its upper end: its default
        0..3 is ``(0, 2)`` here). Values lie in [0, 2]. The action history the policy sees stays undelayed, the
        bookkeeping runs on the true sensors, the noise is added after the delay. With an encoder delay
        duck_fleet_sensor_delay takes duck_fleet_sense_delay's place. ``set_latency(None)``, or all zeros, turns the
        latency off. A latency starts anew when set: its period count ``lat_tick`` at 0, the delay lines empty
        (``lat_base`` = the periods run since ``restart()``)."""
        from .native import DuckError
        self.graph = None
        rows, enc = latency_rows(self.num_robots, action, sense, encoder)
        if int(seed) != seed:
            raise DuckError(f"the latency seed must be an integer, got {seed!r}")
        if not rows.any() and not enc.any():
            self.lat = self.lat_tick = self.line = self.enc = self.eline = None
            self.lat_seed, self.lat_sense, self.lat_encoder = 0, False, False
            return
        self._load_latency(rows, seed, enc)

    def _load_latency(self, rows: np.ndarray, seed: int, enc: Optional[np.ndarray] = None) -> None:
        """The latency table ``rows`` [N][4] as it is (all zeros included): new buffers, the count at 0. ``enc``
        [N][2], the encoder table beside it; without one, or with no ``enc_hi`` above 0, the loop is the one without
        an encoder delay."""
        from .native import FLEET_MAX_DELAY
        n = self.num_robots
        self.graph = None
        self.lat = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
        self.lat_tick = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.line = torch.zeros(n, FLEET_MAX_DELAY + 1, 6, dtype=torch.float32, device=self.device)
        self.lat_seed, self.lat_base = int(seed) & 0xFFFFFFFFFFFFFFFF, self.periods_done
        self.lat_sense = bool((np.asarray(rows)[:, 3] > 0).any())
        self.enc = self.eline = None
        self.lat_encoder = enc is not None and bool((np.asarray(enc)[:, 1] > 0).any())
        if self.lat_encoder:
            self.enc = torch.as_tensor(np.ascontiguousarray(enc, dtype=np.int32)).to(self.device)
            self.eline = torch.zeros(n, FLEET_MAX_DELAY + 1, 2 * self.num_dofs, dtype=torch.float32, device=self.device)

    # --- following a log (include/duck_fleet.h duck_fleet_follow) ---------------------------------------
    def set_log(self, log, ids=None) -> None:
        """Follow a recorded robot log instead of the policy: ``log`` [T][W] or [L][T][W] float32, W =
        DUCK_FLEET_LOG_SIZE(nu), row p the observation the logged robot's policy saw in period p and then the
        action it answered with (``log_from_saved_obs``, ``load_log``); robot r follows log ``ids[r]`` ([N],
        default r mod L). From now on ``act()`` enqueues duck_fleet_follow where it enqueued duck_policy_act: the
        robots are fed the log's actions and commands, and ``score`` [N][obs] sums, per robot and column, the
        squared distance of the simulated observation from the logged one (a NaN log word is a missing sample).
        A robot's IMU delay, encoder delay and sensor noise are in what is scored, its action delay acts on the fed
        action.
        The log starts anew when set: ``log_tick`` and ``score`` zeroed, row 0's command written
        (``log_base`` = the periods run since ``restart()``). The loop's start state is its own: a log that starts
        elsewhere is the caller's to load with ``load_state``. A log rewritten with the same shape keeps the
        captured graph. A command schedule and a log both write the command: setting both raises. ``log=None``
        turns the mode off (the commands stay)."""
        n = self.num_robots
        if log is None:
            if self.log is not None:
                self.log = self.log_id = self.log_tick = self.score = None
                self.graph = None
            return
        tab, idv = log_arguments(log, ids, n, self.num_dofs, scheduled=self.sched is not None)
        if self.log is None or tuple(self.log.shape) != tab.shape:    # new buffers, or sizes the captured launch took by value
            self.log = torch.empty(tab.shape, dtype=torch.float32, device=self.device)
            self.log_id = torch.empty(n, dtype=torch.int32, device=self.device)
            self.log_tick = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.score = torch.zeros(n, self.obs_size, dtype=torch.float32, device=self.device)
            self.graph = None
        self.log.copy_(torch.as_tensor(tab))
        self.log_id.copy_(torch.as_tensor(idv))
        self.log_tick.zero_()
        self.score.zero_()
        self.log_base = self.periods_done
        self._log_command()

    def _log_command(self) -> None:
        """``ctl.command`` = columns 6-12 of the log's row of the current log_tick (row 0 after ``set_log``)."""
        row = torch.clamp(self.log_tick.long(), min=0, max=int(self.log.shape[1]) - 1)
        self.ctl_field("command").copy_(self.log[self.log_id.long(), row, 6:13])

    def scores(self) -> np.ndarray:
        """``score`` [N][obs] float32: per robot and obs column, the sum over the periods followed of the squared
        difference between the simulated and the logged observation."""
        from .native import DuckError
        if self.log is None:
            raise DuckError("no log is set (set_log)")
        torch.cuda.synchronize(self.device)
        return self.score.cpu().numpy()

    def score_report(self, weights=None) -> Dict[str, np.ndarray]:
        """Per robot, the rms distance from its log per column group (``score_groups``: gyro, accelerometer,
        joint_position, joint_velocity, action_history, motor_targets, contacts, phase), ``"total"``, the sum of
        weight x rms over the groups (``weights``: {group: weight}, default 1 on the four sensor groups, 0 on the
        rest), and ``"periods"``, the rows followed. A group's count is the log's own non-NaN words in its columns
        over the rows followed (``score_report``, the module's function). The action-history and motor-target
        groups are checks of the feeding, not of the model: they compare what the loop fed with what the log says
        was fed, and are 0 unless the log is inconsistent with itself or an action delay moved the targets."""
        score = self.scores()
        return score_report(score, self.log.cpu().numpy(), self.log_id.cpu().numpy(), self.log_tick.cpu().numpy(), weights)

    def save_log(self, path: str) -> None:
        """The log being followed to ``path`` (``save_log``, the module's function)."""
        from .native import DuckError
        if self.log is None:
            raise DuckError("no log is set (set_log)")
        save_log(path, self.log.cpu().numpy())

    @staticmethod
    def load_log(path: str) -> np.ndarray:
        """A log from ``path`` (``load_log``, the module's function), for ``set_log``."""
        return load_log(path)

    # --- gait and servo load (include/duck_fleet.h duck_fleet_gait) ---------------------------------------
    def set_gait(self, on: bool = True, force_frac: float = 0.9, speed_frac: float = 1.0) -> None:
        """Keep the gait record: from now on a period enqueues duck_fleet_gait after the actuation. A period counts
        as force-saturated for an actuator at ``force_frac`` of its force limit and above, as speed-saturated at
        ``speed_frac`` of the reference loop's max_motor_velocity (5.24 rad/s) and above (``gait_desc``). A new
        record of zeros, [N][DUCK_FLEET_GAIT_SIZE(nu)] float32 on the device; it equals ``acc`` in its periods
        when set right after ``restart()`` or ``reset_report()``, which zero both. ``on=False`` turns it off.
        Switching it drops the captured graph."""
        self.graph = None
        if not on:
            self.gait_desc = self.gait_rec = None
            return
        self.gait_desc = gait_desc(self.model, force_frac, speed_frac)
        width = HEADERS.value(f"DUCK_FLEET_GAIT_SIZE({self.num_dofs})")
        self.gait_rec = torch.zeros(self.num_robots, width, dtype=torch.float32, device=self.device)

    def gait_records(self) -> np.ndarray:
        """The raw gait record [N][DUCK_FLEET_GAIT_SIZE(nu)] float32 (``gait_fields``; ``gait_report`` reads it)."""
        from .native import DuckError
        if self.gait_rec is None:
            raise DuckError("no gait record is kept (set_gait)")
        torch.cuda.synchronize(self.device)
        return self.gait_rec.cpu().numpy()

    # --- the flight recorder (include/duck_fleet.h duck_fleet_record) ----------------------------------
    def set_recorder(self, depth: Optional[int], post: int = 0) -> None:
        """Keep every robot's last ``depth`` control periods on the device, frozen ``post`` periods after the
        one in which the robot fell (0: the ring ends at the fall frame). A new, empty ring: the frame written
        by the j-th period run from now on is period ``rec_base + j``, with ``rec_base`` the periods run since
        ``restart()``. ``depth=None`` turns the recorder off. [N][depth][F] float32 on the device (232 MB
        for 4,096 robots of the shipped model at depth 50)."""
        from .native import DuckError
        self.graph = None
        if depth is None:
            self.ring = self.rec_head = self.rec_after = None
            self.rec_depth = self.rec_post = 0
            return
        if int(depth) != depth or int(depth) < 1 or int(post) != post or int(post) < 0 or max(depth, post) >= 2 ** 31 - 1:
            raise DuckError(f"a recorder needs integers depth >= 1 and post >= 0, got {depth!r}, {post!r}")
        n, F = self.num_robots, sum(w for _, w in self.frame_fields.values())
        self.rec_depth, self.rec_post, self.rec_base = int(depth), int(post), self.periods_done
        self.ring = torch.zeros(n, self.rec_depth, F, dtype=torch.float32, device=self.device)
        self.rec_head = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.rec_after = torch.zeros(n, dtype=torch.int32, device=self.device)

    def _frames(self, robot: int) -> Tuple[np.ndarray, np.ndarray]:
        from .native import DuckError
        if self.ring is None:
            raise DuckError("no recorder is set (set_recorder)")
        if not 0 <= int(robot) < self.num_robots:
            raise DuckError(f"robot must lie in [0, {self.num_robots}), got {robot!r}")
        torch.cuda.synchronize(self.device)
        return unroll_ring(self.ring[int(robot)].cpu().numpy(), int(self.rec_head[int(robot)]), self.rec_depth, self.rec_base)

    def recorded(self, robot: int) -> Dict[str, np.ndarray]:
        """Robot ``robot``'s recorded frames, oldest first: ``"period"`` [T] (1-based, counted from
        ``restart()``), every field of ``frame_fields`` by name as [T][width] float32, and ``"fell"``. A robot
        that fell holds the periods up to the one in which it fell and ``post`` more; one that did not, the
        last ``depth``."""
        frames, period = self._frames(robot)
        out = {"period": period, "fell": bool(self.alive[int(robot)] == 0)}
        for name, (o, w) in self.frame_fields.items():
            out[name] = np.ascontiguousarray(frames[:, o:o + w])
        return out

    def replay(self, robot: int, frame: int = 0) -> "FleetInfer":
        """A one-robot fleet that continues robot ``robot`` from its recorded frame ``frame`` (an index into
        ``recorded(robot)``; negative from the newest): the same model, policy, ``standing`` flag and noise,
        the robot's randomisation record, schedule, push row and latency row, and its global id in the disturbance
        and latency streams. With an IMU delay the delay line is rebuilt from the raw sensors of the frame and of
        the one before it, with an encoder delay the encoder line from their ``qpos`` and ``qvel``; a robot whose
        IMU or encoder delay reaches 2 cannot be replayed from the oldest frame it holds.
        Of a following fleet the replay carries the robot's log and ``log_tick`` at the frame's period (its scores
        start at zero). The replay keeps no gait record (``gaited()`` False): a frame does not carry the gait state.
        The loop is a pure function of what a frame holds, that record and that stream, so running the replay
        k periods reproduces the k periods the robot ran after that frame, bit for bit. The fleet's settings
        are taken as they are now: they must not have changed since the frame was written."""
        from .native import DuckError
        frames, period = self._frames(robot)
        if not -len(frames) <= int(frame) < len(frames):
            raise DuckError(f"robot {robot} holds {len(frames)} frames, got frame {frame!r}")
        robot = int(robot)
        f, p = torch.tensor(frames[int(frame)], device=self.device), int(period[int(frame)])
        follow = None
        if self.following():   # the robot's own log (before the frame: set_log writes a command)
            follow = (self.log[int(self.log_id[robot])].cpu().numpy(), None)
        made = dict(self._made_from)
        if self._multi_args is not None:   # the robot's own policy file, through duck_policy_act: the same bits
            made["onnx_model_path"] = made["onnx_model_path"][int(self.policy_of[robot])]
        r = FleetInfer(num_robots=1, randomize=None if self.dr is None else 0,
                       robot_offset=self.robot_offset + robot, follow=follow, **made)
        if self.dr is not None:
            r.dr.copy_(self.dr.view(-1, self.num_robots)[:, robot])
        # the disturbances first, the frame last: set_command_schedule writes a command
        r.set_noise(1.0, int(self.dis.seed), np.array(self.dis.noise_scale[:self.obs_size], dtype=np.float64))
        if self.sched is not None:
            r.set_command_schedule(self.sched.cpu().numpy(), [int(self.sched_id[robot])], int(self.dis.seg_periods))
        if self.push is not None:
            r.set_pushes(0)
            r.push.copy_(self.push[robot:robot + 1])
        part = lambda name: f[self.frame_fields[name][0]:][:self.frame_fields[name][1]]  # noqa: E731
        for dst, name in ((r.qpos, "qpos"), (r.qvel, "qvel"), (r.warm, "qacc_warmstart")):
            dst[:, 0].copy_(part(name))
        r.ctl[0].copy_(part("ctl"))
        r.ctrl[:, 0].copy_(r.ctl_field("motor_targets")[0])
        if self.disturbed():   # the device's period count at that frame: it has advanced once per period since
            r.tick.copy_(self.tick[robot:robot + 1] - (self.periods_done - p))
        if self.following():   # log_tick once the frame's period was done, as tick; the scores start at zero
            after = int(self.log_tick[robot]) - (self.periods_done - p)
            if p < self.log_base:
                raise DuckError(f"frame {frame!r} of robot {robot} was written before the log was set")
            r.log_tick.fill_(after)
            r.log_base = p - after
        if self.latent():
            row = self.lat[robot:robot + 1].cpu().numpy()
            enc = None if self.enc is None else self.enc[robot:robot + 1].cpu().numpy()
            r._load_latency(row, self.lat_seed, enc)
            after = int(self.lat_tick[robot]) - (self.periods_done - p)   # lat_tick once the frame's period was done
            if after < 0:
                raise DuckError(f"frame {frame!r} of robot {robot} was written before the latency was set")
            r.lat_tick.fill_(after)
            r.lat_base = p - after
            q = after - 1                     # ... and in the period that wrote the frame
            o, _ = self.frame_fields["sensors"]
            k = int(frame) % len(frames)

            def sample(fr):   # obs columns 0-5 as duck_fleet_observe wrote them, from a frame's raw sensors
                w = np.array(fr[o:o + 6], dtype=np.float32)
                w[3] = w[3] + np.float32(self.desc.accel_x_offset)
                return torch.tensor(w, device=self.device)
            if q >= 0:
                r.line[0, q % 3].copy_(sample(frames[k]))
            if q >= 1 and int(row[0, 3]) == 2:
                if k == 0:
                    raise DuckError(f"robot {robot}'s IMU delay reaches 2 periods back and the frame before frame "
                                    f"{frame!r} is not held: replay from a later frame")
                r.line[0, (q - 1) % 3].copy_(sample(frames[k - 1]))
            if r.lat_encoder:     # the encoder line by the same rule, from the frames' qpos and qvel
                nu, d = self.num_dofs, self.desc
                if self.push is not None and min(d.act_dof[:nu]) < 2:
                    raise DuckError("an actuated joint's velocity is qvel[0] or qvel[1], where a frame holds the next "
                                    "period's push: the encoder line cannot be rebuilt from the frames")
                oq, ov = self.frame_fields["qpos"][0], self.frame_fields["qvel"][0]

                def joints(fr):   # obs columns 13 .. 13 + 2 nu - 1 as duck_fleet_observe wrote them
                    fr = np.asarray(fr, dtype=np.float32)
                    pos = fr[oq + np.array(d.act_qpos[:nu])] - np.array(d.act_default[:nu], dtype=np.float32)
                    vel = np.float32(d.dof_vel_scale) * fr[ov + np.array(d.act_dof[:nu])]
                    return torch.tensor(np.concatenate([pos, vel]).astype(np.float32), device=self.device)
                if q >= 0:
                    r.eline[0, q % 3].copy_(joints(frames[k]))
                if q >= 1 and int(enc[0, 1]) == 2:
                    if k == 0:
                        raise DuckError(f"robot {robot}'s encoder delay reaches 2 periods back and the frame before "
                                        f"frame {frame!r} is not held: replay from a later frame")
                    r.eline[0, (q - 1) % 3].copy_(joints(frames[k - 1]))
        r.periods_done = p
        return r

    def state(self):
        """(qpos [N][nq], qvel [N][nv], ctrl [N][nu]) as numpy float32."""
        return tuple(t.t().contiguous().cpu().numpy() for t in (self.qpos, self.qvel, self.ctrl))

    def load_state(self, qpos=None, qvel=None, ctrl=None, qacc_warmstart=None, **ctl) -> None:
        """Overwrite physics state ([k] for every robot or [N][k]) and control-record fields by name."""
        def put(dst, a):   # dst [N, k] view
            a = torch.as_tensor(np.asarray(a, dtype=np.float32), device=self.device).reshape(-1, dst.shape[1])
            dst.copy_(a.expand(dst.shape[0], -1))
        for t, a in ((self.qpos, qpos), (self.qvel, qvel), (self.ctrl, ctrl), (self.warm, qacc_warmstart)):
            if a is not None:
                put(t.t(), a)
        for name, a in ctl.items():
            put(self.ctl_field(name), a)

    def reset_report(self) -> None:
        self.acc.zero_()
        self.alive.fill_(1.0)
        if self.gait_rec is not None:
            self.gait_rec.zero_()

    def report(self) -> Dict[str, np.ndarray]:
        """Per robot: periods survived, fell, mean vx / vy / wz while alive, rms linear and yaw tracking
        error while alive (NaN for a robot that survived no period)."""
        acc = self.acc.cpu().numpy().astype(np.float64)
        alive = self.alive.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = acc[:, 1:] / acc[:, :1]
        return {"periods": acc[:, 0], "fell": alive == 0, "mean_vx": mean[:, 0], "mean_vy": mean[:, 1],
                "mean_wz": mean[:, 2], "rms_lin_err": np.sqrt(mean[:, 3]), "rms_yaw_err": np.sqrt(mean[:, 4])}


def command_grid(spec: str) -> np.ndarray:
    """``NXxNYxNT`` -> the [NX * NY * NT][7] commands over the reference's COMMANDS_RANGE_X / Y / THETA
    (both ends included; a single point is the range's middle)."""
    try:
        nx, ny, nt = (int(v) for v in spec.lower().split("x"))
        assert min(nx, ny, nt) >= 1
    except Exception:
        raise ValueError(f"--command_grid wants NXxNYxNT with positive integers, got {spec!r}") from None
    axis = lambda r, k: np.linspace(r[0], r[1], k) if k > 1 else np.array([0.5 * (r[0] + r[1])])  # noqa: E731
    cells = [(x, y, t) for x in axis(COMMANDS_RANGE_X, nx) for y in axis(COMMANDS_RANGE_Y, ny)
             for t in axis(COMMANDS_RANGE_THETA, nt)]
    out = np.zeros((len(cells), 7), dtype=np.float32)
    out[:, :3] = cells
    return out


def grid_report(rep: Dict[str, np.ndarray], acc: np.ndarray, cells: np.ndarray, n_periods: int, cell=None) -> list:
    """Per command cell (robot r belongs to cell r mod the number of cells, or to ``cell[r]`` when the [N] ids are
    given: a fleet of several policies tiles one segment's cells): the count, the share that never fell, the mean
    tracked velocity and the rms errors over the cell's surviving periods."""
    out = []
    cell = np.arange(len(acc)) % len(cells) if cell is None else np.asarray(cell)
    for c in range(len(cells)):
        a = acc[cell == c].astype(np.float64)
        tot = a.sum(0)
        stat = (lambda v: float(v / tot[0])) if tot[0] > 0 else (lambda v: None)
        out.append({"command": [float(v) for v in cells[c][:3]], "count": int(len(a)),
                    "survival_rate": float(np.mean(~np.asarray(rep["fell"])[cell == c])) if len(a) else None,
                    "mean_periods": float(a[:, 0].mean()) if len(a) else None, "periods": int(n_periods),
                    "mean_vx": stat(tot[1]), "mean_vy": stat(tot[2]), "mean_wz": stat(tot[3]),
                    "rms_lin_err": None if stat(tot[4]) is None else float(np.sqrt(stat(tot[4]))),
                    "rms_yaw_err": None if stat(tot[5]) is None else float(np.sqrt(stat(tot[5])))})
    return out


def _gait_nu(width: int) -> int:
    """nu of a gait record ``width`` = DUCK_FLEET_GAIT_SIZE(nu) words wide."""
    from .native import FLEET_MAX_NU, DuckError
    for nu in range(1, FLEET_MAX_NU + 1):
        if HEADERS.value(f"DUCK_FLEET_GAIT_SIZE({nu})") == int(width):
            return nu
    raise DuckError(f"{width} words are no gait record (DUCK_FLEET_GAIT_SIZE(nu), nu <= {FLEET_MAX_NU})")


def _gait_stats(g: np.ndarray, distance: np.ndarray, weight: float, dt: float) -> Dict[str, np.ndarray]:
    """The statistics of gait records ``g`` [R][G] float64 whose robots covered ``distance`` [R] metres and weigh
    ``weight`` newtons: what ``gait_report`` returns. A zero denominator gives NaN."""
    F = gait_fields(_gait_nu(g.shape[1]))
    col = lambda name: g[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    feet = lambda name: np.concatenate([col(f"{foot}_{name}") for foot in GAIT_FEET], 1)  # noqa: E731

    def over(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b != 0)
        return out
    per = col("periods")
    some = per > 0
    contact, touchdowns = feet("contact"), feet("touchdowns")
    with np.errstate(invalid="ignore"):
        return {"periods": per[:, 0],
                "force_rms": np.sqrt(over(col("force_sq"), per)), "force_peak": np.where(some, col("force_max"), np.nan),
                "force_sat": over(col("force_sat"), per), "speed_peak": np.where(some, col("speed_max"), np.nan),
                "speed_sat": over(col("speed_sat"), per), "mean_power": over(col("work"), per),
                "action_rate_rms": np.sqrt(over(col("action_rate"), per)),
                "duty_factor": over(contact, per), "step_frequency": over(touchdowns, per * dt),
                "slip_rms": np.sqrt(over(feet("slip"), contact)), "clearance": over(feet("apex_sum"), touchdowns),
                "double_support": over(col("double_support"), per)[:, 0], "flight": over(col("flight"), per)[:, 0],
                "cost_of_transport": over(col("work").sum(1) * dt, weight * np.asarray(distance, dtype=np.float64))}


def _gait_weight(model) -> float:
    """M g of the nominal model, in newtons: its bodies' total mass times the norm of its gravity."""
    return float(np.sum(np.asarray(model.body_mass, dtype=np.float64)) *
                 np.linalg.norm(np.asarray(model.opt_gravity, dtype=np.float64)))


def gait_report(gait, acc, model, dt: float = 0.02) -> Dict[str, np.ndarray]:
    """Per robot, in float64, from the gait record ``gait`` [N][G] (``FleetInfer.gait_records()``), ``acc`` [N][6]
    and the compiled ``model`` (its total mass and gravity; the nominal one, whatever a robot's randomisation):
    per actuator [N][nu] ``force_rms`` and ``force_peak`` (the actuator's force unit, N m for the duck's joints),
    ``force_sat`` and ``speed_sat`` (the share of the periods at the limit), ``speed_peak`` (rad/s), ``mean_power``
    (mean |force x joint speed|, W) and ``action_rate_rms``; per foot [N][2] (left, right) ``duty_factor``,
    ``step_frequency`` (Hz: touchdowns / (periods dt)), ``slip_rms`` (m/s, over the contact periods) and
    ``clearance`` (m: the mean over the touchdowns of the swing's highest sample over the landing sample); per
    robot [N] ``periods``, ``double_support`` and ``flight`` (shares of the periods) and ``cost_of_transport`` =
    sum of work dt / (M g |(mean_vx, mean_vy)| periods dt). All of 50 Hz samples. A zero denominator gives NaN."""
    g, a = np.asarray(gait, dtype=np.float64), np.asarray(acc, dtype=np.float64)
    return _gait_stats(g, np.hypot(a[:, 1], a[:, 2]) * dt, _gait_weight(model), dt)


def gait_summary(gait, acc, rows, model, dt: float = 0.02) -> dict:
    """``gait_report`` of the robots ``rows`` (indices or a mask; None: all) pooled into one: sums of the sums, maxima
    of the maxima, the distance the sum of the robots' distances. A plain dict for a JSON report: ``"count"``,
    ``"actuators"`` (their names), ``"feet"``, and every statistic as a float or a list, None where ``gait_report``
    gives NaN."""
    g, a = np.asarray(gait, dtype=np.float64), np.asarray(acc, dtype=np.float64)
    if rows is not None:
        g, a = g[rows], a[rows]
    F = gait_fields(_gait_nu(g.shape[1]))
    pooled = g.sum(0, keepdims=True)
    for name in ("force_max", "speed_max"):
        o, w = F[name]
        pooled[0, o:o + w] = g[:, o:o + w].max(0) if len(g) else 0.0
    for foot in GAIT_FEET:      # the state words mean nothing once pooled
        pooled[0, F[f"{foot}_prev"][0]] = pooled[0, F[f"{foot}_apex"][0]] = 0.0
    stats = _gait_stats(pooled, [np.hypot(a[:, 1], a[:, 2]).sum() * dt], _gait_weight(model), dt)
    num = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    out = {"count": int(len(g)), "actuators": list(model.names["actuator"]), "feet": list(GAIT_FEET)}
    for key, v in stats.items():
        out[key] = num(v[0]) if np.ndim(v[0]) == 0 else [num(x) for x in v[0]]
    return out


def default_noise_scales(nu: int, dof_vel_scale: float = 0.05) -> np.ndarray:
    """float64 [17 + 6 nu]: the training env's noise scale of every obs column of the deployment loop
    (``FleetInfer.default_noise_scales``)."""
    from . import config
    cfg = config.default_config()
    sc = cfg.noise_config.scales
    out = np.zeros(fleet_obs_size(nu))
    out[0:3], out[3:6] = sc.gyro, sc.accelerometer
    out[13:13 + nu] = config.qpos_noise_scale(cfg, max(nu, len(constants.JOINTS_ORDER_NO_HEAD)))[:nu]
    out[13 + nu:13 + 2 * nu] = sc.joint_vel * dof_vel_scale
    return out


def push_grid(spec: str, magnitude_range=None) -> np.ndarray:
    """``NMxND`` -> the [NM * ND][2] (magnitude, theta) push cells: NM magnitudes over
    push_config.magnitude_range (both ends included; a single one is the middle) x ND directions over
    [0, 2 pi), the end excluded."""
    try:
        nm, nd = (int(v) for v in spec.lower().split("x"))
        assert min(nm, nd) >= 1
    except Exception:
        raise ValueError(f"--push_grid wants NMxND with positive integers, got {spec!r}") from None
    if magnitude_range is None:
        from . import config
        magnitude_range = config.default_config().push_config.magnitude_range
    lo, hi = (float(v) for v in magnitude_range)
    mags = np.linspace(lo, hi, nm) if nm > 1 else np.array([0.5 * (lo + hi)])
    return np.array([(m, 2.0 * np.pi * d / nd) for m in mags for d in range(nd)], dtype=np.float32)


def robot_cells(num_robots: int, n_command: int, n_push: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """Round-robin over command cell x push cell: robot r has command cell r mod n_command (as without
    pushes) and push cell (r div n_command) mod n_push."""
    r = np.arange(num_robots)
    return r % n_command, (r // n_command) % n_push


def resample_schedule(cells: np.ndarray, n_periods: int, every: int) -> np.ndarray:
    """[S][K][7]: schedule s starts at command cell s and steps to the next cell (wrapping) every ``every``
    periods, for as many segments as ``n_periods`` needs."""
    k = max(1, -(-int(n_periods) // int(every)))
    s = len(cells)
    return np.stack([cells[(c + np.arange(k)) % s] for c in range(s)]).astype(np.float32)


def push_report(rep: Dict[str, np.ndarray], push_cells: np.ndarray, first, interval, n_periods: int, window: int) -> list:
    """Per push cell (``push_cells`` [N], each robot's cell): the count, the share that never fell, and the
    share that fell within ``window`` periods after a push. A robot falls once: one that survived
    ``rep["periods"]`` = P periods fell in period P, and a push at the start of period t (t = first, first +
    interval, ... < n_periods; ``first``, ``interval`` scalars or [N]) is blamed when t <= P < t + window."""
    cell = np.asarray(push_cells)
    n = len(cell)
    first = np.broadcast_to(np.asarray(first, dtype=np.int64), (n,))
    interval = np.broadcast_to(np.asarray(interval, dtype=np.int64), (n,))
    P, fell = np.asarray(rep["periods"]).astype(np.int64), np.asarray(rep["fell"], dtype=bool)
    since = P - first                      # periods between the first push and the fall
    last = np.where(interval > 0, since % np.maximum(interval, 1), since)   # ... and the latest push before it
    pushed = (first >= 1) & (first < n_periods) & (since >= 0)
    after = fell & pushed & (last < window)
    out = []
    for c in range(int(cell.max()) + 1 if n else 0):
        m = cell == c
        k = int(m.sum())
        out.append({"cell": c, "count": k, "survival_rate": float(np.mean(~fell[m])) if k else None,
                    "fell_after_push_rate": float(np.mean(after[m])) if k else None, "window": int(window)})
    return out


def add_disturbance_arguments(p) -> None:
    p.add_argument("--push_grid", type=str, default=None, metavar="NMxND",
                   help="NM push magnitudes over push_config.magnitude_range x ND directions over [0, 2 pi)")
    p.add_argument("--push_magnitude", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="the push grid's magnitude range in m/s (default: push_config.magnitude_range)")
    p.add_argument("--push_at", type=int, default=100, metavar="PERIOD", help="the first push (>= 1)")
    p.add_argument("--push_every", type=int, default=0, metavar="PERIODS", help="repeat the push (0 = once)")
    p.add_argument("--recovery_window", type=int, default=100, metavar="PERIODS",
                   help="a fall within this many periods after a push counts against the push")
    p.add_argument("--noise", type=float, default=0.0, metavar="LEVEL",
                   help="sensor noise at LEVEL x the training env's scales (1 = as trained)")
    p.add_argument("--noise_seed", type=int, default=0, metavar="SEED")
    p.add_argument("--resample_commands", type=int, default=0, metavar="PERIODS",
                   help="step every robot through the command grid's cells every PERIODS periods")


def disturbance_plan(args, cells: np.ndarray):
    """The setters' arguments for the command line's disturbance flags, or None when none is given:
    {"schedule": (table, ids, seg_periods) | None, "pushes": (first, interval, magnitude [N], theta [N]) | None,
    "push_cells" [P][2], "push_cell" [N], "echo": the settings for the report}."""
    if args.push_grid is None and not args.noise and not args.resample_commands:
        return None
    if args.resample_commands < 0 or args.push_every < 0 or args.recovery_window < 0:
        raise ValueError("--resample_commands, --push_every and --recovery_window must be >= 0")
    n = args.num_robots
    plan = {"schedule": None, "pushes": None, "push_cells": None, "push_cell": None}
    echo = {"push_grid": args.push_grid, "noise": args.noise, "noise_seed": args.noise_seed,
            "resample_commands": args.resample_commands}
    magnitude = getattr(args, "push_magnitude", None)
    if magnitude is not None and not (np.isfinite(magnitude).all() and 0 <= magnitude[0] <= magnitude[1]):
        raise ValueError("--push_magnitude wants finite 0 <= LO <= HI")
    pcells = push_grid(args.push_grid, magnitude) if args.push_grid is not None else np.zeros((1, 2), np.float32)
    ccell, pcell = robot_cells(n, len(cells), len(pcells))
    if args.push_grid is not None:
        if args.push_at < 1:
            raise ValueError("--push_at must be >= 1 (the first period cannot be pushed)")
        plan["pushes"] = (args.push_at, args.push_every, pcells[pcell, 0], pcells[pcell, 1])
        plan["push_cells"], plan["push_cell"] = pcells, pcell
        echo.update(push_at=args.push_at, push_every=args.push_every, recovery_window=args.recovery_window)
        if magnitude is not None:
            echo["push_magnitude"] = [float(v) for v in magnitude]
    if args.resample_commands:
        plan["schedule"] = (resample_schedule(cells, args.periods, args.resample_commands), ccell.astype(np.int32),
                            args.resample_commands)
    plan["echo"] = echo
    return plan


PERIOD_MS = 20.0   # one control period: sim_dt * decimation = 0.002 s * 10


def latency_rows(n: int, action=0, sense=0, encoder=0) -> Tuple[np.ndarray, np.ndarray]:
    """``FleetInfer.set_latency``'s arguments for ``n`` robots as the device's tables: (``lat`` [n][4] int32 =
    {act_lo, act_hi, sense_lo, sense_hi}, ``enc`` [n][2] int32 = {enc_lo, enc_hi}). Each argument is a scalar, [n],
    or a tuple (lo, hi) of such, whole periods in [0, DUCK_FLEET_MAX_DELAY]; DuckError otherwise. ``action=None``
    is all zeros."""
    from .native import FLEET_ENC_SIZE, FLEET_LAT_SIZE, FLEET_MAX_DELAY, DuckError
    both = np.zeros((n, FLEET_LAT_SIZE + FLEET_ENC_SIZE), dtype=np.int32)
    if action is not None:
        for k, (name, v) in enumerate((("action", action), ("sense", sense), ("encoder", encoder))):
            if isinstance(v, tuple) and len(v) != 2:
                raise DuckError(f"{name} as a tuple is (lo, hi), got {len(v)} values")
            for j, (end, w) in enumerate(zip(("lo", "hi"), v if isinstance(v, tuple) else (v, v))):
                try:
                    a = np.asarray(w, dtype=np.float64)
                except (TypeError, ValueError):
                    raise DuckError(f"{name} must be integers, got {w!r}") from None
                if a.shape not in ((), (n,)):
                    raise DuckError(f"{name} must be a scalar or [{n}], got {tuple(a.shape)}")
                if not np.isfinite(a).all() or (a != np.floor(a)).any():
                    raise DuckError(f"{name} must be integers (whole control periods)")
                if (a < 0).any() or (a > FLEET_MAX_DELAY).any():
                    raise DuckError(f"{name} must lie in [0, {FLEET_MAX_DELAY}] control periods")
                both[:, 2 * k + j] = a
            if (both[:, 2 * k] > both[:, 2 * k + 1]).any():
                raise DuckError(f"{name} as (lo, hi) needs lo <= hi")
    return np.ascontiguousarray(both[:, :FLEET_LAT_SIZE]), np.ascontiguousarray(both[:, FLEET_LAT_SIZE:])


def delay_grid(spec: str, encoder: bool = False) -> np.ndarray:
    """``NAxNS`` -> the [NA * NS][2] (action delay, sense delay) cells in control periods: a in range(NA), s in
    range(NS), 1 <= NA, NS <= DUCK_FLEET_MAX_DELAY + 1. With ``encoder=True`` (the command line's way) a third
    field is allowed too: ``NAxNSxNE`` -> the [NA * NS * NE][3] (action, sense, encoder delay) cells, the encoder
    delay e in range(NE) fastest. Without it a spec of three fields is refused, as it always was: a caller that
    unpacks two columns is never handed three."""
    from .native import FLEET_MAX_DELAY
    try:
        sizes = [int(v) for v in spec.lower().split("x")]
        assert len(sizes) in ((2, 3) if encoder else (2,)) and 1 <= min(sizes) and max(sizes) <= FLEET_MAX_DELAY + 1
    except Exception:
        form = "NAxNS or NAxNSxNE with 1 <= NA, NS, NE" if encoder else "NAxNS with 1 <= NA, NS"
        raise ValueError(f"--delay_grid wants {form} <= {FLEET_MAX_DELAY + 1}, got {spec!r}") from None
    return np.array(list(np.ndindex(*sizes)), dtype=np.int32)


def robot_delay_cells(num_robots: int, n_command: int, n_push: int, n_delay: int) -> np.ndarray:
    """Round-robin over command cell x push cell x delay cell: ``robot_cells``' two, then delay cell
    (r div (n_command * n_push)) mod n_delay."""
    return (np.arange(num_robots) // (n_command * n_push)) % n_delay


def latency_plan(args, n_command: int, n_push: int = 1):
    """The command line's latency flags, or None without ``--delay_grid``: {"cells" [D][2], "cell" [N],
    "latency": ``set_latency``'s arguments, "echo": the settings for the report}. With ``--delay_jitter`` a robot
    draws per period from [0, its cell's value] instead of holding it. A grid ``NAxNSxNE`` has cells [D][3] and
    the encoder delay as the fourth of ``set_latency``'s arguments."""
    if args.delay_grid is None:
        if args.delay_jitter:
            raise ValueError("--delay_jitter needs --delay_grid NAxNS")
        return None
    cells = delay_grid(args.delay_grid, encoder=True)
    cell = robot_delay_cells(args.num_robots, n_command, n_push, len(cells))
    latency = cell_latency(cells, cell, args.delay_jitter, args.delay_seed)
    echo = {"delay_grid": args.delay_grid, "delay_jitter": bool(args.delay_jitter), "delay_seed": args.delay_seed}
    return {"cells": cells, "cell": cell, "latency": latency, "echo": echo}


def cell_latency(cells: np.ndarray, cell: np.ndarray, jitter: bool, seed: int) -> tuple:
    """``set_latency``'s arguments (action, sense, seed[, encoder]) for robots in the delay cells ``cell`` [N] of
    ``cells`` [D][2 or 3]: each robot's cell values held, or with ``jitter`` drawn from [0, the value]."""
    zero = np.zeros_like(cells[cell, 0])
    cols =[((zero, cells[cell, k]) if jitter else cells[cell, k]) for k in range(cells.shape[1])]
    return (cols[0], cols[1], seed, *cols[2:])


def latency_report(rep: Dict[str, np.ndarray], acc: np.ndarray, delay_cell: np.ndarray, cells: np.ndarray,
                   n_periods: int, jitter: bool = False) -> list:
    """Per delay cell (``delay_cell`` [N], each robot's cell): the delays in periods and ms (with ``jitter`` the
    upper end of the drawn range), the count, the share that never fell, the mean periods survived and the rms
    errors over the cell's surviving periods (``grid_report``'s aggregation of ``acc``)."""
    cell = np.asarray(delay_cell)
    out = []
    for c in range(len(cells)):
        m = cell == c
        a = np.asarray(acc)[m].astype(np.float64)
        tot = a.sum(0) if len(a) else np.zeros(6)
        rms = (lambda v: float(np.sqrt(v / tot[0]))) if tot[0] > 0 else (lambda v: None)
        da, ds = int(cells[c][0]), int(cells[c][1])
        row = {"cell": c, "action_delay": da, "sense_delay": ds, "action_delay_ms": da * PERIOD_MS,
               "sense_delay_ms": ds * PERIOD_MS, "jitter": bool(jitter), "count": int(len(a)),
               "survival_rate": float(np.mean(~np.asarray(rep["fell"], dtype=bool)[m])) if len(a) else None,
               "mean_periods": float(a[:, 0].mean()) if len(a) else None, "periods": int(n_periods),
               "rms_lin_err": rms(tot[4]), "rms_yaw_err": rms(tot[5])}
        if len(cells[c]) > 2:     # a grid with the encoder axis
            row["encoder_delay"], row["encoder_delay_ms"] = int(cells[c][2]), int(cells[c][2]) * PERIOD_MS
        out.append(row)
    return out


def add_latency_arguments(p) -> None:
    p.add_argument("--delay_grid", type=str, default=None, metavar="NAxNS[xNE]",
                   help="action delays 0..NA-1 x IMU delays 0..NS-1 [x joint-encoder delays 0..NE-1] in control "
                        "periods of 20 ms (NA, NS, NE <= 3)")
    p.add_argument("--delay_jitter", action="store_true", default=False,
                   help="draw each robot's delays per period from [0, its cell's value] instead of holding them")
    p.add_argument("--delay_seed", type=int, default=0, metavar="SEED")


def add_recorder_arguments(p) -> None:
    p.add_argument("--record_falls", type=int, default=None, metavar="DEPTH",
                   help="keep every robot's last DEPTH periods on the device, frozen at its fall")
    p.add_argument("--record_post", type=int, default=0, metavar="K", help="periods kept after the fall frame")
    p.add_argument("--record_out", type=str, default=None, metavar="falls.npz",
                   help="write the fallen robots' frames (needs --record_falls)")
    p.add_argument("--record_max", type=int, default=64, metavar="R", help="at most R robots, lowest ids first")


def falls_archive(fleet: "FleetInfer", max_robots: int) -> Dict[str, np.ndarray]:
    """The arrays of the command line's ``--record_out`` file: the frames of the fallen robots, lowest ids
    first and at most ``max_robots`` of them. ``robots`` [R], ``count`` [R] (frames held), ``survived`` [R] (the
    report's periods survived: the robot fell in the next one), ``period`` [R][depth] (-1 past ``count``), every field of ``frame_fields`` as [R][depth][width] (zero past
    ``count``), and ``fields``: the field map {name: [first word, width]} as a JSON string."""
    import json
    rep = fleet.report()
    fell = np.flatnonzero(rep["fell"])[:max(0, int(max_robots))]
    depth = fleet.rec_depth
    out = {"robots": fell.astype(np.int64), "count": np.zeros(len(fell), np.int64),
           "survived": rep["periods"][fell].astype(np.int64),
           "period": np.full((len(fell), depth), -1, np.int64)}
    for name, (_, w) in fleet.frame_fields.items():
        out[name] = np.zeros((len(fell), depth, w), np.float32)
    for k, robot in enumerate(fell):
        rec = fleet.recorded(int(robot))
        t = out["count"][k] = len(rec["period"])
        out["period"][k, :t] = rec["period"]
        for name in fleet.frame_fields:
            out[name][k, :t] = rec[name]
    out["fields"] = np.array(json.dumps({k: list(v) for k, v in fleet.frame_fields.items()}))
    return out


# --- following a log (include/duck_fleet.h duck_fleet_follow) -------------------------------------------
def fleet_log_size(nu: int) -> int:
    """DUCK_FLEET_LOG_SIZE(nu): the width of a log row, an obs row and then the action that answered it."""
    return HEADERS.value(f"DUCK_FLEET_LOG_SIZE({int(nu)})")


def log_arguments(log, ids, num_robots: int, nu: int, scheduled: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """``FleetInfer.set_log``'s arguments, validated on the host: (log [L][T][W] float32 C-contiguous, ids [N]
    int32). DuckError on a command schedule set at the same time (``scheduled``: both write the command), a shape
    that is not [T][W] or [L][T][W] with L, T >= 1 and W = DUCK_FLEET_LOG_SIZE(nu), and ids that are not [N]
    integers in [0, L). NaN words are data: a NaN observation word is a missing sample."""
    from .native import DuckError
    n, W = int(num_robots), fleet_log_size(nu)
    if scheduled:
        raise DuckError("a command schedule is set and a log writes the command itself: set_command_schedule(None) first")
    try:
        tab = np.ascontiguousarray(log, dtype=np.float32)
    except (TypeError, ValueError):
        raise DuckError("a log is a float32 array [T][W] or [L][T][W]") from None
    if tab.ndim == 2:
        tab = tab[None]
    if tab.ndim != 3 or tab.shape[2] != W:
        raise DuckError(f"a log is [T][{W}] or [L][T][{W}] ({fleet_obs_size(nu)} obs words, then {int(nu)} actions), "
                        f"got {tuple(np.shape(log))}")
    if tab.shape[0] < 1 or tab.shape[1] < 1:
        raise DuckError(f"a log needs L >= 1 logs of T >= 1 rows, got {tuple(tab.shape)}")
    if tab.shape[1] >= 2 ** 31 - 1 or tab.shape[0] >= 2 ** 31 - 1:
        raise DuckError("a log's L and T must fit an int32")
    idv = np.arange(n) % tab.shape[0] if ids is None else np.asarray(ids)
    if idv.shape != (n,) or not np.issubdtype(idv.dtype, np.integer):
        raise DuckError(f"log ids must be [{n}] integers, got {idv.dtype} {tuple(idv.shape)}")
    if idv.min() < 0 or idv.max() >= tab.shape[0]:
        raise DuckError(f"log ids must lie in [0, {tab.shape[0]}), got [{idv.min()}, {idv.max()}]")
    return tab, idv.astype(np.int32)


def _obs_nu(width: int) -> int:
    from .native import DuckError
    nu, rest = divmod(int(width) - 17, 6)
    if rest or nu < 1:
        raise DuckError(f"an observation row is 17 + 6 nu words wide, got {width}")
    return nu


def log_from_saved_obs(obs) -> np.ndarray:
    """The reference's ``saved_obs`` form -- [T + 1][OBS] (or [L][T + 1][OBS]), the observations a loop's policy
    saw period by period (mujoco_infer.py:202, :241; ``FleetInfer.run(record=True)[:, robot]``) -- as a log of T
    rows: row p is observation p, then action p, which is the ``last_action`` columns of observation p + 1 (the
    action the policy answered observation p with). Words are copied, whatever their bits."""
    from .native import DuckError
    a = np.ascontiguousarray(obs, dtype=np.float32)
    if a.ndim not in (2, 3) or a.shape[-2] < 2:
        raise DuckError(f"saved observations are [T + 1][OBS] or [L][T + 1][OBS] with T >= 1, got {tuple(a.shape)}")
    nu = _obs_nu(a.shape[-1])
    last = 13 + 2 * nu          # gyro 3, accelerometer 3, command 7, joint angles nu, joint velocities nu
    return np.ascontiguousarray(np.concatenate([a[..., :-1, :], a[..., 1:, last:last + nu]], axis=-1))


def saved_obs_from_log(log) -> np.ndarray:
    """``log_from_saved_obs`` the other way, for a log whose actions are the ``last_action`` columns of its next
    row: [T + 1][OBS], the last row NaN (no sample) but for its ``last_action`` columns. DuckError for a log that
    does not have that form (it cannot be held as observation rows alone)."""
    from .native import DuckError
    a = np.ascontiguousarray(log, dtype=np.float32)
    nu, rest = divmod(a.shape[-1] - 17, 7) if a.ndim in (2, 3) else (0, 1)
    if rest or nu < 1 or a.shape[-2] < 1:
        raise DuckError(f"a log is [T][17 + 7 nu] or [L][T][17 + 7 nu] with T >= 1, got {tuple(a.shape)}")
    O, last = 17 + 6 * nu, 13 + 2 * nu
    if a[..., :-1, O:].view(np.int32).tobytes() != a[..., 1:, last:last + nu].view(np.int32).tobytes():
        raise DuckError("the log's actions are not the last_action columns of its next rows: it is not a saved_obs "
                        "form, save it as .npz (obs and action)")
    end = np.full(a.shape[:-2] + (1, O), np.nan, dtype=np.float32)
    end[..., 0, last:last + nu] = a[..., -1, O:]
    return np.ascontiguousarray(np.concatenate([a[..., :O], end], axis=-2))


def save_log(path: str, log) -> None:
    """A log ([T][W] or [L][T][W]) to ``path``: ``.npz`` holds ``obs`` [..][T][OBS] and ``action`` [..][T][nu], any
    log; ``.npy`` holds the observation rows alone, the reference's saved_obs form [..][T + 1][OBS]
    (``saved_obs_from_log``: only a log whose actions are its next rows' ``last_action`` columns)."""
    from .native import DuckError
    a = np.ascontiguousarray(log, dtype=np.float32)
    if path.endswith(".npy"):
        np.save(path, saved_obs_from_log(a), allow_pickle=False)
    elif path.endswith(".npz"):
        nu, rest = divmod(a.shape[-1] - 17, 7) if a.ndim in (2, 3) else (0, 1)
        if rest or nu < 1:
            raise DuckError(f"a log is [T][17 + 7 nu] or [L][T][17 + 7 nu], got {tuple(a.shape)}")
        np.savez(path, obs=a[..., :17 + 6 * nu], action=a[..., 17 + 6 * nu:])
    else:
        raise DuckError(f"a log file is .npy or .npz, got {path!r}")


def load_log(path: str) -> np.ndarray:
    """A log from ``path``. ``.npy``: the observation rows [T + 1][OBS] (or [L][T + 1][OBS]) of a saved_obs
    (``log_from_saved_obs``). ``.npz``: ``obs`` and, optionally, ``action`` [..][T][nu] of the same leading shape;
    without ``action``, ``obs`` is the saved_obs form again. Pickles are not read: the reference pickles its
    saved_obs list (mujoco_infer.py:241), and the one-line conversion on the user's side is
    ``np.save("log.npy", np.asarray(pickle.load(open("saved_obs.pkl", "rb")), dtype=np.float32))``."""
    from .native import DuckError
    if path.endswith(".npy"):
        return log_from_saved_obs(np.load(path, allow_pickle=False))
    if not path.endswith(".npz"):
        raise DuckError(f"a log file is .npy or .npz (pickles are not read), got {path!r}")
    with np.load(path, allow_pickle=False) as z:
        if "obs" not in z.files:
            raise DuckError(f"{path!r} holds no array 'obs' (it holds {z.files})")
        obs = np.ascontiguousarray(z["obs"], dtype=np.float32)
        if "action" not in z.files:
            return log_from_saved_obs(obs)
        act = np.ascontiguousarray(z["action"], dtype=np.float32)
    if obs.ndim not in (2, 3) or act.shape != obs.shape[:-1] + (_obs_nu(obs.shape[-1]),):
        raise DuckError(f"'obs' [..][T][17 + 6 nu] and 'action' [..][T][nu] do not fit: {tuple(obs.shape)}, {tuple(act.shape)}")
    return np.ascontiguousarray(np.concatenate([obs, act], axis=-1))


SENSOR_GROUPS = ("gyro", "accelerometer", "joint_position", "joint_velocity")   # weight 1 by default


def score_groups(nu: int) -> Dict[str, Tuple[int, int]]:
    """(first obs column, width) of each scored column group. The command columns (6-12) are fed from the log and
    belong to none."""
    return {"gyro": (0, 3), "accelerometer": (3, 3), "joint_position": (13, nu), "joint_velocity": (13 + nu, nu),
            "action_history": (13 + 2 * nu, 3 * nu), "motor_targets": (13 + 5 * nu, nu), "contacts": (13 + 6 * nu, 2),
            "phase": (15 + 6 * nu, 2)}


def score_weights(weights=None, nu: int = 1) -> Dict[str, float]:
    """{group: weight} over every group of ``score_groups``: 1 on the four sensor groups and 0 on the rest, then
    ``weights`` ({group: weight}) over that. DuckError on an unknown group or a weight that is not finite."""
    from .native import DuckError
    out = {g: (1.0 if g in SENSOR_GROUPS else 0.0) for g in score_groups(nu)}
    for g, w in (weights or {}).items():
        if g not in out:
            raise DuckError(f"no score group {g!r} (the groups: {', '.join(out)})")
        if not np.isfinite(w):
            raise DuckError(f"the weight of {g!r} must be finite, got {w!r}")
        out[g] = float(w)
    return out


def score_report(score, log, log_id, log_tick, weights=None) -> Dict[str, np.ndarray]:
    """``FleetInfer.score_report`` on host arrays: score [N][OBS], log [L][T][W], log_id [N], log_tick [N] (the rows
    each robot has followed). Per group [N] float64: sqrt(sum of the group's score words / count), the count being
    the non-NaN log words of the group's columns in rows 0 .. log_tick - 1 of the robot's log (NaN when that is 0);
    ``"total"`` = sum of weight x rms over the groups with a non-zero weight and a count (a robot with a NaN score
    has a NaN total, and so has one with no such group: they rank last), and ``"periods"``. The action_history and motor_targets groups are checks of
    the feeding, not of the model."""
    score = np.asarray(score, dtype=np.float64)
    log = np.asarray(log, dtype=np.float32)
    log = log[None] if log.ndim == 2 else log
    n, O = score.shape
    nu = _obs_nu(O)
    T = log.shape[1]
    ids = np.clip(np.asarray(log_id, dtype=np.int64), 0, log.shape[0] - 1)
    rows = np.clip(np.asarray(log_tick, dtype=np.int64), 0, T)
    present = np.concatenate([np.zeros((log.shape[0], 1, O), np.int64),
                              np.cumsum(~np.isnan(log[:, :, :O]), axis=1, dtype=np.int64)], axis=1)   # [L][T + 1][OBS]
    count = present[ids, rows]                                                                       # [N][OBS]
    w = score_weights(weights, nu)
    out, total, counted = {}, np.zeros(n), np.zeros(n, bool)
    for g, (o, width) in score_groups(nu).items():
        c = count[:, o:o + width].sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[g] = np.sqrt(score[:, o:o + width].sum(1) / np.where(c > 0, c, np.nan))
        if w[g] != 0.0:
            total = total + np.where(c > 0, w[g] * out[g], 0.0)
            counted |= c > 0
    out["total"], out["periods"] = np.where(counted, total, np.nan), rows   # nothing compared: no rank
    return out


def rank_totals(total) -> np.ndarray:
    """Robot ids from the best (smallest) total to the worst, ties by id; NaN totals last."""
    t = np.asarray(total, dtype=np.float64)
    return np.lexsort((np.arange(len(t)), np.where(np.isnan(t), np.inf, t), np.isnan(t)))


def refine_population(dr, total, elite: int, rng, lo, hi) -> np.ndarray:
    """The next round's randomisation record of a search over the randomisation box. ``dr`` [R][N] float32 (a
    column per robot, ``FleetInfer.dr.view(-1, N)``), ``total`` [N] the robots' score totals. The ``elite`` best
    columns (``rank_totals``: NaN last) are kept unchanged, as columns 0 .. elite - 1 in rank order; every other
    column is drawn per row from a normal with the elite's mean and standard deviation (``rng``: a
    numpy.random.Generator) and clipped to [``lo``, ``hi``] ([R] each: the per-row minimum and maximum of round 0's
    duck_randomize population, so the search never leaves the box that was randomised). The rows are drawn
    independently: a correlation between rows of the elite is not kept. Pure numpy; returns [R][N] float32."""
    from .native import DuckError
    dr = np.asarray(dr, dtype=np.float32)
    total = np.asarray(total, dtype=np.float64)
    if dr.ndim != 2 or total.shape != (dr.shape[1],):
        raise DuckError(f"dr is [R][N] and total [N], got {tuple(dr.shape)} and {tuple(total.shape)}")
    R, n = dr.shape
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    if int(elite) != elite or not 1 <= int(elite) <= n:
        raise DuckError(f"elite must be an integer in [1, {n}], got {elite!r}")
    if lo.shape != (R,) or hi.shape != (R,) or not (lo <= hi).all():
        raise DuckError(f"lo and hi are [{R}] with lo <= hi")
    elite = int(elite)
    best = dr[:, rank_totals(total)[:elite]]
    mean, std = best.astype(np.float64).mean(1), best.astype(np.float64).std(1)
    draw = mean[:, None] + std[:, None] * rng.standard_normal((R, n - elite))
    draw = np.minimum(np.maximum(draw.astype(np.float32), lo[:, None]), hi[:, None])
    return np.ascontiguousarray(np.concatenate([best, draw], axis=1), dtype=np.float32)


def add_follow_arguments(p) -> None:
    p.add_argument("--follow", type=str, default=None, metavar="LOG",
                   help="follow a recorded robot log (.npy obs rows, or .npz obs + action) instead of a policy and "
                        "score every robot's observations against it")
    p.add_argument("--follow_weights", type=str, default=None, metavar="g=w,...",
                   help="weights of the score groups in the total (default: 1 on gyro, accelerometer, joint_position, "
                        "joint_velocity)")
    p.add_argument("--rounds", type=int, default=1, metavar="R",
                   help="rounds of the search: round 0 is --randomize SEED, each later one refines around the best")
    p.add_argument("--elite", type=int, default=8, metavar="K", help="the best K robots a round keeps and reports")
    p.add_argument("--fit_out", type=str, default=None, metavar="fit.json", help="write the last round's best robots")


def follow_plan(args):
    """The command line's follow flags, or None without ``--follow``: {"log": the path, "weights": {group: weight}
    as given, "rounds", "elite" (at most num_robots), "fit_out"}. ValueError on a flag that needs ``--follow``, a bad
    weight list, ``--rounds`` < 1, ``--elite`` < 1, or more than one round without ``--randomize``."""
    if args.follow is None:
        if args.follow_weights is not None or args.rounds != 1 or args.fit_out is not None:
            raise ValueError("--follow_weights, --rounds and --fit_out need --follow LOG")
        return None
    weights = {}
    for item in (args.follow_weights or "").split(","):
        if not item.strip():
            continue
        try:
            g, w = item.split("=")
            weights[g.strip()] = float(w)
            assert g.strip() in score_groups(1) and np.isfinite(weights[g.strip()])
        except Exception:
            raise ValueError(f"--follow_weights wants group=weight,... over {', '.join(score_groups(1))}, got {item!r}") from None
    if args.rounds < 1 or args.elite < 1:
        raise ValueError("--rounds and --elite must be >= 1")
    if args.rounds > 1 and args.randomize is None:
        raise ValueError("--rounds above 1 searches the randomisation box: it needs --randomize SEED")
    if args.resample_commands:
        raise ValueError("--resample_commands and --follow both write the command")
    return {"log": args.follow, "weights": weights, "rounds": int(args.rounds),
            "elite": min(int(args.elite), int(args.num_robots)), "fit_out": args.fit_out}


def follow_round(fleet: "FleetInfer", rep: Dict[str, np.ndarray], survived, elite: int, delays=None) -> dict:
    """One round of the report's ``"follow"`` key: the best total and, for the best ``elite`` robots, the id, the
    group rms values, the total, the periods survived, the delay cell (with a delay grid) and the randomisation
    record by ``cabi.dr_layout``'s field names (with ``--randomize``)."""
    num = lambda v: None if np.isnan(v) else float(v)  # noqa: E731
    order = rank_totals(rep["total"])[:elite]
    dr = None if fleet.dr is None else fleet.dr.view(-1, fleet.num_robots).cpu().numpy()
    layout = dr_layout(fleet.model.nbody, fleet.num_dofs)
    names = [k for k in layout if k != "nfloat"]
    best = []
    for e in order:
        row = {"id": int(e), "total": num(rep["total"][e]), "rms": {g: num(rep[g][e]) for g in score_groups(fleet.num_dofs)},
               "periods_followed": int(rep["periods"][e]), "periods_survived": int(survived[e])}
        if delays is not None:
            c = int(delays["cell"][e])
            row["delay_cell"] = {"cell": c, "action_delay": int(delays["cells"][c][0]), "sense_delay": int(delays["cells"][c][1])}
            if len(delays["cells"][c]) > 2:
                row["delay_cell"]["encoder_delay"] = int(delays["cells"][c][2])
        if dr is not None:
            ends = [layout[k] for k in names[1:]] + [layout["nfloat"]]
            row["randomization"] = {k: [float(v) for v in dr[layout[k]:end, e]] for k, end in zip(names, ends)}
        best.append(row)
    return {"best_total": best[0]["total"], "best": best}


# --- several policies in one fleet (include/duck_ppo.h duck_policy_act_multi) ----------------------------
def policy_segments(num_policies: int, num_robots: int, policy_robots=None) -> np.ndarray:
    """``policy_seg`` [K + 1] int32: segment k is robots seg[k] .. seg[k + 1] - 1. ``policy_robots`` [K] gives the
    lengths (0 is allowed), by default ``num_robots / K`` each. DuckError when the lengths are not K non-negative
    integers that sum to ``num_robots``, or the default does not divide."""
    from .native import DuckError
    K, n = int(num_policies), int(num_robots)
    if policy_robots is None:
        if n % K:
            raise DuckError(f"{n} robots do not split equally over {K} policies: give policy_robots")
        lengths = np.full(K, n // K, dtype=np.int64)
    else:
        lengths = np.asarray(policy_robots)
        if lengths.shape != (K,) or not np.issubdtype(lengths.dtype, np.integer) or (lengths < 0).any():
            raise DuckError(f"policy_robots must be {K} non-negative integers, got {policy_robots!r}")
        if int(lengths.sum()) != n:
            raise DuckError(f"policy_robots {lengths.tolist()} sum to {int(lengths.sum())}, the fleet has {n} robots")
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def load_policies(paths, num_robots: int, policy_robots=None, following: bool = False):
    """The K policy files of a fleet, validated on the host before any device work: (``dense_policy`` of every
    file, ``policy_seg``). DuckError, naming the offending file, for an empty list, more than
    DUCK_POLICY_MAX_POLICIES files, a list together with a followed log, a file outside duck_policy_act's limits,
    layer sizes that differ from the first file's, and a normaliser in some files and not in others."""
    from .native import DuckError
    from .onnx_infer import OnnxGraph, dense_policy
    from .ppo import POLICY_ACT_MAX_LAYERS, POLICY_ACT_MAX_WIDTH
    paths, most = list(paths), HEADERS.consts["DUCK_POLICY_MAX_POLICIES"]
    if not paths:
        raise DuckError("a list of policies needs at least one file")
    if len(paths) > most:
        raise DuckError(f"a fleet holds at most {most} policies (DUCK_POLICY_MAX_POLICIES), got {len(paths)}: "
                        f"{paths[most]!r} is one too many")
    if following:
        raise DuckError(f"a followed log takes the policy's place: it cannot be combined with a list of policies "
                        f"({paths[0]!r}, ...)")
    seg = policy_segments(len(paths), num_robots, policy_robots)
    pols = []
    for path in paths:
        with open(path, "rb") as f:
            pol = dense_policy(OnnxGraph(f.read()))
        sizes = pol["sizes"]
        if len(pol["W"]) > POLICY_ACT_MAX_LAYERS or max(sizes) > POLICY_ACT_MAX_WIDTH:
            raise DuckError(f"{path!r}: policy layers {sizes} are outside duck_policy_act's limits (at most "
                            f"{POLICY_ACT_MAX_LAYERS} layers, at most {POLICY_ACT_MAX_WIDTH} wide); there is no host fallback")
        if pols and list(sizes) != list(pols[0]["sizes"]):
            raise DuckError(f"{path!r} has layers {list(sizes)}, {paths[0]!r} has {list(pols[0]['sizes'])}: "
                            "the policies of one fleet share one architecture")
        if pols and (pol["mean"] is None) != (pols[0]["mean"] is None):
            with_, without = (paths[0], path) if pol["mean"] is None else (path, paths[0])
            raise DuckError(f"{with_!r} has an observation normaliser and {without!r} has none: all or none")
        pols.append(pol)
    return pols, seg


def tile_over_policies(a, num_policies: int) -> np.ndarray:
    """An [S, ...] per-robot table repeated ``num_policies`` times along its first axis, [K S, ...]: robot j of
    every (equal) segment of a policy-major fleet gets row j."""
    a = np.asarray(a)
    return np.tile(a, (int(num_policies),) + (1,) * (a.ndim - 1))


def policy_report(rep: Dict[str, np.ndarray], acc: np.ndarray, seg, n_periods: int, cells=None, push=None,
                  delay=None) -> list:
    """Per policy k (robots seg[k] .. seg[k + 1] - 1 of ``FleetInfer.report()``'s ``rep`` and of ``acc`` [N][6]):
    the robot count, ``survival_rate``, ``mean_periods``, the rms tracking errors pooled over the segment's surviving
    periods (None for an empty segment or one that survived no period), and the per-cell rows over the segment's
    slice: ``"cells"`` = ``grid_report`` with ``cells`` [C][7]; ``"pushes"`` = ``push_report`` with ``push`` =
    (push_cell [N], first, interval, window); ``"latency"`` = ``latency_report`` with ``delay`` = (delay_cell [N],
    cells [D][2], jitter). The cell of a robot is what the fleet-wide tables say, sliced: with tiled tables a
    segment's slice is the one-segment table."""
    seg = np.asarray(seg, dtype=np.int64)
    acc = np.asarray(acc)
    fell = np.asarray(rep["fell"], dtype=bool)
    out = []
    for k in range(len(seg) - 1):
        s = slice(int(seg[k]), int(seg[k + 1]))
        a = acc[s].astype(np.float64)
        cnt = len(a)
        tot = a.sum(0) if cnt else np.zeros(acc.shape[1])
        rms = (lambda v: float(np.sqrt(v / tot[0]))) if tot[0] > 0 else (lambda v: None)
        sub = {key: np.asarray(v)[s] for key, v in rep.items()}
        row = {"policy": k, "count": int(cnt), "survival_rate": float(np.mean(~fell[s])) if cnt else None,
               "mean_periods": float(a[:, 0].mean()) if cnt else None, "periods": int(n_periods),
               "rms_lin_err": rms(tot[4]), "rms_yaw_err": rms(tot[5])}
        if cells is not None:
            row["cells"] = grid_report(sub, acc[s], cells, n_periods)
        if push is not None:
            cell, first, interval, window = push
            part = lambda v: np.asarray(v)[s] if np.ndim(v) else v  # noqa: E731
            row["pushes"] = push_report(sub, np.asarray(cell)[s], part(first), part(interval), n_periods, window)
        if delay is not None:
            cell, dcells, jitter = delay
            row["latency"] = latency_report(sub, acc[s], np.asarray(cell)[s], dcells, n_periods, jitter)
        out.append(row)
    return out


def paired_wins(periods, num_policies: int) -> np.ndarray:
    """[K][K] int64 from ``periods`` [K S] (policy-major, equal segments: the periods each robot survived): entry
    [a][b] counts the scenarios j in which policy a's robot j survived strictly more periods than policy b's. Ties
    count for neither, so [a][b] + [b][a] <= S and the diagonal is 0."""
    from .native import DuckError
    K = int(num_policies)
    p = np.asarray(periods, dtype=np.float64)
    if K < 1 or p.ndim != 1 or p.shape[0] % K:
        raise DuckError(f"paired wins need periods [K S] of K = {K} equal segments, got {tuple(p.shape)}")
    p = p.reshape(K, -1)
    return (p[:, None, :] > p[None, :, :]).sum(-1).astype(np.int64)


def rank_policies(rows) -> list:
    """The policies of ``policy_report``'s rows, best first: ``survival_rate`` descending, then ``mean_periods``
    descending, then ``rms_lin_err`` ascending with None / NaN last, then the index. A policy without robots
    (rates None) ranks after every policy with some."""
    def key(k):
        r = rows[k]
        num = lambda v: float("nan") if v is None else float(v)  # noqa: E731
        s, p, e = num(r["survival_rate"]), num(r["mean_periods"]), num(r["rms_lin_err"])
        return (np.isnan(s), -s if not np.isnan(s) else 0.0, np.isnan(p), -p if not np.isnan(p) else 0.0,
                np.isnan(e), e if not np.isnan(e) else 0.0, k)
    return sorted(range(len(rows)), key=key)


def policies_doc(paths, rep: Dict[str, np.ndarray], acc: np.ndarray, seg, n_periods: int, cells=None, push=None,
                 delay=None) -> dict:
    """The three keys ``--policies`` adds to the command line's report: ``"policies"``, ``policy_report``'s rows
    with each policy's ``"path"``; ``"ranking"``, the policy indices best first (``rank_policies``);
    ``"paired_wins"``, the [K][K] matrix of ``paired_wins`` as lists."""
    rows = policy_report(rep, acc, seg, n_periods, cells, push, delay)
    for row, path in zip(rows, paths):
        row["path"] = str(path)
    return {"policies": rows, "ranking": rank_policies(rows),
            "paired_wins": paired_wins(rep["periods"], len(rows)).tolist()}


def add_gait_arguments(p) -> None:
    p.add_argument("--gait", action="store_true", default=False,
                   help="keep the gait and servo-load record and report it: for the fleet, per command cell and per policy")
    p.add_argument("--gait_force_frac", type=float, default=0.9, metavar="F",
                   help="a period counts as force-saturated at this fraction of the actuator's force limit")
    p.add_argument("--gait_speed_frac", type=float, default=1.0, metavar="F",
                   help="a period counts as speed-saturated at this fraction of the motors' 5.24 rad/s")


def gait_plan(args) -> Optional[tuple]:
    """``FleetInfer``'s ``gait`` keyword from the command line's arguments: None without ``--gait``."""
    if not args.gait:
        return None
    if not (args.gait_force_frac >= 0 and args.gait_speed_frac >= 0):
        raise ValueError("--gait_force_frac and --gait_speed_frac want fractions >= 0")
    return (True, float(args.gait_force_frac), float(args.gait_speed_frac))


def add_gait_report(doc: dict, gait, acc, model, cell, seg=None, dt: float = 0.02) -> dict:
    """What ``--gait`` adds to the command line's report ``doc``, in place: ``"gait"``, ``gait_summary`` of the
    whole fleet; ``"gait"`` in every row of ``doc["cells"]``, the summary of the cell's robots (``cell`` [N], each
    robot's command cell); and, with ``seg`` [K + 1] (several policies), ``"gait"`` in every row of
    ``doc["policies"]``. ``gait=None`` (no record was kept) adds nothing."""
    if gait is None:
        return doc
    cell = np.asarray(cell)
    doc["gait"] = gait_summary(gait, acc, None, model, dt)
    for c, row in enumerate(doc.get("cells", ())):
        row["gait"] = gait_summary(gait, acc, cell == c, model, dt)
    if seg is not None:
        for k, row in enumerate(doc.get("policies", ())):
            row["gait"] = gait_summary(gait, acc, slice(int(seg[k]), int(seg[k + 1])), model, dt)
    return doc


def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="Run an exported policy in the deployment loop for a fleet of robots")
    p.add_argument("-o", "--onnx_model_path", type=str, default=None,
                   help="the exported policy (optional with --follow LOG)")
    p.add_argument("--reference_data", type=str, default=None)
    p.add_argument("--model_path", type=str, default="flat_terrain")
    p.add_argument("--standing", action="store_true", default=False)
    p.add_argument("--num_robots", type=int, default=1024)
    p.add_argument("--periods", type=int, default=500)
    p.add_argument("--command_grid", type=str, default="1x1x1")
    p.add_argument("--randomize", type=int, default=None, metavar="SEED")
    p.add_argument("--out", type=str, default=None, metavar="report.json")
    p.add_argument("--device", type=str, default="cuda:0")
    add_disturbance_arguments(p)
    add_latency_arguments(p)
    add_recorder_arguments(p)
    add_follow_arguments(p)
    add_gait_arguments(p)
    p.add_argument("--policies", type=str, nargs="+", default=None, metavar="P",
                   help="several exported policies in one fleet, --num_robots / K robots each on the same models, "
                        "commands, pushes and delays; the report ranks them")
    return p


def parse_arguments(argv=None):
    """The command line's arguments; a flag that needs another one is a usage error."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.policies is not None:
        if args.onnx_model_path is not None or args.follow is not None:
            p.error("--policies P1 P2 ... takes the place of -o and cannot be combined with --follow")
        if len(args.policies) > HEADERS.consts["DUCK_POLICY_MAX_POLICIES"]:
            p.error(f"--policies takes at most {HEADERS.consts['DUCK_POLICY_MAX_POLICIES']} files")
        if args.num_robots % len(args.policies):
            p.error(f"--num_robots {args.num_robots} (the total) is not divisible by the {len(args.policies)} --policies")
    elif args.onnx_model_path is None and args.follow is None:
        p.error("-o/--onnx_model_path is required (unless --follow LOG or --policies P1 P2 ... is given)")
    try:
        follow_plan(args)
        gait_plan(args)
    except ValueError as e:
        p.error(str(e))
    if args.record_falls is None and args.record_out is not None:
        p.error("--record_out needs --record_falls DEPTH")
    if args.record_falls is not None and (args.record_falls < 1 or args.record_post < 0 or args.record_max < 0):
        p.error("--record_falls wants DEPTH >= 1, --record_post K >= 0 and --record_max R >= 0")
    return args


def main(argv=None) -> int:
    import json
    import copy
    args = parse_arguments(argv)
    cells = command_grid(args.command_grid)
    # several policies: every grid is built for one segment of num_robots / K robots and tiled over the K segments
    K = 1 if args.policies is None else len(args.policies)
    one = copy.copy(args)
    one.num_robots = args.num_robots // K
    over = lambda v: tile_over_policies(v, K) if K > 1 and np.ndim(v) else v  # noqa: E731
    plan = disturbance_plan(one, cells)
    n_push = 1 if plan is None or plan["push_cells"] is None else len(plan["push_cells"])
    delays = latency_plan(one, len(cells), n_push)
    following = follow_plan(args)
    log = None if following is None else load_log(following["log"])
    if log is not None:
        args.periods = min(args.periods, int(log.shape[-2]))      # a run cannot pass the log's end
    fleet = FleetInfer(args.model_path, args.onnx_model_path if args.policies is None else list(args.policies),
                       args.num_robots, reference_data=args.reference_data,
                       standing=args.standing, device=args.device, randomize=args.randomize,
                       follow=None if log is None else (log, None), gait=gait_plan(args))
    if log is None:            # (a followed log brings its own commands)
        fleet.set_commands(over(cells[np.arange(one.num_robots) % len(cells)]))
    if plan is not None:
        if plan["schedule"] is not None:
            table, ids, seg_periods = plan["schedule"]
            fleet.set_command_schedule(table, over(ids), seg_periods)
        if plan["pushes"] is not None:
            plan["pushes"] = tuple(over(v) for v in plan["pushes"])
            plan["push_cell"] = over(plan["push_cell"])
            fleet.set_pushes(*plan["pushes"])
        if args.noise:
            fleet.set_noise(args.noise, args.noise_seed)
    if delays is not None:
        delays["cell"] = over(delays["cell"])
        delays["latency"] = tuple(tuple(over(w) for w in v) if isinstance(v, tuple) else over(v) for v in delays["latency"])
        fleet.set_latency(*delays["latency"])
    if args.record_falls is not None:
        fleet.set_recorder(args.record_falls, args.record_post)
    t0 = time.time()
    fleet.run(args.periods)
    dt = time.time() - t0
    follow_doc = None
    if following is not None:
        # system identification by search: score, keep the best, draw the next population around them, run again
        n, elite = args.num_robots, following["elite"]
        weights = score_weights(following["weights"], fleet.num_dofs)
        follow_doc = {"log": following["log"], "log_rows": int(log.shape[-2]), "periods": args.periods, "weights": weights,
                      "elite": elite, "rounds": []}
        rng = np.random.default_rng(args.randomize)
        box = None if fleet.dr is None else fleet.dr.view(-1, n).cpu().numpy()
        for rnd in range(following["rounds"]):
            if rnd > 0:
                order = rank_totals(srep["total"])
                new = refine_population(fleet.dr.view(-1, n).cpu().numpy(), srep["total"], elite, rng, box.min(1), box.max(1))
                fleet.dr.copy_(torch.as_tensor(new.reshape(-1)))
                if delays is not None:     # an elite robot keeps its delay cell, a new one draws an elite's
                    cell = delays["cell"][order[:elite]]
                    cell = delays["cell"] = np.concatenate([cell, rng.choice(cell, n - elite)])
                    fleet.set_latency(*cell_latency(delays["cells"], cell, args.delay_jitter, args.delay_seed))
                fleet.restart()
                fleet.run(args.periods)
            srep = fleet.score_report(weights)
            follow_doc["rounds"].append({"round": rnd, **follow_round(fleet, srep, fleet.report()["periods"], elite, delays)})
    rep = fleet.report()
    rows = grid_report(rep, fleet.acc.cpu().numpy(), cells, args.periods,
                       None if K == 1 else over(np.arange(one.num_robots) % len(cells)))
    doc = {"model_path": args.model_path, "onnx_model_path": args.onnx_model_path, "num_robots": args.num_robots,
           "periods": args.periods, "randomize": args.randomize, "standing": args.standing,
           "robot_periods_per_s": args.num_robots * args.periods / max(dt, 1e-9), "cells": rows}
    if plan is not None:
        doc["disturbance"] = plan["echo"]
        if plan["pushes"] is not None:
            doc["pushes"] = push_report(rep, plan["push_cell"], args.push_at, args.push_every, args.periods,
                                        args.recovery_window)
            for row in doc["pushes"]:
                row["magnitude"], row["theta"] = (float(v) for v in plan["push_cells"][row["cell"]])
    if delays is not None:
        doc["delay"] = delays["echo"]
        doc["latency"] = latency_report(rep, fleet.acc.cpu().numpy(), delays["cell"], delays["cells"], args.periods,
                                        args.delay_jitter)
    if args.record_falls is not None:
        written = 0
        if args.record_out:
            arrays = falls_archive(fleet, args.record_max)
            np.savez(args.record_out, **arrays)
            written = int(len(arrays["robots"]))
        doc["recorder"] = {"depth": args.record_falls, "post": args.record_post, "fallen": int(rep["fell"].sum()),
                           "written": written}
    if args.policies is not None:
        doc.update(policies_doc(args.policies, rep, fleet.acc.cpu().numpy(), fleet.policy_seg, args.periods, cells,
                                None if plan is None or plan["pushes"] is None else
                                (plan["push_cell"], args.push_at, args.push_every, args.recovery_window),
                                None if delays is None else (delays["cell"], delays["cells"], args.delay_jitter)))
    if gait_plan(args) is not None:
        add_gait_report(doc, fleet.gait_records(), fleet.acc.cpu().numpy(), fleet.model,
                        over(np.arange(one.num_robots) % len(cells)), fleet.policy_seg if args.policies is not None else None)
    if follow_doc is not None:
        doc["follow"] = follow_doc
        if following["fit_out"]:
            with open(following["fit_out"], "w") as f:
                f.write(json.dumps({**{k: v for k, v in follow_doc.items() if k != "rounds"}, "model_path": args.model_path,
                                    "randomize": args.randomize, **follow_doc["rounds"][-1]}, indent=1) + "\n")
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for r in rows:
        print(json.dumps(r))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
