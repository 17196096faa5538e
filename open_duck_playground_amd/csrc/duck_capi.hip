// duck_capi.hip — the C ABI of libduck.so (include/duck.h): argument checks, handle
// lifetime, device uploads of the shared tables, and dispatch to the compiled model
// variant (variant_*.hip). Every entry returns DUCK_OK or a negative code with a
// thread-local message; no entry allocates, synchronises or throws on the step path.
#include "duck_common.h"
#include "duck_lspairs.h"
#include "duck_math.h"
#include "../../include/duck_fleet.h"
#include "../../include/duck_ppo.h"

// the compiled model variants of this library (codegen.variant_registry; generated/ for libduck.so,
// a per-model build directory for a library compiled for another model, native.model_library)
#define DUCK_VARIANT(name) const VariantOps* duck_variant_##name();
#include "duck_variants.inc"
#undef DUCK_VARIANT
#define DUCK_VARIANT(name) duck_variant_##name(),
static const VariantOps* const kVariants[] = {
#include "duck_variants.inc"
};
#undef DUCK_VARIANT
static constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

static thread_local std::string g_err;
int duck_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// a kernel of this handle set the sticky device error word (DUCK_DEVERR_*): every later launch on the
// handle is refused until duck_device_error(clear) -- the state the failed launch wrote is not valid
static int device_error_fail(const duck_sim* s) {
  const unsigned w = *s->err_h;
  std::string why;
  if (w & DUCK_DEVERR_LAT_TIMEOUT)
    why += "a latency-kernel cross-wave event wait timed out (broken stage schedule); the envs of that "
           "workgroup were written with NaN qpos";
  return duck_fail(DUCK_EDEVICE, "device error word 0x" + [&] {
    char b[16];
    snprintf(b, sizeof(b), "%x", w);
    return std::string(b);
  }() + " set by an earlier launch: " + why);
}

// FNV-1a 64 over the model values a compiled variant bakes (duck_model_fingerprint)
namespace {
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
  }
  void i32(const int* a, int n) {
    for (int i = 0; i < n; i++) { int32_t v = a ? a[i] : 0; bytes(&v, 4); }
  }
  void f32(const double* a, int n) {  // the kernels bake float32: hash what they see
    for (int i = 0; i < n; i++) { float v = a ? (float)a[i] : 0.0f; bytes(&v, 4); }
  }
};

// The episode bookkeeping brax wraps around an env (include/duck_ppo.h: duck_episode_accumulate), one thread
// per env over its F = nmetrics + 2 accumulator columns: plain fp32 adds in step order. It reads the step
// kernel's outputs (reward, done, the metrics rows of the SoA state), so it lives in this unit and ships
// with every model's library.
// duck_debug_ls_flag: both forms of the line search's activity flag, each from the word in memory
__global__ __launch_bounds__(256) void ls_flag_kernel(int n, const float* __restrict__ x, float* __restrict__ sel,
                                                      float* __restrict__ sat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  sel[i] = ls_flag_select(x[i]);
  sat[i] = ls_flag_sat(x[i]);
}

__global__ __launch_bounds__(256) void episode_accumulate_kernel(int n, int nmetrics, const float* __restrict__ reward,
                                                                 const float* __restrict__ done,
                                                                 const float* __restrict__ metrics, int stride,
                                                                 int mode, float* __restrict__ run,
                                                                 float* __restrict__ fin, float* __restrict__ flag) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int F = nmetrics + 2;
  float* r = run + (size_t)e * F;
  const bool d = done[e] != 0.f;
  if (mode == DUCK_EPISODE_EVAL) {
    if (flag[e] == 0.f) return;
    r[0] += reward[e];
    for (int k = 0; k < nmetrics; k++) r[1 + k] += metrics[(size_t)k * stride + e];
    r[F - 1] += 1.f;
    if (d) flag[e] = 0.f;
    return;
  }
  r[0] += reward[e];
  for (int k = 0; k < nmetrics; k++) r[1 + k] += metrics[(size_t)k * stride + e];
  r[F - 1] += 1.f;
  if (d) {
    float* f = fin + (size_t)e * F;
    for (int c = 0; c < F; c++) {
      f[c] += r[c];
      r[c] = 0.f;
    }
    flag[e] += 1.f;
  }
}

// The deployment loop's host code on the device (include/duck_fleet.h): the observation, the action history,
// the motor targets and an evaluation's bookkeeping for N robots, driven by a descriptor of the model instead
// of a compiled variant, so they live in this unit and ship with every model's library. A 16-lane group
// takes a robot: its lanes read the SoA rows next to the neighbouring groups' (64-byte segments) and write 16
// consecutive words of the robot's row. Lanes past the last robot run on robot n - 1 with their stores
// masked, so that the group votes below see whole waves.
constexpr int FLEET_TEAM = 16;
constexpr int FLEET_TPB = 256;

// x / y correctly rounded for normal x, y and quotient (this library is compiled with approximate fp32
// division): a Newton step on v_rcp, then the quotient's residual
__device__ __forceinline__ float fleet_div_rn(float x, float y) {
  float r = __builtin_amdgcn_rcpf(y);
  r = fmaf(fmaf(-y, r, 1.f), r, r);
  const float q = x * r;
  return fmaf(fmaf(-q, y, x), r, q);
}

// A thread's place: its lane of the 16-lane group and the group's robot; false when the group is past robot
// n - 1 and leaves. (fleet_observe_kernel, whose groups past the end stay for the votes, places itself.)
__device__ __forceinline__ bool fleet_place(int n, int& lane, size_t& e) {
  lane = threadIdx.x % FLEET_TEAM;
  const int e0 = blockIdx.x * (FLEET_TPB / FLEET_TEAM) + threadIdx.x / FLEET_TEAM;
  e = e0;
  return e0 < n;
}

__global__ __launch_bounds__(FLEET_TPB) void fleet_observe_kernel(const duck_fleet_desc D, int n,
                                                                  const float* __restrict__ qpos,
                                                                  const float* __restrict__ qvel,
                                                                  const float* __restrict__ aux, float* ctl,
                                                                  float* __restrict__ obs, float* __restrict__ acc,
                                                                  float* __restrict__ alive) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x % FLEET_TEAM;
  const int e0 = blockIdx.x * (FLEET_TPB / FLEET_TEAM) + threadIdx.x / FLEET_TEAM;
  const bool on = e0 < n;
  const size_t e = on ? e0 : n - 1, N = n;
  const int shift = (threadIdx.x % 64) / FLEET_TEAM * FLEET_TEAM;  // this group's bits of a wave vote
  const int nu = D.nu, C = DUCK_FLEET_CTL_SIZE(nu), O = DUCK_FLEET_OBS_SIZE(nu);
  float* c = ctl + e * C;
  const float* sens = aux + (size_t)D.sens_off * N + e;

  // mujoco_infer.py:175-197
  float ii = c[DUCK_FLEET_CTL_IMITATION_I(nu)], ph0 = c[DUCK_FLEET_CTL_IMITATION_PHASE(nu)],
        ph1 = c[DUCK_FLEET_CTL_IMITATION_PHASE(nu) + 1];
  if (!D.standing) {
    const float nb = (float)D.nb_steps_in_period;
    ii = fmodf(ii + c[DUCK_FLEET_CTL_PHASE_FREQUENCY_FACTOR(nu)], nb);
    const float a = fleet_div_rn(ii, nb) * 6.2831855f;
    ph0 = cosf(a);
    ph1 = sinf(a);
  }

  // the feet: lanes 0-3 the left foot's four contact slots, 4-7 the right foot's
  bool pen = false;
  if (lane < 8) pen = aux[(size_t)(D.con_off + D.foot_con[lane / 4] + lane % 4) * N + e] < 0.f;
  const unsigned feet = (unsigned)(__ballot(pen) >> shift) & 0xffu;
  // a NaN anywhere in the state (joystick.py:483-485)
  bool bad = false;
  for (int k = lane; k < D.nq + D.nv; k += FLEET_TEAM) {
    const float v = k < D.nq ? qpos[(size_t)k * N + e] : qvel[(size_t)(k - D.nq) * N + e];
    bad |= v != v;
  }
  const bool nan_state = ((unsigned)(__ballot(bad) >> shift) & 0xffffu) != 0;

  // mujoco_infer.py:67-103, one column per lane and pass
  for (int k = lane; k < O; k += FLEET_TEAM) {
    float v;
    int j = k;
    if (j < 3) {
      v = sens[(size_t)(D.gyro + j) * N];
    } else if ((j -= 3) < 3) {
      v = sens[(size_t)(D.accelerometer + j) * N];
      if (j == 0) v = v + D.accel_x_offset;
    } else if ((j -= 3) < 7) {
      v = c[DUCK_FLEET_CTL_COMMAND(nu) + j];
    } else if ((j -= 7) < nu) {
      v = qpos[(size_t)D.act_qpos[j] * N + e] - D.act_default[j];
    } else if ((j -= nu) < nu) {
      v = qvel[(size_t)D.act_dof[j] * N + e] * D.dof_vel_scale;
    } else if ((j -= nu) < 4 * nu) {
      v = c[j];  // the three past actions, then the motor targets: relies on the record's order, [0, 4 nu)
    } else if ((j -= 4 * nu) < 2) {
      v = ((feet >> (4 * j)) & 0xfu) ? 1.f : 0.f;
    } else {
      v = j == 2 ? ph0 : ph1;
    }
    if (on) obs[e * O + k] = v;
  }

  if (on && lane == 0) {
    if (alive[e] != 0.f) {
      const float vx = sens[(size_t)D.local_linvel * N], vy = sens[(size_t)(D.local_linvel + 1) * N];
      const float wz = sens[(size_t)(D.gyro + 2) * N];
      if (nan_state || sens[(size_t)(D.upvector + 2) * N] < 0.f) {
        alive[e] = 0.f;
      } else {
        float* r = acc + e * DUCK_FLEET_ACC_SIZE;
        const int cmd = DUCK_FLEET_CTL_COMMAND(nu);
        const float dx = vx - c[cmd], dy = vy - c[cmd + 1], dz = wz - c[cmd + 2];
        const float dx2 = dx * dx, dy2 = dy * dy;
        r[0] += 1.f;
        r[1] += vx;
        r[2] += vy;
        r[3] += wz;
        r[4] += dx2 + dy2;
        r[5] += dz * dz;
      }
    }
    if (!D.standing) {
      c[DUCK_FLEET_CTL_IMITATION_I(nu)] = ii;
      c[DUCK_FLEET_CTL_IMITATION_PHASE(nu)] = ph0;
      c[DUCK_FLEET_CTL_IMITATION_PHASE(nu) + 1] = ph1;
    }
  }
}

// mujoco_infer.py:208-231 for actuator a of robot e: the history shift, the motor target from entry d of the
// shifted history (0: this period's action), the speed-limit clip, ctl and ctrl. Both actuate kernels are this
// body, so that with d == 0 the delayed one is the plain one bit for bit.
__device__ __forceinline__ void fleet_actuate_body(const duck_fleet_desc& D, int n, size_t e, int a, int d,
                                                   const float* __restrict__ action, float* ctl,
                                                   float* __restrict__ ctrl) {
#pragma clang fp contract(off)
  const int nu = D.nu;
  float* c = ctl + e * DUCK_FLEET_CTL_SIZE(nu);
  const float act = action[e * nu + a], last = c[DUCK_FLEET_CTL_ACTION(nu, 0) + a],
              last_last = c[DUCK_FLEET_CTL_ACTION(nu, 1) + a];
  c[DUCK_FLEET_CTL_ACTION(nu, 2) + a] = last_last;
  c[DUCK_FLEET_CTL_ACTION(nu, 1) + a] = last;
  c[DUCK_FLEET_CTL_ACTION(nu, 0) + a] = act;
  const float used = d == 0 ? act : (d == 1 ? last : last_last);  // entry d of the shifted history
  const float scaled = used * D.action_scale;
  float mt = D.act_default[a] + scaled;
  if (D.speed_limits) {
    const float prev = c[DUCK_FLEET_CTL_PREV_MOTOR_TARGETS(nu) + a];
    const float lo = prev - D.target_step, hi = prev + D.target_step;
    mt = mt < lo ? lo : mt;  // np.clip: a NaN target stays NaN
    mt = mt > hi ? hi : mt;
    c[DUCK_FLEET_CTL_PREV_MOTOR_TARGETS(nu) + a] = mt;
  }
  c[DUCK_FLEET_CTL_MOTOR_TARGETS(nu) + a] = mt;
  ctrl[(size_t)a * n + e] = mt;
}

// one lane per (robot, actuator)
__global__ __launch_bounds__(FLEET_TPB) void fleet_actuate_kernel(const duck_fleet_desc D, int n,
                                                                  const float* __restrict__ action, float* ctl,
                                                                  float* __restrict__ ctrl) {
  int a;
  size_t e;
  const int nu = D.nu;
  if (!fleet_place(n, a, e) || a >= nu) return;
  fleet_actuate_body(D, n, e, a, 0, action, ctl, ctrl);
}

// The loop's disturbances (include/duck_fleet.h: duck_fleet_disturb), the same 16-lane group per robot. Lane l
// takes the noise of the obs columns l, l + 16, ...: columns l + 32 j and l + 32 j + 16 are the two words of
// threefry block 1 + l + 16 j, evaluated once and only when one of the two has a scale. Lanes 0-6 copy the
// next period's command, lane 0 pushes the base and advances the tick. Every lane has read the tick (one
// load of the whole wave) before lane 0's store, which depends on it, can issue. No LDS, no votes: lanes
// past the last robot leave.
__device__ __forceinline__ float fleet_u23(uint32_t w) { return (float)(w >> 9) * (1.0f / 8388608.0f); }

__global__ __launch_bounds__(FLEET_TPB) void fleet_disturb_kernel(const duck_fleet_disturbance S, int nu, int noisy,
                                                                  int n, long long robot_offset, int* tick,
                                                                  const float* __restrict__ sched,
                                                                  const int* __restrict__ sched_id,
                                                                  const float* __restrict__ push,
                                                                  float* __restrict__ qvel, float* __restrict__ ctl,
                                                                  float* __restrict__ obs) {
#pragma clang fp contract(off)
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e)) return;
  const size_t N = n;
  const int C = DUCK_FLEET_CTL_SIZE(nu), O = DUCK_FLEET_OBS_SIZE(nu);
  const int p = tick[e], t = p + 1;
  Rng r;
  derive_key(S.seed, robot_offset + (long long)e, DUCK_FLEET_KEY_TAG, r.k0, r.k1);
  r.ctr = (uint32_t)p;

  if (noisy) {
    float* o = obs + e * O;
    for (int k = lane; k < O; k += 2 * FLEET_TEAM) {
      const int k1 = k + FLEET_TEAM;
      const float s0 = S.noise_scale[k], s1 = k1 < O ? S.noise_scale[k1] : 0.f;
      if (s0 != 0.f || s1 != 0.f) {
        uint32_t a, b;
        threefry2x32(r.k0, r.k1, r.ctr, 1u + (uint32_t)lane + (uint32_t)(k / (2 * FLEET_TEAM)) * FLEET_TEAM, a, b);
        if (s0 != 0.f) {
          const float d = (2.f * fleet_u23(a) - 1.f) * s0;
          o[k] = o[k] + d;
        }
        if (s1 != 0.f) {
          const float d = (2.f * fleet_u23(b) - 1.f) * s1;
          o[k1] = o[k1] + d;
        }
      }
    }
  }

  if (sched && lane < 7) {
    int id = sched_id[e], seg = t / S.seg_periods;
    id = id < 0 ? 0 : (id > S.n_sched - 1 ? S.n_sched - 1 : id);
    seg = seg < 0 ? 0 : (seg > S.n_seg - 1 ? S.n_seg - 1 : seg);  // (a negative tick reads segment 0, not before the table)
    ctl[e * C + DUCK_FLEET_CTL_COMMAND(nu) + lane] = sched[((size_t)id * S.n_seg + seg) * 7 + lane];
  }

  if (lane == 0) {
    if (push) {  // joystick.py:381-400
      const float* w = push + e * DUCK_FLEET_PUSH_SIZE;
      const int first = (int)w[0], interval = (int)w[1];
      if (first >= 1 && (t == first || (interval > 0 && t > first && (t - first) % interval == 0))) {
        uint32_t a, b;
        threefry2x32(r.k0, r.k1, r.ctr, 0u, a, b);
        const float dm = (w[3] - w[2]) * fleet_u23(a), dt = (w[5] - w[4]) * fleet_u23(b);
        const float mag = w[2] + dm, theta = w[4] + dt;
        const float dx = cosf(theta) * mag, dy = sinf(theta) * mag;
        qvel[e] = qvel[e] + dx;
        qvel[N + e] = qvel[N + e] + dy;
      }
    }
    tick[e] = t;
  }
}

// The flight recorder (include/duck_fleet.h: duck_fleet_record), the same 16-lane group per robot. The lanes
// stride over the frame's words: word k's source is found by walking the fields in the frame's order; the SoA
// rows are read next to the neighbouring groups', the robot's own rows and the frame in runs of 16 consecutive
// words. Words travel as uint32_t: a copy, whatever the bits. Every lane of a group loads head, after and alive
// (one broadcast load each), so the frozen exit is taken by the whole group; lane 0 stores the two counters at
// the end, after the wave's loads of them (fleet_disturb_kernel's argument for tick). No LDS, no votes: lanes
// past the last robot leave.
__global__ __launch_bounds__(FLEET_TPB) void fleet_record_kernel(
    const duck_fleet_desc D, int n, int depth, int post, const uint32_t* __restrict__ qpos,
    const uint32_t* __restrict__ qvel, const uint32_t* __restrict__ warm, const uint32_t* __restrict__ aux,
    const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ obs, const uint32_t* __restrict__ action,
    const float* __restrict__ alive, int* head, int* after, uint32_t* __restrict__ ring) {
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e)) return;
  const size_t N = n;
  const int h = head[e], af = after[e];
  const bool dead = alive[e] == 0.f;
  if (dead && af > post) return;  // frozen
  const int nq = D.nq, nv = D.nv, nu = D.nu, C = DUCK_FLEET_CTL_SIZE(nu), O = DUCK_FLEET_OBS_SIZE(nu);
  const int F = DUCK_FLEET_FRAME_SIZE(nq, nv, nu);
  // (unsigned: a head the caller did not zero, or one past 2^31 calls, still lands inside the robot's ring)
  uint32_t* frame = ring + (e * (size_t)depth + (size_t)((unsigned)h % (unsigned)depth)) * F;
  for (int k = lane; k < F; k += FLEET_TEAM) {
    uint32_t v;
    int j = k;
    if (j < nq) {
      v = qpos[(size_t)j * N + e];
    } else if ((j -= nq) < nv) {
      v = qvel[(size_t)j * N + e];
    } else if ((j -= nv) < nv) {
      v = warm[(size_t)j * N + e];
    } else if ((j -= nv) < C) {
      v = ctl[e * C + j];
    } else if ((j -= C) < O) {
      v = obs[e * O + j];
    } else if ((j -= O) < nu) {
      v = action[e * nu + j];
    } else if ((j -= nu) < nu) {
      v = aux[(size_t)(4 * nv + j) * N + e];  // actuator_force
    } else {
      j -= nu;
      const int s = j / 3;
      const int adr = s == 0 ? D.gyro : s == 1 ? D.accelerometer : s == 2 ? D.upvector : D.local_linvel;
      v = aux[(size_t)(D.sens_off + adr + j % 3) * N + e];
    }
    frame[k] = v;
  }
  if (lane == 0) {
    head[e] = h + 1;
    if (dead) after[e] = af + 1;
  }
}

// The loop's latency (include/duck_fleet.h: duck_fleet_sense_delay, duck_fleet_sensor_delay,
// duck_fleet_actuate_delayed), the same 16-lane group per robot. Every lane of a group loads the robot's counter
// and its row of the table (broadcast loads) and evaluates the threefry block itself when the row asks for a
// draw, so the delay is a value of the whole group with no LDS and no votes. A bad row is clamped: lo into
// [0, MAX_DELAY], hi into [lo, MAX_DELAY]. `pair` is the {lo, hi} of one delay; its draw is word `word` of block
// `block` of period p (both constants at every call, so each kernel holds the one block it needs).
__device__ __forceinline__ int fleet_delay(const int* __restrict__ pair, uint32_t block, int word,
                                           unsigned long long seed, long long id, uint32_t p) {
  int lo = pair[0], hi = pair[1];
  lo = lo < 0 ? 0 : (lo > DUCK_FLEET_MAX_DELAY ? DUCK_FLEET_MAX_DELAY : lo);
  hi = hi < lo ? lo : (hi > DUCK_FLEET_MAX_DELAY ? DUCK_FLEET_MAX_DELAY : hi);
  if (hi == lo) return lo;
  uint32_t k0, k1, w0, w1;
  derive_key(seed, id, DUCK_FLEET_LAT_TAG, k0, k1);
  threefry2x32(k0, k1, p, block, w0, w1);
  return lo + (int)((((word ? w1 : w0) >> 9) * (uint32_t)(hi - lo + 1)) >> 23);
}

// Lanes 0-5 carry the six IMU words: into the line's slot p % 3, then, when the delay reaches back, out of the
// slot an earlier period's launch wrote. lat_tick is read only.
__global__ __launch_bounds__(FLEET_TPB) void fleet_sense_delay_kernel(int nu, int n, unsigned long long seed,
                                                                      long long robot_offset,
                                                                      const int* __restrict__ lat_tick,
                                                                      const int* __restrict__ lat, uint32_t* line,
                                                                      uint32_t* obs) {
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e) || lane >= 6) return;
  const int p0 = lat_tick[e];
  const uint32_t p = p0 < 0 ? 0u : (uint32_t)p0;
  const int d = fleet_delay(lat + e * DUCK_FLEET_LAT_SIZE + 2, 0u, 1, seed, robot_offset + (long long)e, p);
  const uint32_t fill = p < (uint32_t)DUCK_FLEET_MAX_DELAY ? p : (uint32_t)DUCK_FLEET_MAX_DELAY;
  const uint32_t d_eff = (uint32_t)d < fill ? (uint32_t)d : fill;
  constexpr uint32_t SLOTS = DUCK_FLEET_MAX_DELAY + 1;
  uint32_t* o = obs + e * DUCK_FLEET_OBS_SIZE(nu) + lane;
  uint32_t* l = line + e * (SLOTS * 6) + lane;
  l[(p % SLOTS) * 6] = *o;
  if (d_eff > 0) *o = l[((p - d_eff) % SLOTS) * 6];
}

// fleet_sense_delay_kernel and, by its rule, the joint encoders: lanes 0-5 carry the six IMU words, lane l the
// encoder words l and l + 16 of obs columns 13 .. 13 + 2 nu - 1, each when < 2 nu (nu <= 16: at most two a lane).
// The IMU delay is word 1 of block 0, the encoder delay word 0 of block 1; a fixed row evaluates neither.
// lat_tick is read only.
__global__ __launch_bounds__(FLEET_TPB) void fleet_sensor_delay_kernel(int nu, int n, unsigned long long seed,
                                                                       long long robot_offset,
                                                                       const int* __restrict__ lat_tick,
                                                                       const int* __restrict__ lat,
                                                                       const int* __restrict__ enc, uint32_t* line,
                                                                       uint32_t* eline, uint32_t* obs) {
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e)) return;
  const int p0 = lat_tick[e];
  const uint32_t p = p0 < 0 ? 0u : (uint32_t)p0;
  const long long id = robot_offset + (long long)e;
  const int ds = fleet_delay(lat + e * DUCK_FLEET_LAT_SIZE + 2, 0u, 1, seed, id, p);
  const int de = fleet_delay(enc + e * DUCK_FLEET_ENC_SIZE, 1u, 0, seed, id, p);
  const uint32_t fill = p < (uint32_t)DUCK_FLEET_MAX_DELAY ? p : (uint32_t)DUCK_FLEET_MAX_DELAY;
  const uint32_t s_eff = (uint32_t)ds < fill ? (uint32_t)ds : fill;
  const uint32_t e_eff = (uint32_t)de < fill ? (uint32_t)de : fill;
  constexpr uint32_t SLOTS = DUCK_FLEET_MAX_DELAY + 1;
  const uint32_t now = p % SLOTS;
  uint32_t* o = obs + e * DUCK_FLEET_OBS_SIZE(nu);
  if (lane < 6) {
    uint32_t* l = line + e * (SLOTS * 6) + lane;
    l[now * 6] = o[lane];
    if (s_eff > 0) o[lane] = l[((p - s_eff) % SLOTS) * 6];
  }
  const uint32_t W = 2 * (uint32_t)nu;
  uint32_t* el = eline + e * (SLOTS * W);
  const uint32_t then = (p - e_eff) % SLOTS;
  for (uint32_t k = lane; k < W; k += FLEET_TEAM) {
    el[now * W + k] = o[13 + k];
    if (e_eff > 0) o[13 + k] = el[then * W + k];
  }
}

// fleet_actuate_kernel on history entry d. Every lane has read the counter (one load of the whole wave) before
// lane 0's store, which depends on it, can issue; it is the kernel's last store.
__global__ __launch_bounds__(FLEET_TPB) void fleet_actuate_delayed_kernel(const duck_fleet_desc D, int n,
                                                                          unsigned long long seed,
                                                                          long long robot_offset, int* lat_tick,
                                                                          const int* __restrict__ lat,
                                                                          const float* __restrict__ action,
                                                                          float* ctl, float* __restrict__ ctrl) {
  int a;
  size_t e;
  if (!fleet_place(n, a, e)) return;
  const int p0 = lat_tick[e];
  if (a >= D.nu) return;
  const int d = fleet_delay(lat + e * DUCK_FLEET_LAT_SIZE, 0u, 0, seed, robot_offset + (long long)e,
                            p0 < 0 ? 0u : (uint32_t)p0);
  fleet_actuate_body(D, n, e, a, d, action, ctl, ctrl);
  if (a == 0) lat_tick[e] = (int)((uint32_t)p0 + 1u);
}

// Following a log (include/duck_fleet.h: duck_fleet_follow), the same 16-lane group per robot, in
// duck_policy_act's place. The lanes stride over the observation columns, reading the log's row and the robot's
// obs and score rows in runs of 16 consecutive words; lanes < nu carry the actions, lanes 0-6 the next period's
// command. Log words travel as uint32_t: the actions and the command are copies, whatever the bits. Every lane
// has read the tick (one load of the whole wave) before lane 0's store, which depends on it, can issue; it is
// the kernel's last store. No LDS, no votes: lanes past the last robot leave.
__global__ __launch_bounds__(FLEET_TPB) void fleet_follow_kernel(int nu, int n, int n_log, int T,
                                                                 const uint32_t* __restrict__ log,
                                                                 const int* __restrict__ log_id, int* log_tick,
                                                                 const float* __restrict__ obs,
                                                                 float* __restrict__ score, uint32_t* __restrict__ ctl,
                                                                 uint32_t* __restrict__ action) {
#pragma clang fp contract(off)
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e)) return;
  const int O = DUCK_FLEET_OBS_SIZE(nu), W = DUCK_FLEET_LOG_SIZE(nu), C = DUCK_FLEET_CTL_SIZE(nu);
  const int p0 = log_tick[e], p = p0 < 0 ? 0 : p0;
  int id = log_id[e];
  id = id < 0 ? 0 : (id > n_log - 1 ? n_log - 1 : id);
  const bool inside = p < T;
  // (row p of the robot's log; past the end the pointer is not formed from p, nor read)
  const uint32_t* row = log + ((size_t)id * (size_t)T + (size_t)(inside ? p : 0)) * W;
  if (inside) {
    const float* o = obs + e * O;
    float* s = score + e * O;
    for (int k = lane; k < O; k += FLEET_TEAM) {
      const float r = __uint_as_float(row[k]);
      if (r == r) {
        const float d = o[k] - r;
        const float q = d * d;
        s[k] = s[k] + q;
      }
    }
  }
  if (lane < nu) action[e * nu + lane] = inside ? row[O + lane] : 0u;
  if (lane < 7 && p < T - 1) ctl[e * C + DUCK_FLEET_CTL_COMMAND(nu) + lane] = row[W + 6 + lane];
  if (lane == 0) log_tick[e] = inside ? p + 1 : T;
}

// Gait and servo load (include/duck_fleet.h: duck_fleet_gait), the same 16-lane group per robot, after the
// actuation. Lane a < nu carries actuator a through the seven per-actuator blocks of the record, so the group reads
// and writes runs of nu consecutive words of the robot's row, and reads the actuator_force and qvel rows next to
// the neighbouring groups'. Lanes 0 and 1 also carry the left and the right foot (six consecutive words each;
// both look at both feet's contact slots, eight loads of a wave either way), lane 0 the three whole-body words.
// Every lane has read the periods word, which tells `first` (one load of the whole wave), before lane 0's store
// of it, which depends on that load, can issue; it is the robot's last store. A dead robot's group leaves before
// any store. No LDS, no votes: lanes past the last robot leave.
__global__ __launch_bounds__(FLEET_TPB) void fleet_gait_kernel(const duck_fleet_desc D, const duck_fleet_gait_desc S,
                                                               int n, const float* __restrict__ qvel,
                                                               const float* __restrict__ aux,
                                                               const float* __restrict__ ctl,
                                                               const float* __restrict__ alive, float* gait) {
#pragma clang fp contract(off)
  int lane;
  size_t e;
  if (!fleet_place(n, lane, e)) return;
  if (alive[e] == 0.f) return;
  const size_t N = n;
  const int nu = D.nu, B = DUCK_FLEET_GAIT_PERIODS(nu);
  float* g = gait + e * DUCK_FLEET_GAIT_SIZE(nu);
  const float periods = g[B];
  const bool first = periods == 0.f;
  if (lane < nu) {
    const int a = lane;
    const float* c = ctl + e * DUCK_FLEET_CTL_SIZE(nu);
    const float f = aux[(size_t)(4 * D.nv + a) * N + e], w = qvel[(size_t)D.act_dof[a] * N + e];
    const float af = __builtin_fabsf(f), aw = __builtin_fabsf(w);
    const float ff = f * f, fw = f * w;
    const float d = c[DUCK_FLEET_CTL_ACTION(nu, 0) + a] - c[DUCK_FLEET_CTL_ACTION(nu, 1) + a];
    const float dd = d * d;
    float* r = g + a;
    const float fmax = r[DUCK_FLEET_GAIT_FORCE_MAX(nu)], wmax = r[DUCK_FLEET_GAIT_SPEED_MAX(nu)];
    r[DUCK_FLEET_GAIT_FORCE_SQ(nu)] = r[DUCK_FLEET_GAIT_FORCE_SQ(nu)] + ff;
    r[DUCK_FLEET_GAIT_FORCE_MAX(nu)] = af > fmax ? af : fmax;  // a NaN never enters
    if (af >= S.force_sat[a]) r[DUCK_FLEET_GAIT_FORCE_SAT(nu)] = r[DUCK_FLEET_GAIT_FORCE_SAT(nu)] + 1.f;
    r[DUCK_FLEET_GAIT_SPEED_MAX(nu)] = aw > wmax ? aw : wmax;
    if (aw >= S.speed_sat) r[DUCK_FLEET_GAIT_SPEED_SAT(nu)] = r[DUCK_FLEET_GAIT_SPEED_SAT(nu)] + 1.f;
    r[DUCK_FLEET_GAIT_WORK(nu)] = r[DUCK_FLEET_GAIT_WORK(nu)] + __builtin_fabsf(fw);
    r[DUCK_FLEET_GAIT_ACTION_RATE(nu)] = r[DUCK_FLEET_GAIT_ACTION_RATE(nu)] + dd;
  }
  if (lane < 2) {
    // duck_fleet_observe's contact of both feet
    const float* l = aux + (size_t)(D.con_off + D.foot_con[0]) * N + e;
    const float* r4 = aux + (size_t)(D.con_off + D.foot_con[1]) * N + e;
    const bool c0 = (l[0] < 0.f) | (l[N] < 0.f) | (l[2 * N] < 0.f) | (l[3 * N] < 0.f);
    const bool c1 = (r4[0] < 0.f) | (r4[N] < 0.f) | (r4[2 * N] < 0.f) | (r4[3 * N] < 0.f);
    const bool cf = lane ? c1 : c0;
    const float* sens = aux + (size_t)D.sens_off * N + e;
    const int lin = lane ? S.foot_linvel[1] : S.foot_linvel[0], pos = lane ? S.foot_pos[1] : S.foot_pos[0];
    float* r = g + DUCK_FLEET_GAIT_FOOT(nu, lane);
    const float prev = r[DUCK_FLEET_GAIT_FOOT_PREV], apex = r[DUCK_FLEET_GAIT_FOOT_APEX];
    const float z = sens[(size_t)(pos + 2) * N];
    const bool touchdown = !first && prev == 0.f && cf, liftoff = !first && prev != 0.f && !cf;
    if (cf) {
      const float vx = sens[(size_t)lin * N], vy = sens[(size_t)(lin + 1) * N];
      const float xx = vx * vx, yy = vy * vy;
      const float s = xx + yy;
      r[DUCK_FLEET_GAIT_FOOT_CONTACT] = r[DUCK_FLEET_GAIT_FOOT_CONTACT] + 1.f;
      r[DUCK_FLEET_GAIT_FOOT_SLIP] = r[DUCK_FLEET_GAIT_FOOT_SLIP] + s;
    } else {
      r[DUCK_FLEET_GAIT_FOOT_APEX] = (first || liftoff) ? z : (z > apex ? z : apex);
    }
    if (touchdown) {
      const float h = apex - z;
      r[DUCK_FLEET_GAIT_FOOT_TOUCHDOWNS] = r[DUCK_FLEET_GAIT_FOOT_TOUCHDOWNS] + 1.f;
      r[DUCK_FLEET_GAIT_FOOT_APEX_SUM] = r[DUCK_FLEET_GAIT_FOOT_APEX_SUM] + h;
    }
    r[DUCK_FLEET_GAIT_FOOT_PREV] = cf ? 1.f : 0.f;
    if (lane == 0) {
      if (c0 && c1) g[DUCK_FLEET_GAIT_DOUBLE_SUPPORT(nu)] = g[DUCK_FLEET_GAIT_DOUBLE_SUPPORT(nu)] + 1.f;
      if (!c0 && !c1) g[DUCK_FLEET_GAIT_FLIGHT(nu)] = g[DUCK_FLEET_GAIT_FLIGHT(nu)] + 1.f;
      g[B] = periods + 1.f;
    }
  }
}

static const char* fleet_desc_error(const duck_fleet_desc* d) {
  if (d->nq < 1 || d->nv < 1 || d->nu < 1 || d->nu > DUCK_FLEET_MAX_NU) return "nq, nv >= 1 and 1 <= nu <= 16";
  for (int a = 0; a < d->nu; a++)
    if (d->act_qpos[a] < 0 || d->act_qpos[a] >= d->nq || d->act_dof[a] < 0 || d->act_dof[a] >= d->nv)
      return "actuator address outside qpos / qvel";
  return nullptr;
}

// The checks every fleet entry shares, in their order: the pointers (`null`: one of the entry's is), N's range,
// `own` (the entry's own complaint about its sizes, or nullptr), the descriptor.
static int fleet_check(const char* entry, bool null, const duck_fleet_desc* d, int n, const char* own = nullptr) {
  const char* why = own;
  if (null || !d) why = "null pointer";
  else if (n < 0 || n > (1 << 27)) why = "bad size (0 <= N <= 2^27)";
  else if (!own) why = fleet_desc_error(d);
  return why ? duck_fail(DUCK_EINVAL, std::string(entry) + ": " + why) : DUCK_OK;
}

// every sensor row duck_fleet_observe and duck_fleet_record read lies inside the aux record
static bool fleet_sensors_inside(const duck_fleet_desc* d) {
  for (int s : {d->gyro, d->accelerometer, d->upvector, d->local_linvel})
    if (s < 0 || d->sens_off < 0 || (long long)d->sens_off + s + 3 > d->naux) return false;
  return true;
}

// a 16-lane group per robot, FLEET_TPB threads a block; N == 0 launches nothing
template <typename... P, typename... A>
static int fleet_launch(void (*kernel)(P...), int n, void* stream, A... args) {
  if (n == 0) return DUCK_OK;
  const int per = FLEET_TPB / FLEET_TEAM;
  hipLaunchKernelGGL(kernel, dim3((n + per - 1) / per), dim3(FLEET_TPB), 0, (hipStream_t)stream, args...);
  HIPCHECK(hipGetLastError());
  return DUCK_OK;
}
}  // namespace

extern "C" {

int duck_episode_accumulate(int n, int nmetrics, const float* reward, const float* done, const float* metrics,
                            int metrics_stride, int mode, float* run, float* fin, float* flag, void* stream) {
  if (n < 0 || nmetrics < 0 || (nmetrics > 0 && metrics_stride < n))
    return duck_fail(DUCK_EINVAL, "duck_episode_accumulate: bad size");
  if (mode != DUCK_EPISODE_EVAL && mode != DUCK_EPISODE_TRAIN)
    return duck_fail(DUCK_EINVAL, "duck_episode_accumulate: mode must be DUCK_EPISODE_EVAL or DUCK_EPISODE_TRAIN");
  if (n == 0) return DUCK_OK;
  if (!reward || !done || (nmetrics > 0 && !metrics) || !run || !flag || (mode == DUCK_EPISODE_TRAIN && !fin))
    return duck_fail(DUCK_EINVAL, "duck_episode_accumulate: null pointer");
  hipLaunchKernelGGL(episode_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, nmetrics,
                     reward, done, metrics, metrics_stride, mode, run, fin, flag);
  HIPCHECK(hipGetLastError());
  return DUCK_OK;
}

int duck_fleet_observe(const duck_fleet_desc* d, int n, const float* qpos, const float* qvel, const float* aux,
                       float* ctl, float* obs, float* acc, float* alive, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_observe", !qpos || !qvel || !aux || !ctl || !obs || !acc || !alive, d, n))
    return rc;
  if (!fleet_sensors_inside(d))
    return duck_fail(DUCK_EINVAL, "duck_fleet_observe: sensor address outside the aux record");
  for (int f : d->foot_con)
    if (f < 0 || d->con_off < 0 || (long long)d->con_off + f + 4 > d->naux)
      return duck_fail(DUCK_EINVAL, "duck_fleet_observe: contact slot outside the aux record");
  if (!d->standing && d->nb_steps_in_period < 1)
    return duck_fail(DUCK_EINVAL, "duck_fleet_observe: nb_steps_in_period must be >= 1 unless standing");
  return fleet_launch(fleet_observe_kernel, n, stream, *d, n, qpos, qvel, aux, ctl, obs, acc, alive);
}

int duck_fleet_actuate(const duck_fleet_desc* d, int n, const float* action, float* ctl, float* ctrl, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_actuate", !action || !ctl || !ctrl, d, n)) return rc;
  return fleet_launch(fleet_actuate_kernel, n, stream, *d, n, action, ctl, ctrl);
}

int duck_fleet_disturb(const duck_fleet_desc* d, const duck_fleet_disturbance* dis, int n, int64_t robot_offset,
                       int32_t* tick, const float* sched, const int32_t* sched_id, const float* push, float* qvel,
                       float* ctl, float* obs, void* stream) {
  g_err.clear();
  // (the schedule's complaints come before N's, so the pointers are looked at here)
  if (!d || !dis || !tick || !qvel || !ctl || !obs) return duck_fail(DUCK_EINVAL, "duck_fleet_disturb: null pointer");
  if (sched && !sched_id) return duck_fail(DUCK_EINVAL, "duck_fleet_disturb: a schedule needs sched_id");
  if (sched && (dis->n_sched < 1 || dis->n_seg < 1 || dis->seg_periods < 1))
    return duck_fail(DUCK_EINVAL, "duck_fleet_disturb: a schedule needs n_sched, n_seg, seg_periods >= 1");
  if (int rc = fleet_check("duck_fleet_disturb", false, d, n)) return rc;
  if (push && d->nv < 2) return duck_fail(DUCK_EINVAL, "duck_fleet_disturb: a push table needs nv >= 2");
  int noisy = 0;
  for (int k = 0; k < DUCK_FLEET_OBS_SIZE(d->nu); k++) noisy |= dis->noise_scale[k] != 0.f;
  return fleet_launch(fleet_disturb_kernel, n, stream, *dis, d->nu, noisy, n, (long long)robot_offset, tick, sched,
                      sched_id, push, qvel, ctl, obs);
}

int duck_fleet_record(const duck_fleet_desc* d, int n, int depth, int post, const float* qpos, const float* qvel,
                      const float* warm, const float* aux, const float* ctl, const float* obs, const float* action,
                      const float* alive, int32_t* head, int32_t* after, float* ring, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_record",
                           !qpos || !qvel || !warm || !aux || !ctl || !obs || !action || !alive || !head || !after || !ring,
                           d, n, depth < 1 || post < 0 ? "depth >= 1 and post >= 0" : nullptr))
    return rc;
  if (!fleet_sensors_inside(d))
    return duck_fail(DUCK_EINVAL, "duck_fleet_record: sensor address outside the aux record");
  if (4LL * d->nv + d->nu > d->naux)
    return duck_fail(DUCK_EINVAL, "duck_fleet_record: actuator_force rows (4 nv + nu) outside the aux record");
  return fleet_launch(fleet_record_kernel, n, stream, *d, n, depth, post, (const uint32_t*)qpos, (const uint32_t*)qvel,
                      (const uint32_t*)warm, (const uint32_t*)aux, (const uint32_t*)ctl, (const uint32_t*)obs,
                      (const uint32_t*)action, alive, head, after, (uint32_t*)ring);
}

int duck_fleet_sense_delay(const duck_fleet_desc* d, int n, uint64_t seed, int64_t robot_offset, const int32_t* lat_tick,
                           const int32_t* lat, float* line, float* obs, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_sense_delay", !lat_tick || !lat || !line || !obs, d, n)) return rc;
  return fleet_launch(fleet_sense_delay_kernel, n, stream, d->nu, n, (unsigned long long)seed, (long long)robot_offset,
                      lat_tick, lat, (uint32_t*)line, (uint32_t*)obs);
}

int duck_fleet_sensor_delay(const duck_fleet_desc* d, int n, uint64_t seed, int64_t robot_offset, const int32_t* lat_tick,
                            const int32_t* lat, const int32_t* enc, float* line, float* eline, float* obs, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_sensor_delay", !lat_tick || !lat || !enc || !line || !eline || !obs, d, n))
    return rc;
  return fleet_launch(fleet_sensor_delay_kernel, n, stream, d->nu, n, (unsigned long long)seed, (long long)robot_offset,
                      lat_tick, lat, enc, (uint32_t*)line, (uint32_t*)eline, (uint32_t*)obs);
}

int duck_fleet_actuate_delayed(const duck_fleet_desc* d, int n, uint64_t seed, int64_t robot_offset, int32_t* lat_tick,
                               const int32_t* lat, const float* action, float* ctl, float* ctrl, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_actuate_delayed", !lat_tick || !lat || !action || !ctl || !ctrl, d, n)) return rc;
  return fleet_launch(fleet_actuate_delayed_kernel, n, stream, *d, n, (unsigned long long)seed, (long long)robot_offset,
                      lat_tick, lat, action, ctl, ctrl);
}

int duck_fleet_follow(const duck_fleet_desc* d, int n, int n_log, int T, const float* log, const int32_t* log_id,
                      int32_t* log_tick, const float* obs, float* score, float* ctl, float* action, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_follow", !log || !log_id || !log_tick || !obs || !score || !ctl || !action, d, n,
                           n_log < 1 || T < 1 ? "a log needs n_log >= 1 and T >= 1" : nullptr))
    return rc;
  return fleet_launch(fleet_follow_kernel, n, stream, d->nu, n, n_log, T, (const uint32_t*)log, log_id, log_tick, obs,
                      score, (uint32_t*)ctl, (uint32_t*)action);
}

int duck_fleet_gait(const duck_fleet_desc* d, const duck_fleet_gait_desc* s, int n, const float* qvel, const float* aux,
                    const float* ctl, const float* alive, float* gait, void* stream) {
  g_err.clear();
  if (int rc = fleet_check("duck_fleet_gait", !s || !qvel || !aux || !ctl || !alive || !gait, d, n)) return rc;
  if (!fleet_sensors_inside(d))
    return duck_fail(DUCK_EINVAL, "duck_fleet_gait: sensor address outside the aux record");
  for (int f : d->foot_con)
    if (f < 0 || d->con_off < 0 || (long long)d->con_off + f + 4 > d->naux)
      return duck_fail(DUCK_EINVAL, "duck_fleet_gait: contact slot outside the aux record");
  if (4LL * d->nv + d->nu > d->naux)
    return duck_fail(DUCK_EINVAL, "duck_fleet_gait: actuator_force rows (4 nv + nu) outside the aux record");
  for (int adr : {s->foot_linvel[0], s->foot_linvel[1], s->foot_pos[0], s->foot_pos[1]})
    if (adr < 0 || (long long)d->sens_off + adr + 3 > d->con_off)
      return duck_fail(DUCK_EINVAL, "duck_fleet_gait: foot sensor address outside the sensordata rows");
  return fleet_launch(fleet_gait_kernel, n, stream, *d, *s, n, qvel, aux, ctl, alive, gait);
}

uint64_t duck_model_fingerprint(const duck_model_desc* m) {
  if (!m) return 0;
  Fnv f;
  const int nb = m->nbody, nj = m->njnt, nv = m->nv, ng = m->ngeom, np = m->npair, ns = m->nsite, nu = m->nu;
  const int sizes[] = {m->nq, m->nv, m->nu, m->nbody, m->njnt, m->ngeom, m->nsite, m->nsensor, m->nsensordata,
                       m->npair, m->iterations, m->ls_iterations, m->eulerdamp};
  f.i32(sizes, 13);
  const double opt[] = {m->timestep, m->gravity[0], m->gravity[1], m->gravity[2], m->impratio, m->tolerance,
                        m->ls_tolerance, m->meaninertia};
  f.f32(opt, 8);
  f.i32(m->body_parentid, nb); f.i32(m->body_rootid, nb); f.i32(m->body_weldid, nb); f.i32(m->body_jntnum, nb);
  f.i32(m->body_jntadr, nb); f.i32(m->body_dofnum, nb); f.i32(m->body_dofadr, nb);
  f.f32(m->body_pos, 3 * nb); f.f32(m->body_quat, 4 * nb); f.f32(m->body_ipos, 3 * nb); f.f32(m->body_iquat, 4 * nb);
  f.f32(m->body_mass, nb); f.f32(m->body_inertia, 3 * nb); f.f32(m->body_invweight0, 2 * nb);
  f.i32(m->jnt_type, nj); f.i32(m->jnt_qposadr, nj); f.i32(m->jnt_dofadr, nj); f.i32(m->jnt_bodyid, nj);
  f.i32(m->jnt_limited, nj);
  f.f32(m->jnt_pos, 3 * nj); f.f32(m->jnt_axis, 3 * nj); f.f32(m->jnt_range, 2 * nj); f.f32(m->jnt_margin, nj);
  f.f32(m->jnt_solref, 2 * nj); f.f32(m->jnt_solimp, 5 * nj);
  f.i32(m->dof_bodyid, nv); f.i32(m->dof_jntid, nv); f.i32(m->dof_parentid, nv);
  f.f32(m->dof_armature, nv); f.f32(m->dof_damping, nv); f.f32(m->dof_frictionloss, nv); f.f32(m->dof_invweight0, nv);
  f.f32(m->dof_solref, 2 * nv); f.f32(m->dof_solimp, 5 * nv);
  f.i32(m->geom_type, ng); f.i32(m->geom_bodyid, ng); f.i32(m->geom_dataid, ng);
  f.f32(m->geom_pos, 3 * ng); f.f32(m->geom_quat, 4 * ng); f.f32(m->geom_rbound, ng); f.f32(m->geom_size, 3 * ng);
  f.i32(m->pair_geom1, np); f.i32(m->pair_geom2, np); f.i32(m->pair_condim, np);
  f.f32(m->pair_friction, 5 * np); f.f32(m->pair_solref, 2 * np); f.f32(m->pair_solimp, 5 * np);
  f.f32(m->pair_margin, np);
  const int hull[] = {m->hull_nvert, m->hull_nface, m->hull_nedge, m->hfield_nrow, m->hfield_ncol};
  f.i32(hull, 5);
  f.f32(m->hull_vert, 3 * m->hull_nvert); f.f32(m->hull_face_normal, 3 * m->hull_nface);
  f.f32(m->hull_face_offset, m->hull_nface); f.i32(m->hull_edge, 2 * m->hull_nedge);
  f.f32(m->hfield_size, 4);  // the elevation itself is uploaded by duck_create, not baked
  f.i32(m->site_bodyid, ns); f.f32(m->site_pos, 3 * ns); f.f32(m->site_quat, 4 * ns);
  f.i32(m->actuator_trnid, nu); f.i32(m->actuator_ctrllimited, nu); f.i32(m->actuator_forcelimited, nu);
  f.f32(m->actuator_kp, nu); f.f32(m->actuator_kv, nu); f.f32(m->actuator_gear, nu);
  f.f32(m->actuator_ctrlrange, 2 * nu); f.f32(m->actuator_forcerange, 2 * nu);
  f.i32(m->sensor_type, m->nsensor); f.i32(m->sensor_objid, m->nsensor); f.i32(m->sensor_adr, m->nsensor);
  f.i32(m->sensor_dim, m->nsensor);
  f.f32(m->qpos0, m->nq);
  return f.h;
}

int duck_version(void) { return DUCK_VERSION; }

#ifndef DUCK_BUILD_ID
#define DUCK_BUILD_ID "unknown"
#endif
const char* duck_build_id(void) { return DUCK_BUILD_ID; }

int duck_model_supported(const duck_model_desc* model) {
  if (!model) return 0;
  for (int i = 0; i < kNumVariants; i++)
    if (kVariants[i]->matches(model)) return 1;
  return 0;
}
const char* duck_last_error(void) { return g_err.c_str(); }

int duck_layout_get(int nq, int nv, int nu, int imitation, int task, duck_layout* out) {
  if (!out) return duck_fail(DUCK_EINVAL, "null out");
  *out = duck_layout_make(nq, nv, nu, imitation, task);
  return DUCK_OK;
}

int duck_aux_size(const duck_sim* sim) {
  if (!sim) return duck_fail(DUCK_EINVAL, "null sim");
  return kVariants[sim->variant]->aux_size();
}

void duck_destroy(duck_sim* s) {
  if (!s) return;
  if (s->frames_d) (void)hipFree(s->frames_d);
  if (s->hfield_d) (void)hipFree(s->hfield_d);
  if (s->err_h) (void)hipHostFree((void*)s->err_h);
  delete s;
}

int duck_create(const duck_model_desc* model, const duck_env_config* cfg, const duck_refmotion* ref, int device,
                duck_sim** out) {
  g_err.clear();
  if (!model || !cfg || !out) return duck_fail(DUCK_EINVAL, "null argument");
  int v = -1;
  for (int i = 0; i < kNumVariants && v < 0; i++)
    if (kVariants[i]->matches(model)) v = i;
  if (v < 0)
    return duck_fail(DUCK_EUNSUPPORTED,
                     "no kernel of this library is compiled for this model (duck_model_fingerprint differs); "
                     "compile one with native.model_library / codegen");
  if (cfg->use_imitation && !ref) return duck_fail(DUCK_EINVAL, "use_imitation requires a reference-motion table");
  if (cfg->n_substeps < 1 || cfg->action_max_delay < 1 || cfg->action_max_delay > 3)
    return duck_fail(DUCK_EINVAL, "bad config (n_substeps >= 1, 1 <= action_max_delay <= 3)");
  // the throughput kernel must fit; a latency split that does not is simply not compiled (lds 0)
  if (kVariants[v]->lds_bytes() > 160 * 1024) return duck_fail(DUCK_EUNSUPPORTED, "per-workgroup LDS over 160 KiB");
  // the elevation is uploaded here, not baked (the fingerprint covers nrow / ncol / size only)
  if (kVariants[v]->floor_type == 1 && (!model->hfield_data || model->hfield_nrow < 2 || model->hfield_ncol < 2))
    return duck_fail(DUCK_EINVAL, "height-field model without hfield_data [nrow >= 2][ncol >= 2]");
  HIPCHECK(hipSetDevice(device));
  duck_sim* s = new duck_sim();
  memset(s, 0, sizeof(*s));
  s->device = device;
  s->variant = v;
  s->step_mode = DUCK_STEP_AUTO;
  s->lat_ok = kVariants[v]->lds_bytes_lat() != 0;
  s->lat2_ok = kVariants[v]->lds_bytes_lat2() != 0;
  s->latx2_ok = kVariants[v]->lds_bytes_lat_x2() != 0;
  {
    hipError_t e = hipDeviceGetAttribute(&s->n_cu, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) {
      delete s;
      return duck_fail(DUCK_EHIP, std::string("hipDeviceGetAttribute: ") + hipGetErrorString(e));
    }
  }
  {
    // the sticky device error word: host memory the kernels write through their device mapping, so
    // that the next call reads it without synchronising (duck_device_error)
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->err_d, p, 0);
    if (e != hipSuccess) {
      if (p) (void)hipHostFree(p);
      delete s;
      return duck_fail(DUCK_EHIP, std::string("device error word: ") + hipGetErrorString(e));
    }
    s->err_h = (volatile unsigned*)p;
    *s->err_h = 0;
  }
  s->cfg = *cfg;
  s->nq = model->nq; s->nv = model->nv; s->nu = model->nu;
  s->lay = duck_layout_make(model->nq, model->nv, model->nu, cfg->use_imitation, cfg->task);
  s->drl = duck_dr_layout_make(model->nbody, model->nu);
  if (ref) {
    if (ref->n_dim != 40 || ref->n_dx > 16 || ref->n_dy > 16 || ref->n_dtheta > 16 || ref->nb_steps_in_period < 1 ||
        !ref->frames) {
      duck_destroy(s);  // frees the pinned error word allocated above
      return duck_fail(DUCK_EINVAL, "reference-motion table must be [<=16][<=16][<=16][nb][40] frames");
    }
    s->ref.n_dx = ref->n_dx; s->ref.n_dy = ref->n_dy; s->ref.n_dtheta = ref->n_dtheta;
    s->ref.n_dim = ref->n_dim; s->ref.n_coef = ref->n_coef; s->ref.nb = ref->nb_steps_in_period;
    memcpy(s->ref.dxs, ref->dxs, sizeof(ref->dxs)); memcpy(s->ref.dys, ref->dys, sizeof(ref->dys));
    memcpy(s->ref.dthetas, ref->dthetas, sizeof(ref->dthetas));
    memcpy(s->ref.dx_range, ref->dx_range, 8); memcpy(s->ref.dy_range, ref->dy_range, 8);
    memcpy(s->ref.dtheta_range, ref->dtheta_range, 8);
    const size_t nbytes =
        sizeof(float) * (size_t)ref->n_dx * ref->n_dy * ref->n_dtheta * ref->nb_steps_in_period * ref->n_dim;
    hipError_t e = hipMalloc(&s->frames_d, nbytes);
    if (e == hipSuccess) e = hipMemcpy(s->frames_d, ref->frames, nbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      duck_destroy(s);
      return duck_fail(DUCK_EHIP, std::string("reference table upload: ") + hipGetErrorString(e));
    }
  }
  if (kVariants[v]->floor_type == 1) {  // height field elevation, [nrow][ncol] in [0, 1]
    const size_t nn = (size_t)model->hfield_nrow * model->hfield_ncol;
    float* h = new float[nn];
    for (size_t i = 0; i < nn; i++) h[i] = (float)model->hfield_data[i];
    hipError_t e = hipMalloc(&s->hfield_d, nn * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(s->hfield_d, h, nn * sizeof(float), hipMemcpyHostToDevice);
    delete[] h;
    if (e != hipSuccess) {
      duck_destroy(s);
      return duck_fail(DUCK_EHIP, std::string("height field upload: ") + hipGetErrorString(e));
    }
  }
  *out = s;
  return DUCK_OK;
}

int duck_reset(duck_sim* s, int n, float* fstate, int32_t* istate, const uint8_t* mask, uint64_t seed,
               int64_t env_offset, const float* dr, float* obs, float* priv, void* stream) {
  g_err.clear();
  if (!s || n < 0 || !fstate || !istate || !obs || !priv) return duck_fail(DUCK_EINVAL, "bad argument");
  if (*s->err_h) return device_error_fail(s);
  if (n == 0) return DUCK_OK;
  HIPCHECK(hipSetDevice(s->device));
  return kVariants[s->variant]->reset(s, n, fstate, istate, mask, seed, env_offset, dr, obs, priv,
                                      (hipStream_t)stream);
}

int duck_step(duck_sim* s, int n, float* fstate, int32_t* istate, const float* dr, const float* action, float* obs,
              float* priv, float* reward, float* done, void* stream) {
  g_err.clear();
  if (!s || n < 0 || !fstate || !istate || !action || !obs || !priv || !reward || !done)
    return duck_fail(DUCK_EINVAL, "bad argument");
  if (*s->err_h) return device_error_fail(s);
  if (n == 0) return DUCK_OK;
  HIPCHECK(hipSetDevice(s->device));
  return kVariants[s->variant]->step(s, n, fstate, istate, dr, action, obs, priv, reward, done, (hipStream_t)stream);
}

int duck_randomize(duck_sim* s, int n, float* dr, uint64_t seed, int64_t env_offset, void* stream) {
  g_err.clear();
  if (!s || n < 0 || !dr) return duck_fail(DUCK_EINVAL, "bad argument");
  if (n == 0) return DUCK_OK;
  HIPCHECK(hipSetDevice(s->device));
  return kVariants[s->variant]->randomize(s, n, dr, seed, env_offset, (hipStream_t)stream);
}

int duck_physics_step(duck_sim* s, int n, float* qpos, float* qvel, float* warm, const float* ctrl, const float* dr,
                      int nsub, float* aux, void* stream) {
  g_err.clear();
  if (!s || n < 0 || !qpos || !qvel || !warm || !ctrl || nsub < 0) return duck_fail(DUCK_EINVAL, "bad argument");
  if (*s->err_h) return device_error_fail(s);
  if (n == 0) return DUCK_OK;
  HIPCHECK(hipSetDevice(s->device));
  return kVariants[s->variant]->physics(s, n, qpos, qvel, warm, ctrl, dr, nsub, aux, (hipStream_t)stream);
}

int duck_set_step_mode(duck_sim* s, int mode) {
  g_err.clear();
  if (!s || mode < DUCK_STEP_AUTO || mode > DUCK_STEP_LATENCY_X2) return duck_fail(DUCK_EINVAL, "bad argument");
  if ((mode == DUCK_STEP_LATENCY && !s->lat_ok) || (mode == DUCK_STEP_PAIRED && !s->lat2_ok) ||
      (mode == DUCK_STEP_LATENCY_X2 && !s->latx2_ok))
    return duck_fail(DUCK_EUNSUPPORTED, "that step kernel is not compiled for this model (LDS budget, or "
                                        "LATENCY_X2 outside the plane-floor scenes; AUTO skips it)");
  s->step_mode = mode;
  return DUCK_OK;
}

int duck_step_kernel_for(const duck_sim* s, int n) {
  if (!s || n < 0) return duck_fail(DUCK_EINVAL, "bad argument");
  return step_kernel_choice(s, n);
}

int duck_device_error(duck_sim* s, unsigned* out, int clear) {
  if (!s || !out) return duck_fail(DUCK_EINVAL, "bad argument");
  *out = *s->err_h;
  if (clear) *s->err_h = 0;
  return DUCK_OK;
}

int duck_debug_lat_timeouts(const duck_sim* s, unsigned* out, int reset) {
  if (!s || !out) return duck_fail(DUCK_EINVAL, "bad argument");
  HIPCHECK(hipSetDevice(s->device));
  return kVariants[s->variant]->lat_timeouts(out, reset);
}

int duck_debug_ls_flag(int n, const float* x, float* sel, float* sat, void* stream) {
  if (n < 0) return duck_fail(DUCK_EINVAL, "duck_debug_ls_flag: bad size");
  if (n == 0) return DUCK_OK;
  if (!x || !sel || !sat) return duck_fail(DUCK_EINVAL, "duck_debug_ls_flag: null pointer");
  hipLaunchKernelGGL(ls_flag_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, x, sel, sat);
  HIPCHECK(hipGetLastError());
  return DUCK_OK;
}

// debug: the cycle counters of a stage-profile build into out[DUCK_STAGE_CYCLES_WORDS] (DUCK_EUNSUPPORTED otherwise)
int duck_debug_stage_cycles(const duck_sim* s, unsigned long long* out, int reset) {
  if (!s || !out) return duck_fail(DUCK_EINVAL, "bad argument");
  return kVariants[s->variant]->stage_cycles(out, reset);
}

}  // extern "C"
