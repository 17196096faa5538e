"""float32 restatements of the fleet deployment loop's two kernels (include/duck_fleet.h:
duck_fleet_observe, duck_fleet_actuate) -- mujoco_infer.py:175-197, :67-103 and :208-231 for N robots -- and
the tests' one statement of the loop's record sizes and offsets, its flush to zero and its stream keys. The
header is tested against this module, so it reads neither the header nor the package.

Every value is formed as the header states it: one float32 operation on float32 words, so the kernels'
outputs equal these bit for bit (the phase's cos / sin excepted: they are compared against float64).
The accumulators are restated in torch float32 on the CPU, in call order. Test infrastructure only.
"""

from types import SimpleNamespace

import numpy as np
import torch

from tests.mlp_reference import threefry2x32

f32 = np.float32
TWO_PI = f32(6.2831855)
M32 = 0xFFFFFFFF


def ctl_fields(nu):
    """(first column, width) of the control record's fields (include/duck_fleet.h)."""
    return {"last_action": (0, nu), "last_last_action": (nu, nu), "last_last_last_action": (2 * nu, nu),
            "motor_targets": (3 * nu, nu), "prev_motor_targets": (4 * nu, nu), "command": (5 * nu, 7),
            "imitation_i": (5 * nu + 7, 1), "phase_frequency_factor": (5 * nu + 8, 1),
            "imitation_phase": (5 * nu + 9, 2)}


def ctl_size(nu):
    return 5 * nu + 11       # DUCK_FLEET_CTL_SIZE


def obs_size(nu):
    return 17 + 6 * nu       # DUCK_FLEET_OBS_SIZE


def log_size(nu):
    return 17 + 7 * nu       # DUCK_FLEET_LOG_SIZE: an obs row, then the action


def frame_size(nq, nv, nu):
    return nq + 2 * nv + ctl_size(nu) + obs_size(nu) + 2 * nu + 12       # DUCK_FLEET_FRAME_SIZE


def ftz(x):
    """float32 with values below the smallest normal flushed to a signed zero, as the library runs."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(invalid="ignore"):
        tiny = np.abs(x) < np.finfo(f32).tiny
    return np.where(tiny, np.copysign(f32(0), x), x).astype(f32)


def derive_key(seed, ids, tag):
    """csrc/duck_math.h derive_key(seed, id, tag) for int64 global robot ids [N]."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    hi = (ids >> np.uint64(32)) & np.uint64(M32)
    return threefry2x32(seed & M32, seed >> 32, ids & np.uint64(M32), np.uint64(tag) ^ hi)


def desc_values(d):
    """A ctypes duck_fleet_desc as plain Python values."""
    out = {}
    for name, _ in d._fields_:
        v = getattr(d, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    for k in ("dof_vel_scale", "action_scale", "accel_x_offset", "target_step"):
        out[k] = f32(out[k])
    return SimpleNamespace(**out)


def make_desc(nu=3, nsensordata=14, ncon=12, nb=40, standing=0, speed_limits=1, **kw):
    """A small synthetic descriptor: a free joint, nu + 3 hinges of which nu are actuated (out of order),
    sensors and contact slots scattered inside the aux record."""
    nq, nv = 7 + nu + 3, 6 + nu + 3
    sens_off = 4 * nv + nu
    d = dict(nq=nq, nv=nv, nu=nu, sens_off=sens_off, con_off=sens_off + nsensordata,
             naux=sens_off + nsensordata + ncon + 5, gyro=3, accelerometer=8, upvector=0, local_linvel=11,
             act_qpos=[7 + (5 * a) % (nu + 3) for a in range(nu)], act_dof=[6 + (5 * a) % (nu + 3) for a in range(nu)],
             act_default=[f32(0.1 * a - 0.3) for a in range(nu)], foot_con=[4, 0], dof_vel_scale=f32(0.05),
             action_scale=f32(0.25), accel_x_offset=f32(1.3), target_step=f32(5.24 * 0.002 * 10),
             nb_steps_in_period=nb, standing=standing, speed_limits=speed_limits)
    d.update(kw)
    return SimpleNamespace(**d)


def phase_step(d, i, factor):
    """The phase advance: (new imitation_i float32 [N], float32 angle [N])."""
    nb = f32(d.nb_steps_in_period)
    i = np.fmod((i.astype(f32) + factor.astype(f32)).astype(f32), nb).astype(f32)
    return i, ((i / nb).astype(f32) * TWO_PI).astype(f32)


def contacts(d, aux):
    """[N][2] float32: 1.0 where any of a foot's four con_dist values is < 0 (NaN, +-0: no contact)."""
    with np.errstate(invalid="ignore"):
        return np.stack([(aux[d.con_off + s:d.con_off + s + 4] < 0).any(0) for s in d.foot_con], 1).astype(f32)


def observe(d, qpos, qvel, aux, ctl, acc, alive):
    """duck_fleet_observe. qpos [nq][N], qvel [nv][N], aux [naux][N], ctl [N][C] float32 numpy (ctl is
    updated in place); acc [N][6], alive [N] torch float32 CPU tensors (updated in place). Returns
    (obs float32 [N][17 + 6 nu], the phase [N][2] in float64: its whole chain evaluated in float64 from the
    float32 imitation_i and factor; the obs and ctl phase columns hold it rounded to float32)."""
    nu = d.nu
    F = ctl_fields(nu)
    col = lambda name: ctl[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    sens = aux[d.sens_off:]
    if not d.standing:
        i0, fac = col("imitation_i")[:, 0].astype(np.float64), col("phase_frequency_factor")[:, 0].astype(np.float64)
        ang = np.fmod(i0 + fac, d.nb_steps_in_period) / d.nb_steps_in_period * 2 * np.pi   # the whole chain in float64
        ph64 = np.stack([np.cos(ang), np.sin(ang)], 1)
        col("imitation_i")[:, 0] = phase_step(d, col("imitation_i")[:, 0], col("phase_frequency_factor")[:, 0])[0]
        col("imitation_phase")[:] = ph64.astype(f32)
    else:
        ph64 = col("imitation_phase").astype(np.float64)
    accel = sens[d.accelerometer:d.accelerometer + 3].T.copy()
    accel[:, 0] = accel[:, 0] + d.accel_x_offset
    obs = np.concatenate([
        sens[d.gyro:d.gyro + 3].T, accel, col("command"),
        (qpos[d.act_qpos[:nu]].T - np.asarray(d.act_default[:nu], f32)).astype(f32),
        (qvel[d.act_dof[:nu]].T * d.dof_vel_scale).astype(f32),
        col("last_action"), col("last_last_action"), col("last_last_last_action"), col("motor_targets"),
        contacts(d, aux), col("imitation_phase")], 1).astype(f32)
    # the bookkeeping, in torch float32
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=f32))  # noqa: E731
    vx, vy, wz = t(sens[d.local_linvel]), t(sens[d.local_linvel + 1]), t(sens[d.gyro + 2])
    cmd = t(col("command"))
    state = torch.cat([t(qpos), t(qvel)], 0)
    fallen = (t(sens[d.upvector + 2]) < 0) | torch.isnan(state).any(0)
    was = alive != 0
    alive[was & fallen] = 0.0
    add = was & ~fallen
    dx, dy, dz = vx - cmd[:, 0], vy - cmd[:, 1], wz - cmd[:, 2]
    terms = torch.stack([torch.ones_like(vx), vx, vy, wz, dx * dx + dy * dy, dz * dz], 1)
    acc[add] = acc[add] + terms[add]
    return obs, ph64


def actuate(d, action, ctl):
    """duck_fleet_actuate. action [N][nu] float32; ctl updated in place. Returns ctrl [nu][N] float32."""
    nu = d.nu
    F = ctl_fields(nu)
    col = lambda name: ctl[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    col("last_last_last_action")[:] = col("last_last_action")
    col("last_last_action")[:] = col("last_action")
    col("last_action")[:] = action
    mt = (np.asarray(d.act_default[:nu], f32) + (action.astype(f32) * d.action_scale).astype(f32)).astype(f32)
    if d.speed_limits:
        prev = col("prev_motor_targets")
        lo, hi = (prev - d.target_step).astype(f32), (prev + d.target_step).astype(f32)
        mt = np.minimum(np.maximum(mt, lo), hi).astype(f32)
        col("prev_motor_targets")[:] = mt
    col("motor_targets")[:] = mt
    return np.ascontiguousarray(mt.T)
