"""numpy float32 restatement of the fleet loop's gait launch (include/duck_fleet.h: duck_fleet_gait) -- the servo
loads, the action rate, the feet's contacts, touchdowns, slip and swing clearance and the whole-body counts for N
robots -- with the record's sizes and offsets stated here on their own.

Every value is formed as the header states it: one float32 operation per statement, operands and results below the
smallest normal flushed to zero as the library runs; maxima, the apex and the state words are selections of loaded
words and keep their bits; a dead robot's row is not touched. The kernel's output equals this bit for bit. It
imports nothing from the package. Test infrastructure only.
"""

from types import SimpleNamespace

import numpy as np

from tests.fleet_reference import ctl_fields, ftz

f32 = np.float32
ACTUATOR_FIELDS = ("force_sq", "force_max", "force_sat", "speed_max", "speed_sat", "work", "action_rate")
FOOT_FIELDS = ("contact", "touchdowns", "slip", "apex_sum", "prev", "apex")
FEET = ("left", "right")


def gait_size(nu):
    return 7 * nu + 15       # DUCK_FLEET_GAIT_SIZE


def gait_fields(nu):
    """(first column, width) of the gait record's fields (include/duck_fleet.h)."""
    out = {name: (k * nu, nu) for k, name in enumerate(ACTUATOR_FIELDS)}
    B = 7 * nu
    out.update(periods=(B, 1), double_support=(B + 1, 1), flight=(B + 2, 1))
    for f, foot in enumerate(FEET):
        for k, name in enumerate(FOOT_FIELDS):
            out[f"{foot}_{name}"] = (B + 3 + 6 * f + k, 1)
    return out


def make_gait_desc(d, force_sat=None, speed_sat=5.24, foot_linvel=(5, 1), foot_pos=(10, 2)):
    """A small synthetic duck_fleet_gait_desc for tests.fleet_reference.make_desc's ``d`` (14 sensordata words)."""
    force_sat = [f32(1.0 + 0.25 * a) for a in range(16)] if force_sat is None else [f32(v) for v in force_sat]
    return SimpleNamespace(foot_linvel=list(foot_linvel), foot_pos=list(foot_pos), force_sat=force_sat,
                           speed_sat=f32(speed_sat))


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ftz(ftz(a) * ftz(b))


def _add(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ftz(ftz(a) + ftz(b))


def _sub(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ftz(ftz(a) - ftz(b))


def gait(d, s, qvel, aux, ctl, alive, rec):
    """duck_fleet_gait. qvel [nv][N], aux [naux][N], ctl [N][C], alive [N] float32 (read only); rec [N][G] float32
    updated in place. ``d`` the fleet descriptor's values, ``s`` the gait descriptor's. Returns the call's own
    bookkeeping: live [N], first [N], contact [N][2], touchdown [N][2], liftoff [N][2] (booleans, False for a dead
    robot) and force_at [N][nu], speed_at [N][nu] (the saturation counted)."""
    nu, n = d.nu, rec.shape[0]
    assert rec.shape == (n, gait_size(nu)) and rec.dtype == f32 and aux.dtype == f32 and qvel.dtype == f32
    assert ctl.dtype == f32 and alive.shape == (n,)
    F, C = gait_fields(nu), ctl_fields(nu)
    with np.errstate(invalid="ignore"):
        live = alive != 0
    e = np.flatnonzero(live)
    g = rec[e]                                         # a copy: written back at the end, the live rows only
    col = lambda name: g[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    first = col("periods")[:, 0] == 0
    # the actuators
    f = aux[4 * d.nv:4 * d.nv + nu][:, e].T
    w = qvel[np.asarray(d.act_dof[:nu])][:, e].T
    af, aw = np.abs(f), np.abs(w)
    ff = _mul(f, f)
    fw = _mul(f, w)
    a0 = ctl[e][:, C["last_action"][0]:C["last_action"][0] + nu]
    a1 = ctl[e][:, C["last_last_action"][0]:C["last_last_action"][0] + nu]
    dd = _sub(a0, a1)
    dd = _mul(dd, dd)
    one = f32(1)
    with np.errstate(invalid="ignore"):
        col("force_sq")[:] = _add(col("force_sq"), ff)
        col("force_max")[:] = np.where(af > col("force_max"), af, col("force_max"))
        force_at = af >= np.asarray(s.force_sat[:nu], f32)
        col("force_sat")[:] = np.where(force_at, _add(col("force_sat"), one), col("force_sat"))
        col("speed_max")[:] = np.where(aw > col("speed_max"), aw, col("speed_max"))
        speed_at = aw >= f32(s.speed_sat)
        col("speed_sat")[:] = np.where(speed_at, _add(col("speed_sat"), one), col("speed_sat"))
        col("work")[:] = _add(col("work"), np.abs(fw))
        col("action_rate")[:] = _add(col("action_rate"), dd)
    # the feet
    sens = aux[d.sens_off:]
    contact = np.zeros((len(e), 2), bool)
    touchdown, liftoff = np.zeros((len(e), 2), bool), np.zeros((len(e), 2), bool)
    for k, foot in enumerate(FEET):
        slots = aux[d.con_off + d.foot_con[k]:d.con_off + d.foot_con[k] + 4][:, e]
        with np.errstate(invalid="ignore"):
            c = (slots < 0).any(0)
        vx, vy = sens[s.foot_linvel[k]][e], sens[s.foot_linvel[k] + 1][e]
        z = sens[s.foot_pos[k] + 2][e]
        name = lambda field: col(f"{foot}_{field}")[:, 0]  # noqa: E731
        prev, apex = name("prev").copy(), name("apex").copy()
        with np.errstate(invalid="ignore"):
            td = ~first & (prev == 0) & c
            lo = ~first & (prev != 0) & ~c
            xx, yy = _mul(vx, vx), _mul(vy, vy)
            slip = _add(xx, yy)
            name("contact")[:] = np.where(c, _add(name("contact"), one), name("contact"))
            name("slip")[:] = np.where(c, _add(name("slip"), slip), name("slip"))
            swing = np.where(first | lo, z, np.where(z > apex, z, apex))
            name("apex")[:] = np.where(c, apex, swing)
            h = _sub(apex, z)
            name("touchdowns")[:] = np.where(td, _add(name("touchdowns"), one), name("touchdowns"))
            name("apex_sum")[:] = np.where(td, _add(name("apex_sum"), h), name("apex_sum"))
        name("prev")[:] = np.where(c, one, f32(0))
        contact[:, k], touchdown[:, k], liftoff[:, k] = c, td, lo
    # the whole body
    both, none = contact.all(1), ~contact.any(1)
    col("double_support")[:, 0] = np.where(both, _add(col("double_support")[:, 0], one), col("double_support")[:, 0])
    col("flight")[:, 0] = np.where(none, _add(col("flight")[:, 0], one), col("flight")[:, 0])
    col("periods")[:, 0] = _add(col("periods")[:, 0], one)
    rec.view(np.int32)[e] = g.view(np.int32)

    def full(a):
        out = np.zeros((n,) + a.shape[1:], bool)
        out[e] = a
        return out
    return SimpleNamespace(live=live, first=full(first), contact=full(contact), touchdown=full(touchdown),
                           liftoff=full(liftoff), force_at=full(force_at), speed_at=full(speed_at))
