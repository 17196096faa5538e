"""numpy restatement of the fleet loop's latency launches (include/duck_fleet.h: duck_fleet_sense_delay,
duck_fleet_actuate_delayed) -- the stream's key, the integer draw, the IMU delay line and the delayed entry of
the action history for N robots.

The draw is uint32 / uint64 integer arithmetic, the delay line copies words (as int32 views: NaN payloads and -0
keep their bits), and the actuate part repeats tests/fleet_reference.actuate's float32 expressions on the
delayed action, so the kernels' outputs equal these bit for bit. The cipher is tests/mlp_reference.threefry2x32,
pinned by known-answer tests. Test infrastructure only.
"""

import numpy as np

from tests.fleet_reference import M32, ctl_fields, derive_key
from tests.mlp_reference import threefry2x32

f32 = np.float32
LAT_TAG = 0x1A7E      # DUCK_FLEET_LAT_TAG
MAX_DELAY = 2         # DUCK_FLEET_MAX_DELAY
LAT_SIZE = 4          # DUCK_FLEET_LAT_SIZE
SLOTS = MAX_DELAY + 1


def draw_map(word, lo, hi):
    """d = lo + (((word >> 9) * (hi - lo + 1)) >> 23) in uint32 arithmetic (the product is < 2^25)."""
    word = np.asarray(word).astype(np.uint64) & np.uint64(M32)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    span = (hi - lo + 1).astype(np.uint64)
    return lo + ((((word >> np.uint64(9)) * span) & np.uint64(M32)) >> np.uint64(23)).astype(np.int64)


def clamp_rows(lat):
    """The kernels' clamp of a table row: lo into [0, MAX_DELAY], hi into [lo, MAX_DELAY]. [N][4] int64."""
    lat = np.asarray(lat, dtype=np.int64).reshape(-1, LAT_SIZE).copy()
    for k in (0, 2):
        lat[:, k] = np.clip(lat[:, k], 0, MAX_DELAY)
        lat[:, k + 1] = np.clip(np.maximum(lat[:, k + 1], lat[:, k]), 0, MAX_DELAY)
    return lat


def period(lat_tick):
    """p: the counter with a negative value read as 0. int64 [N]."""
    return np.maximum(np.asarray(lat_tick, dtype=np.int64), 0)


def delays(seed, robot_offset, lat_tick, lat, tag=LAT_TAG):
    """(action delay [N], sensor delay [N]) of the period ``lat_tick`` counts: words 0 and 1 of block 0 at counter
    (p, 0), each through the integer map of its (lo, hi); lo == hi is that value."""
    lat = clamp_rows(lat)
    n = len(lat)
    p = period(lat_tick)
    k0, k1 = derive_key(seed, int(robot_offset) + np.arange(n, dtype=np.int64), tag)
    a, b = threefry2x32(k0, k1, p.astype(np.uint64) & np.uint64(M32), np.zeros(n, np.uint64))
    return draw_map(a, lat[:, 0], lat[:, 1]), draw_map(b, lat[:, 2], lat[:, 3])


def sense_delay(seed, robot_offset, lat_tick, lat, line, obs):
    """duck_fleet_sense_delay. line [N][3][6], obs [N][O] float32 numpy, updated in place through int32 views;
    lat_tick int32 [N] is not written. Returns (d_eff [N], whether obs was written [N])."""
    n = obs.shape[0]
    assert line.shape == (n, SLOTS, 6) and line.dtype == f32 and obs.dtype == f32
    lw, ow = line.view(np.int32), obs.view(np.int32)
    p = period(lat_tick)
    d = delays(seed, robot_offset, lat_tick, lat)[1]
    d_eff = np.minimum(d, np.minimum(p, MAX_DELAY))
    e = np.arange(n)
    lw[e, p % SLOTS] = ow[:, :6]
    wrote = d_eff > 0
    ow[wrote, :6] = lw[e, (p - d_eff) % SLOTS][wrote]
    return d_eff, wrote


def actuate_delayed(d, seed, robot_offset, lat_tick, lat, action, ctl):
    """duck_fleet_actuate_delayed. ``d`` the descriptor (tests/fleet_reference.make_desc / desc_values); action
    [N][nu] float32; ctl [N][C] and lat_tick int32 [N] updated in place. Returns ctrl [nu][N] float32."""
    nu = d.nu
    F = ctl_fields(nu)
    col = lambda name: ctl[:, F[name][0]:F[name][0] + F[name][1]]  # noqa: E731
    delay = delays(seed, robot_offset, lat_tick, lat)[0]
    col("last_last_last_action")[:] = col("last_last_action")
    col("last_last_action")[:] = col("last_action")
    col("last_action")[:] = action
    hist = np.stack([col("last_action"), col("last_last_action"), col("last_last_last_action")])   # entry d, shifted
    used = hist[delay, np.arange(len(delay))].astype(f32)
    mt = (np.asarray(d.act_default[:nu], f32) + (used * d.action_scale).astype(f32)).astype(f32)
    if d.speed_limits:
        prev = col("prev_motor_targets")
        lo, hi = (prev - d.target_step).astype(f32), (prev + d.target_step).astype(f32)
        mt = np.minimum(np.maximum(mt, lo), hi).astype(f32)
        col("prev_motor_targets")[:] = mt
    col("motor_targets")[:] = mt
    lat_tick[:] = (np.asarray(lat_tick, dtype=np.int64) + 1).astype(np.int32)
    return np.ascontiguousarray(mt.T)
