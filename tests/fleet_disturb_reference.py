"""float32 restatement of the fleet loop's disturbance launch (include/duck_fleet.h: duck_fleet_disturb) --
the stream's key and slots, the sensor noise, the schedule lookup, the push rule and the tick for N robots.

Every value is formed as the header states it: one float32 operation on float32 words, results below the
smallest normal flushed to zero as the library runs, so the kernel's outputs equal these bit for bit (the
push's cos / sin excepted, unless theta is 0: they are compared against float64). The cipher is
tests/mlp_reference.threefry2x32, pinned by known-answer tests. Test infrastructure only.
"""

import numpy as np

from tests.fleet_reference import M32, ctl_fields, ctl_size, derive_key, ftz, obs_size
from tests.mlp_reference import threefry2x32

f32 = np.float32
KEY_TAG = 0xF1EE      # DUCK_FLEET_KEY_TAG
PUSH_SIZE = 6         # DUCK_FLEET_PUSH_SIZE
TEAM = 16             # lanes of a robot's group: the slot assignment pairs columns k and k + 16


def noise_slot(k):
    """The slot of obs column k."""
    k = np.asarray(k)
    return 2 * (1 + k % TEAM + TEAM * (k // (2 * TEAM))) + (k // TEAM) % 2


def uniform(key, p, slot):
    """u of ``slot`` at period ``p`` (int32 [N], the counter's first word): (word >> 9) * 2^-23, float32.
    key = (k0 [N], k1 [N]); slot a scalar or [N]."""
    slot = np.broadcast_to(np.asarray(slot, dtype=np.int64), np.shape(key[0]))
    ctr = np.asarray(p, dtype=np.int64).astype(np.uint64) & np.uint64(M32)
    a, b = threefry2x32(key[0], key[1], ctr, (slot >> 1).astype(np.uint64))
    w = np.where(slot & 1, b, a)
    return ((w >> np.uint32(9)).astype(f32) * f32(2.0 ** -23)).astype(f32)


def push_due(t, first, interval):
    """Whether a push acts before period t's physics. first, interval integer-valued."""
    t, first, interval = (np.asarray(v).astype(np.int64) for v in (t, first, interval))
    rep = (interval > 0) & (t > first) & ((t - first) % np.maximum(interval, 1) == 0)
    return (first >= 1) & ((t == first) | rep)


def segment(t, seg_periods, n_seg):
    return np.minimum(np.asarray(t, dtype=np.int64) // int(seg_periods), int(n_seg) - 1)


def disturb(nu, seed, noise_scale, robot_offset, tick, qvel, ctl, obs, sched=None, sched_id=None, seg_periods=1,
            push=None):
    """duck_fleet_disturb. tick int32 [N], qvel [nv][N], ctl [N][C], obs [N][O] float32 numpy, all updated in
    place; noise_scale [>= O] float32; sched [S][K][7], sched_id [N], push [N][6] or None.
    Returns {"due" bool [N], "mag", "theta" float32 [N]} of this call's pushes (zeros without a table)."""
    n, O = obs.shape
    assert O == obs_size(nu) and ctl.shape == (n, ctl_size(nu))
    p = tick.astype(np.int64)
    t = p + 1
    key = derive_key(seed, int(robot_offset) + np.arange(n, dtype=np.int64), KEY_TAG)
    scale = np.asarray(noise_scale, dtype=f32)
    for k in range(O):
        if scale[k] != 0:
            u = uniform(key, p, int(noise_slot(k)))
            centred = (f32(2) * u).astype(f32) - f32(1)            # exact
            obs[:, k] = ftz(obs[:, k] + ftz(centred * scale[k]))
    if sched is not None:
        sched = np.asarray(sched, dtype=f32)
        sid = np.clip(np.asarray(sched_id, dtype=np.int64), 0, sched.shape[0] - 1)
        c0 = ctl_fields(nu)["command"][0]
        ctl[:, c0:c0 + 7] = sched[sid, segment(t, seg_periods, sched.shape[1])]
    out = {"due": np.zeros(n, bool), "mag": np.zeros(n, f32), "theta": np.zeros(n, f32)}
    if push is not None:
        w = np.asarray(push, dtype=f32)
        due = push_due(t, w[:, 0], w[:, 1])
        u0, u1 = uniform(key, p, 0), uniform(key, p, 1)
        mag = ftz(w[:, 2] + ftz(ftz(w[:, 3] - w[:, 2]) * u0))
        theta = ftz(w[:, 4] + ftz(ftz(w[:, 5] - w[:, 4]) * u1))
        cos, sin = np.cos(theta.astype(np.float64)).astype(f32), np.sin(theta.astype(np.float64)).astype(f32)
        qvel[0, due] = ftz(qvel[0, due] + ftz(cos * mag)[due])
        qvel[1, due] = ftz(qvel[1, due] + ftz(sin * mag)[due])
        out = {"due": due, "mag": mag, "theta": theta}
    tick[:] = t.astype(np.int32)
    return out
