"""numpy restatement of the fleet loop's flight recorder (include/duck_fleet.h: duck_fleet_record): the
frame's layout and the rule that freezes a robot's ring after its fall, for N robots.

Nothing is computed: words are copied through int32 views, so NaN payloads, -0 and denormals keep their bits
and the kernel's ring equals this one bit for bit. Test infrastructure only.
"""

import numpy as np

from tests.fleet_reference import frame_size

SENSORS = ("gyro", "accelerometer", "upvector", "local_linvel")


def _words(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.view(np.int32)


def frames(d, qpos, qvel, warm, aux, ctl, obs, action):
    """[N][F] int32: every robot's frame of this call. qpos [nq][N], qvel and warm [nv][N], aux [naux][N] (SoA);
    ctl [N][C], obs [N][O], action [N][nu] (row-major); ``d`` has nv, nu, sens_off and the four sensor addresses."""
    sens = [_words(aux)[d.sens_off + getattr(d, s):][:3].T for s in SENSORS]
    force = _words(aux)[4 * d.nv:][:d.nu].T
    out = np.concatenate([_words(qpos).T, _words(qvel).T, _words(warm).T, _words(ctl), _words(obs), _words(action),
                          force] + sens, axis=1)
    assert out.shape[1] == frame_size(d.nq, d.nv, d.nu)
    return out


def record_step(d, depth, post, qpos, qvel, warm, aux, ctl, obs, action, alive, head, after, ring):
    """duck_fleet_record. alive [N] float32; head, after [N] int32 and ring [N][depth][F] (float32 or int32) are
    updated in place. Returns the robots written by this call, a bool [N]."""
    fr = frames(d, qpos, qvel, warm, aux, ctl, obs, action)
    r = _words(ring)
    assert r.shape == (len(alive), depth, fr.shape[1]) and np.shares_memory(r, ring)
    dead = np.asarray(alive) == 0
    wrote = ~(dead & (after >= post + 1))
    for e in np.flatnonzero(wrote):
        r[e, head[e] % depth] = fr[e]
        head[e] += 1
        if dead[e]:
            after[e] += 1
    return wrote
