"""numpy float32 restatement of the fleet loop's follow launch (include/duck_fleet.h: duck_fleet_follow) -- the
score against the log's row, the fed action, the next period's command and the tick for N robots.

Every score word is formed as the header states it: d = obs - r, q = d * d, score + q, each one float32 operation,
operands and results below the smallest normal flushed to zero as the library runs; a NaN log word leaves its score
word untouched. Actions and commands are copied through int32 views, so NaN payloads and -0 keep their bits. The
kernel's outputs equal these bit for bit. It imports nothing from the package. Test infrastructure only.
"""

import numpy as np

from tests.fleet_reference import ctl_fields, ctl_size, ftz, log_size, obs_size

f32 = np.float32


def follow(nu, log, log_id, log_tick, obs, score, ctl, action):
    """duck_fleet_follow. log [n_log][T][W], obs [N][O] float32 (read only); log_id int32 [N] (read only); score
    [N][O], ctl [N][C], action [N][nu] float32 and log_tick int32 [N] updated in place. Returns (p [N] the period
    each robot read, inside [N] whether p < T)."""
    O, W, C = obs_size(nu), log_size(nu), ctl_size(nu)
    n_log, T = log.shape[:2]
    n = obs.shape[0]
    assert log.shape == (n_log, T, W) and obs.shape == (n, O) and score.shape == (n, O)
    assert ctl.shape == (n, C) and action.shape == (n, nu)
    assert all(a.dtype == f32 for a in (log, obs, score, ctl, action)) and log_tick.dtype == np.int32
    lw, cw, aw = log.view(np.int32), ctl.view(np.int32), action.view(np.int32)
    p = np.maximum(np.asarray(log_tick, dtype=np.int64), 0)
    ids = np.clip(np.asarray(log_id, dtype=np.int64), 0, n_log - 1)
    inside = p < T
    e = np.flatnonzero(inside)
    # score: only the words whose log word is a number are written
    r = log[ids[e], p[e], :O]
    with np.errstate(invalid="ignore", over="ignore"):
        d = ftz(ftz(obs[e]) - ftz(r))
        q = ftz(d * d)
        new = ftz(ftz(score[e]) + q)
    keep = np.isnan(r)
    sw = score.view(np.int32)
    sw[e] = np.where(keep, sw[e], new.view(np.int32))
    # action: the log's words, or +0.0 past the end
    aw[:] = 0
    aw[e] = lw[ids[e], p[e], O:]
    # command: row p + 1's, while there is one
    nxt = np.flatnonzero(p + 1 < T)
    c0 = ctl_fields(nu)["command"][0]
    cw[nxt, c0:c0 + 7] = lw[ids[nxt], p[nxt] + 1, 6:13]
    log_tick[:] = np.minimum(p + 1, T).astype(np.int32)
    return p, inside
