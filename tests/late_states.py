"""Late-episode states for the teacher-forced suite: falls, the steps around them, touchdowns, step 60.

Test infrastructure, CPU only (the oracle; nothing here opens the GPU library). The teacher-forced
cases of tests/teacher_forcing.py see states within 6 env-steps of a reset (10 in the long rough
cases), where no env falls: termination by fall, the auto-reset restore after one, the fall step's
reward and the tilted, fast states training lives in never reach a comparison. Here the oracle is run
freely for T env-steps from the case's reset (`harvest`: the batch of teacher_forcing.run, U(-1, 1)
actions, fp32-rounded state before every step, every pre-state kept), and `mosaics` cuts six
teacher-forced "steps" out of that record. A mosaic holds one state per env column: column e holds
env e's own pre-state at a time t_e chosen per class, so env ids, RNG keys, DR columns and the
auto-reset snapshot stay consistent with the GPU env of the same seed.

Classes (CLASSES, the order of the steps):
  fall           t_e = env e's first step that ends in done by fall (upvector z < 0)
  pre_fall       3 steps before it
  after_fall     the step after it: the first step from the restored state
  late           t_e = 60
  touchdown      the first t_e >= 10 where a foot is in the air in the pre-state (feet_air_time > 0,
                 last_contact = 0) and has last_contact = 1 after the step
  fall_at_limit  the fall mosaic with ep_steps = episode_length - 1 in every even column: where the env
                 falls, fall and limit coincide (truncation 0); in a `late` fallback column the episode
                 only runs out (truncation 1)
An env with no event of a class takes its `late` state (a fallback column).

Conditioning. The reference can judge a kernel only where it is itself well conditioned. A candidate
(e, t) is accepted only if the oracle's one step from it, over DRAWS draws of qpos and qvel scaled by
1 + 1e-7 N(0, 1) and rounded to fp32, stays within half of every default_tol() bar of its unperturbed
step and never flips done or an integer word. Otherwise the class's next candidate is tried -- the env's
next later event; the next earlier step for pre_fall; t + 1 for late -- and after TRIES rejections (or
when the candidates run out) the column takes its `late` state. Computed without the library under
test. LATE_SEEDS[case] is the first seed from 7 up at which every class of the case has >= MIN_OWN of 256
columns from the class itself and <= MAX_COND (5 %) fallbacks caused by conditioning
(tests/test_late_states_host.py checks it, as test_gpu_slice_layout.py does for its RESET_SEEDS).
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

from open_duck_playground_amd import constants
from open_duck_playground_amd.config import default_config, env_config_struct
from open_duck_playground_amd.mjcf import Model
from tests.teacher_forcing import LATE_CASES, LATE_EPISODE, _fs_err, _rel, default_tol, oracle_batch

CLASSES = ("fall", "pre_fall", "after_fall", "late", "touchdown", "fall_at_limit")
LATE_T = 60
TOUCHDOWN_FROM = 10
PRE_FALL = 3
LEVEL = 1e-7
DRAWS = 4
TRIES = 5
MIN_OWN = 192
MAX_COND = 0.05
LATE_SEEDS = {"late_flat": 7, "late_flat_backlash_imitation": 7, "late_rough_backlash_dr": 7,
              "late_flat_throughput_kernel": 7}
# where a column's state comes from
OWN, NO_EVENT, CONDITIONING = 0, 1, 2


@dataclass
class Harvest:
    case: str
    seed: int
    n: int
    T: int
    L: object            # cabi.Layout
    cfg: object          # the DuckEnvConfig the oracle ran
    model: Model
    models: object       # the OracleModel(s)
    ob: object           # the OracleBatch (reused by oracle_step)
    fs: np.ndarray       # [T + 1, nfloat * n] float32: pre-state of step t; row T = the state after the last
    is_: np.ndarray      # [T + 1, nint * n] int32
    act: np.ndarray      # [T, n, nu] float32
    done: np.ndarray     # [T, n] done after step t
    trunc: np.ndarray    # [T, n] truncation after step t


@dataclass
class Mosaic:
    fs: np.ndarray       # [nfloat * n] float64 (fp32 values)
    is_: np.ndarray      # [nint * n] int32
    act: np.ndarray      # [n, nu] float32
    t: np.ndarray        # [n] the harvest step each column was taken at
    source: np.ndarray   # [n] OWN / NO_EVENT / CONDITIONING
    rejected: np.ndarray = None   # [n] candidates the conditioning rule rejected before this one


def oracle_step(h: Harvest, fs, is_, act) -> dict:
    """One oracle env-step of all columns from (fs, is_) with act; the harvest's batch is the scratch."""
    ob = h.ob
    ob.fs[:] = fs
    ob.is_[:] = is_
    ob.step(np.asarray(act, dtype=np.float64))
    return {"fs": ob.fs.copy(), "is_": ob.is_.copy(), "obs": ob.obs.copy(), "priv": ob.priv.copy(),
            "rew": ob.rew.copy(), "done": ob.done.copy()}


@functools.lru_cache(maxsize=None)
def harvest(case: str, seed: int, n: int = 256, T: int = 100) -> Harvest:
    """The oracle's free run of the case (teacher_forcing.LATE_CASES): the batch run() builds for it --
    training wrappers with LATE_EPISODE steps, DR models from seed + 1 -- stepped T times with
    default_rng(action_seed) U(-1, 1) actions, fs rounded to fp32 before every step as run() does."""
    kw = LATE_CASES[case]
    m = Model.load(constants.task_to_xml(kw["task"]))
    config = default_config()
    config.episode_length = LATE_EPISODE
    dr = bool(kw.get("dr", False))
    cfg = env_config_struct(m, config, kw["imitation"], True, dr)
    models, ob = oracle_batch(m, cfg, n, seed, dr)
    L = ob.L
    rng = np.random.default_rng(kw.get("action_seed", 0))
    fs = np.zeros((T + 1, L.nfloat * n), dtype=np.float32)
    is_ = np.zeros((T + 1, L.nint * n), dtype=np.int32)
    act = np.zeros((T, n, m.nu), dtype=np.float32)
    done, trunc = np.zeros((T, n)), np.zeros((T, n))
    for t in range(T):
        ob.fs[:] = ob.fs.astype(np.float32).astype(np.float64)
        fs[t], is_[t] = ob.fs, ob.is_
        act[t] = rng.uniform(-1, 1, (n, m.nu)).astype(np.float32)
        ob.step(act[t].astype(np.float64))
        done[t] = ob.done
        trunc[t] = ob.fs.reshape(L.nfloat, n)[L.off["truncation"]]
    fs[T], is_[T] = ob.fs, ob.is_
    return Harvest(case, seed, n, T, L, cfg, m, models, ob, fs, is_, act, done, trunc)


def falls(h: Harvest) -> np.ndarray:
    """[T, n] bool: step t of env e ends in done by fall (not by the episode's limit)."""
    return (h.done != 0) & (h.trunc == 0)


def touchdowns(h: Harvest) -> np.ndarray:
    """[T, n] bool: some foot in the air before step t (feet_air_time > 0, last_contact = 0) is in
    contact after it."""
    L, n = h.L, h.n
    F = h.fs.reshape(h.T + 1, L.nfloat, n)
    air = F[:, L.off["feet_air_time"]:L.off["feet_air_time"] + 2]
    con = F[:, L.off["last_contact"]:L.off["last_contact"] + 2]
    ev = (air[:-1] > 0) & (con[:-1] == 0) & (con[1:] == 1)
    ev[:TOUCHDOWN_FROM] = False
    return ev.any(axis=1)


def candidates(h: Harvest) -> Dict[str, List[List[int]]]:
    """Per class and env the candidate steps in the order they are tried."""
    fl, td = falls(h), touchdowns(h)
    out = {c: [] for c in ("fall", "pre_fall", "after_fall", "late", "touchdown")}
    for e in range(h.n):
        tf = [int(t) for t in np.nonzero(fl[:, e])[0]]
        out["fall"].append(tf)
        out["pre_fall"].append([t for t in range(tf[0] - PRE_FALL, -1, -1)] if tf else [])
        out["after_fall"].append([t + 1 for t in tf if t + 1 < h.T])
        out["late"].append(list(range(LATE_T, min(LATE_T + TRIES, h.T))))
        out["touchdown"].append([int(t) for t in np.nonzero(td[:, e])[0]])
    return out


def assemble(h: Harvest, t: np.ndarray):
    """(fs, is_, act) with column e taken at harvest step t[e]."""
    L, n = h.L, h.n
    cols = np.arange(n)
    fs = h.fs.reshape(h.T + 1, L.nfloat, n)[t, :, cols].T.astype(np.float64)
    is_ = h.is_.reshape(h.T + 1, L.nint, n)[t, :, cols].T
    return np.ascontiguousarray(fs).ravel(), np.ascontiguousarray(is_).ravel(), h.act[t, cols].copy()


def step_errors(L, n: int, a: dict, b: dict) -> Dict[str, np.ndarray]:
    """Per-env error of step result a against b, per group, as teacher_forcing.run measures it."""
    err = _fs_err(L, a["fs"], b["fs"], n)
    err["obs"] = _rel(a["obs"], b["obs"]).max(axis=1)
    err["priv"] = _rel(a["priv"], b["priv"]).max(axis=1)
    err["reward"] = _rel(a["rew"], b["rew"])
    return err


def well_conditioned(h: Harvest, fs, is_, act, rng) -> np.ndarray:
    """[n] bool, the conditioning rule of this module's docstring for every column of one mosaic."""
    L, n = h.L, h.n
    tol = default_tol()
    base = oracle_step(h, fs, is_, act)
    ok = np.ones(n, dtype=bool)
    for _ in range(DRAWS):
        P = fs.reshape(L.nfloat, n).copy()
        for name, k in (("qpos", L.nq), ("qvel", L.nv)):
            o = L.off[name]
            P[o:o + k] *= 1.0 + LEVEL * rng.standard_normal((k, n))
        P = P.astype(np.float32).astype(np.float64)
        r = oracle_step(h, P.ravel(), is_, act)
        for g, e in step_errors(L, n, r, base).items():
            ok &= e <= 0.5 * tol[g]        # a NaN error rejects
        ok &= r["done"] == base["done"]
        ok &= (r["is_"].reshape(L.nint, n) == base["is_"].reshape(L.nint, n)).all(axis=0)
    return ok


def choose(h: Harvest, cands: List[List[int]], rng, fill: np.ndarray):
    """The first accepted candidate per env among its first TRIES; (t, source, rejected), t = fill[e]
    where none is (the late state; NO_EVENT when the env had no candidate, else CONDITIONING)."""
    n = h.n
    t = np.asarray(fill).copy()
    source = np.array([CONDITIONING if c else NO_EVENT for c in cands])
    pending = source == CONDITIONING
    rejected = np.zeros(n, dtype=int)
    for k in range(TRIES):
        cols = np.array([pending[e] and len(cands[e]) > k for e in range(n)])
        if not cols.any():
            break
        tt = np.asarray(fill).copy()
        tt[cols] = [cands[e][k] for e in np.nonzero(cols)[0]]
        ok = well_conditioned(h, *assemble(h, tt), rng) & cols
        t[ok] = tt[ok]
        source[ok] = OWN
        pending &= ~ok
        rejected[cols & ~ok] += 1
    return t, source, rejected


@functools.lru_cache(maxsize=None)
def _mosaics(case: str, seed: int, n: int, T: int) -> Dict[str, Mosaic]:
    h = harvest(case, seed, n, T)
    L = h.L
    rng = np.random.default_rng(seed)
    cands = candidates(h)
    late = choose(h, cands["late"], rng, np.full(n, LATE_T))
    out = {}
    for c in ("fall", "pre_fall", "after_fall", "late", "touchdown"):
        t, src, rej = late if c == "late" else choose(h, cands[c], rng, late[0])
        out[c] = Mosaic(*assemble(h, t), t=t, source=src, rejected=rej)
    f = out["fall"]
    is_ = f.is_.reshape(L.nint, n).copy()
    is_[L.ioff["ep_steps"], 0::2] = h.cfg.episode_length - 1
    out["fall_at_limit"] = Mosaic(f.fs.copy(), is_.ravel(), f.act.copy(), f.t.copy(), f.source.copy(), f.rejected.copy())
    return out


def mosaics(case: str, seed: int = None, n: int = 256, T: int = 100) -> Dict[str, Mosaic]:
    """The case's mosaics by class, at LATE_SEEDS[case] unless a seed is given. Cached: treat as read-only."""
    return _mosaics(case, LATE_SEEDS[case] if seed is None else seed, n, T)


def seed_ok(case: str, seed: int) -> bool:
    """LATE_SEEDS' rule at this seed."""
    mos = mosaics(case, seed)
    return all((mos[c].source == OWN).sum() >= MIN_OWN and
               (mos[c].source == CONDITIONING).mean() <= MAX_COND for c in CLASSES)


def inject_nan(L, n: int, fs: np.ndarray, row: int, envs) -> np.ndarray:
    """A copy of fs with NaN in fstate row `row` of the given env columns."""
    F = fs.reshape(L.nfloat, n).copy()
    F[row, list(envs)] = np.nan
    return F.ravel()
