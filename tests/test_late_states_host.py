"""The late-state harvest (tests/late_states.py) on the CPU: the oracle alone, no GPU library.

What the GPU cases of tests/test_gpu_late_states.py rely on is pinned here: the seeds follow their rule,
the harvest is deterministic, every mosaic column has the property its class names (recomputed with the
oracle), and the oracle's own behaviour at a NaN state (test_nan_reference).
"""
import numpy as np
import pytest

from tests import late_states as ls
from tests.teacher_forcing import LATE_CASES, oracle_batch

NAN_ENVS = (0, 3, 15, 16, 36)
NAN_N = 37


def _rows(L, n, fs, name, k):
    return fs.reshape(L.nfloat, n)[L.off[name]:L.off[name] + k]


@pytest.mark.parametrize("case", list(LATE_CASES))
def test_late_seeds_follow_the_rule(case):
    """LATE_SEEDS[case] is the first seed from 7 up at which every class has >= 192 of 256 columns of its
    own and <= 5 % conditioning fallbacks."""
    for seed in range(7, ls.LATE_SEEDS[case] + 1):
        assert ls.seed_ok(case, seed) == (seed == ls.LATE_SEEDS[case]), seed
    mos = ls.mosaics(case)
    for c in ls.CLASSES:
        s = mos[c].source
        print(f"{case} {c}: own {(s == ls.OWN).sum()}, no event {(s == ls.NO_EVENT).sum()}, "
              f"conditioning fallbacks {(s == ls.CONDITIONING).sum()}, candidates rejected {mos[c].rejected.sum()}")


def test_harvest_is_deterministic():
    case = "late_flat"
    seed = ls.LATE_SEEDS[case]
    a, b = ls.harvest(case, seed), ls.harvest.__wrapped__(case, seed)
    for name in ("fs", "is_", "act", "done", "trunc"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=name == "fs"), name
    ma, mb = ls.mosaics(case), ls._mosaics.__wrapped__(case, seed, 256, 100)
    for c in ls.CLASSES:
        for name in ("fs", "is_", "act", "t", "source"):
            assert np.array_equal(getattr(ma[c], name), getattr(mb[c], name)), (c, name)


@pytest.mark.parametrize("case", list(LATE_CASES))
def test_mosaic_columns_have_their_class_property(case):
    h = ls.harvest(case, ls.LATE_SEEDS[case])
    mos = ls.mosaics(case)
    L, n = h.L, h.n
    I = lambda r, name: r["is_"].reshape(L.nint, n)[L.ioff[name]]  # noqa: E731
    F = lambda r, name, k=1: _rows(L, n, r["fs"], name, k)        # noqa: E731
    post = {c: ls.oracle_step(h, mos[c].fs, mos[c].is_, mos[c].act) for c in ls.CLASSES}
    late = mos["late"]
    assert ((late.t >= ls.LATE_T) & (late.t < ls.LATE_T + ls.TRIES)).all()
    for c in ls.CLASSES:
        m = mos[c]
        assert np.isfinite(m.fs).all() and np.array_equal(m.fs, m.fs.astype(np.float32).astype(np.float64))
        fb = m.source != ls.OWN                       # a fallback column is the env's late column
        assert np.array_equal(m.fs.reshape(L.nfloat, n)[:, fb], late.fs.reshape(L.nfloat, n)[:, fb])
        assert np.array_equal(m.t[fb], late.t[fb])
        if c != "fall_at_limit":
            assert np.array_equal(m.is_.reshape(L.nint, n)[:, fb], late.is_.reshape(L.nint, n)[:, fb])
    # fall: done with truncation 0, the physics state restored from the snapshot bit for bit, step = 0
    own = mos["fall"].source == ls.OWN
    r = post["fall"]
    assert (r["done"][own] == 1).all() and (F(r, "truncation")[0][own] == 0).all()
    for name, k in (("qpos", L.nq), ("qvel", L.nv), ("qacc_warmstart", L.nv), ("ctrl", L.nu)):
        assert np.array_equal(F(r, name, k)[:, own], F(r, "first_" + name, k)[:, own]), name
    assert np.array_equal(r["obs"][own], F(r, "first_obs", L.obs_size)[:, own].T)
    assert np.array_equal(r["priv"][own], F(r, "first_priv", L.priv_size)[:, own].T)
    assert (I(r, "step")[own] == 0).all()
    # pre_fall: no done, 3 or more steps ahead of the env's first fall
    own = mos["pre_fall"].source == ls.OWN
    assert (post["pre_fall"]["done"][own] == 0).all()
    first_fall = np.array([ls.falls(h)[:, e].argmax() for e in range(n)])
    assert (mos["pre_fall"].t[own] <= first_fall[own] - ls.PRE_FALL).all()
    # after_fall: the pre-state is the restored one (done = 1, qpos = the snapshot), the episode restarts
    own = mos["after_fall"].source == ls.OWN
    pre = {"fs": mos["after_fall"].fs}
    assert (F(pre, "done")[0][own] == 1).all()
    assert np.array_equal(F(pre, "qpos", L.nq)[:, own], F(pre, "first_qpos", L.nq)[:, own])
    assert (I(post["after_fall"], "ep_steps")[own] == 1).all()
    # touchdown: a foot in the air before the step is in contact after it
    own = mos["touchdown"].source == ls.OWN
    pre = {"fs": mos["touchdown"].fs}
    td = ((F(pre, "feet_air_time", 2) > 0) & (F(pre, "last_contact", 2) == 0)
          & (F(post["touchdown"], "last_contact", 2) == 1)).any(axis=0)
    assert td[own].all() and (mos["touchdown"].t[own] >= ls.TOUCHDOWN_FROM).all()
    # fall_at_limit: even columns at the episode's last step. A falling column: fall and limit coincide,
    # truncation 0; a late fallback column only runs out of steps: truncation 1 (unless its pre-state is
    # itself a restored one, done = 1, which restarts the step count). Odd columns: the fall mosaic's result
    m, r = mos["fall_at_limit"], post["fall_at_limit"]
    even = np.arange(n) % 2 == 0
    own = m.source == ls.OWN
    assert (m.is_.reshape(L.nint, n)[L.ioff["ep_steps"], even] == h.cfg.episode_length - 1).all()
    assert (r["done"][even & own] == 1).all() and (F(r, "truncation")[0][even & own] == 0).all()
    running = F({"fs": m.fs}, "done")[0] == 0
    fb = even & ~own & running & (r["done"] == 1)
    assert fb.sum() >= 1
    sel = even & ~own & running
    fell = post["fall"]["done"][sel] == 1            # a late column may fall on this very step
    assert (r["done"][sel] == 1).all() and np.array_equal(F(r, "truncation")[0][sel], 1.0 - fell)
    assert np.array_equal(r["fs"].reshape(L.nfloat, n)[:, ~even], post["fall"]["fs"].reshape(L.nfloat, n)[:, ~even])
    print(f"{case}: fall_at_limit even columns: {int((even & own).sum())} fall at the limit (truncation 0), "
          f"{int(F(r, 'truncation')[0][even].sum())} truncated")


@pytest.mark.parametrize("case", ["late_flat_throughput_kernel", "late_flat_backlash_imitation"])
@pytest.mark.parametrize("where", ["hinge_qvel", "qpos_z", "quat_word"])
def test_nan_reference(case, where):
    """The reference's behaviour at a NaN state (joystick.py:483-485: NaN in qpos or qvel is done, every
    reward term goes through nan_to_num), on the oracle alone: the first 37 columns of the `late` mosaic
    with NaN in one word of envs 0, 3, 15, 16 and 36 (env 3 also on its episode's last step). Those envs
    come out done with truncation 0 (done by NaN is a termination, not a time-out, at the limit too), a
    finite reward, and the physics state, obs and privileged obs restored from the first_* snapshot bit
    for bit; every other column is bit-identical to the run without the injection.

    The reference's behaviour, not something to fix: the restore replaces data and obs only, info carries
    on (BraxAutoResetWrapper), so the NaN sensor readings of the fall step stay behind in info. The only
    non-finite words left are 3 of imu_history's 9 per env (one reading of the three it keeps), and one
    step later 3 of the 9 are still non-finite while everything else, the reward included, is finite."""
    h = ls.harvest(case, ls.LATE_SEEDS[case])
    L, n = h.L, NAN_N
    kw = LATE_CASES[case]
    _, ob = oracle_batch(h.model, h.cfg, n, h.seed, bool(kw.get("dr", False)))
    sub = ls.Harvest(case, h.seed, n, 0, L, h.cfg, h.model, None, ob, None, None, None, None, None)
    late = ls.mosaics(case)["late"]
    fs = np.ascontiguousarray(late.fs.reshape(L.nfloat, 256)[:, :n]).ravel()
    is_ = late.is_.reshape(L.nint, 256)[:, :n].copy()
    is_[L.ioff["ep_steps"], 3] = h.cfg.episode_length - 1
    is_ = is_.ravel()
    act = late.act[:n]
    row = {"hinge_qvel": L.off["qvel"] + 6 + 3, "qpos_z": L.off["qpos"] + 2, "quat_word": L.off["qpos"] + 4}[where]
    ref = ls.oracle_step(sub, fs, is_, act)
    r = ls.oracle_step(sub, ls.inject_nan(L, n, fs, row, NAN_ENVS), is_, act)
    bad = np.zeros(n, dtype=bool)
    bad[list(NAN_ENVS)] = True
    R, R0 = r["fs"].reshape(L.nfloat, n), ref["fs"].reshape(L.nfloat, n)
    assert (r["done"][bad] == 1).all() and (R[L.off["truncation"], bad] == 0).all()
    assert np.isfinite(r["rew"][bad]).all() and (r["rew"][bad] >= 0).all()
    for name, k in (("qpos", L.nq), ("qvel", L.nv), ("qacc_warmstart", L.nv), ("ctrl", L.nu)):
        a, b = L.off[name], L.off["first_" + name]
        assert np.array_equal(R[a:a + k, bad], R[b:b + k, bad]), name
    assert np.array_equal(r["obs"][bad], R[L.off["first_obs"]:L.off["first_obs"] + L.obs_size, bad].T)
    assert np.array_equal(r["priv"][bad], R[L.off["first_priv"]:L.off["first_priv"] + L.priv_size, bad].T)
    # the other columns: bit-identical to the run without the injection
    for key in ("fs", "is_"):
        k = L.nfloat if key == "fs" else L.nint
        assert np.array_equal(r[key].reshape(k, n)[:, ~bad], ref[key].reshape(k, n)[:, ~bad]), key
    for key in ("obs", "priv", "rew", "done"):
        assert np.array_equal(r[key][~bad], ref[key][~bad]), key
    # integer words of the NaN envs: as in the run without the injection, but for the step counter (done)
    for name in L.ioff:
        a = r["is_"].reshape(L.nint, n)[L.ioff[name], bad]
        if name == "step":
            assert (a == 0).all()
        else:
            assert np.array_equal(a, ref["is_"].reshape(L.nint, n)[L.ioff[name], bad]), name
    # what stays non-finite: 3 of imu_history's 9 words per env, one step later too
    imu = L.off["imu_history"]
    nf = ~np.isfinite(R)
    assert not nf[:, ~bad].any()
    assert not nf[:imu, bad].any() and not nf[imu + 9:, bad].any(), np.nonzero(nf[:, bad].any(axis=1))[0]
    assert (nf[imu:imu + 9, bad].sum(axis=0) == 3).all()
    r2 = ls.oracle_step(sub, r["fs"].astype(np.float32).astype(np.float64), r["is_"], act)
    nf2 = ~np.isfinite(r2["fs"].reshape(L.nfloat, n))
    assert not nf2[:, ~bad].any() and not nf2[:imu, bad].any() and not nf2[imu + 9:, bad].any()
    assert (nf2[imu:imu + 9, bad].sum(axis=0) == 3).all()
    assert np.isfinite(r2["rew"]).all()


def test_substep_trace_ends_in_the_physics_result_on_a_fall():
    """explain() compares its substep chain with the trace's last row. On a step that ends in done the
    wrappers restore the snapshot over the physics result: the trace must end in the result (the oracle's
    own last substep from the row before), not in the snapshot; on a running step it is the batch's state."""
    from types import SimpleNamespace

    from tests.teacher_forcing import Report, oracle_substep, substep_trace
    case = "late_flat"
    h = ls.harvest(case, ls.LATE_SEEDS[case])
    L, n, m = h.L, h.n, h.model
    env = SimpleNamespace(_layout=L, mj_model=m, num_envs=n, _cfg_struct=h.cfg, n_substeps=h.cfg.n_substeps)
    for c, done in (("fall", 1), ("pre_fall", 0)):
        mo = ls.mosaics(case)[c]
        e = int(np.nonzero(mo.source == ls.OWN)[0][0])
        rep = Report(env=env, models=h.models, pre=[(mo.fs, mo.is_, mo.act)])
        _, tr = substep_trace(rep, e, 0)
        post = ls.oracle_step(h, mo.fs, mo.is_, mo.act)
        assert post["done"][e] == done and h.cfg.auto_reset == 1
        P = post["fs"].reshape(L.nfloat, n)[:, e]
        k = m.nq + 2 * m.nv
        assert np.array_equal(tr[-1, :k], oracle_substep(h.models, tr[-2])[:k])
        same = np.array_equal(tr[-1, :k], P[:k])            # qpos, qvel, qacc_warmstart lead the layout
        assert same == (done == 0)
