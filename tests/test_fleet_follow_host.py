"""Host side of following a log (include/duck_fleet.h duck_fleet_follow; sim2sim.FleetInfer.set_log): the C-ABI
symbol, constants and refusals, the restatement (tests/fleet_follow_reference.py) on hand-written rows, the log's
file forms, the score report, the population refinement, and the command line's flags and plan. No GPU."""

import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from open_duck_playground_amd import cabi, native, sim2sim
from tests import fleet_follow_reference as F
from tests import fleet_reference as R
from tests.fleet_helpers import f32_bits as bits, host_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN_PAYLOAD, NEG_ZERO = np.int32(0x7FC12345), np.int32(-0x80000000)


# --- the C ABI --------------------------------------------------------------------------
def test_symbol_and_constants():
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    L = native.lib()
    assert re.search(r"^int duck_fleet_follow\(", hdr, flags=re.M)
    assert "duck_fleet_follow" in native.EXPORTS and "duck_fleet_follow" in cabi.HEADERS.funcs
    assert L.duck_fleet_follow.argtypes is not None
    ret, args = cabi.HEADERS.funcs["duck_fleet_follow"]
    assert ret is C.c_int and len(args) == 12 and args[1] is C.c_int and args[2] is C.c_int and args[3] is C.c_int
    for nu in (1, 3, 14, 16):
        assert cabi.HEADERS.value(f"DUCK_FLEET_LOG_SIZE({nu})") == sim2sim.fleet_log_size(nu) == F.log_size(nu)
        assert F.log_size(nu) == cabi.HEADERS.value(f"DUCK_FLEET_OBS_SIZE({nu})") + nu == F.obs_size(nu) + nu
        assert F.ctl_size(nu) == cabi.HEADERS.value(f"DUCK_FLEET_CTL_SIZE({nu})")
    # the period order names the new entry
    assert "policy or follow, actuate or actuate_delayed, [record]" in hdr


def test_refusals_come_before_any_launch():
    L = native.lib()
    d = host_desc()
    one = C.c_void_p(16)   # (never dereferenced: every call below is refused before any launch)

    def call(desc=C.byref(d), n=1, n_log=1, T=1, null=None):
        return L.duck_fleet_follow(desc, n, n_log, T, *[None if k == null else one for k in range(7)], None)
    assert call(desc=None) == -1 and b"duck_fleet_follow: null pointer" in L.duck_last_error()
    for k in range(7):
        assert call(null=k) == -1 and b"duck_fleet_follow: null pointer" in L.duck_last_error(), k
    for n in (-1, (1 << 27) + 1):
        assert call(n=n) == -1 and b"duck_fleet_follow: bad size" in L.duck_last_error()
    for kw in (dict(n_log=0), dict(n_log=-2), dict(T=0), dict(T=-1)):
        assert call(**kw) == -1 and b"n_log >= 1 and T >= 1" in L.duck_last_error(), kw
    d.nu = 17
    assert call() == -1 and b"nu" in L.duck_last_error()
    d.nu = 14
    d.act_dof[3] = 20
    assert call() == -1 and b"actuator address" in L.duck_last_error()
    d.act_dof[3] = 9
    assert call(n=0) == 0          # an empty fleet


# --- the restatement's own properties ---------------------------------------------------------
def _buffers(n, nu, n_log, T, seed=0):
    rng = np.random.default_rng(seed)
    O, W, Cw = F.obs_size(nu), F.log_size(nu), F.ctl_size(nu)
    return dict(log=rng.normal(size=(n_log, T, W)).astype(f32), obs=rng.normal(size=(n, O)).astype(f32),
                score=np.zeros((n, O), f32), ctl=rng.normal(size=(n, Cw)).astype(f32), action=np.full((n, nu), 3, f32))


def test_a_nan_log_word_leaves_its_score_words_bits():
    nu, n = 3, 2
    b = _buffers(n, nu, 1, 4)
    O = F.obs_size(nu)
    b["log"].view(np.int32)[0, 0, [1, 20]] = NAN_PAYLOAD
    b["score"].view(np.int32)[:, 1] = NEG_ZERO                     # bits an addition would not keep
    b["score"][:, 20] = 5.0
    b["score"][:, 2] = 0.25
    tick, ids = np.zeros(n, np.int32), np.zeros(n, np.int32)
    F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
    assert (b["score"].view(np.int32)[:, 1] == NEG_ZERO).all() and (b["score"][:, 20] == 5.0).all()
    d = (b["obs"][:, 2] - b["log"][0, 0, 2]).astype(f32)
    np.testing.assert_array_equal(b["score"][:, 2], (f32(0.25) + (d * d).astype(f32)).astype(f32))
    d = (b["obs"][:, O - 1] - b["log"][0, 0, O - 1]).astype(f32)
    np.testing.assert_array_equal(b["score"][:, O - 1], (d * d).astype(f32))
    # a NaN in the simulated observation makes the score NaN
    b["obs"][0, 5] = np.nan
    F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
    assert np.isnan(b["score"][0, 5]) and not np.isnan(b["score"][1, 5]) and list(tick) == [2, 2]


def test_actions_and_commands_are_copied_and_the_end_is_held():
    nu, n, T = 3, 3, 3
    b = _buffers(n, nu, 1, T, seed=1)
    O = F.obs_size(nu)
    lw = b["log"].view(np.int32)
    lw[0, 0, O] = NAN_PAYLOAD
    lw[0, 1, O + 1] = NEG_ZERO
    lw[0, 1, 6] = NEG_ZERO
    tick = np.array([0, -5, 1], np.int32)                         # a negative tick is period 0
    ids = np.zeros(n, np.int32)
    ctl0 = b["ctl"].copy()
    p, inside = F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
    assert list(p) == [0, 0, 1] and inside.all() and list(tick) == [1, 1, 2]
    np.testing.assert_array_equal(bits(b["action"][:2]), bits(np.tile(b["log"][0, 0, O:], (2, 1))))
    np.testing.assert_array_equal(bits(b["action"][2]), bits(b["log"][0, 1, O:]))
    assert b["action"].view(np.int32)[0, 0] == NAN_PAYLOAD and b["action"].view(np.int32)[2, 1] == NEG_ZERO
    c0 = R.ctl_fields(nu)["command"][0]
    cmd = slice(c0, c0 + 7)
    np.testing.assert_array_equal(bits(b["ctl"][:2, cmd]), bits(np.tile(b["log"][0, 1, 6:13], (2, 1))))   # row p + 1's
    np.testing.assert_array_equal(bits(b["ctl"][2, cmd]), bits(b["log"][0, 2, 6:13]))
    assert b["ctl"].view(np.int32)[0, c0] == NEG_ZERO
    keep = np.ones(b["ctl"].shape[1], bool)
    keep[cmd] = False
    np.testing.assert_array_equal(bits(b["ctl"][:, keep]), bits(ctl0[:, keep]))                           # nothing else of ctl
    # on to the end: row T - 1 has no next row (the command is kept), then p >= T
    for _ in range(2):
        F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
    assert list(tick) == [3, 3, 3]
    score, ctl = b["score"].copy(), b["ctl"].copy()
    for _ in range(2):
        p, inside = F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
        assert list(p) == [3, 3, 3] and not inside.any() and list(tick) == [T, T, T]                      # held at T
        assert not b["action"].view(np.int32).any()                                                       # +0.0
        assert b["score"].tobytes() == score.tobytes() and b["ctl"].tobytes() == ctl.tobytes()            # no scoring
    np.testing.assert_array_equal(bits(ctl[:, cmd]), bits(np.tile(b["log"][0, 2, 6:13], (n, 1))))


def test_the_log_id_is_clamped():
    nu, n, n_log = 2, 5, 3
    b = _buffers(n, nu, n_log, 2, seed=2)
    O, c0 = F.obs_size(nu), R.ctl_fields(nu)["command"][0]
    ids = np.array([-7, 0, 1, 2, 9], np.int32)
    tick = np.zeros(n, np.int32)
    F.follow(nu, b["log"], ids, tick, b["obs"], b["score"], b["ctl"], b["action"])
    for e, want in enumerate([0, 0, 1, 2, 2]):
        np.testing.assert_array_equal(b["action"][e], b["log"][want, 0, O:])
        np.testing.assert_array_equal(b["ctl"][e, c0:c0 + 7], b["log"][want, 1, 6:13])
    assert list(ids) == [-7, 0, 1, 2, 9]


def test_tiny_differences_are_flushed_as_the_library_runs():
    nu = 1
    b = _buffers(1, nu, 1, 1)
    b["log"][0, 0, 0], b["obs"][0, 0] = f32(1.0), f32(1.0) + f32(2.0 ** -23)
    b["log"][0, 0, 1], b["obs"][0, 1] = f32(2.0 ** -70), f32(0)
    F.follow(nu, b["log"], np.zeros(1, np.int32), np.zeros(1, np.int32), b["obs"], b["score"], b["ctl"], b["action"])
    assert b["score"][0, 0] == f32(2.0 ** -46)
    assert f32(2.0 ** -70) * f32(2.0 ** -70) > 0                  # a denormal in IEEE float32 ...
    assert b["score"].view(np.int32)[0, 1] == 0                   # ... below the smallest normal: +0.0 here


# --- the log's forms ------------------------------------------------------------------------
def _consistent_log(T, nu, seed=3, n_log=None):
    """A log as a closed loop leaves it: row p + 1's last_action columns are row p's actions."""
    rng = np.random.default_rng(seed)
    O, last = F.obs_size(nu), 13 + 2 * nu
    shape = (T,) if n_log is None else (n_log, T)
    log = rng.normal(size=shape + (F.log_size(nu),)).astype(f32)
    log[..., 1:, last:last + nu] = log[..., :-1, O:]
    w = log.view(np.int32)
    w[..., 1, O] = NAN_PAYLOAD
    w[..., 2, last] = NAN_PAYLOAD
    w[..., 0, O + 1] = NEG_ZERO
    w[..., 1, last + 1] = NEG_ZERO
    w[..., 0, 3] = NAN_PAYLOAD                                     # a missing sample
    return log


@pytest.mark.parametrize("n_log", [None, 2])
def test_log_from_saved_obs_round_trips(n_log):
    nu, T = 3, 6
    log = _consistent_log(T, nu, n_log=n_log)
    saved = sim2sim.saved_obs_from_log(log)
    assert saved.shape == log.shape[:-2] + (T + 1, F.obs_size(nu))
    back = sim2sim.log_from_saved_obs(saved)
    assert back.dtype == f32 and back.flags.c_contiguous
    np.testing.assert_array_equal(bits(back), bits(log))
    # action p is the last_action columns of row p + 1
    np.testing.assert_array_equal(bits(back[..., :, F.obs_size(nu):]), bits(saved[..., 1:, 13 + 2 * nu:13 + 3 * nu]))
    np.testing.assert_array_equal(bits(back[..., :, :F.obs_size(nu)]), bits(saved[..., :-1, :]))
    broken = log.copy()
    broken[..., 2, F.obs_size(nu)] += 1
    with pytest.raises(native.DuckError, match="not a saved_obs"):
        sim2sim.saved_obs_from_log(broken)
    for bad in (np.zeros((1, 35)), np.zeros((4, 36)), np.zeros(35), np.zeros((4, 17))):
        with pytest.raises(native.DuckError):
            sim2sim.log_from_saved_obs(bad)


def test_save_and_load_round_trip_the_bits(tmp_path):
    nu, T = 14, 5
    log = _consistent_log(T, nu)
    for name in ("log.npz", "log.npy"):
        path = str(tmp_path / name)
        sim2sim.save_log(path, log)
        np.testing.assert_array_equal(bits(sim2sim.load_log(path)), bits(log), err_msg=name)
        np.testing.assert_array_equal(bits(sim2sim.FleetInfer.load_log(path)), bits(log))
    free = np.random.default_rng(4).normal(size=(2, T, F.log_size(nu))).astype(f32)     # actions of no history
    path = str(tmp_path / "free.npz")
    sim2sim.save_log(path, free)
    np.testing.assert_array_equal(bits(sim2sim.load_log(path)), bits(free))
    with pytest.raises(native.DuckError, match="npz"):
        sim2sim.save_log(str(tmp_path / "free.npy"), free)
    # .npz with obs alone is the saved_obs form
    path = str(tmp_path / "obs_only.npz")
    np.savez(path, obs=sim2sim.saved_obs_from_log(log))
    np.testing.assert_array_equal(bits(sim2sim.load_log(path)), bits(log))
    # pickles are not read, other files neither
    pkl = str(tmp_path / "saved_obs.npy")
    np.save(pkl, np.array([{"a": 1}], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError):
        sim2sim.load_log(pkl)
    raw = str(tmp_path / "saved_obs.pkl")
    saved = [row for row in sim2sim.saved_obs_from_log(log)]
    with open(raw, "wb") as f:
        pickle.dump(saved, f)
    with pytest.raises(native.DuckError, match="pickles are not read"):
        sim2sim.load_log(raw)
    # the documented conversion on the user's side
    conv = str(tmp_path / "converted.npy")
    np.save(conv, np.asarray(pickle.load(open(raw, "rb")), dtype=np.float32))
    np.testing.assert_array_equal(bits(sim2sim.load_log(conv)), bits(log))
    np.savez(str(tmp_path / "none.npz"), other=np.zeros(3))
    with pytest.raises(native.DuckError, match="'obs'"):
        sim2sim.load_log(str(tmp_path / "none.npz"))
    np.savez(str(tmp_path / "misfit.npz"), obs=log[:, :F.obs_size(nu)], action=np.zeros((T, nu + 1), f32))
    with pytest.raises(native.DuckError, match="do not fit"):
        sim2sim.load_log(str(tmp_path / "misfit.npz"))


def test_set_logs_validation_errors():
    nu, n = 14, 6
    W = F.log_size(nu)
    log = np.zeros((3, 5, W), f32)
    tab, ids = sim2sim.log_arguments(log, None, n, nu)
    assert tab.shape == (3, 5, W) and tab.dtype == f32 and ids.dtype == np.int32 and list(ids) == [0, 1, 2, 0, 1, 2]
    tab, ids = sim2sim.log_arguments(log[0], None, n, nu)
    assert tab.shape == (1, 5, W) and not ids.any()
    tab, ids = sim2sim.log_arguments(log.astype(np.float64), [2, 2, 1, 1, 0, 0], n, nu)
    assert tab.dtype == f32 and list(ids) == [2, 2, 1, 1, 0, 0]
    bad = [dict(log=np.zeros((5, W - 1))), dict(log=np.zeros((5, F.obs_size(nu)))), dict(log=np.zeros(W)),
           dict(log=np.zeros((1, 2, 5, W))), dict(log=np.zeros((0, W))), dict(log=np.zeros((0, 5, W))),
           dict(log=np.zeros((3, 0, W))), dict(log="a log"),
           dict(log=log, ids=[0, 1, 2, 3, 0, 0]), dict(log=log, ids=[0, -1, 2, 0, 0, 0]), dict(log=log, ids=[0, 1, 2]),
           dict(log=log, ids=np.zeros(n)), dict(log=log, ids=np.zeros((n, 1), int)),
           dict(log=log, scheduled=True)]
    for k, kw in enumerate(bad):
        kw.setdefault("ids", None)
        with pytest.raises(native.DuckError):
            sim2sim.log_arguments(kw.pop("log"), kw.pop("ids"), n, nu, **kw)
    with pytest.raises(native.DuckError, match="schedule"):
        sim2sim.log_arguments(log, None, n, nu, scheduled=True)
    with pytest.raises(native.DuckError, match=rf"\[T\]\[{W}\]"):
        sim2sim.log_arguments(np.zeros((5, W + 1)), None, n, nu)
    with pytest.raises(native.DuckError, match=r"lie in \[0, 3\)"):
        sim2sim.log_arguments(log, [3] * n, n, nu)
    # a NaN is data: a missing sample
    log[0, 0, 0] = np.nan
    assert np.isnan(sim2sim.log_arguments(log, None, n, nu)[0][0, 0, 0])


# --- the score report -------------------------------------------------------------------------
def test_score_report_counts_the_logs_own_words():
    nu, n, T = 2, 3, 4
    O, W = F.obs_size(nu), F.log_size(nu)
    log = np.zeros((2, T, W), f32)
    log[0, :, 0] = np.nan                   # log 0 has no gyro x at all
    log[0, 2:, 3:6] = np.nan                # ... and an accelerometer for two rows only
    log[1, :, 13:13 + nu] = np.nan          # log 1 has no joint positions
    score = np.zeros((n, O), f32)
    score[:, 1], score[:, 2] = 8.0, 10.0    # gyro y, z
    score[:, 3:6] = 6.0
    score[:, 13 + nu] = 2.0                 # a joint velocity
    score[:, 13 + 5 * nu] = 99.0            # a motor target: weight 0 by default
    ids, tick = np.array([0, 1, 0]), np.array([4, 4, 3])
    rep = sim2sim.score_report(score, log, ids, tick)
    assert set(rep) == set(sim2sim.score_groups(nu)) | {"total", "periods"} and list(rep["periods"]) == [4, 4, 3]
    # robot 0, log 0, 4 rows: gyro 2 columns x 4 = 8 words; accelerometer 3 x 2 = 6; robot 2 followed 3 rows
    np.testing.assert_allclose(rep["gyro"], np.sqrt([18 / 8, 18 / 12, 18 / 6]))
    np.testing.assert_allclose(rep["accelerometer"], np.sqrt([18 / 6, 18 / 12, 18 / 6]))
    assert rep["joint_position"][0] == 0 and np.isnan(rep["joint_position"][1])        # no sample: no figure
    np.testing.assert_allclose(rep["joint_velocity"], np.sqrt([2 / 8, 2 / 8, 2 / 6]))
    np.testing.assert_allclose(rep["motor_targets"], np.sqrt([99 / 8, 99 / 8, 99 / 6]))
    assert (rep["contacts"] == 0).all() and (rep["phase"] == 0).all() and (rep["action_history"] == 0).all()
    sensor = [rep[g] for g in sim2sim.SENSOR_GROUPS]
    np.testing.assert_allclose(rep["total"][0], sum(s[0] for s in sensor))
    np.testing.assert_allclose(rep["total"][1], rep["gyro"][1] + rep["accelerometer"][1] + rep["joint_velocity"][1])   # the group without samples is left out
    w = sim2sim.score_report(score, log, ids, tick, {"gyro": 0, "motor_targets": 2.0, "accelerometer": 0.5})
    np.testing.assert_allclose(w["total"][0], 2 * rep["motor_targets"][0] + 0.5 * rep["accelerometer"][0]
                               + rep["joint_position"][0] + rep["joint_velocity"][0])
    # a NaN score (a model that blew up) is a NaN total; so is that of a robot that followed nothing
    score[1, 4] = np.nan
    rep = sim2sim.score_report(score, log, ids, np.array([4, 4, 0]))
    assert np.isnan(rep["total"][1]) and not np.isnan(rep["total"][0])
    assert np.isnan(rep["total"][2]) and np.isnan(rep["gyro"][2])
    with pytest.raises(native.DuckError, match="no score group"):
        sim2sim.score_weights({"gyroscope": 1.0})
    with pytest.raises(native.DuckError, match="finite"):
        sim2sim.score_weights({"gyro": float("nan")})
    doc = sim2sim.FleetInfer.score_report.__doc__
    assert "checks of the feeding, not of the model" in " ".join(doc.split())


# --- the population refinement ------------------------------------------------------------------
def test_refine_population():
    R_, n, elite = 7, 40, 5
    rng = np.random.default_rng(5)
    dr = rng.uniform(0.5, 1.5, size=(R_, n)).astype(f32)
    dr[3] = 1.25                                             # a row the randomisation does not move
    lo, hi = dr.min(1), dr.max(1)
    total = rng.uniform(1, 2, n)
    total[[4, 9]] = np.nan                                   # models that blew up
    total[[17, 30, 2, 8, 21]] = [0.0, 0.1, 0.2, 0.3, 0.4]
    total[11] = 0.4                                          # a tie: the lower id first
    order = sim2sim.rank_totals(total)
    assert list(order[:6]) == [17, 30, 2, 8, 11, 21] and set(order[-2:]) == {4, 9} and sorted(order) == list(range(n))
    new = sim2sim.refine_population(dr, total, elite, np.random.default_rng(6), lo, hi)
    assert new.shape == dr.shape and new.dtype == f32 and new.flags.c_contiguous
    np.testing.assert_array_equal(bits(new[:, :elite]), bits(dr[:, [17, 30, 2, 8, 11]]))       # kept, bit for bit
    assert (new >= lo[:, None]).all() and (new <= hi[:, None]).all()
    assert (new[3] == f32(1.25)).all()
    again = sim2sim.refine_population(dr, total, elite, np.random.default_rng(6), lo, hi)
    assert again.tobytes() == new.tobytes()                                                  # the generator's seed decides
    other = sim2sim.refine_population(dr, total, elite, np.random.default_rng(7), lo, hi)
    assert other.tobytes() != new.tobytes() and other[:, :elite].tobytes() == new[:, :elite].tobytes()
    # the draws gather around the elite: their spread is about the elite's, not the population's
    best = dr[:, order[:elite]]
    rows = [r for r in range(R_) if r != 3]
    assert (np.abs(new[rows, elite:].mean(1) - best[rows].mean(1)) < 3 * best[rows].std(1) + 1e-6).all()
    # a tight box clips
    tight = sim2sim.refine_population(dr, total, elite, np.random.default_rng(6), np.full(R_, 0.9, f32), np.full(R_, 1.0, f32))
    assert (tight[:, elite:] >= f32(0.9)).all() and (tight[:, elite:] <= f32(1.0)).all()
    assert {float(tight[0, elite:].min()), float(tight[0, elite:].max())} == {float(f32(0.9)), float(f32(1.0))}
    # NaN ranks last even when everything else is worse than nothing
    assert sim2sim.rank_totals([np.nan, 5.0, np.inf, 1.0]).tolist() == [3, 1, 2, 0]
    everything = sim2sim.refine_population(dr, total, n, np.random.default_rng(6), lo, hi)
    np.testing.assert_array_equal(bits(everything), bits(dr[:, order]))
    for kw in (dict(elite=0), dict(elite=n + 1), dict(elite=2.5), dict(lo=hi + 1), dict(lo=lo[:-1]), dict(total=total[:-1])):
        args = dict(dr=dr, total=total, elite=elite, rng=np.random.default_rng(0), lo=lo, hi=hi)
        args.update(kw)
        with pytest.raises(native.DuckError):
            sim2sim.refine_population(**args)


# --- the command line -------------------------------------------------------------------------
def test_parser_and_plan():
    parse = sim2sim.parse_arguments
    args = parse(["--follow", "walk.npz", "--num_robots", "64", "--randomize", "3", "--rounds", "4", "--elite", "6",
                  "--follow_weights", "gyro=2, contacts=0.5", "--fit_out", "fit.json", "--delay_grid", "3x3"])
    assert args.onnx_model_path is None and args.follow == "walk.npz"
    plan = sim2sim.follow_plan(args)
    assert plan == {"log": "walk.npz", "weights": {"gyro": 2.0, "contacts": 0.5}, "rounds": 4, "elite": 6, "fit_out": "fit.json"}
    w = sim2sim.score_weights(plan["weights"], 14)
    assert w == {"gyro": 2.0, "accelerometer": 1.0, "joint_position": 1.0, "joint_velocity": 1.0, "action_history": 0.0,
                 "motor_targets": 0.0, "contacts": 0.5, "phase": 0.0}
    # the defaults: one round, the policy still welcome, the elite no larger than the fleet
    args = parse(["-o", "policy.onnx", "--follow", "walk.npy", "--num_robots", "4"])
    assert sim2sim.follow_plan(args) == {"log": "walk.npy", "weights": {}, "rounds": 1, "elite": 4, "fit_out": None}
    # without the flag there is no plan, and the policy is required as before
    args = parse(["-o", "policy.onnx"])
    assert args.follow is None and sim2sim.follow_plan(args) is None
    for argv in ([], ["--rounds", "2", "-o", "p.onnx"], ["-o", "p.onnx", "--fit_out", "fit.json"],
                 ["-o", "p.onnx", "--follow_weights", "gyro=1"],
                 ["--follow", "l.npz", "--rounds", "2"],                          # a search needs a box to search
                 ["--follow", "l.npz", "--rounds", "0"], ["--follow", "l.npz", "--elite", "0"],
                 ["--follow", "l.npz", "--follow_weights", "gyroscope=1"], ["--follow", "l.npz", "--follow_weights", "gyro"],
                 ["--follow", "l.npz", "--follow_weights", "gyro=nan"],
                 ["--follow", "l.npz", "--resample_commands", "10"]):
        with pytest.raises(SystemExit):
            parse(argv)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--follow" in readme and "--rounds" in readme
