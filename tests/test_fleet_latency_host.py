"""Host side of the fleet loop's latency (include/duck_fleet.h duck_fleet_sense_delay, duck_fleet_actuate_delayed;
sim2sim.FleetInfer.set_latency): the C-ABI symbols, constants and refusals, the restatement
(tests/fleet_latency_reference.py) on hand-written rows, and the command line's delay grid and report. No GPU."""

import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from open_duck_playground_amd import cabi, native, sim2sim
from tests import fleet_disturb_reference as D
from tests import fleet_latency_reference as T
from tests import fleet_reference as R
from tests.fleet_helpers import host_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DRAW_SEED = 5        # the seed of test_every_robot_sees_every_delay, pinned


# --- the C ABI --------------------------------------------------------------------------
def test_symbols_and_constants():
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    L = native.lib()
    for name in ("duck_fleet_sense_delay", "duck_fleet_actuate_delayed"):
        assert re.search(rf"^int {name}\(", hdr, flags=re.M)
        assert name in native.EXPORTS and name in cabi.HEADERS.funcs
        assert getattr(L, name).argtypes is not None
    consts = cabi.HEADERS.consts
    assert consts["DUCK_FLEET_MAX_DELAY"] == native.FLEET_MAX_DELAY == T.MAX_DELAY == 2
    assert consts["DUCK_FLEET_LAT_SIZE"] == native.FLEET_LAT_SIZE == T.LAT_SIZE == 4
    assert consts["DUCK_FLEET_LAT_TAG"] == native.FLEET_LAT_TAG == T.LAT_TAG == 0x1A7E
    assert consts["DUCK_FLEET_LAT_TAG"] != consts["DUCK_FLEET_KEY_TAG"]
    # the seed travels by value: no new struct
    sense, act = cabi.HEADERS.funcs["duck_fleet_sense_delay"], cabi.HEADERS.funcs["duck_fleet_actuate_delayed"]
    assert sense[1][2] is C.c_uint64 and sense[1][3] is C.c_int64 and len(sense[1]) == 9
    assert act[1][2] is C.c_uint64 and act[1][3] is C.c_int64 and len(act[1]) == 10


def test_refusals_come_before_any_launch():
    L = native.lib()
    d = host_desc()
    one = C.c_void_p(16)   # (never dereferenced: every call below is refused before any launch)
    for name, nptr in (("duck_fleet_sense_delay", 4), ("duck_fleet_actuate_delayed", 5)):
        f = getattr(L, name)

        def call(desc=C.byref(d), n=1, null=None):
            return f(desc, n, 3, 0, *[None if k == null else one for k in range(nptr)], None)
        assert call(desc=None) == -1 and f"{name}: null pointer".encode() in L.duck_last_error()
        for k in range(nptr):
            assert call(null=k) == -1 and f"{name}: null pointer".encode() in L.duck_last_error(), (name, k)
        for n in (-1, (1 << 27) + 1):
            assert call(n=n) == -1 and f"{name}: bad size".encode() in L.duck_last_error()
        d.nu = 17
        assert call() == -1 and b"nu" in L.duck_last_error()
        d.nu = 14
        d.act_dof[3] = 20
        assert call() == -1 and b"actuator address" in L.duck_last_error()
        d.act_dof[3] = 9
        assert call(n=0) == 0          # an empty fleet


# --- the draw -----------------------------------------------------------------------------
def test_integer_map_stays_inside_its_range():
    words = np.array([0, 1, 0x1FF, 0x200, 0x55555555, 0x55555600, 0x7FFFFFFF, 0x80000000, 0xAAAAAAAA, 0xAAAAAC00,
                      0xFFFFFE00, 0xFFFFFFFF], np.uint64)
    words = np.concatenate([words, np.random.default_rng(0).integers(0, 2 ** 32, 4096, dtype=np.uint64)])
    for lo in range(3):
        for hi in range(lo, 3):
            d = T.draw_map(words, lo, hi)
            assert d.min() >= lo and d.max() <= hi, (lo, hi)
            assert d[0] == lo and d[11] == hi                       # both ends are reached
            if lo == hi:
                assert (d == lo).all()
    # thirds of the 23-bit range: floor(3 u) with u = (word >> 9) / 2^23
    u = (words >> np.uint64(9)).astype(np.float64) / 2 ** 23
    np.testing.assert_array_equal(T.draw_map(words, 0, 2), np.floor(3 * u).astype(np.int64))
    np.testing.assert_array_equal(T.draw_map(words, 1, 2), 1 + np.floor(2 * u).astype(np.int64))


def test_every_robot_sees_every_delay():
    """64 robots x 50 periods over (0, 2) on both words, seed DRAW_SEED with DUCK_FLEET_LAT_TAG: every robot
    sees all three values of both delays, and the three values are about equally frequent."""
    n, periods = 64, 50
    lat = np.tile(np.array([0, 2, 0, 2]), (n, 1))
    seen = np.zeros((2, n, 3), int)
    for p in range(periods):
        a, s = T.delays(DRAW_SEED, 0, np.full(n, p, np.int32), lat)
        seen[0, np.arange(n), a] += 1
        seen[1, np.arange(n), s] += 1
    assert (seen > 0).all()
    total = seen.sum(1)                    # [word][value] of 3200 each
    assert (total.sum(1) == n * periods).all()
    # a third each: 1067 +- 4 sigma of a binomial (sigma = sqrt(3200 * 2 / 9) = 26.7)
    assert (np.abs(total - n * periods / 3) < 4 * 26.7).all(), total
    # the two words are not the same draw, and the stream is not the disturbances'
    a, s = T.delays(DRAW_SEED, 0, np.zeros(n, np.int32), lat)
    assert not np.array_equal(a, s)
    assert not np.array_equal(a, T.delays(DRAW_SEED, 0, np.zeros(n, np.int32), lat, tag=D.KEY_TAG)[0])
    assert not np.array_equal(a, T.delays(DRAW_SEED + 1, 0, np.zeros(n, np.int32), lat)[0])


def test_draws_are_the_global_id_and_the_period():
    n = 40
    lat = np.tile(np.array([0, 2, 0, 2]), (n, 1))
    tick = np.arange(n, dtype=np.int32) % 7
    a0, s0 = T.delays(9, 0, tick, lat)
    a5, s5 = T.delays(9, 5, tick[5:], lat[5:])
    assert a0[5:].tobytes() == a5.tobytes() and s0[5:].tobytes() == s5.tobytes()
    big = T.delays(9, 2 ** 33, np.zeros(n, np.int32), lat)[0]
    assert not np.array_equal(big, T.delays(9, 0, np.zeros(n, np.int32), lat)[0])      # the id's high word counts
    # a negative counter is period 0; a fixed row needs no draw; a bad row is clamped
    neg = T.delays(9, 0, np.full(n, -3, np.int32), lat)
    zero = T.delays(9, 0, np.zeros(n, np.int32), lat)
    assert neg[0].tobytes() == zero[0].tobytes() and neg[1].tobytes() == zero[1].tobytes()
    a, s = T.delays(9, 0, tick, np.tile(np.array([1, 1, 2, 2]), (n, 1)))
    assert (a == 1).all() and (s == 2).all()
    a, s = T.delays(9, 0, tick, np.tile(np.array([-4, -1, 7, 1]), (n, 1)))
    assert (a == 0).all() and (s == 2).all()


# --- the restatement on hand-written rows ---------------------------------------------------
def test_zero_delay_is_the_plain_actuate():
    nu, n = 3, 6
    d = R.make_desc(nu=nu)
    rng = np.random.default_rng(2)
    ctl_a = rng.normal(size=(n, R.ctl_size(nu))).astype(f32)
    ctl_b = ctl_a.copy()
    tick = np.zeros(n, np.int32)
    lat = np.zeros((n, 4), np.int32)
    for call in range(4):
        action = (3 * rng.normal(size=(n, nu))).astype(f32)      # some targets hit the speed limit
        want = R.actuate(d, action, ctl_a)
        got = T.actuate_delayed(d, 1, 0, tick, lat, action, ctl_b)
        assert got.tobytes() == want.tobytes() and ctl_a.tobytes() == ctl_b.tobytes()
        assert (tick == call + 1).all()


def test_fixed_action_delay_takes_the_older_entry():
    nu, n = 2, 3
    d = R.make_desc(nu=nu, speed_limits=0)
    ctl = np.zeros((n, R.ctl_size(nu)), f32)
    tick = np.zeros(n, np.int32)
    lat = np.array([[0, 0, 0, 0], [1, 1, 0, 0], [2, 2, 0, 0]], np.int32)
    default = np.asarray(d.act_default[:nu], f32)
    sent = []
    for call in range(5):
        action = np.full((n, nu), call + 1, f32)
        sent.append(T.actuate_delayed(d, 0, 0, tick, lat, action, ctl).T.copy())
        np.testing.assert_array_equal(ctl[:, :nu], action)            # the history holds the undelayed actions
    for call in range(5):
        for e in range(3):
            used = max(call + 1 - e, 0)                                # the history starts at zero actions
            np.testing.assert_array_equal(sent[call][e], default + f32(used) * d.action_scale)
    assert list(tick) == [5, 5, 5]


def test_delay_line_fills_wraps_and_keeps_bits():
    n, O = 4, R.obs_size(3)
    line, tick = np.zeros((n, 3, 6), f32), np.zeros(n, np.int32)
    lat = np.array([[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 2, 2], [2, 2, 0, 2]], np.int32)
    seen = []
    for p in range(7):
        obs = np.full((n, O), 100.0 + p, f32)
        obs[:, 0] = -0.0 if p == 3 else p
        obs.view(np.int32)[:, 5] = 0x7FC00000 + p                     # a NaN whose payload is the period
        d_eff, wrote = T.sense_delay(7, 0, tick, lat, line, obs)   # seed 7: robot 3 draws 0, 2, 0, 2, 1, 0, 1
        assert list(d_eff[:3]) == [0, min(1, p), min(2, p)] and list(wrote[:3]) == [False, p >= 1, p >= 1]
        assert 0 <= d_eff[3] <= min(2, p)
        assert (obs[:, 6:] == 100.0 + p).all()
        seen.append(obs.view(np.int32)[:, 5] - 0x7FC00000)            # the period the policy's sample is from
        for e in range(n):
            assert seen[-1][e] == p - d_eff[e]
            src = p - d_eff[e]
            assert np.signbit(obs[e, 0]) == (src == 3) and obs[e, 0] == (0 if src == 3 else src)
        tick += 1                                                      # (duck_fleet_actuate_delayed's store)
    assert len({int(s[3]) - p for p, s in enumerate(seen)}) == 3      # robot 3 drew 0, 1 and 2 over the run


# --- the command line -------------------------------------------------------------------------
def test_delay_grid_cells_and_errors():
    g = sim2sim.delay_grid("3x2")
    assert g.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [2, 1]]
    assert sim2sim.delay_grid("1x1").tolist() == [[0, 0]] and len(sim2sim.delay_grid("3X3")) == 9
    for bad in ("3", "0x3", "4x1", "1x4", "axb", "2x2x2", ""):
        with pytest.raises(ValueError, match="delay_grid"):
            sim2sim.delay_grid(bad)


def _args(*argv):
    p = argparse.ArgumentParser()
    p.add_argument("--num_robots", type=int, default=8)
    p.add_argument("--periods", type=int, default=12)
    sim2sim.add_disturbance_arguments(p)
    sim2sim.add_latency_arguments(p)
    return p.parse_args(list(argv))


def test_robots_go_round_robin_over_all_three_grids():
    n, nc, npush, nd = 48, 2, 3, 4
    ccell, pcell = sim2sim.robot_cells(n, nc, npush)
    dcell = sim2sim.robot_delay_cells(n, nc, npush, nd)
    assert list(dcell[:13]) == [0] * 6 + [1] * 6 + [2]
    triples = {(c, q, d) for c, q, d in zip(ccell, pcell, dcell)}
    assert triples == {(c, q, d) for c in range(nc) for q in range(npush) for d in range(nd)}   # every triple is run
    assert list(sim2sim.robot_cells(n, nc, npush)[0]) == [0, 1] * 24                          # and its result stands


def test_latency_plan():
    assert sim2sim.latency_plan(_args(), 2) is None
    with pytest.raises(ValueError, match="delay_grid"):
        sim2sim.latency_plan(_args("--delay_jitter"), 2)
    plan = sim2sim.latency_plan(_args("--num_robots", "18", "--delay_grid", "3x3", "--delay_seed", "7"), 1)
    assert list(plan["cell"]) == list(range(9)) * 2 and plan["cells"].shape == (9, 2)
    a, s, seed = plan["latency"]
    assert list(a) == [0, 0, 0, 1, 1, 1, 2, 2, 2] * 2 and list(s) == [0, 1, 2] * 6 and seed == 7
    assert plan["echo"] == {"delay_grid": "3x3", "delay_jitter": False, "delay_seed": 7}
    jit = sim2sim.latency_plan(_args("--num_robots", "8", "--delay_grid", "2x2", "--delay_jitter"), 2, 1)
    (alo, ahi), (slo, shi), seed = jit["latency"]
    assert not alo.any() and not slo.any() and list(jit["cell"]) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert list(ahi) == [0, 0, 0, 0, 1, 1, 1, 1] and list(shi) == [0, 0, 1, 1, 0, 0, 1, 1] and seed == 0


def test_latency_report_on_synthetic_accumulators():
    cells = sim2sim.delay_grid("2x2")
    #                periods vx vy wz  lin  yaw
    acc = np.array([[10, 0, 0, 0, 0.4, 0.9],
                    [30, 0, 0, 0, 1.2, 2.7],
                    [20, 0, 0, 0, 5.0, 0.0],
                    [0, 0, 0, 0, 0.0, 0.0]], f32)
    rep = {"fell": np.array([True, False, False, True])}
    cell = np.array([0, 0, 1, 3])
    out = sim2sim.latency_report(rep, acc, cell, cells, 30, jitter=True)
    assert [r["cell"] for r in out] == [0, 1, 2, 3] and [r["count"] for r in out] == [2, 1, 0, 1]
    assert [(r["action_delay"], r["sense_delay"]) for r in out] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [(r["action_delay_ms"], r["sense_delay_ms"]) for r in out] == [(0, 0), (0, 20), (20, 0), (20, 20)]
    assert all(r["jitter"] is True and r["periods"] == 30 for r in out)
    assert out[0]["survival_rate"] == 0.5 and out[0]["mean_periods"] == 20.0
    assert out[0]["rms_lin_err"] == pytest.approx(np.sqrt(1.6 / 40)) and out[0]["rms_yaw_err"] == pytest.approx(0.3)
    assert out[1]["survival_rate"] == 1.0 and out[1]["rms_lin_err"] == pytest.approx(0.5) and out[1]["rms_yaw_err"] == 0.0
    assert out[2]["survival_rate"] is None and out[2]["mean_periods"] is None and out[2]["rms_lin_err"] is None
    assert out[3]["survival_rate"] == 0.0 and out[3]["mean_periods"] == 0.0 and out[3]["rms_yaw_err"] is None
    assert set(out[0]) == {"cell", "action_delay", "sense_delay", "action_delay_ms", "sense_delay_ms", "jitter", "count",
                           "survival_rate", "mean_periods", "periods", "rms_lin_err", "rms_yaw_err"}
