"""Host side of the fleet loop's joint-encoder latency (include/duck_fleet.h duck_fleet_sensor_delay;
sim2sim.FleetInfer.set_latency's ``encoder``): the C-ABI symbol, its constant and refusals, the restatement
(tests/fleet_encoder_reference.py) on hand-written rows, the validation of ``encoder``, and the command line's
delay grid, plan and report with and without the third axis. No GPU."""

import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from open_duck_playground_amd import cabi, native, sim2sim
from tests import fleet_encoder_reference as E
from tests import fleet_latency_reference as T
from tests import fleet_reference as R
from tests.fleet_helpers import host_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# --- the C ABI --------------------------------------------------------------------------
def test_symbol_and_constant():
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    L = native.lib()
    name = "duck_fleet_sensor_delay"
    assert re.search(rf"^int {name}\(", hdr, flags=re.M)
    assert name in native.EXPORTS and name in cabi.HEADERS.funcs and getattr(L, name).argtypes is not None
    assert cabi.HEADERS.consts["DUCK_FLEET_ENC_SIZE"] == native.FLEET_ENC_SIZE == E.ENC_SIZE == 2
    f = cabi.HEADERS.funcs[name]
    assert f[1][2] is C.c_uint64 and f[1][3] is C.c_int64 and len(f[1]) == 11      # the seed travels by value
    assert "joint-encoder latency is not modelled" not in hdr


def test_refusals_come_before_any_launch():
    L = native.lib()
    d = host_desc()
    one = C.c_void_p(16)   # (never dereferenced: every call below is refused before any launch)
    name, nptr = "duck_fleet_sensor_delay", 6
    f = getattr(L, name)

    def call(desc=C.byref(d), n=1, null=None):
        return f(desc, n, 3, 0, *[None if k == null else one for k in range(nptr)], None)
    assert call(desc=None) == -1 and f"{name}: null pointer".encode() in L.duck_last_error()
    for k in range(nptr):
        assert call(null=k) == -1 and f"{name}: null pointer".encode() in L.duck_last_error(), k
    for n in (-1, (1 << 27) + 1):
        assert call(n=n) == -1 and f"{name}: bad size".encode() in L.duck_last_error()
    d.nu = 17
    assert call() == -1 and b"nu" in L.duck_last_error()
    d.nu = 14
    d.act_dof[3] = 20
    assert call() == -1 and b"actuator address" in L.duck_last_error()
    d.act_dof[3] = 9
    assert call(n=0) == 0          # an empty fleet


# --- the restatement -------------------------------------------------------------------------
def _stamped(n, nu, p):
    """An observation whose every word tells its column and the period: 1000 p + column."""
    return np.tile(np.arange(R.obs_size(nu), dtype=f32) + f32(1000 * p), (n, 1))


def test_zero_delay_leaves_obs_untouched():
    n, nu = 3, 3
    O = R.obs_size(nu)
    line, eline, tick = np.zeros((n, 3, 6), f32), np.zeros((n, 3, 2 * nu), f32), np.zeros(n, np.int32)
    lat, enc = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.int32)
    for p in range(5):
        obs = _stamped(n, nu, p)
        obs.view(np.int32)[:, 13] = 0x7FC00000 + p       # a NaN payload and a -0 in the encoder columns
        obs[:, 14] = -0.0
        before = obs.copy()
        s_eff, s_wrote, d_eff, wrote = E.sensor_delay(5, 0, tick, lat, enc, line, eline, obs, nu)
        assert not s_eff.any() and not s_wrote.any() and not d_eff.any() and not wrote.any()
        assert obs.tobytes() == before.tobytes()
        assert eline[:, p % 3].tobytes() == before[:, 13:13 + 2 * nu].tobytes()      # the line is kept for every robot
        assert line[:, p % 3].tobytes() == before[:, :6].tobytes()
        tick += 1
    assert O == 35


def test_fixed_delay_returns_the_older_words():
    n, nu = 4, 3
    W = 2 * nu
    line, eline, tick = np.zeros((n, 3, 6), f32), np.zeros((n, 3, W), f32), np.zeros(n, np.int32)
    lat = np.array([[0, 0, 0, 0], [0, 0, 2, 2], [0, 0, 1, 1], [0, 0, 0, 0]], np.int32)
    enc = np.array([[0, 0], [1, 1], [2, 2], [2, 2]], np.int32)
    for p in range(7):
        obs = _stamped(n, nu, p)
        obs.view(np.int32)[:, 13 + W - 1] = 0x7FC00000 + p                # a NaN whose payload is the period
        obs[:, 13] = -0.0 if p == 3 else p
        s_eff, _, d_eff, wrote = E.sensor_delay(7, 0, tick, lat, enc, line, eline, obs, nu)
        assert list(d_eff) == [0, min(1, p), min(2, p), min(2, p)] and list(wrote) == [False] + [p >= 1] * 3
        assert list(s_eff) == [0, min(2, p), min(1, p), 0]                 # the IMU delay is the other table's
        for e in range(n):
            src = p - d_eff[e]                    # once p >= d: period p - d; before that the oldest, period 0
            assert src == max(p - int(enc[e, 0]), 0)
            want = _stamped(1, nu, src)[0, 13:13 + W]
            np.testing.assert_array_equal(obs[e, 14:13 + W - 1], want[1:-1])
            assert obs.view(np.int32)[e, 13 + W - 1] == 0x7FC00000 + src
            assert np.signbit(obs[e, 13]) == (src == 3) and obs[e, 13] == (0 if src == 3 else src)
            np.testing.assert_array_equal(obs[e, :6], _stamped(1, nu, p - s_eff[e])[0, :6])
            # nothing else moves: the command, and everything behind the encoder columns
            np.testing.assert_array_equal(obs[e, 6:13], _stamped(1, nu, p)[0, 6:13])
            np.testing.assert_array_equal(obs[e, 13 + W:], _stamped(1, nu, p)[0, 13 + W:])
        tick += 1


def test_drawn_delay_stays_in_range_and_is_seed_id_period():
    n = 64
    tick = np.arange(n, dtype=np.int32) % 7
    for lo in range(3):
        for hi in range(lo, 3):
            d = E.encoder_delay(9, 0, tick, np.tile([lo, hi], (n, 1)))
            assert d.min() >= lo and d.max() <= hi
            if lo == hi:
                assert (d == lo).all()
    rows = np.tile([0, 2], (n, 1))
    seen = np.zeros((n, 3), int)
    for p in range(50):
        seen[np.arange(n), E.encoder_delay(5, 0, np.full(n, p, np.int32), rows)] += 1
    assert (seen > 0).all()                         # every robot sees every delay
    # (seed, id, p) only: a robot alone at its offset, the id's high word, the seed, a negative counter, a bad row
    d0 = E.encoder_delay(9, 0, tick, rows)
    assert d0[5:].tobytes() == E.encoder_delay(9, 5, tick[5:], rows[5:]).tobytes()
    assert not np.array_equal(E.encoder_delay(9, 2 ** 33, tick, rows), d0)
    assert not np.array_equal(E.encoder_delay(10, 0, tick, rows), d0)
    assert E.encoder_delay(9, 0, np.full(n, -3, np.int32), rows).tobytes() == \
        E.encoder_delay(9, 0, np.zeros(n, np.int32), rows).tobytes()
    assert (E.encoder_delay(9, 0, tick, np.tile([-4, -1], (n, 1))) == 0).all()
    assert (E.encoder_delay(9, 0, tick, np.tile([7, 1], (n, 1))) == 2).all()


def test_block_0_keeps_its_draws():
    """The encoder's draw is block 1: the action and IMU delays of a seed are what they were, whatever the encoder
    table says, and the encoder delay is neither of them."""
    n, nu = 64, 2
    lat = np.tile(np.array([0, 2, 0, 2], np.int32), (n, 1))
    tick = (np.arange(n, dtype=np.int32) * 3) % 11
    a, s = T.delays(5, 0, tick, lat)
    d = E.encoder_delay(5, 0, tick, np.tile([0, 2], (n, 1)))
    assert not np.array_equal(d, a) and not np.array_equal(d, s)
    # the IMU part of the new entry is the old entry on the same inputs, drawn encoder delay or none
    rng = np.random.default_rng(1)
    obs = rng.normal(size=(n, R.obs_size(nu))).astype(f32)
    line = rng.normal(size=(n, 3, 6)).astype(f32)
    for enc in (np.zeros((n, 2), np.int32), np.tile(np.array([0, 2], np.int32), (n, 1))):
        o1, l1, o2, l2 = obs.copy(), line.copy(), obs.copy(), line.copy()
        s1, w1 = T.sense_delay(5, 0, tick, lat, l1, o1)
        s2, w2, _, _ = E.sensor_delay(5, 0, tick, lat, enc, l2, np.zeros((n, 3, 2 * nu), f32), o2, nu)
        assert s1.tobytes() == s2.tobytes() and w1.tobytes() == w2.tobytes() and l1.tobytes() == l2.tobytes()
        assert o1[:, :13].tobytes() == o2[:, :13].tobytes() and o1[:, 13 + 2 * nu:].tobytes() == o2[:, 13 + 2 * nu:].tobytes()
        if not enc.any():
            assert o1.tobytes() == o2.tobytes()
    assert (np.minimum(s, np.minimum(tick, 2)) == s1).all()


# --- set_latency's validation --------------------------------------------------------------------
def test_latency_rows_validates_encoder():
    n = 4
    rows, enc = sim2sim.latency_rows(n, [0, 1, 2, 0], (0, [0, 1, 2, 2]), encoder=(0, [0, 1, 2, 0]))
    assert rows.tolist() == [[0, 0, 0, 0], [1, 1, 0, 1], [2, 2, 0, 2], [0, 0, 0, 2]] and rows.dtype == np.int32
    assert enc.tolist() == [[0, 0], [0, 1], [0, 2], [0, 0]] and enc.dtype == np.int32
    assert sim2sim.latency_rows(n, 1, 2)[1].tolist() == [[0, 0]] * n                 # no encoder: a zero table
    assert sim2sim.latency_rows(n, 0, 0, 2)[1].tolist() == [[2, 2]] * n
    assert not sim2sim.latency_rows(n, None, 2, 2)[0].any() and not sim2sim.latency_rows(n, None, 2, 2)[1].any()
    bad = [(1.5, "encoder must be integers"), (3, r"encoder must lie in \[0, 2\]"), (-1, "encoder must lie in"),
           ((2, 1), r"encoder as \(lo, hi\) needs lo <= hi"), ((1, 2, 2), r"encoder as a tuple is \(lo, hi\), got 3"),
           ([0, 1], r"encoder must be a scalar or \[4\]"), ("a", "encoder must be integers, got 'a'"),
           (float("nan"), "encoder must be integers")]
    for v, message in bad:
        with pytest.raises(native.DuckError, match=message):
            sim2sim.latency_rows(n, 0, 0, encoder=v)
    # the sisters' messages are the same words
    with pytest.raises(native.DuckError, match=r"sense must lie in \[0, 2\]"):
        sim2sim.latency_rows(n, 0, 3)


# --- the command line -------------------------------------------------------------------------
def test_delay_grid_with_and_without_the_encoder_axis():
    """The third field is asked for with ``encoder=True``, as the command line does: tests/test_fleet_latency_host.py
    holds that a plain ``delay_grid("2x2x2")`` is refused, and it still is."""
    g = sim2sim.delay_grid("2x3x2", encoder=True)
    assert g.shape == (12, 3) and g.dtype == np.int32
    assert g.tolist() == [[a, s, e] for a in range(2) for s in range(3) for e in range(2)]
    assert len(sim2sim.delay_grid("3X3x3", encoder=True)) == 27
    assert sim2sim.delay_grid("1x1x1", encoder=True).tolist() == [[0, 0, 0]]
    for two in (sim2sim.delay_grid("3x3"), sim2sim.delay_grid("3x3", encoder=True)):       # today's array, either way
        assert two.dtype == np.int32 and two.tolist() == [[a, s] for a in range(3) for s in range(3)]
    for bad in ("3", "0x3x1", "3x3x4", "1x1x0", "axbxc", "2x2x2x2", "2x2x", ""):
        with pytest.raises(ValueError, match="delay_grid"):
            sim2sim.delay_grid(bad, encoder=True)
    with pytest.raises(ValueError, match="delay_grid wants NAxNS with"):
        sim2sim.delay_grid("2x3x2")


def _args(*argv):
    p = argparse.ArgumentParser()
    p.add_argument("--num_robots", type=int, default=8)
    p.add_argument("--periods", type=int, default=12)
    sim2sim.add_disturbance_arguments(p)
    sim2sim.add_latency_arguments(p)
    return p.parse_args(list(argv))


def test_latency_plan_with_and_without_the_encoder_axis():
    plan = sim2sim.latency_plan(_args("--num_robots", "16", "--delay_grid", "2x2x2", "--delay_seed", "7"), 1)
    assert list(plan["cell"]) == list(range(8)) * 2 and plan["cells"].shape == (8, 3)
    a, s, seed, e = plan["latency"]
    assert list(a) == [0, 0, 0, 0, 1, 1, 1, 1] * 2 and list(s) == [0, 0, 1, 1] * 4 and list(e) == [0, 1] * 8 and seed == 7
    rows, enc = sim2sim.latency_rows(16, a, s, e)                       # and set_latency takes them in that order
    assert rows[:, 1].tolist() == list(a) and enc[:, 0].tolist() == enc[:, 1].tolist() == list(e)
    assert plan["echo"] == {"delay_grid": "2x2x2", "delay_jitter": False, "delay_seed": 7}
    # robots go round-robin over command x push x delay cell
    plan = sim2sim.latency_plan(_args("--num_robots", "24", "--delay_grid", "1x1x3"), 2, 2)
    assert list(plan["cell"]) == [0] * 4 + [1] * 4 + [2] * 4 + [0] * 4 + [1] * 4 + [2] * 4
    jit = sim2sim.latency_plan(_args("--num_robots", "8", "--delay_grid", "1x2x2", "--delay_jitter"), 2, 1)
    (alo, ahi), (slo, shi), seed, (elo, ehi) = jit["latency"]
    assert not alo.any() and not slo.any() and not elo.any() and not ahi.any() and seed == 0
    assert list(shi) == [0, 0, 0, 0, 1, 1, 1, 1] and list(ehi) == [0, 0, 1, 1, 0, 0, 1, 1]
    # without the axis: three arguments, as before
    two = sim2sim.latency_plan(_args("--num_robots", "18", "--delay_grid", "3x3", "--delay_seed", "7"), 1)
    assert len(two["latency"]) == 3 and two["cells"].shape == (9, 2)
    a, s, seed = two["latency"]
    assert list(a) == [0, 0, 0, 1, 1, 1, 2, 2, 2] * 2 and list(s) == [0, 1, 2] * 6 and seed == 7
    assert len(sim2sim.latency_plan(_args("--delay_grid", "2x2", "--delay_jitter"), 1)["latency"]) == 3
    assert "NE" in [a for a in _parser_actions() if a.dest == "delay_grid"][0].metavar


def _parser_actions():
    p = argparse.ArgumentParser()
    sim2sim.add_latency_arguments(p)
    return p._actions


def test_latency_report_with_and_without_the_encoder_axis():
    #                periods vx vy wz  lin  yaw
    acc = np.array([[10, 0, 0, 0, 0.4, 0.9],
                    [30, 0, 0, 0, 1.2, 2.7],
                    [20, 0, 0, 0, 5.0, 0.0]], f32)
    rep = {"fell": np.array([True, False, False])}
    cell = np.array([0, 0, 5])
    out = sim2sim.latency_report(rep, acc, cell, sim2sim.delay_grid("1x2x3", encoder=True), 30)
    assert [(r["action_delay"], r["sense_delay"], r["encoder_delay"]) for r in out] == \
        [(0, s, e) for s in range(2) for e in range(3)]
    assert [r["encoder_delay_ms"] for r in out] == [0.0, 20.0, 40.0] * 2 and [r["count"] for r in out] == [2, 0, 0, 0, 0, 1]
    assert out[0]["survival_rate"] == 0.5 and out[0]["mean_periods"] == 20.0 and out[5]["rms_lin_err"] == pytest.approx(0.5)
    base = {"cell", "action_delay", "sense_delay", "action_delay_ms", "sense_delay_ms", "jitter", "count",
            "survival_rate", "mean_periods", "periods", "rms_lin_err", "rms_yaw_err"}
    assert set(out[0]) == base | {"encoder_delay", "encoder_delay_ms"}
    two = sim2sim.latency_report(rep, acc, np.array([0, 0, 1]), sim2sim.delay_grid("1x2"), 30)
    assert set(two[0]) == base and [r["count"] for r in two] == [2, 1]
    assert two[0]["survival_rate"] == out[0]["survival_rate"] and two[1]["rms_lin_err"] == out[5]["rms_lin_err"]
