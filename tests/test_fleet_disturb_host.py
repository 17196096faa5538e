"""Host side of the fleet loop's disturbances (include/duck_fleet.h duck_fleet_disturb; sim2sim.FleetInfer's
set_command_schedule / set_pushes / set_noise): the C-ABI symbol, its structure and refusals, the float32
restatement (tests/fleet_disturb_reference.py) on hand-written rows, push_report and the command line's
plan. No GPU."""

import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from open_duck_playground_amd import native, sim2sim
from tests import fleet_disturb_reference as D
from tests import fleet_reference as R
from tests.fleet_helpers import host_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# --- the C ABI --------------------------------------------------------------------------
def test_symbol_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    assert re.search(r"^int duck_fleet_disturb\(", hdr, flags=re.M)
    assert "duck_fleet_disturb" in native.EXPORTS
    L = native.lib()
    assert hasattr(L, "duck_fleet_disturb") and L.duck_fleet_disturb.argtypes is not None
    assert int(re.search(r"#define DUCK_FLEET_PUSH_SIZE (\d+)", hdr).group(1)) == native.FLEET_PUSH_SIZE == D.PUSH_SIZE
    assert int(re.search(r"#define DUCK_FLEET_KEY_TAG 0x([0-9A-Fa-f]+)u", hdr).group(1), 16) == D.KEY_TAG


def test_refusals_come_before_any_launch():
    L = native.lib()
    d, s = host_desc(), native.DuckFleetDisturbance()
    one = C.c_void_p(16)   # (never dereferenced: every call below is refused before any launch)
    D_, S_ = C.byref(d), C.byref(s)

    def call(desc=D_, dis=S_, n=1, tick=one, sched=None, sched_id=None, push=None, qvel=one, ctl=one, obs=one):
        return L.duck_fleet_disturb(desc, dis, n, 0, tick, sched, sched_id, push, qvel, ctl, obs, None)

    for kw in (dict(desc=None), dict(dis=None), dict(tick=None), dict(qvel=None), dict(ctl=None), dict(obs=None)):
        assert call(**kw) == -1 and b"duck_fleet_disturb: null pointer" in L.duck_last_error(), kw
    s.n_sched, s.n_seg, s.seg_periods = 1, 1, 1
    assert call(sched=one) == -1 and b"needs sched_id" in L.duck_last_error()
    for field in ("n_sched", "n_seg", "seg_periods"):
        setattr(s, field, 0)
        assert call(sched=one, sched_id=one) == -1 and b"n_sched, n_seg, seg_periods >= 1" in L.duck_last_error(), field
        setattr(s, field, 1)
    s.n_sched = s.n_seg = s.seg_periods = 0      # without a schedule the shape is unused
    for n in (-1, (1 << 27) + 1):
        assert call(n=n) == -1 and b"bad size" in L.duck_last_error()
    d.nu = 17
    assert call() == -1 and b"nu" in L.duck_last_error()
    d.nu = 14
    d.act_dof[3] = 20
    assert call() == -1 and b"actuator address" in L.duck_last_error()
    d.act_dof[3] = 9
    d.nv, d.nq = 1, 21
    for a in range(14):
        d.act_dof[a] = 0
    assert call(push=one) == -1 and b"nv >= 2" in L.duck_last_error()
    d = host_desc()
    assert L.duck_fleet_disturb(C.byref(d), S_, 0, 0, one, None, None, one, one, one, one, None) == 0   # an empty fleet


# --- the restatement on hand-written rows ---------------------------------------------------
def _blank(n, nu=3, nv=12):
    return (np.zeros(n, np.int32), np.zeros((nv, n), f32), np.zeros((n, R.ctl_size(nu)), f32),
            np.zeros((n, R.obs_size(nu)), f32))


def test_push_is_due_at_first_and_every_interval():
    n, nu = 4, 3
    tick, qvel, ctl, obs = _blank(n, nu)
    #        first interval mag_lo mag_hi theta_lo theta_hi
    push = np.array([[3, 4, 0.5, 0.5, 0.0, 0.0],     # at 3, 7, 11
                     [3, 0, 0.5, 0.5, 0.0, 0.0],     # at 3 only
                     [0, 4, 0.5, 0.5, 0.0, 0.0],     # never: first == 0
                     [1, 1, 0.25, 0.25, 0.0, 0.0]], f32)   # before every period from 1 on
    when = [[] for _ in range(n)]
    for call in range(12):
        out = D.disturb(nu, 5, np.zeros(R.obs_size(nu), f32), 0, tick, qvel, ctl, obs, push=push)
        for e in np.flatnonzero(out["due"]):
            when[e].append(call + 1)      # the call of period p = call decides period t = call + 1
    assert when == [[3, 7, 11], [3], [], list(range(1, 13))]
    assert list(tick) == [12] * n
    assert list(qvel[0]) == [1.5, 0.5, 0.0, 3.0] and not qvel[1:].any()       # theta 0: x only, exactly
    assert not D.push_due(0, 0, 0) and not D.push_due(4, 0, 4) and D.push_due(3, 3, 0) and not D.push_due(6, 3, 0)


def test_push_ranges_and_direction():
    n, nu = 64, 3
    tick, qvel, ctl, obs = _blank(n, nu)
    push = np.tile(np.array([1, 0, 0.1, 1.0, -1.0, 2.0], f32), (n, 1))
    out = D.disturb(nu, 9, np.zeros(R.obs_size(nu), f32), 0, tick, qvel, ctl, obs, push=push)
    assert out["due"].all() and (out["mag"] >= f32(0.1)).all() and (out["mag"] <= f32(1.0)).all()
    assert (out["theta"] >= -1).all() and (out["theta"] <= 2).all() and len(set(out["mag"])) > 32
    np.testing.assert_allclose(np.hypot(qvel[0], qvel[1]), out["mag"], rtol=1e-6)
    np.testing.assert_allclose(np.arctan2(qvel[1], qvel[0]), out["theta"], atol=1e-6)
    assert not qvel[2:].any()


def test_last_segment_is_held_and_ids_are_clamped():
    n, nu = 3, 3
    tick, qvel, ctl, obs = _blank(n, nu)
    sched = np.arange(2 * 3 * 7, dtype=f32).reshape(2, 3, 7)
    ids = np.array([0, 1, 7], np.int32)         # 7 is clamped to the last schedule
    c0 = R.ctl_fields(nu)["command"][0]
    seen = []
    for call in range(9):
        D.disturb(nu, 0, np.zeros(R.obs_size(nu), f32), 0, tick, qvel, ctl, obs, sched=sched, sched_id=ids, seg_periods=2)
        seen.append(int(ctl[0, c0]) // 7)       # the segment robot 0's command of period call + 1 comes from
        assert ctl[1, c0:c0 + 7].tobytes() == ctl[2, c0:c0 + 7].tobytes()
        assert ctl[1, c0] == ctl[0, c0] + 21
    assert seen == [0, 1, 1, 2, 2, 2, 2, 2, 2]   # t = 1 .. 9 at two periods a segment, three segments
    assert not ctl[:, :c0].any() and not ctl[:, c0 + 7:].any() and not obs.any() and not qvel.any()


def test_noise_bounds_zero_scale_and_independence():
    n, nu = 40, 3
    O = R.obs_size(nu)
    tick, qvel, ctl, obs = _blank(n, nu)
    scale = np.zeros(O, f32)
    scale[[0, 5, 16, 17, 33, O - 1]] = [0.1, 0.05, 0.03, 2.5, 1.0, 0.5]
    obs[:, 1] = -0.0
    base = np.linspace(-1, 1, n * O, dtype=f32).reshape(n, O)
    base[:, 1] = -0.0
    rows = []
    for call in range(4):
        obs[:] = base
        D.disturb(nu, 77, scale, 0, tick, qvel, ctl, obs)
        rows.append(obs.astype(np.float64) - base)     # exact
        assert np.signbit(obs[:, 1]).all() and (obs[:, 1] == 0).all()        # scale 0: the -0 keeps its bits
        assert obs[:, scale == 0].tobytes() == base[:, scale == 0].tobytes()
    d = np.array(rows)                                     # [period][robot][column]
    # |2u - 1| <= 1 and the product is at most the scale; the sum rounds by at most 2^-24 of itself
    assert (np.abs(d) <= scale + 2.0 ** -23 * (np.abs(base) + scale)).all()
    on = np.flatnonzero(scale)
    assert (np.abs(d[..., on]).max((0, 1)) > 0.8 * scale[on]).all()          # and the range is used
    assert len({d[0, e, on].tobytes() for e in range(n)}) == n               # differs between robots
    assert len({d[p, 0, on].tobytes() for p in range(4)}) == 4               # and between periods
    assert len({float(v) for v in (d[0, 0, on] / scale[on])}) == len(on)     # and between columns
    # another seed, another stream; robot e at offset 5 is robot e + 5 (on a zero row the noise itself is left)
    def fresh(seed, offset):
        tick[:] = 0
        obs[:] = 0
        D.disturb(nu, seed, scale, offset, tick, qvel, ctl, obs)
        return obs.copy()
    a, b, c = fresh(77, 0), fresh(78, 0), fresh(77, 5)
    assert not np.array_equal(a, b)
    assert a[5:].tobytes() == c[:n - 5].tobytes() and a[:n - 5].tobytes() != c[:n - 5].tobytes()


def test_slots_pair_columns_sixteen_apart():
    k = np.arange(113)
    slot = D.noise_slot(k)
    assert len(set(slot)) == len(k) and slot.min() == 2          # distinct, behind the push's block 0
    even = k[(k // 16) % 2 == 0]
    even = even[even + 16 < 113]
    assert (slot[even] % 2 == 0).all() and (slot[even + 16] == slot[even] + 1).all()   # one block, both words
    assert ((slot // 2 - 1) % 16 == k % 16).all()                # a lane's blocks are its own


def test_key_is_the_global_robot_id():
    a = D.derive_key(3, [0, 1, 2 ** 32 + 1], D.KEY_TAG)
    b = D.derive_key(3, [1], D.KEY_TAG)
    assert a[0][1] == b[0][0] and a[1][1] == b[1][0]
    assert (a[0][2], a[1][2]) != (a[0][1], a[1][1])              # the id's high word counts
    assert D.derive_key(4, [1], D.KEY_TAG)[0][0] != b[0][0]


# --- push_report ------------------------------------------------------------------------------
def test_push_report_on_a_hand_made_vector():
    #                      never fell | fell at 12 (push at 10) | fell at 4 (before) | fell at 25 (push at 20) | at 19: late
    rep = {"periods": np.array([30.0, 12.0, 4.0, 25.0, 19.0, 30.0]),
           "fell": np.array([False, True, True, True, True, False])}
    cells = np.array([0, 0, 1, 1, 1, 2])
    out = sim2sim.push_report(rep, cells, first=10, interval=10, n_periods=30, window=6)
    assert [r["count"] for r in out] == [2, 3, 1] and [r["cell"] for r in out] == [0, 1, 2]
    assert out[0]["survival_rate"] == 0.5 and out[0]["fell_after_push_rate"] == 0.5
    assert out[1]["survival_rate"] == 0.0 and out[1]["fell_after_push_rate"] == pytest.approx(1 / 3)
    assert out[2]["survival_rate"] == 1.0 and out[2]["fell_after_push_rate"] == 0.0
    once = sim2sim.push_report(rep, cells, first=10, interval=0, n_periods=30, window=6)
    assert once[1]["fell_after_push_rate"] == 0.0            # a single push at 10: the fall at 25 is not its
    wide = sim2sim.push_report(rep, cells, first=10, interval=0, n_periods=30, window=16)
    assert wide[1]["fell_after_push_rate"] == pytest.approx(2 / 3)
    never = sim2sim.push_report(rep, cells, first=0, interval=10, n_periods=30, window=100)
    assert [r["fell_after_push_rate"] for r in never] == [0.0, 0.0, 0.0]


# --- the command line -------------------------------------------------------------------------
def _args(*argv):
    p = argparse.ArgumentParser()
    p.add_argument("--num_robots", type=int, default=8)
    p.add_argument("--periods", type=int, default=12)
    sim2sim.add_disturbance_arguments(p)
    return p.parse_args(list(argv))


def test_no_flag_is_no_plan():
    assert sim2sim.disturbance_plan(_args(), sim2sim.command_grid("2x1x1")) is None


def test_push_grid_cells():
    g = sim2sim.push_grid("2x4")
    assert g.shape == (8, 2) and g.dtype == f32
    assert sorted(set(g[:, 0])) == [f32(0.1), f32(1.0)]                  # push_config.magnitude_range, ends included
    np.testing.assert_allclose(sorted(set(g[:, 1])), [0, np.pi / 2, np.pi, 3 * np.pi / 2], rtol=1e-6)   # 2 pi excluded
    assert sim2sim.push_grid("1x1")[0, 0] == f32(0.55)
    for bad in ("2", "0x3", "axb", "2x2x2"):
        with pytest.raises(ValueError, match="push_grid"):
            sim2sim.push_grid(bad)


def test_plan_assigns_robots_round_robin():
    cells = sim2sim.command_grid("2x1x1")
    args = _args("--num_robots", "12", "--push_grid", "1x3", "--push_at", "5", "--push_every", "4", "--noise", "1",
                 "--noise_seed", "9", "--resample_commands", "4")
    plan = sim2sim.disturbance_plan(args, cells)
    ccell, pcell = sim2sim.robot_cells(12, 2, 3)
    assert list(ccell) == [0, 1] * 6 and list(pcell) == [0, 0, 1, 1, 2, 2] * 2
    assert {(c, q) for c, q in zip(ccell, pcell)} == {(c, q) for c in range(2) for q in range(3)}   # every pair is run
    first, every, mag, theta = plan["pushes"]
    assert (first, every) == (5, 4) and list(plan["push_cell"]) == list(pcell)
    assert (mag == f32(0.55)).all() and theta.tobytes() == plan["push_cells"][pcell, 1].tobytes()
    table, ids, seg = plan["schedule"]
    assert table.shape == (2, 3, 7) and seg == 4 and list(ids) == list(ccell)      # 12 periods: 3 segments of 4
    assert table[0, 0].tobytes() == cells[0].tobytes() and table[0, 1].tobytes() == cells[1].tobytes()
    assert table[1, 0].tobytes() == cells[1].tobytes() and table[1, 1].tobytes() == cells[0].tobytes()
    assert plan["echo"] == {"push_grid": "1x3", "noise": 1.0, "noise_seed": 9, "resample_commands": 4, "push_at": 5,
                            "push_every": 4, "recovery_window": 100}
    only_noise = sim2sim.disturbance_plan(_args("--noise", "0.5"), cells)
    assert only_noise["pushes"] is None and only_noise["schedule"] is None and "push_at" not in only_noise["echo"]
    with pytest.raises(ValueError, match="push_at"):
        sim2sim.disturbance_plan(_args("--push_grid", "1x1", "--push_at", "0"), cells)


def test_default_noise_scales_follow_the_training_config():
    from open_duck_playground_amd import config
    cfg = config.default_config()
    sc = cfg.noise_config.scales
    s = sim2sim.default_noise_scales(14)
    assert s.shape == (101,)
    assert (s[0:3] == sc.gyro).all() and (s[3:6] == sc.accelerometer).all() and not s[6:13].any()
    np.testing.assert_array_equal(s[13:27], config.qpos_noise_scale(cfg, 14))
    np.testing.assert_allclose(s[27:41], sc.joint_vel * 0.05)
    assert not s[41:].any()          # actions, motor targets, contacts and the phase are not sensors
