"""The fleet loop's disturbances on the GPU (include/duck_fleet.h duck_fleet_disturb; sim2sim.FleetInfer):
the kernel alone against its float32 restatement (tests/fleet_disturb_reference.py), robot identity, then the
loop: graph replay against eager with all three disturbances on, a push as a velocity edit at the right
moment, off means off, noise reaches the policy and not the bookkeeping, the setters and the command line."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native
from open_duck_playground_amd.sim2sim import FleetInfer
from tests import fleet_disturb_reference as D
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, c_dis, commands, dev, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PUSH_TOL = 2.0 ** -22     # x mag: 2 ulp of the accurate cosf / sinf (|.| <= 1) plus the product's rounding


# --- the kernel alone -----------------------------------------------------------------------
def _push_rows(n, rng):
    """first in {3, 0, 1} and interval in {0, 2} mixed over the robots; by turns a fixed magnitude along x, a
    drawn magnitude along x (theta 0: cos and sin are exact), and twice a drawn magnitude and direction."""
    e = np.arange(n)
    push = np.zeros((n, 6), f32)
    push[:, 0], push[:, 1] = np.array([3, 0, 1])[e % 3], np.array([0, 2])[(e // 3) % 2]
    kind = (e // 2) % 4
    lo = rng.uniform(0.1, 0.5, n).astype(f32)
    push[:, 2], push[:, 3] = lo, np.where(kind == 0, lo, lo + f32(0.5))
    tlo = rng.uniform(-3, 3, n).astype(f32)
    push[:, 4] = np.where(kind >= 2, tlo, 0)
    push[:, 5] = np.where(kind == 3, tlo + f32(2.0), push[:, 4])
    return push, kind >= 2


@pytest.mark.parametrize("n,nu,offset", [(1, 14, 0), (17, 3, (1 << 33) + 7), (130, 14, 0), (17, 16, 3)])
def test_disturb_kernel_alone(gpu, n, nu, offset):
    """Seven calls: a segment boundary, the held last segment, first / repeated / never pushes, the last partial
    wave, a global id above 2^32. Measured on MI355X: the worst push increment of a drawn direction against
    float64 is 0.15, 0.32 and 0.23 of its bound at (17, 3), (130, 14) and (17, 16); (1, 14) has none."""
    L = native.lib()
    d = R.make_desc(nu=nu)
    Dc = c_desc(d)
    rng = np.random.default_rng(300 + n + nu)
    O, Cw = R.obs_size(nu), R.ctl_size(nu)
    scale = np.where(rng.random(O) < 0.5, rng.uniform(0.01, 2.0, O), 0.0).astype(f32)
    scale[0], scale[1], scale[O - 1] = 0.1, 0.0, 0.5         # first and last column noisy, column 1 not
    sched = rng.normal(size=(3, 3, 7)).astype(f32)
    ids = rng.integers(-1, 5, n).astype(np.int32)             # some outside [0, 3): clamped
    push, general = _push_rows(n, rng)
    S = c_dis(41, scale, sched, seg_periods=2)
    ctl, qvel = rng.normal(size=(n, Cw)).astype(f32), rng.normal(size=(d.nv, n)).astype(f32)
    tick = np.zeros(n, np.int32)
    # guard rows behind the last robot / the last row
    ctl_d, qvel_d = dev(np.vstack([ctl, np.full((1, Cw), 7, f32)]), gpu), dev(np.vstack([qvel, np.full((1, n), 7, f32)]), gpu)
    tick_d = dev(np.concatenate([tick, np.array([7], np.int32)]), gpu)
    obs_d = torch.full((n + 1, O), 7.0, device=gpu)
    sched_d, ids_d, push_d = dev(sched, gpu), dev(ids, gpu), dev(push, gpu)
    worst, pushes = 0.0, np.zeros(n, int)
    for call in range(7):
        obs = rng.normal(size=(n, O)).astype(f32)
        obs[:, 1] = -0.0                                       # a column of scale 0
        obs_d[:n] = dev(obs, gpu)
        qvel[:2, general] = 0.0                                # a drawn direction: the increment alone is compared
        qvel_d[:2, dev(np.flatnonzero(general), gpu)] = 0.0
        before = qvel.copy()
        out = D.disturb(nu, 41, scale, offset, tick, qvel, ctl, obs, sched=sched, sched_id=ids, seg_periods=2, push=push)
        native.check(L.duck_fleet_disturb(C.byref(Dc), C.byref(S), n, offset, tick_d.data_ptr(), sched_d.data_ptr(),
                                          ids_d.data_ptr(), push_d.data_ptr(), qvel_d.data_ptr(), ctl_d.data_ptr(),
                                          obs_d.data_ptr(), stream(gpu)), L)
        got_obs, got_ctl, got_qvel, got_tick = (t.cpu().numpy() for t in (obs_d, ctl_d, qvel_d, tick_d))
        assert (got_obs[n] == 7).all() and (got_ctl[n] == 7).all() and (got_qvel[d.nv] == 7).all() and got_tick[n] == 7
        np.testing.assert_array_equal(bits(got_obs[:n]), bits(obs))
        assert np.signbit(got_obs[:n, 1]).all()
        np.testing.assert_array_equal(bits(got_ctl[:n]), bits(ctl))
        np.testing.assert_array_equal(got_tick[:n], tick)
        assert (tick == call + 1).all()
        np.testing.assert_array_equal(bits(got_qvel[2:d.nv]), bits(qvel[2:]))
        due = out["due"]
        exact = ~(general & due)                               # no push, or along x: bit for bit
        np.testing.assert_array_equal(bits(got_qvel[:2, exact]), bits(qvel[:2, exact]))
        assert (bits(qvel[:, ~due]) == bits(before[:, ~due])).all()
        g = np.flatnonzero(general & due)
        if len(g):
            th, mag = out["theta"][g].astype(np.float64), out["mag"][g].astype(np.float64)
            err = np.abs(got_qvel[:2, g].astype(np.float64) - np.stack([np.cos(th), np.sin(th)]) * mag)
            worst = max(worst, float((err / (PUSH_TOL * mag)).max()))
        pushes += due
    print(f"disturb n={n} nu={nu}: worst push increment error / bound (2^-22 mag) = {worst:.3f}")
    assert worst <= 1.0
    first, interval = push[:, 0].astype(int), push[:, 1].astype(int)
    want = np.where(first == 0, 0, np.where(interval == 0, 1, 1 + (7 - first) // 2))   # t = 1 .. 7
    np.testing.assert_array_equal(pushes, want)


def test_a_robot_is_its_global_id(gpu):
    """Robot 0 of a 1-robot launch at offset 20 equals robot 20 of a 33-robot launch at offset 0."""
    L = native.lib()
    nu = 14
    d = R.make_desc(nu=nu)
    Dc = c_desc(d)
    rng = np.random.default_rng(7)
    O, Cw = R.obs_size(nu), R.ctl_size(nu)
    scale = rng.uniform(0.01, 1.0, O).astype(f32)
    sched = rng.normal(size=(2, 2, 7)).astype(f32)
    S = c_dis(5, scale, sched, seg_periods=2)
    push = np.tile(np.array([2, 1, 0.1, 1.0, -3.0, 3.0], f32), (33, 1))
    ids = (np.arange(33) % 2).astype(np.int32)
    ctl, qvel = rng.normal(size=(33, Cw)).astype(f32), rng.normal(size=(d.nv, 33)).astype(f32)
    big = dict(tick=dev(np.zeros(33, np.int32), gpu), ctl=dev(ctl, gpu), qvel=dev(qvel, gpu), ids=dev(ids, gpu),
               push=dev(push, gpu), obs=torch.empty(33, O, device=gpu))
    one = dict(tick=dev(np.zeros(1, np.int32), gpu), ctl=dev(ctl[20:21], gpu), qvel=dev(qvel[:, 20:21], gpu),
               ids=dev(ids[20:21], gpu), push=dev(push[20:21], gpu), obs=torch.empty(1, O, device=gpu))
    sched_d = dev(sched, gpu)
    for call in range(5):
        obs = rng.normal(size=(33, O)).astype(f32)
        big["obs"].copy_(dev(obs, gpu))
        one["obs"].copy_(dev(obs[20:21], gpu))
        for b, n, off in ((big, 33, 0), (one, 1, 20)):
            native.check(L.duck_fleet_disturb(C.byref(Dc), C.byref(S), n, off, b["tick"].data_ptr(), sched_d.data_ptr(),
                                              b["ids"].data_ptr(), b["push"].data_ptr(), b["qvel"].data_ptr(),
                                              b["ctl"].data_ptr(), b["obs"].data_ptr(), stream(gpu)), L)
        for name in ("obs", "ctl", "tick"):
            np.testing.assert_array_equal(bits(big[name].cpu().numpy()[20:21]), bits(one[name].cpu().numpy()))
        np.testing.assert_array_equal(bits(big["qvel"].cpu().numpy()[:, 20:21]), bits(one["qvel"].cpu().numpy()))
        assert not np.array_equal(big["obs"].cpu().numpy()[19] - obs[19], big["obs"].cpu().numpy()[20] - obs[20])
    assert int(one["tick"][0]) == 5
    assert not np.array_equal(one["qvel"].cpu().numpy()[:2, 0], qvel[:2, 20])      # pushed at 2, 3, 4, 5


# --- the loop --------------------------------------------------------------------------------
def _all_three(fleet, n):
    table = commands(2 * 4, seed=21).reshape(2, 4, 7)
    fleet.set_command_schedule(table, np.arange(n) % 2, 3)
    fleet.set_pushes(5, 4, (0.1, 0.5), (0.0, 6.0))
    fleet.set_noise(1.0, seed=3)


def test_graph_replay_equals_eager_disturbed(policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 4)
    a = FleetInfer("flat_terrain", policy_file, 8, device=gpu)
    b = FleetInfer("flat_terrain", policy_file, 8, device=gpu)
    _all_three(a, 8)
    _all_three(b, 8)
    assert a.disturbed() and b.disturbed()
    a.run(3)      # the first call is eager
    assert a.graph is None
    a.run(8)      # two replays of the 4-period graph: segments of 3 periods and the pushes at 5 and 9 straddle them
    assert a.graph is not None and a.graph[1] == 4
    b.run(11)
    assert b.graph is None
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in ("ctl", "obs", "acc", "alive", "warm", "tick"):
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()))
    assert (a.tick.cpu().numpy() == 11).all()
    # the schedule did move the command: period 11 reads segment min(11 // 3, 3)
    np.testing.assert_array_equal(a.ctl_field("command").cpu().numpy(), a.sched.cpu().numpy()[np.arange(8) % 2, 3])


def test_push_is_a_velocity_edit_before_the_periods_physics(policy_file, gpu):
    mag = f32(0.3)
    cmd = commands(4, seed=13)
    a = FleetInfer("flat_terrain", policy_file, 4, device=gpu, pushes=(3, 0, float(mag), 0.0))
    b = FleetInfer("flat_terrain", policy_file, 4, device=gpu)
    a.set_commands(cmd)
    b.set_commands(cmd)
    a.run(6)
    b.run(3)
    qvel = b.state()[1]
    qvel[:, 0] = qvel[:, 0] + mag
    b.load_state(qvel=qvel)
    b.run(3)
    assert a.graph is None and b.graph is None
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    np.testing.assert_array_equal(bits(a.ctl.cpu().numpy()), bits(b.ctl.cpu().numpy()))
    c = FleetInfer("flat_terrain", policy_file, 4, device=gpu)       # and the push did change the run
    c.set_commands(cmd)
    c.run(6)
    assert not np.array_equal(c.state()[1], a.state()[1])


def test_off_means_off(policy_file, gpu, monkeypatch):
    cmd = commands(6, seed=14)
    a = FleetInfer("flat_terrain", policy_file, 6, device=gpu)
    b = FleetInfer("flat_terrain", policy_file, 6, device=gpu)
    a.set_commands(cmd)
    b.set_commands(cmd)
    b.set_command_schedule(cmd[:, None, :], np.arange(6), 1)
    b.set_pushes(0, 0, 0.5, 0.0)
    b.set_noise(0.0, seed=1)
    assert not a.disturbed() and b.disturbed()
    assert a._lib is b._lib
    calls, real = [0], a._lib.duck_fleet_disturb

    def counting(*args):
        calls[0] += 1
        return real(*args)
    monkeypatch.setattr(a._lib, "duck_fleet_disturb", counting)
    obs_a = a.run(10, record=True)
    assert calls[0] == 0
    obs_b = b.run(10, record=True)
    assert calls[0] == 10
    np.testing.assert_array_equal(bits(obs_a), bits(obs_b))
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    np.testing.assert_array_equal(bits(a.ctl.cpu().numpy()), bits(b.ctl.cpu().numpy()))
    assert (b.tick.cpu().numpy() == 10).all() and (a.tick.cpu().numpy() == 0).all()


def test_noise_reaches_the_policy_and_not_the_bookkeeping(policy_file, gpu):
    cmd = commands(5, seed=15)
    a = FleetInfer("flat_terrain", policy_file, 5, device=gpu)
    b = FleetInfer("flat_terrain", policy_file, 5, device=gpu, noise=(1.0, 8))
    a.set_commands(cmd)
    b.set_commands(cmd)
    noisy = b.default_noise_scales() != 0
    assert noisy.sum() == 6 + 10 + 14 and b.disturbed() and b.sched is None and b.push is None
    first_a, first_b = a.run(1, record=True)[0], b.run(1, record=True)[0]
    np.testing.assert_array_equal(bits(a.acc.cpu().numpy()), bits(b.acc.cpu().numpy()))     # the true sensors
    np.testing.assert_array_equal(bits(first_a[:, ~noisy]), bits(first_b[:, ~noisy]))
    diff = (first_b.astype(np.float64) - first_a)[:, noisy]
    scale = b.default_noise_scales()[noisy]
    assert (diff != 0).mean() > 0.95 and (np.abs(diff) <= scale * (1 + 1e-6) + 1e-6).all()
    assert len({diff[e].tobytes() for e in range(5)}) == 5
    rest_a, rest_b = a.run(4, record=True), b.run(4, record=True)
    for t in range(4):
        assert not np.array_equal(rest_a[t][:, noisy], rest_b[t][:, noisy])
    assert not np.array_equal(rest_a[-1][:, 41:55], rest_b[-1][:, 41:55])       # the policy saw it: other actions


def test_setters_validate_and_drop_the_graph_when_they_must(policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 2)
    n = 4
    f = FleetInfer("flat_terrain", policy_file, n, device=gpu)
    table = commands(6, seed=22).reshape(2, 3, 7)
    bad = [lambda: f.set_command_schedule(table, [0, 1, 2, 0], 2),            # id out of range
           lambda: f.set_command_schedule(table, [0, 1, 0], 2),               # shape
           lambda: f.set_command_schedule(table[:, :, :6], None, 2),
           lambda: f.set_command_schedule(table, None, 0),
           lambda: f.set_pushes(2.5, 0, 0.1, 0.0),                            # first not integral
           lambda: f.set_pushes(2, -1, 0.1, 0.0),
           lambda: f.set_pushes(2, 0, (0.1, float("inf")), 0.0),
           lambda: f.set_pushes(2, 0, [0.1, 0.2], 0.0),                       # a list is per robot: [N]
           lambda: f.set_noise(float("nan")),
           lambda: f.set_noise(1.0, 0, np.ones(5))]
    for k, call in enumerate(bad):
        with pytest.raises(native.DuckError):
            call()
        assert not f.disturbed(), k
    _all_three(f, n)
    f.run(1)
    f.run(2)
    g = f.graph
    assert g is not None
    f.set_pushes(3, 0, 0.2, 1.0)                      # same buffers: the graph reads the new rows
    f.set_command_schedule(commands(8, seed=23).reshape(2, 4, 7), np.arange(n) % 2, 3)
    f.set_noise(1.0, seed=3)                          # nothing changed
    assert f.graph is g
    f.set_noise(1.0, seed=4)                          # the seed is passed by value
    assert f.graph is None
    f.run(2)
    assert f.graph is not None
    f.set_command_schedule(commands(8, seed=23).reshape(2, 4, 7), np.arange(n) % 2, 5)   # so is seg_periods
    assert f.graph is None
    f.run(2)
    f.set_pushes(None)                                # a disturbance switched off
    assert f.graph is None and f.push is None
    f.restart()
    assert (f.tick == 0).all()
    np.testing.assert_array_equal(f.ctl_field("command").cpu().numpy(), f.sched.cpu().numpy()[np.arange(n) % 2, 0])


def test_command_line_reports_pushes_and_disturbance(policy_file, gpu, tmp_path):
    out = str(tmp_path / "report.json")
    subprocess.run([sys.executable, "-m", "open_duck_playground_amd.sim2sim", "-o", policy_file, "--num_robots", "8",
                    "--periods", "12", "--command_grid", "2x1x1", "--push_grid", "2x2", "--push_at", "5", "--noise", "1",
                    "--resample_commands", "4", "--out", out, "--device", gpu], cwd=ROOT, check=True, timeout=300)
    doc = json.load(open(out))
    assert len(doc["pushes"]) == 4 and sum(r["count"] for r in doc["pushes"]) == 8
    for r in doc["pushes"]:
        assert 0.0 <= r["survival_rate"] <= 1.0 and 0.0 <= r["fell_after_push_rate"] <= 1.0 and r["magnitude"] in (
            pytest.approx(0.1), pytest.approx(1.0))
    assert doc["disturbance"] == {"push_grid": "2x2", "noise": 1.0, "noise_seed": 0, "resample_commands": 4,
                                  "push_at": 5, "push_every": 0, "recovery_window": 100}
    cells = doc["cells"]
    assert len(cells) == 2 and sum(c["count"] for c in cells) == 8
    assert set(cells[0]) == {"command", "count", "survival_rate", "mean_periods", "periods", "mean_vx", "mean_vy",
                             "mean_wz", "rms_lin_err", "rms_yaw_err"}
