"""The fleet loop's latency on the GPU (include/duck_fleet.h duck_fleet_sense_delay, duck_fleet_actuate_delayed;
sim2sim.FleetInfer.set_latency): the two kernels alone against their numpy restatement
(tests/fleet_latency_reference.py) and their refusals, then the loop: zero latency is the plain loop, fixed
delays teacher-forced from the recorder's frames, robot identity, graph replay against eager, the replay of a
recorded robot, and the command line. Every comparison is bit for bit."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests import fleet_latency_reference as T
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, commands, dev, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GUARD = f32(7.0)
NAN_PAYLOAD, NEG_ZERO = np.int32(0x7FC12345), np.int32(-0x80000000)


# --- the kernels alone ----------------------------------------------------------------------
ROWS = np.array([[0, 2, 0, 2], [1, 2, 0, 1], [0, 1, 1, 2], [0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2]], np.int32)


@pytest.mark.parametrize("n,nu,offset", [(1, 14, 0), (17, 3, (1 << 33) + 7), (130, 14, 0), (17, 16, 3)])
def test_latency_kernels_alone(gpu, n, nu, offset):
    """Seven periods of sense_delay then actuate_delayed on fresh observations and actions: the slots wrap and the
    fill clamp is passed; rows of fixed 0 / 1 / 2 and drawn ranges; NaN payloads and -0 in the IMU columns; a
    guard row behind the last robot in every buffer; the last partial wave; a global id above 2^32."""
    L = native.lib()
    d = R.make_desc(nu=nu)
    Dc = c_desc(d)
    seed = 41
    rng = np.random.default_rng(500 + n + nu)
    O, Cw = R.obs_size(nu), R.ctl_size(nu)
    lat = ROWS[np.arange(n) % len(ROWS)]
    ctl, line, tick = rng.normal(size=(n, Cw)).astype(f32), np.zeros((n, 3, 6), f32), np.zeros(n, np.int32)
    guard = lambda a: np.concatenate([a, np.full((1,) + a.shape[1:], 7, a.dtype)])  # noqa: E731
    ctl_d, line_d, tick_d, lat_d = (dev(guard(a), gpu) for a in (ctl, line, tick, lat))
    obs_d = torch.full((n + 1, O), float(GUARD), device=gpu)
    act_d = torch.full((n + 1, nu), float(GUARD), device=gpu)
    ctrl_d = torch.full((nu + 1, n), float(GUARD), device=gpu)
    delayed_obs = delayed_act = 0
    for call in range(7):
        obs = rng.normal(size=(n, O)).astype(f32)
        w = obs.view(np.int32)
        w[:, call % 6] = NAN_PAYLOAD + call                       # a NaN whose payload tells the period
        w[:, (call + 3) % 6] = NEG_ZERO
        obs_d[:n] = dev(obs, gpu)
        before = obs.copy()
        d_eff, wrote = T.sense_delay(seed, offset, tick, lat, line, obs)
        native.check(L.duck_fleet_sense_delay(C.byref(Dc), n, seed, offset, tick_d.data_ptr(), lat_d.data_ptr(),
                                              line_d.data_ptr(), obs_d.data_ptr(), stream(gpu)), L)
        got_obs, got_line, got_tick = obs_d.cpu().numpy(), line_d.cpu().numpy(), tick_d.cpu().numpy()
        np.testing.assert_array_equal(bits(got_obs[:n]), bits(obs))
        np.testing.assert_array_equal(bits(got_obs[:n, 6:]), bits(before[:, 6:]))            # columns >= 6 untouched
        np.testing.assert_array_equal(bits(got_obs[:n][~wrote]), bits(before[~wrote]))       # d_eff == 0: as observed
        np.testing.assert_array_equal(bits(got_line[:n]), bits(line))
        np.testing.assert_array_equal(got_tick[:n], tick)                                    # not the sense kernel's
        assert (tick == call).all()
        assert (got_obs[n] == GUARD).all() and (got_line[n] == GUARD).all() and got_tick[n] == 7
        delayed_obs += int(wrote.sum())

        action = (3 * rng.normal(size=(n, nu))).astype(f32)        # some targets hit the speed limit
        act_d[:n] = dev(action, gpu)
        a_delay = T.delays(seed, offset, tick, lat)[0]
        ctrl = T.actuate_delayed(d, seed, offset, tick, lat, action, ctl)
        native.check(L.duck_fleet_actuate_delayed(C.byref(Dc), n, seed, offset, tick_d.data_ptr(), lat_d.data_ptr(),
                                                  act_d.data_ptr(), ctl_d.data_ptr(), ctrl_d.data_ptr(), stream(gpu)), L)
        got_ctl, got_ctrl, got_tick = ctl_d.cpu().numpy(), ctrl_d.cpu().numpy(), tick_d.cpu().numpy()
        np.testing.assert_array_equal(bits(got_ctl[:n]), bits(ctl))
        np.testing.assert_array_equal(bits(got_ctrl[:nu]), bits(ctrl))
        np.testing.assert_array_equal(got_tick[:n], tick)
        assert (tick == call + 1).all()
        assert (got_ctl[n] == GUARD).all() and (got_ctrl[nu] == GUARD).all() and got_tick[n] == 7
        np.testing.assert_array_equal(lat_d.cpu().numpy()[:n], lat)
        delayed_act += int((a_delay > 0).sum())
    # the run did what it was built for
    drawn = lat[:, 1] > lat[:, 0]
    assert delayed_obs > 0 and delayed_act > 0 and drawn.any()
    if n > 1:
        assert (lat[:, 3] == 0).any() and (lat[:, 2] == 2).any()


def test_latency_arguments(gpu):
    L = native.lib()
    n, nu = 5, 3
    d = R.make_desc(nu=nu)
    D = c_desc(d)
    O, Cw = R.obs_size(nu), R.ctl_size(nu)
    EINVAL, OK = native.HEADERS.consts["DUCK_EINVAL"], native.HEADERS.consts["DUCK_OK"]
    tick = torch.zeros(n, dtype=torch.int32, device=gpu)
    lat = dev(np.tile(np.array([1, 1, 1, 1], np.int32), (n, 1)), gpu)
    line, obs = torch.zeros(n, 3, 6, device=gpu), torch.full((n, O), 2.0, device=gpu)
    action, ctl, ctrl = torch.ones(n, nu, device=gpu), torch.zeros(n, Cw, device=gpu), torch.zeros(nu, n, device=gpu)
    cases = (("duck_fleet_sense_delay", [tick, lat, line, obs]),
             ("duck_fleet_actuate_delayed", [tick, lat, action, ctl, ctrl]))
    for name, tensors in cases:
        f = getattr(L, name)
        ptrs = [t.data_ptr() for t in tensors]

        def call(desc=D, n=n, null=None):
            p = [None if k == null else v for k, v in enumerate(ptrs)]
            return f(None if desc is None else C.byref(desc), n, 3, 0, *p, stream(gpu))
        assert call(desc=None) == EINVAL and f"{name}: null pointer".encode() in L.duck_last_error()
        for k in range(len(ptrs)):
            assert call(null=k) == EINVAL and f"{name}: null pointer".encode() in L.duck_last_error(), (name, k)
        for bad in (-1, (1 << 27) + 1):
            assert call(n=bad) == EINVAL and f"{name}: bad size".encode() in L.duck_last_error()
        wide = c_desc(d)
        wide.nu = 17
        assert call(desc=wide) == EINVAL and f"{name}: nq, nv >= 1".encode() in L.duck_last_error()
        assert call(n=0) == OK
    torch.cuda.synchronize()
    assert (tick == 0).all() and (line == 0).all() and (ctl == 0).all() and (ctrl == 0).all()      # nothing ran
    native.check(L.duck_fleet_sense_delay(C.byref(D), n, 3, 0, *[t.data_ptr() for t in cases[0][1]], stream(gpu)), L)
    native.check(L.duck_fleet_actuate_delayed(C.byref(D), n, 3, 0, *[t.data_ptr() for t in cases[1][1]], stream(gpu)), L)
    assert (tick == 1).all() and (line[:, 0] == 2).all() and (line[:, 1:] == 0).all() and (ctl[:, :nu] == 1).all()


# --- the loop --------------------------------------------------------------------------------
def _disturbed_fleet(path, n, gpu, **kw):
    """DR, a 3-segment schedule, drawn pushes first at period 2 and every 3 after, noise at level 1."""
    table = commands(2 * 3, seed=21).reshape(2, 3, 7)
    return FleetInfer("flat_terrain", path, n, device=gpu, randomize=7, command_schedule=(table, np.arange(n) % 2, 5),
                      pushes=(2, 3, (0.1, 0.5), (0.0, 6.0)), noise=(1.0, 3), **kw)


LOOP_BUFFERS = ("warm", "ctl", "obs", "action", "acc", "alive", "tick", "aux")


def _assert_same_loop(a, b, names=LOOP_BUFFERS):
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in names:
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()),
                                      err_msg=name)


def test_zero_latency_is_the_plain_loop(policy_file, gpu, monkeypatch):
    n, periods = 33, 12
    a = _disturbed_fleet(policy_file, n, gpu)
    a.run(periods)
    # an all-zero table through both new entries, period by period
    b = _disturbed_fleet(policy_file, n, gpu)
    b._load_latency(np.zeros((n, 4), np.int32), 9)
    assert b.latent() and not b.lat_sense
    for _ in range(periods):
        b._physics(b.decimation)
        b.observe()
        b.sense_delay()
        b.disturb()
        b.policy()
        b.actuate_delayed()
    torch.cuda.synchronize()
    _assert_same_loop(a, b)
    assert (b.lat_tick.cpu().numpy() == periods).all()
    # and switched off, the loop never enters them
    c = _disturbed_fleet(policy_file, n, gpu, latency=(0, 0, 5))
    assert not c.latent()
    c.set_latency(1, (0, 2), 5)
    assert c.latent() and c.lat_sense
    c.set_latency(None)
    assert not c.latent() and c.lat is None and c.lat_tick is None and c.line is None
    calls = [0]
    for name in ("duck_fleet_sense_delay", "duck_fleet_actuate_delayed"):
        real = getattr(c._lib, name)

        def counting(*args, real=real):
            calls[0] += 1
            return real(*args)
        monkeypatch.setattr(c._lib, name, counting)
    c.run(periods)
    assert calls[0] == 0
    _assert_same_loop(a, c)


@pytest.mark.parametrize("action,sense", [(1, 0), (0, 2), (2, 1)])
def test_fixed_delays_teacher_forced(policy_file, gpu, action, sense):
    """An eager run with a recorder; per period the restatement is applied to the GPU's own previous control
    record, its raw sensors and its actions, and reproduces ctl, ctrl and the IMU columns the policy saw."""
    n, periods, seed = 5, 8, 13
    fleet = FleetInfer("flat_terrain", policy_file, n, device=gpu, recorder=(periods, 0), latency=(action, sense, seed))
    fleet.set_commands(commands(n, seed=33))
    assert fleet.latent() and fleet.lat_sense == (sense > 0)
    nu = fleet.num_dofs
    d = R.desc_values(fleet.desc)
    ctl_prev = fleet.ctl.cpu().numpy()
    seen = fleet.run(periods, record=True)
    assert fleet.graph is None
    recs = [fleet.recorded(e) for e in range(n)]
    assert all(list(r["period"]) == list(range(1, periods + 1)) for r in recs)
    frame = lambda name, t: np.stack([r[name][t] for r in recs])  # noqa: E731
    lat = np.tile(np.array([action, action, sense, sense], np.int32), (n, 1))
    np.testing.assert_array_equal(fleet.lat.cpu().numpy(), lat)
    tick, line = np.zeros(n, np.int32), np.zeros((n, 3, 6), f32)
    undelayed = 0
    for t in range(periods):
        # the IMU columns: duck_fleet_observe's words from the frame's raw sensors, then the delay
        sensors = frame("sensors", t)
        obs = frame("obs", t).copy()
        obs[:, :6] = sensors[:, :6]
        obs[:, 3] = obs[:, 3] + d.accel_x_offset
        d_eff, _ = T.sense_delay(seed, 0, tick, lat, line, obs)
        assert (d_eff == min(sense, t)).all()
        np.testing.assert_array_equal(bits(obs), bits(frame("obs", t)))
        np.testing.assert_array_equal(bits(obs), bits(seen[t]))
        np.testing.assert_array_equal(bits(obs[:, 13 + 2 * nu:13 + 6 * nu]), bits(ctl_prev[:, :4 * nu]))   # undelayed
        # the control record: the previous one's history and targets, this period's phase, the GPU's action
        ctl = frame("ctl", t).copy()
        c0 = R.ctl_fields(nu)["command"][0]                # the history and the two targets lie before the command
        ctl[:, :c0] = ctl_prev[:, :c0]
        plain = ctl.copy()
        ctrl = T.actuate_delayed(d, seed, 0, tick, lat, frame("action", t), ctl)
        np.testing.assert_array_equal(bits(ctl), bits(frame("ctl", t)))
        np.testing.assert_array_equal(bits(ctrl.T), bits(frame("ctl", t)[:, 3 * nu:4 * nu]))
        undelayed += int(np.array_equal(R.actuate(d, frame("action", t), plain), ctrl))
        ctl_prev = ctl
    np.testing.assert_array_equal(bits(fleet.ctrl.cpu().numpy()), bits(ctrl))
    np.testing.assert_array_equal(fleet.lat_tick.cpu().numpy(), tick)
    if sense > 0:
        np.testing.assert_array_equal(bits(fleet.line.cpu().numpy()), bits(line))
    else:                                         # no robot's sense_hi > 0: duck_fleet_sense_delay is not enqueued
        assert not bits(fleet.line.cpu().numpy()).any()
    assert (tick == periods).all()
    assert undelayed == (periods if action == 0 else 0)         # the delay did change the targets, or none was asked


def test_a_robot_is_its_global_id_in_the_loop(policy_file, gpu):
    """Robot 20 of 33 equals the same robot alone at robot_offset 20: delays drawn over (0, 2), DR and noise."""
    n, k, periods = 33, 20, 8
    kw = dict(noise=(1.0, 3), latency=((0, 2), (0, 2), 17))
    big = FleetInfer("flat_terrain", policy_file, n, device=gpu, randomize=7, **kw)
    one = FleetInfer("flat_terrain", policy_file, 1, device=gpu, randomize=0, robot_offset=k, **kw)
    one.dr.copy_(big.dr.view(-1, n)[:, k])
    one.restart()                                   # the loop's first substep runs on the randomised model
    cmd = commands(n, seed=34)
    big.set_commands(cmd)
    one.set_commands(cmd[k])
    seen_big, seen_one = big.run(periods, record=True), one.run(periods, record=True)
    np.testing.assert_array_equal(bits(seen_big[:, k]), bits(seen_one[:, 0]))
    for x, y in zip(big.state(), one.state()):
        np.testing.assert_array_equal(bits(x[k]), bits(y[0]))
    for name in ("ctl", "line", "lat_tick", "acc"):
        np.testing.assert_array_equal(bits(getattr(big, name).cpu().numpy()[k]), bits(getattr(one, name).cpu().numpy()[0]))
    assert int(one.lat_tick[0]) == periods
    assert not np.array_equal(seen_big[:, k], seen_big[:, k - 1])
    # the premise: the robot's draws did delay both over the run
    a, s = zip(*(T.delays(17, k, np.array([p], np.int32), [[0, 2, 0, 2]]) for p in range(periods)))
    assert len({int(v[0]) for v in a}) > 1 and len({int(v[0]) for v in s}) > 1


def test_graph_replay_equals_eager_with_latency(policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    kw = dict(recorder=(7, 1), latency=((0, 2), (0, 2), 17))
    a = _disturbed_fleet(policy_file, 8, gpu, **kw)
    b = _disturbed_fleet(policy_file, 8, gpu, **kw)
    a.run(2)      # the first call is eager
    assert a.graph is None
    a.run(10)     # two replays of the 5-period graph
    assert a.graph is not None and a.graph[1] == 5
    b.run(12)
    assert b.graph is None
    _assert_same_loop(a, b, LOOP_BUFFERS + ("ring", "rec_head", "rec_after", "line", "lat_tick"))
    assert (a.lat_tick.cpu().numpy() == 12).all() and (a.tick.cpu().numpy() == 12).all()
    g = a.graph
    a.set_latency((0, 2), (0, 2), 18)             # the seed is passed by value
    assert a.graph is None and g is not None and a.lat_base == 12 and (a.lat_tick == 0).all()
    a.restart()
    assert a.lat_base == 0 and (a.lat_tick == 0).all()


def test_replay_with_latency(policy_file, gpu):
    """sense_hi = 2: the delay line is rebuilt from the frame and the one before it. From the newest frame, from
    the oldest frame that still has its predecessor, and from frame index 0, which has none."""
    fleet = _disturbed_fleet(policy_file, 9, gpu, recorder=(6, 0), latency=((0, 2), (0, 2), 17))
    robot = 4
    fleet.run(6)
    r = fleet.replay(robot, frame=-1)
    assert r.latent() and r.lat_sense and int(r.lat_tick[0]) == 6 and r.lat_base == 0 and r.lat_seed == 17
    np.testing.assert_array_equal(r.lat.cpu().numpy(), [[0, 2, 0, 2]])
    line = fleet.line.cpu().numpy()[robot]
    np.testing.assert_array_equal(bits(r.line.cpu().numpy()[0, [5 % 3, 4 % 3]]), bits(line[[5 % 3, 4 % 3]]))
    fleet.run(6)
    mine = fleet.recorded(robot)
    assert list(mine["period"]) == list(range(7, 13))
    r.set_recorder(6)
    r.run(6)
    got = r.recorded(0)
    assert list(got["period"]) == list(range(7, 13))
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name]), err_msg=name)
    r2 = fleet.replay(robot, frame=1)             # period 8, with period 7's frame before it
    assert int(r2.lat_tick[0]) == 8
    r2.set_recorder(6)
    r2.run(4)
    got = r2.recorded(0)
    assert list(got["period"]) == list(range(9, 13))
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name][2:]), err_msg=name)
    with pytest.raises(native.DuckError, match="frame before"):
        fleet.replay(robot, frame=0)
    # the premise: the latency acted on the replayed periods (another seed, other frames)
    other = fleet.recorded(robot + 1)
    assert not np.array_equal(mine["obs"][:, :6], other["obs"][:, :6])


def test_set_latency_validates(policy_file, gpu):
    n = 4
    f = FleetInfer("flat_terrain", policy_file, n, device=gpu)
    bad = [lambda: f.set_latency(1.5), lambda: f.set_latency(0, 3), lambda: f.set_latency(-1, 0),
           lambda: f.set_latency((2, 1), 0), lambda: f.set_latency(0, (1, 2, 2)), lambda: f.set_latency([0, 1], 0),
           lambda: f.set_latency("a"), lambda: f.set_latency(0, float("nan")), lambda: f.set_latency(1, 1, 0.5)]
    for k, call in enumerate(bad):
        with pytest.raises(native.DuckError):
            call()
        assert not f.latent(), k
    f.set_latency([0, 1, 2, 0], (0, [0, 1, 2, 2]), seed=-1)
    np.testing.assert_array_equal(f.lat.cpu().numpy(), [[0, 0, 0, 0], [1, 1, 0, 1], [2, 2, 0, 2], [0, 0, 0, 2]])
    assert f.latent() and f.lat_sense and f.lat_seed == 2 ** 64 - 1 and f.line.shape == (n, 3, 6)
    f.set_latency(2)
    assert f.latent() and not f.lat_sense
    f.set_latency(0, 0)
    assert not f.latent()


def test_command_line_reports_latency(policy_file, gpu, tmp_path):
    out = str(tmp_path / "report.json")
    subprocess.run([sys.executable, "-m", "open_duck_playground_amd.sim2sim", "-o", policy_file, "--num_robots", "18",
                    "--periods", "10", "--delay_grid", "3x3", "--delay_seed", "4", "--out", out, "--device", gpu],
                   cwd=ROOT, check=True, timeout=300)
    doc = json.load(open(out))
    rows = doc["latency"]
    assert len(rows) == 9 and [r["count"] for r in rows] == [2] * 9
    assert [(r["action_delay"], r["sense_delay"]) for r in rows] == [(a, s) for a in range(3) for s in range(3)]
    for r in rows:
        assert r["action_delay_ms"] == 20.0 * r["action_delay"] and r["sense_delay_ms"] == 20.0 * r["sense_delay"]
        assert 0.0 <= r["survival_rate"] <= 1.0 and 0 <= r["mean_periods"] <= 10 and r["jitter"] is False
    assert doc["delay"] == {"delay_grid": "3x3", "delay_jitter": False, "delay_seed": 4}
    plain = str(tmp_path / "plain.json")
    assert sim2sim.main(["-o", policy_file, "--num_robots", "2", "--periods", "2", "--out", plain, "--device", gpu]) == 0
    doc = json.load(open(plain))
    assert "latency" not in doc and "delay" not in doc and len(doc["cells"]) == 1
