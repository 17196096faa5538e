"""The fleet loop's joint-encoder latency on the GPU (include/duck_fleet.h duck_fleet_sensor_delay;
sim2sim.FleetInfer.set_latency's ``encoder``): the kernel alone against its numpy restatement
(tests/fleet_encoder_reference.py), against duck_fleet_sense_delay on a zero table, and its refusals; then the loop:
fixed encoder delays teacher-forced from the recorder's frames, robot identity, graph replay against eager, the
launches a period enqueues, the replay of a recorded robot, a 3 x 3 x 3 delay grid that finds the delays a log was
made under, and the command line. Every comparison is bit for bit."""

import ctypes as C
import json

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests import fleet_encoder_reference as E
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, commands, dev, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = f32(7.0)
NAN_PAYLOAD, NEG_ZERO = np.int32(0x7FC12345), np.int32(-0x80000000)
PERIODS = 12          # rows of the followed log

# --- the kernel alone ----------------------------------------------------------------------
# six IMU rows against seven encoder rows: robot e takes row e mod 6 of one and e mod 7 of the other, so fixed and
# drawn delays of the two tables meet in every combination within 42 robots
LAT_ROWS = np.array([[0, 2, 0, 2], [1, 2, 0, 1], [0, 1, 1, 2], [0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 2, 2]], np.int32)
ENC_ROWS = np.array([[0, 2], [1, 1], [0, 0], [2, 2], [1, 2], [0, 1], [0, 0]], np.int32)


def _guard(a):
    return np.concatenate([a, np.full((1,) + a.shape[1:], 7, a.dtype)])


def _salted(rng, n, nu, call):
    """A fresh observation with a NaN whose payload tells the period and a -0 in the IMU and in the encoder columns."""
    obs = rng.normal(size=(n, R.obs_size(nu))).astype(f32)
    w = obs.view(np.int32)
    w[:, call % 6] = NAN_PAYLOAD + call
    w[:, (call + 3) % 6] = NEG_ZERO
    w[:, 13 + call % (2 * nu)] = NAN_PAYLOAD + 16 + call
    w[:, 13 + (call + 3) % (2 * nu)] = NEG_ZERO
    return obs


@pytest.mark.parametrize("n,nu,offset", [(1, 14, 0), (17, 3, (1 << 33) + 7), (130, 14, 0), (17, 16, 3)])
def test_sensor_delay_kernel_alone(gpu, n, nu, offset):
    """Seven periods on fresh observations: the slots wrap and the fill clamp is passed; rows of fixed 0 / 1 / 2 and
    drawn ranges in both tables; NaN payloads and -0 in both column groups; a guard row behind the last robot in
    every buffer; a single group, 2 nu < 16, the last partial wave, 2 nu = 32 (two words a lane), an id above 2^32."""
    L = native.lib()
    Dc = c_desc(R.make_desc(nu=nu))
    seed, W, O = 41, 2 * nu, R.obs_size(nu)
    rng = np.random.default_rng(700 + n + nu)
    lat, enc = LAT_ROWS[np.arange(n) % len(LAT_ROWS)], ENC_ROWS[np.arange(n) % len(ENC_ROWS)]
    line, eline, tick = np.zeros((n, 3, 6), f32), np.zeros((n, 3, W), f32), np.zeros(n, np.int32)
    line_d, eline_d, tick_d, lat_d, enc_d = (dev(_guard(a), gpu) for a in (line, eline, tick, lat, enc))
    obs_d = torch.full((n + 1, O), float(GUARD), device=gpu)
    delayed_imu = delayed_enc = 0
    drawn = set()                                                   # the delays the rows (0, 2) drew over the run
    for call in range(7):
        obs = _salted(rng, n, nu, call)
        obs_d[:n] = dev(obs, gpu)
        before = obs.copy()
        s_eff, s_wrote, d_eff, wrote = E.sensor_delay(seed, offset, tick, lat, enc, line, eline, obs, nu)
        native.check(L.duck_fleet_sensor_delay(C.byref(Dc), n, seed, offset, tick_d.data_ptr(), lat_d.data_ptr(),
                                               enc_d.data_ptr(), line_d.data_ptr(), eline_d.data_ptr(),
                                               obs_d.data_ptr(), stream(gpu)), L)
        got_obs, got_line, got_eline = obs_d.cpu().numpy(), line_d.cpu().numpy(), eline_d.cpu().numpy()
        np.testing.assert_array_equal(bits(got_obs[:n]), bits(obs))
        np.testing.assert_array_equal(bits(got_obs[:n, 6:13]), bits(before[:, 6:13]))               # the command
        np.testing.assert_array_equal(bits(got_obs[:n, 13 + W:]), bits(before[:, 13 + W:]))         # all behind
        np.testing.assert_array_equal(bits(got_obs[:n, 13:13 + W][~wrote]), bits(before[:, 13:13 + W][~wrote]))
        np.testing.assert_array_equal(bits(got_obs[:n, :6][~s_wrote]), bits(before[:, :6][~s_wrote]))
        np.testing.assert_array_equal(bits(got_line[:n]), bits(line))
        np.testing.assert_array_equal(bits(got_eline[:n]), bits(eline))
        np.testing.assert_array_equal(bits(got_eline[:n, call % 3]), bits(before[:, 13:13 + W]))    # every robot's line
        got_tick = tick_d.cpu().numpy()
        np.testing.assert_array_equal(got_tick[:n], tick)                                           # read only
        assert (tick == call).all() and got_tick[n] == 7
        assert (got_obs[n] == GUARD).all() and (got_line[n] == GUARD).all() and (got_eline[n] == GUARD).all()
        np.testing.assert_array_equal(lat_d.cpu().numpy(), _guard(lat))
        np.testing.assert_array_equal(enc_d.cpu().numpy(), _guard(enc))
        delayed_imu += int(s_wrote.sum())
        delayed_enc += int(wrote.sum())
        drawn |= set(E.encoder_delay(seed, offset, tick, enc)[(enc == [0, 2]).all(1)].tolist())
        tick += 1                                                   # (duck_fleet_actuate_delayed's store)
        tick_d[:n] += 1
    # the run did what it was built for: both groups were delayed, and the drawn encoder delay did vary
    assert delayed_imu > 0 and delayed_enc > 0 and len(drawn) > 1
    if n > 1:
        assert (enc[:, 1] == 0).any() and (enc[:, 0] == 2).any() and (lat[:, 3] == 0).any()


def test_zero_encoder_table_is_sense_delay(gpu):
    """enc all zero: obs and line come out as duck_fleet_sense_delay writes them on the same inputs."""
    L = native.lib()
    n, nu, seed, offset = 37, 14, 41, 5
    Dc = c_desc(R.make_desc(nu=nu))
    rng = np.random.default_rng(3)
    lat_d = dev(LAT_ROWS[np.arange(n) % len(LAT_ROWS)], gpu)
    enc_d = torch.zeros(n, 2, dtype=torch.int32, device=gpu)
    tick_d = torch.zeros(n, dtype=torch.int32, device=gpu)
    line_a, line_b = torch.zeros(n, 3, 6, device=gpu), torch.zeros(n, 3, 6, device=gpu)
    eline = torch.zeros(n, 3, 2 * nu, device=gpu)
    changed = 0
    for call in range(7):
        obs = _salted(rng, n, nu, call)
        obs_a, obs_b = dev(obs, gpu), dev(obs, gpu)
        native.check(L.duck_fleet_sense_delay(C.byref(Dc), n, seed, offset, tick_d.data_ptr(), lat_d.data_ptr(),
                                              line_a.data_ptr(), obs_a.data_ptr(), stream(gpu)), L)
        native.check(L.duck_fleet_sensor_delay(C.byref(Dc), n, seed, offset, tick_d.data_ptr(), lat_d.data_ptr(),
                                               enc_d.data_ptr(), line_b.data_ptr(), eline.data_ptr(), obs_b.data_ptr(),
                                               stream(gpu)), L)
        np.testing.assert_array_equal(bits(obs_b.cpu().numpy()), bits(obs_a.cpu().numpy()))
        np.testing.assert_array_equal(bits(line_b.cpu().numpy()), bits(line_a.cpu().numpy()))
        changed += int((bits(obs_a.cpu().numpy()) != bits(obs)).any())
        tick_d += 1
    assert changed > 0                                              # the IMU delay did act
    assert bits(eline.cpu().numpy()).any()                          # and the encoder line was kept all the same


def test_sensor_delay_arguments(gpu):
    L = native.lib()
    n, nu = 5, 3
    d = R.make_desc(nu=nu)
    D = c_desc(d)
    O = R.obs_size(nu)
    EINVAL, OK = native.HEADERS.consts["DUCK_EINVAL"], native.HEADERS.consts["DUCK_OK"]
    name = "duck_fleet_sensor_delay"
    f = getattr(L, name)
    tick = torch.zeros(n, dtype=torch.int32, device=gpu)
    lat = dev(np.tile(np.array([1, 1, 1, 1], np.int32), (n, 1)), gpu)
    enc = dev(np.tile(np.array([1, 1], np.int32), (n, 1)), gpu)
    line, eline, obs = torch.zeros(n, 3, 6, device=gpu), torch.zeros(n, 3, 2 * nu, device=gpu), torch.full((n, O), 2.0, device=gpu)
    ptrs = [t.data_ptr() for t in (tick, lat, enc, line, eline, obs)]

    def call(desc=D, n=n, null=None):
        p = [None if k == null else v for k, v in enumerate(ptrs)]
        return f(None if desc is None else C.byref(desc), n, 3, 0, *p, stream(gpu))
    assert call(desc=None) == EINVAL and f"{name}: null pointer".encode() in L.duck_last_error()
    for k in range(len(ptrs)):
        assert call(null=k) == EINVAL and f"{name}: null pointer".encode() in L.duck_last_error(), k
    for bad in (-1, (1 << 27) + 1):
        assert call(n=bad) == EINVAL and f"{name}: bad size".encode() in L.duck_last_error()
    wide = c_desc(d)
    wide.nu = 17
    assert call(desc=wide) == EINVAL and f"{name}: nq, nv >= 1".encode() in L.duck_last_error()
    assert call(n=0) == OK
    torch.cuda.synchronize()
    assert (line == 0).all() and (eline == 0).all() and (obs == 2).all() and (tick == 0).all()      # nothing ran
    native.check(call(), L)
    assert (line[:, 0] == 2).all() and (line[:, 1:] == 0).all() and (eline[:, 0] == 2).all() and (eline[:, 1:] == 0).all()
    assert (obs == 2).all() and (tick == 0).all()


# --- the loop --------------------------------------------------------------------------------
def _disturbed_fleet(path, n, gpu, **kw):
    """DR, a 3-segment schedule, drawn pushes first at period 2 and every 3 after, noise at level 1."""
    table = commands(2 * 3, seed=21).reshape(2, 3, 7)
    return FleetInfer("flat_terrain", path, n, device=gpu, randomize=7, command_schedule=(table, np.arange(n) % 2, 5),
                      pushes=(2, 3, (0.1, 0.5), (0.0, 6.0)), noise=(1.0, 3), **kw)


LOOP_BUFFERS = ("warm", "ctl", "obs", "action", "acc", "alive", "tick", "aux")
ALL_DRAWN = ((0, 2), (0, 2), 17, (0, 2))      # set_latency's arguments: all three delays drawn over 0..2


def _assert_same_loop(a, b, names=LOOP_BUFFERS):
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in names:
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()),
                                      err_msg=name)


@pytest.mark.parametrize("action,sense,encoder", [(1, 2, 1), (0, 0, 2)])
def test_fixed_encoder_delays_teacher_forced(policy_file, gpu, action, sense, encoder):
    """An eager run with a recorder; per period the true IMU and encoder columns are formed from the frame's raw
    sensors, qpos and qvel, the restatement delays them, and the result is what the policy saw."""
    n, periods, seed = 5, 8, 13
    fleet = FleetInfer("flat_terrain", policy_file, n, device=gpu, recorder=(periods, 0),
                       latency=(action, sense, seed, encoder))
    fleet.set_commands(commands(n, seed=33))
    assert fleet.latent() and fleet.lat_encoder and fleet.lat_sense == (sense > 0)
    nu = fleet.num_dofs
    d = R.desc_values(fleet.desc)
    seen = fleet.run(periods, record=True)
    recs = [fleet.recorded(e) for e in range(n)]
    frame = lambda name, t: np.stack([r[name][t] for r in recs])  # noqa: E731
    lat = np.tile(np.array([action, action, sense, sense], np.int32), (n, 1))
    enc = np.tile(np.array([encoder, encoder], np.int32), (n, 1))
    np.testing.assert_array_equal(fleet.lat.cpu().numpy(), lat)
    np.testing.assert_array_equal(fleet.enc.cpu().numpy(), enc)
    tick, line, eline = np.zeros(n, np.int32), np.zeros((n, 3, 6), f32), np.zeros((n, 3, 2 * nu), f32)
    true = []
    for t in range(periods):
        obs = frame("obs", t).copy()
        obs[:, :6] = frame("sensors", t)[:, :6]
        obs[:, 3] = obs[:, 3] + d.accel_x_offset
        obs[:, 13:13 + nu] = frame("qpos", t)[:, d.act_qpos[:nu]] - np.asarray(d.act_default[:nu], f32)
        obs[:, 13 + nu:13 + 2 * nu] = frame("qvel", t)[:, d.act_dof[:nu]] * d.dof_vel_scale
        true.append(obs[:, 13:13 + 2 * nu].copy())
        s_eff, _, d_eff, _ = E.sensor_delay(seed, 0, tick, lat, enc, line, eline, obs, nu)
        assert (s_eff == min(sense, t)).all() and (d_eff == min(encoder, t)).all()
        np.testing.assert_array_equal(bits(obs), bits(frame("obs", t)))
        np.testing.assert_array_equal(bits(obs), bits(seen[t]))
        np.testing.assert_array_equal(bits(obs[:, 13:13 + 2 * nu]), bits(true[max(t - encoder, 0)]))
        tick += 1
    np.testing.assert_array_equal(fleet.lat_tick.cpu().numpy(), tick)
    np.testing.assert_array_equal(bits(fleet.line.cpu().numpy()), bits(line))
    np.testing.assert_array_equal(bits(fleet.eline.cpu().numpy()), bits(eline))
    assert not np.array_equal(true[-1], true[-1 - encoder])             # the delay did change what the policy saw


def test_a_robot_is_its_global_id_with_an_encoder_delay(policy_file, gpu):
    """Robot 20 of 33 equals the same robot alone at robot_offset 20: all three delays drawn over (0, 2), DR, noise."""
    n, k, periods = 33, 20, 8
    kw = dict(noise=(1.0, 3), latency=ALL_DRAWN)
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
    for name in ("ctl", "line", "eline", "lat_tick", "acc"):
        np.testing.assert_array_equal(bits(getattr(big, name).cpu().numpy()[k]), bits(getattr(one, name).cpu().numpy()[0]))
    assert int(one.lat_tick[0]) == periods
    # the premise: the robot's encoder draws did vary over the run
    e = [int(E.encoder_delay(17, k, np.array([p], np.int32), [[0, 2]])[0]) for p in range(periods)]
    assert len(set(e)) > 1


def test_graph_replay_equals_eager_with_an_encoder_delay(policy_file, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    kw = dict(recorder=(7, 1), latency=ALL_DRAWN)
    a = _disturbed_fleet(policy_file, 8, gpu, **kw)
    b = _disturbed_fleet(policy_file, 8, gpu, **kw)
    a.run(2)      # the first call is eager
    assert a.graph is None
    a.run(10)     # two replays of the 5-period graph
    assert a.graph is not None and a.graph[1] == 5
    b.run(12)
    assert b.graph is None
    _assert_same_loop(a, b, LOOP_BUFFERS + ("ring", "rec_head", "rec_after", "line", "eline", "lat_tick"))
    assert (a.lat_tick.cpu().numpy() == 12).all()
    a.set_latency((0, 2), (0, 2), 17, encoder=1)             # the table is another buffer
    assert a.graph is None and a.lat_base == 12 and (a.lat_tick == 0).all()


def _count(fleet, monkeypatch, names):
    calls = {name: 0 for name in names}
    for name in names:
        real = getattr(fleet._lib, name)

        def counting(*args, real=real, name=name):
            calls[name] += 1
            return real(*args)
        monkeypatch.setattr(fleet._lib, name, counting)
    return calls


def test_launches_of_a_period(policy_file, gpu, monkeypatch):
    """Without ``encoder`` the loop enqueues what it did: the old entry once a period, the new one never. With it the
    new entry takes the old one's place; alone, it brings duck_fleet_actuate_delayed along, lat_tick's writer."""
    n, periods = 4, 5
    names = ("duck_fleet_sense_delay", "duck_fleet_sensor_delay", "duck_fleet_actuate_delayed", "duck_fleet_actuate")
    f = FleetInfer("flat_terrain", policy_file, n, device=gpu, latency=(1, (0, 2), 5))
    assert f.latent() and f.lat_sense and not f.lat_encoder and f.enc is None and f.eline is None
    calls = _count(f, monkeypatch, names)
    f.run(periods)
    assert calls == {"duck_fleet_sense_delay": periods, "duck_fleet_sensor_delay": 0,
                     "duck_fleet_actuate_delayed": periods, "duck_fleet_actuate": 0}
    f.set_latency(1, 0, 5)                                    # no IMU delay either: neither
    for k in calls:
        calls[k] = 0
    f.run(periods)
    assert calls["duck_fleet_sense_delay"] == 0 and calls["duck_fleet_sensor_delay"] == 0
    f.set_latency(1, (0, 2), 5, encoder=(0, 1))
    assert f.lat_sense and f.lat_encoder and f.graph is None and f.eline.shape == (n, 3, 2 * f.num_dofs)
    for k in calls:
        calls[k] = 0
    f.run(periods)
    assert calls == {"duck_fleet_sense_delay": 0, "duck_fleet_sensor_delay": periods,
                     "duck_fleet_actuate_delayed": periods, "duck_fleet_actuate": 0}
    f.set_latency(encoder=[0, 1, 2, 0])                       # the encoder alone makes the fleet latent
    assert f.latent() and not f.lat_sense and f.lat_encoder and not f.lat.cpu().numpy().any()
    np.testing.assert_array_equal(f.enc.cpu().numpy(), [[0, 0], [1, 1], [2, 2], [0, 0]])
    for k in calls:
        calls[k] = 0
    f.run(periods)
    assert calls == {"duck_fleet_sense_delay": 0, "duck_fleet_sensor_delay": periods,
                     "duck_fleet_actuate_delayed": periods, "duck_fleet_actuate": 0}
    assert (f.lat_tick.cpu().numpy() == periods).all()
    f.set_latency(0, 0, 0, encoder=0)
    assert not f.latent() and f.enc is None and f.eline is None and not f.lat_encoder
    with pytest.raises(native.DuckError, match=r"encoder must lie in \[0, 2\]"):
        f.set_latency(0, 0, 0, encoder=3)
    assert not f.latent()


def test_replay_with_an_encoder_delay(policy_file, gpu):
    """enc_hi = 2: the encoder line is rebuilt from the frame's qpos and qvel and the frame before it (with pushes:
    the frames' qvel[0:2] hold the next period's push, no actuated joint is there). From the newest frame, from the
    oldest frame that still has its predecessor, and from frame index 0, which has none."""
    fleet = _disturbed_fleet(policy_file, 9, gpu, recorder=(6, 0), latency=((0, 2), (0, 1), 17, (0, 2)))
    robot = 4
    fleet.run(6)
    r = fleet.replay(robot, frame=-1)
    assert r.latent() and r.lat_sense and r.lat_encoder and int(r.lat_tick[0]) == 6 and r.lat_seed == 17
    np.testing.assert_array_equal(r.lat.cpu().numpy(), [[0, 2, 0, 1]])
    np.testing.assert_array_equal(r.enc.cpu().numpy(), [[0, 2]])
    eline = fleet.eline.cpu().numpy()[robot]
    np.testing.assert_array_equal(bits(r.eline.cpu().numpy()[0, [5 % 3, 4 % 3]]), bits(eline[[5 % 3, 4 % 3]]))
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
    with pytest.raises(native.DuckError, match="encoder delay reaches 2 periods back"):     # sense_hi is 1: the encoder's
        fleet.replay(robot, frame=0)
    # the premise: the encoder delay acted on the replayed periods
    nu = fleet.num_dofs
    delays = [int(E.encoder_delay(17, robot, np.array([p], np.int32), [[0, 2]])[0]) for p in range(6, 12)]
    assert max(delays) > 0
    assert not np.array_equal(mine["obs"][:, 13:13 + 2 * nu], fleet.recorded(robot + 1)["obs"][:, 13:13 + 2 * nu])


def test_a_delay_grid_finds_the_logs_encoder_delay(policy_file, gpu):
    """The test the feature stands on: a log made in closed loop under (action, IMU, encoder) = (1, 2, 1) with a
    non-zero command, followed by the 3 x 3 x 3 grid on the same nominal model. The cell (1, 2, 1) scores exactly
    +0.0 in every column and every other cell more; the cells that differ from it in the encoder delay only are fed
    the same actions under the same action delay, so they move alike and differ in the encoder groups alone."""
    made = FleetInfer("flat_terrain", policy_file, 1, device=gpu, latency=(1, 2, 5, 1))
    cmd = commands(1, seed=36)[0]
    assert np.abs(cmd[:3]).min() > 0
    made.set_commands(cmd)
    log = sim2sim.log_from_saved_obs(made.run(PERIODS + 1, record=True)[:, 0])
    cells = sim2sim.delay_grid("3x3x3", encoder=True)
    fleet = FleetInfer("flat_terrain", None, len(cells), device=gpu, follow=(log, None),
                       latency=(cells[:, 0], cells[:, 1], 5, cells[:, 2]))
    fleet.run(PERIODS)
    score, rep = fleet.scores(), fleet.score_report()
    total = rep["total"]
    print("\n[measure] totals per delay cell:", np.array2string(total, precision=4))
    cell = (1 * 3 + 2) * 3 + 1
    assert cells[cell].tolist() == [1, 2, 1] and not bits(score[cell]).any()
    assert len(total) == 27 and (np.delete(total, cell) > 0).all() and sim2sim.rank_totals(total)[0] == cell
    nu = fleet.num_dofs
    for e in (0, 1, 2):
        c = (1 * 3 + 2) * 3 + e
        assert cells[c].tolist() == [1, 2, e]
        outside = np.delete(score[c], np.arange(13, 13 + 2 * nu))
        assert not bits(outside).any(), e                                      # +0.0 outside the encoder columns
        for g in ("joint_position", "joint_velocity"):
            assert (rep[g][c] > 0) == (e != 1), (e, g)
        for g in ("gyro", "accelerometer", "action_history", "motor_targets", "contacts", "phase"):
            assert rep[g][c] == 0, (e, g)


def test_command_line_reports_the_encoder_axis(policy_file, gpu, tmp_path):
    out = str(tmp_path / "three.json")
    assert sim2sim.main(["-o", policy_file, "--num_robots", "16", "--periods", "4", "--delay_grid", "2x2x2",
                         "--delay_seed", "4", "--out", out, "--device", gpu]) == 0
    doc = json.load(open(out))
    rows = doc["latency"]
    assert len(rows) == 8 and [r["count"] for r in rows] == [2] * 8
    assert [(r["action_delay"], r["sense_delay"], r["encoder_delay"]) for r in rows] == \
        [(a, s, e) for a in range(2) for s in range(2) for e in range(2)]
    assert all(r["encoder_delay_ms"] == 20.0 * r["encoder_delay"] for r in rows)
    assert doc["delay"] == {"delay_grid": "2x2x2", "delay_jitter": False, "delay_seed": 4}
    out = str(tmp_path / "two.json")
    assert sim2sim.main(["-o", policy_file, "--num_robots", "8", "--periods", "4", "--delay_grid", "2x2",
                         "--out", out, "--device", gpu]) == 0
    rows = json.load(open(out))["latency"]
    assert len(rows) == 4 and all("encoder_delay" not in r and "encoder_delay_ms" not in r for r in rows)
