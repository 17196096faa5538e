"""Following a recorded log on the GPU (include/duck_fleet.h duck_fleet_follow; sim2sim.FleetInfer.set_log): the
kernel alone against its numpy restatement (tests/fleet_follow_reference.py) and its refusals, then the loop: a
closed-loop robot's own record followed by 33 randomised robots scores exactly zero for the one that made it, a
delay grid finds the delays the log was made under, graph replay against eager, robot identity, the plain loop
after set_log(None), the replay of a recorded robot, and the end of the log. Every comparison is bit for bit."""

import ctypes as C

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests import fleet_follow_reference as F
from tests import fleet_reference as R
from tests.fleet_helpers import bits, c_desc, commands, guarded, guards_hold, policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = f32(7.0)
NAN_PAYLOAD, NEG_ZERO = np.int32(0x7FC12345), np.int32(-0x80000000)
SEED = 7              # the randomisation seed of the self-consistency tests
ROBOT = 20            # ... and the robot whose model made the log
PERIODS = 12          # rows of the shared log (13 recorded periods)


# --- the kernel alone -----------------------------------------------------------------------
@pytest.mark.parametrize("n,nu,n_log", [(1, 14, 1), (17, 3, 2), (130, 14, 3), (17, 16, 1)])
def test_follow_kernel_alone(gpu, n, nu, n_log):
    """T = 5 over 7 calls on fresh observations: the end of the log is crossed (zero actions, no scoring, the tick
    held, the command kept). NaN payloads and -0 in the log's actions, NaN log observation words (missing samples:
    the score word keeps its bits), out-of-range and negative log_id, a negative starting tick, a guard row before
    and after every buffer, the last partial wave."""
    L = native.lib()
    Dc = c_desc(R.make_desc(nu=nu))
    T, calls = 5, 7
    rng = np.random.default_rng(900 + n + nu)
    O, W, Cw = F.obs_size(nu), F.log_size(nu), F.ctl_size(nu)
    log = rng.normal(size=(n_log, T, W)).astype(f32)
    lw = log.view(np.int32)
    lw[:, :, :O][rng.random((n_log, T, O)) < 0.15] = NAN_PAYLOAD          # missing samples
    lw[:, 1::2, O] = NAN_PAYLOAD + 1                                       # a NaN action with a payload
    lw[:, ::2, O + nu - 1] = NEG_ZERO
    lw[:, 2, 6] = NEG_ZERO                                                 # a command word
    log_id = (np.arange(n) % (n_log + 3) - 1).astype(np.int32)            # -1 .. n_log + 1
    tick = np.zeros(n, np.int32)
    tick[::3] = -3
    tick[1::5] = 2
    ctl = rng.normal(size=(n, Cw)).astype(f32)
    score = np.zeros((n, O), f32)
    score[:, 0] = 0.5                                                      # (the sum goes on from what is there)
    action = np.full((n, nu), 3, f32)
    log_g, log_d = guarded(log.reshape(n_log * T, W), gpu)
    id_g, id_d = guarded(log_id, gpu)
    tick_g, tick_d = guarded(tick, gpu)
    ctl_g, ctl_d = guarded(ctl, gpu)
    score_g, score_d = guarded(score, gpu)
    act_g, act_d = guarded(action, gpu)
    obs_g, obs_d = guarded(np.zeros((n, O), f32), gpu)
    kept = past = 0
    for call in range(calls):
        obs = rng.normal(size=(n, O)).astype(f32)
        obs_d.copy_(torch.tensor(obs))
        score_before = score.copy()
        p, inside = F.follow(nu, log, log_id, tick, obs, score, ctl, action)
        native.check(L.duck_fleet_follow(C.byref(Dc), n, n_log, T, log_d.data_ptr(), id_d.data_ptr(), tick_d.data_ptr(),
                                         obs_d.data_ptr(), score_d.data_ptr(), ctl_d.data_ptr(), act_d.data_ptr(),
                                         stream(gpu)), L)
        for name, got, want in (("score", score_d, score), ("ctl", ctl_d, ctl), ("action", act_d, action),
                                ("log_tick", tick_d, tick), ("obs", obs_d, obs), ("log", log_d, log.reshape(-1, W)),
                                ("log_id", id_d, log_id)):
            np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want), err_msg=f"{name}, call {call}")
        for t in (log_g, id_g, tick_g, ctl_g, score_g, act_g, obs_g):
            assert guards_hold(t), call
        # the restatement did what the header says
        ids = np.clip(log_id, 0, n_log - 1)
        missing = np.isnan(log[ids, np.minimum(p, T - 1), :O]) | ~inside[:, None]
        assert (bits(score)[missing] == bits(score_before)[missing]).all()
        assert not bits(action)[~inside].any()
        kept += int(missing[inside].sum())
        past += int((~inside).sum())
    assert (tick == T).all() and kept > 0 and past > 0
    assert (log_id < 0).any() and (n == 1 or (log_id >= n_log).any())


def test_follow_arguments(gpu):
    L = native.lib()
    n, nu, T = 5, 3, 4
    d = R.make_desc(nu=nu)
    D = c_desc(d)
    O, W, Cw = F.obs_size(nu), F.log_size(nu), F.ctl_size(nu)
    EINVAL, OK = native.HEADERS.consts["DUCK_EINVAL"], native.HEADERS.consts["DUCK_OK"]
    log = torch.full((2, T, W), 2.0, device=gpu)
    ids, tick = torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu)
    obs, score = torch.full((n, O), 3.0, device=gpu), torch.zeros(n, O, device=gpu)
    ctl, action = torch.zeros(n, Cw, device=gpu), torch.ones(n, nu, device=gpu)
    ptrs = [t.data_ptr() for t in (log, ids, tick, obs, score, ctl, action)]

    def call(desc=D, n=n, n_log=2, T=T, null=None):
        p = [None if k == null else v for k, v in enumerate(ptrs)]
        return L.duck_fleet_follow(None if desc is None else C.byref(desc), n, n_log, T, *p, stream(gpu))
    assert call(desc=None) == EINVAL and b"duck_fleet_follow: null pointer" in L.duck_last_error()
    for k in range(len(ptrs)):
        assert call(null=k) == EINVAL and b"duck_fleet_follow: null pointer" in L.duck_last_error(), k
    for bad in (-1, (1 << 27) + 1):
        assert call(n=bad) == EINVAL and b"duck_fleet_follow: bad size" in L.duck_last_error()
    assert call(n_log=0) == EINVAL and b"n_log >= 1 and T >= 1" in L.duck_last_error()
    assert call(T=0) == EINVAL and b"n_log >= 1 and T >= 1" in L.duck_last_error()
    wide = c_desc(d)
    wide.nu = 17
    assert call(desc=wide) == EINVAL and b"duck_fleet_follow: nq, nv >= 1" in L.duck_last_error()
    assert call(n=0) == OK
    torch.cuda.synchronize()
    assert (tick == 0).all() and (score == 0).all() and (ctl == 0).all() and (action == 1).all()      # nothing ran
    native.check(call(), L)
    torch.cuda.synchronize()
    assert (tick == 1).all() and (score == 1).all() and (action == 2).all()
    c0 = R.ctl_fields(nu)["command"][0]
    assert (ctl[:, c0:c0 + 7] == 2).all() and (ctl[:, :c0] == 0).all() and (ctl[:, c0 + 7:] == 0).all()


# --- the loop --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def closed_loop(policy_file, gpu):
    """One closed-loop robot with the test policy on the model of robot ROBOT of duck_randomize(SEED), the command
    changed once; 13 periods recorded, the log of 12 rows made of them, and the robot's frame after 12 periods."""
    src = FleetInfer("flat_terrain", policy_file, 33, device=gpu, randomize=SEED)
    one = FleetInfer("flat_terrain", policy_file, 1, device=gpu, randomize=0, robot_offset=ROBOT, recorder=(PERIODS + 1, 0))
    one.dr.copy_(src.dr.view(-1, 33)[:, ROBOT])
    one.restart()                                   # the loop's first substep runs on the randomised model
    cmd = commands(2, seed=35)
    one.set_commands(cmd[0])
    a = one.run(6, record=True)
    one.set_commands(cmd[1])
    b = one.run(PERIODS + 1 - 6, record=True)
    seen = np.concatenate([a, b])[:, 0]
    frames = one.recorded(0)
    assert list(frames["period"]) == list(range(1, PERIODS + 2))
    log = sim2sim.log_from_saved_obs(seen)
    assert log.shape == (PERIODS, F.log_size(14)) and not np.array_equal(log[5, 6:13], log[6, 6:13])
    np.testing.assert_array_equal(bits(log[:, F.obs_size(14):]), bits(frames["action"][:PERIODS]))   # what the policy answered
    return {"log": log, "seen": seen, "after": {k: frames[k][PERIODS - 1] for k in ("qpos", "qvel", "qacc_warmstart", "ctl")}}


LOOP_BUFFERS = ("warm", "ctl", "obs", "action", "acc", "alive", "tick", "aux")
FOLLOW_BUFFERS = ("score", "log_tick", "log", "log_id")


def _assert_same_loop(a, b, names=LOOP_BUFFERS):
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in names:
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()),
                                      err_msg=name)


def test_the_model_that_made_the_log_scores_zero(closed_loop, gpu):
    """The test the feature stands on: 33 robots of duck_randomize(SEED), no policy loaded, follow the log that
    robot ROBOT's model made in closed loop. That robot reproduces the closed-loop run bit for bit, so its score is
    +0.0 in every column; every other model (its body masses scaled otherwise) is some way off. Seed 7: no other
    robot ties at 0 on an MI355X."""
    n = 33
    fleet = FleetInfer("flat_terrain", None, n, device=gpu, randomize=SEED, follow=(closed_loop["log"], None))
    assert fleet.following() and fleet._policy_args is None
    fleet.run(PERIODS)
    score = fleet.scores()
    assert score.shape == (n, fleet.obs_size) and not bits(score[ROBOT]).any()         # +0.0, every column
    qpos, qvel, _ = fleet.state()
    want = closed_loop["after"]
    np.testing.assert_array_equal(bits(qpos[ROBOT]), bits(want["qpos"]))
    np.testing.assert_array_equal(bits(qvel[ROBOT]), bits(want["qvel"]))
    np.testing.assert_array_equal(bits(fleet.warm.cpu().numpy()[:, ROBOT]), bits(want["qacc_warmstart"]))
    np.testing.assert_array_equal(bits(fleet.ctl.cpu().numpy()[ROBOT]), bits(want["ctl"]))
    rep = fleet.score_report()
    total = rep["total"]
    print("\n[measure] totals:", np.array2string(np.sort(total), precision=3))
    others = np.delete(total, ROBOT)
    assert total[ROBOT] == 0.0 and (others > 0).all()
    assert sim2sim.rank_totals(total)[0] == ROBOT
    assert (rep["periods"] == PERIODS).all() and (fleet.log_tick.cpu().numpy() == PERIODS).all()
    # the feeding: every robot was fed the log's actions and commands, so those groups are 0 for all
    assert (rep["action_history"] == 0).all() and (rep["motor_targets"] == 0).all()
    np.testing.assert_array_equal(bits(fleet.action.cpu().numpy()), bits(np.tile(closed_loop["log"][-1, -14:], (n, 1))))


def test_a_delay_grid_finds_the_logs_delays(policy_file, gpu):
    """A log made under an action delay of 1 and an IMU delay of 2, followed by the 3 x 3 delay grid on the same
    nominal model: the cell (1, 2) scores exactly 0, every other cell more."""
    made = FleetInfer("flat_terrain", policy_file, 1, device=gpu, latency=(1, 2, 5))
    made.set_commands(commands(1, seed=36)[0])
    log = sim2sim.log_from_saved_obs(made.run(PERIODS + 1, record=True)[:, 0])
    cells = sim2sim.delay_grid("3x3")
    fleet = FleetInfer("flat_terrain", None, len(cells), device=gpu, follow=(log, None),
                       latency=(cells[:, 0], cells[:, 1], 5))
    fleet.run(PERIODS)
    score, total = fleet.scores(), fleet.score_report()["total"]
    print("\n[measure] totals per delay cell:", np.array2string(total, precision=4))
    cell = 1 * 3 + 2
    assert cells[cell].tolist() == [1, 2] and not bits(score[cell]).any()
    assert (np.delete(total, cell) > 0).all() and sim2sim.rank_totals(total)[0] == cell


def _following_fleet(log, n, gpu, **kw):
    return FleetInfer("flat_terrain", None, n, device=gpu, randomize=SEED, follow=(log, None), noise=(1.0, 3), **kw)


def test_graph_replay_equals_eager_while_following(closed_loop, gpu, monkeypatch):
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    log = closed_loop["log"]
    a = _following_fleet(log, 8, gpu, recorder=(7, 1))
    b = _following_fleet(log, 8, gpu, recorder=(7, 1))
    a.run(2)      # the first call is eager
    assert a.graph is None
    a.run(10)     # two replays of the 5-period graph
    assert a.graph is not None and a.graph[1] == 5
    b.run(12)
    assert b.graph is None
    _assert_same_loop(a, b, LOOP_BUFFERS + FOLLOW_BUFFERS + ("ring", "rec_head", "rec_after"))
    assert (a.log_tick.cpu().numpy() == 12).all() and bits(a.scores()).any()
    # a log of the same shape goes into the buffers the graph holds; another shape needs another graph
    g = a.graph
    a.set_log(log[::-1].copy())
    assert a.graph is g and (a.log_tick == 0).all() and not bits(a.scores()).any() and a.log_base == 12
    np.testing.assert_array_equal(bits(a.ctl_field("command").cpu().numpy()), bits(np.tile(log[-1, 6:13], (8, 1))))
    a.set_log(log[:11])
    assert a.graph is None and a.log.shape == (1, 11, log.shape[1])
    a.restart()
    assert a.log_base == 0 and (a.log_tick == 0).all()


def test_a_robot_is_its_global_id_while_following(closed_loop, gpu):
    """Robot 20 of 33 equals the same robot alone at robot_offset 20: DR and noise, scores included."""
    n, k = 33, ROBOT
    log = closed_loop["log"]
    big = _following_fleet(log, n, gpu)
    one = FleetInfer("flat_terrain", None, 1, device=gpu, randomize=0, robot_offset=k, follow=(log, None), noise=(1.0, 3))
    one.dr.copy_(big.dr.view(-1, n)[:, k])
    one.restart()
    seen_big, seen_one = big.run(PERIODS, record=True), one.run(PERIODS, record=True)
    np.testing.assert_array_equal(bits(seen_big[:, k]), bits(seen_one[:, 0]))
    for x, y in zip(big.state(), one.state()):
        np.testing.assert_array_equal(bits(x[k]), bits(y[0]))
    for name in ("ctl", "score", "log_tick", "acc", "action"):
        np.testing.assert_array_equal(bits(getattr(big, name).cpu().numpy()[k]), bits(getattr(one, name).cpu().numpy()[0]),
                                      err_msg=name)
    assert bits(one.scores()).any()                                     # with noise even the right model is off
    assert not np.array_equal(big.scores()[k], big.scores()[k - 1])


def test_set_log_none_leaves_the_plain_loop(closed_loop, policy_file, gpu, monkeypatch):
    n, periods = 5, 6
    cmd = commands(n, seed=37)
    a = FleetInfer("flat_terrain", policy_file, n, device=gpu, randomize=SEED, follow=(closed_loop["log"], None))
    a.run(3)
    assert a.following() and (a.log_tick == 3).all()
    a.set_log(None)
    assert not a.following() and a.log is None and a.log_tick is None and a.score is None and a.graph is None
    a.restart()
    a.set_commands(cmd)
    calls = [0]
    real = a._lib.duck_fleet_follow

    def counting(*args):
        calls[0] += 1
        return real(*args)
    monkeypatch.setattr(a._lib, "duck_fleet_follow", counting)
    a.run(periods)
    assert calls[0] == 0
    b = FleetInfer("flat_terrain", policy_file, n, device=gpu, randomize=SEED)
    b.set_commands(cmd)
    b.run(periods)
    _assert_same_loop(a, b)
    with pytest.raises(native.DuckError, match="no log is set"):
        a.scores()


def test_replay_of_a_following_fleet(closed_loop, gpu):
    """Robot 4 of 9 from its frame of period 6: the replay, which carries the robot's log and its log_tick and has
    no policy either, reproduces the next 4 recorded periods, every field."""
    fleet = _following_fleet(closed_loop["log"], 9, gpu, recorder=(12, 0))
    robot = 4
    fleet.run(6)
    r = fleet.replay(robot, frame=-1)
    assert r.following() and r._policy_args is None and int(r.log_tick[0]) == 6 and r.log_base == 0 and r.periods_done == 6
    np.testing.assert_array_equal(bits(r.log.cpu().numpy()[0]), bits(closed_loop["log"]))
    fleet.run(4)
    mine = fleet.recorded(robot)
    assert list(mine["period"]) == list(range(1, 11))
    r.set_recorder(6)
    r.run(4)
    got = r.recorded(0)
    assert list(got["period"]) == list(range(7, 11))
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name][6:]), err_msg=name)
    assert int(r.log_tick[0]) == 10
    with pytest.raises(native.DuckError, match="pass its end"):
        r.run(3)                                   # 10 followed, 12 rows


def test_run_past_the_log_raises_and_enqueues_nothing(closed_loop, gpu, monkeypatch):
    fleet = _following_fleet(closed_loop["log"], 4, gpu)
    fleet.run(10)
    names = LOOP_BUFFERS + ("score", "log_tick", "qpos", "qvel", "ctrl")
    before = {k: getattr(fleet, k).cpu().numpy().copy() for k in names}
    launches = [0]
    for name in ("duck_physics_step", "duck_fleet_observe", "duck_fleet_follow", "duck_fleet_actuate", "duck_fleet_disturb"):
        real = getattr(fleet._lib, name)

        def counting(*args, real=real):
            launches[0] += 1
            return real(*args)
        monkeypatch.setattr(fleet._lib, name, counting)
    calls, done = fleet.calls, fleet.periods_done
    with pytest.raises(native.DuckError, match="pass its end"):
        fleet.run(3)
    torch.cuda.synchronize()
    assert launches[0] == 0 and fleet.calls == calls and fleet.periods_done == done
    for k in names:
        np.testing.assert_array_equal(bits(getattr(fleet, k).cpu().numpy()), bits(before[k]), err_msg=k)
    fleet.run(2)                                   # up to the end is fine
    assert launches[0] == 2 * 5 and (fleet.log_tick.cpu().numpy() == PERIODS).all()
    with pytest.raises(native.DuckError, match="pass its end"):
        fleet.run(1)
    # without a policy and without a log there is nothing to run
    fleet.set_log(None)
    with pytest.raises(native.DuckError, match="no policy is loaded and no log is set"):
        fleet.run(1)
    with pytest.raises(native.DuckError, match="needs a policy"):
        FleetInfer("flat_terrain", None, 1, device=gpu)
