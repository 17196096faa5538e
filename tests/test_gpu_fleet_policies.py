"""Several policies in one fleet on the GPU (sim2sim.FleetInfer with a list of policy files; DESIGN.md §9
"Policies"): every segment is the single-policy fleet of its robots, paired scenarios are paired, the graph
replays the new launch, a ``str`` path stays on the old entry, and a recorded robot replays with its own policy.
Flat scene, 33 robots, at most 12 periods; every comparison is bit for bit."""

import numpy as np
import pytest

from open_duck_playground_amd import native, sim2sim
from open_duck_playground_amd.sim2sim import FleetInfer
from tests.fleet_helpers import bits, commands
from tests.fleet_policy_helpers import policy_files  # noqa: F401

pytestmark = pytest.mark.gpu

K, S = 3, 11
N = K * S
STATE = ("qpos", "qvel", "warm", "ctl", "obs", "action", "acc", "alive")


def _tables(fleet, cmd, push=True, latency=True, noise=True):
    """One segment's tables ([S] scenarios), the same for a fleet of S robots and, tiled, for one of K S."""
    over = fleet.tile_over_policies if fleet.num_robots == N else (lambda a: np.asarray(a))
    fleet.set_commands(over(cmd))
    if noise:
        fleet.set_noise(1.0, 5)
    if push:
        fleet.set_pushes(over(2 + np.arange(S) % 3), 4, over(np.linspace(0.1, 0.5, S)), over(np.linspace(0.0, 6.0, S)))
    if latency:
        fleet.set_latency(1, 2, 9)


def _robot_rows(fleet, name, lo, hi):
    t = getattr(fleet, name)
    t = t.t() if name in ("qpos", "qvel", "warm") else t      # the physics state is [k][N]
    return t[lo:hi].contiguous().cpu().numpy()


def test_every_segment_is_its_single_policy_fleet(policy_files, gpu):  # noqa: F811
    """Three policies x 11 robots with per-scenario commands, noise, pushes and a fixed (1, 2) latency: after 12
    periods segment k holds what a fleet of 11 robots with policy k alone, robot_offset = 11 k and the same tables
    holds, word for word."""
    cmd = commands(S, seed=17)
    fleet = FleetInfer("flat_terrain", policy_files, N, device=gpu)
    assert fleet.num_policies == K and fleet.policy_seg.tolist() == [0, 11, 22, 33]
    assert fleet.policy_of.tolist() == [0] * S + [1] * S + [2] * S
    _tables(fleet, cmd)
    fleet.run(12)
    seen = []
    for k in range(K):
        one = FleetInfer("flat_terrain", policy_files[k], S, device=gpu, robot_offset=S * k)
        _tables(one, cmd)
        one.run(12)
        for name in STATE:
            np.testing.assert_array_equal(bits(_robot_rows(fleet, name, S * k, S * (k + 1))), bits(_robot_rows(one, name, 0, S)),
                                          err_msg=f"policy {k}: {name}")
        seen.append(_robot_rows(one, "action", 0, S))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])     # the policies differ


def test_the_same_policy_three_times_is_paired(policy_files, gpu):  # noqa: F811
    """One file three times, randomize=7, no noise: robot j of every segment has the same model, command, push and
    delays and no random stream, so the three segments are the same bits, the randomisation record's columns
    repeat, and no policy wins a scenario."""
    fleet = FleetInfer("flat_terrain", [policy_files[1]] * K, N, device=gpu, randomize=7)
    _tables(fleet, commands(S, seed=19), noise=False)
    fleet.run(12)
    dr = fleet.dr.view(-1, N).cpu().numpy()
    alone = FleetInfer("flat_terrain", policy_files[1], S, device=gpu, randomize=7)
    np.testing.assert_array_equal(bits(dr[:, :S]), bits(alone.dr.view(-1, S).cpu().numpy()))
    assert not np.array_equal(dr[:, 0], dr[:, 1])                                            # S models, not one
    for k in range(1, K):
        np.testing.assert_array_equal(bits(dr[:, S * k:S * (k + 1)]), bits(dr[:, :S]))
        for name in STATE:
            np.testing.assert_array_equal(bits(_robot_rows(fleet, name, S * k, S * (k + 1))), bits(_robot_rows(fleet, name, 0, S)),
                                          err_msg=f"segment {k}: {name}")
    wins = sim2sim.paired_wins(fleet.report()["periods"], K)
    assert wins.shape == (K, K) and not wins.any()
    with pytest.raises(native.DuckError, match="equal segments"):
        FleetInfer("flat_terrain", policy_files, N, device=gpu, randomize=7, policy_robots=(10, 11, 12))


def test_graph_replay_equals_eager(policy_files, gpu, monkeypatch):  # noqa: F811
    cmd = commands(S, seed=23)
    monkeypatch.setattr(FleetInfer, "CHUNK", 5)
    a = FleetInfer("flat_terrain", policy_files, N, device=gpu, policy_robots=(5, 0, 28))
    a.set_commands(np.resize(cmd, (N, 7)))
    a.set_noise(1.0, 5)
    a.run(2)
    a.run(10)                       # two replays of a 5-period graph
    assert a.graph is not None and a.graph[1] == 5
    monkeypatch.setattr(FleetInfer, "CHUNK", 50)
    b = FleetInfer("flat_terrain", policy_files, N, device=gpu, policy_robots=(5, 0, 28))
    b.set_commands(np.resize(cmd, (N, 7)))
    b.set_noise(1.0, 5)
    b.run(2)
    b.run(10)                       # below the chunk: eager
    assert b.graph is None
    for name in STATE + ("tick",):
        np.testing.assert_array_equal(bits(_robot_rows(a, name, 0, N)), bits(_robot_rows(b, name, 0, N)), err_msg=name)


def test_a_str_path_stays_on_the_old_entry(policy_files, gpu, monkeypatch):  # noqa: F811
    """A ``str`` path never calls duck_policy_act_multi; a list of that one path calls it every period and computes
    the same bits."""
    calls = [0]
    P = native.lib()
    real = P.duck_policy_act_multi

    def counting(*args):
        calls[0] += 1
        return real(*args)
    monkeypatch.setattr(P, "duck_policy_act_multi", counting)
    cmd = commands(7, seed=29)
    a = FleetInfer("flat_terrain", policy_files[0], 7, device=gpu, randomize=3)
    a.set_commands(cmd)
    a.run(6)
    assert calls[0] == 0 and a.num_policies == 1 and a.policy_seg.tolist() == [0, 7] and not a.policy_of.any()
    b = FleetInfer("flat_terrain", [policy_files[0]], 7, device=gpu, randomize=3)
    b.set_commands(cmd)
    b.run(6)
    assert calls[0] == 6 and b.num_policies == 1
    for name in STATE:
        np.testing.assert_array_equal(bits(_robot_rows(a, name, 0, 7)), bits(_robot_rows(b, name, 0, 7)), err_msg=name)


def test_replay_carries_the_robots_policy(policy_files, gpu):  # noqa: F811
    """Robot 15 (segment 1) from its frame of period 6: the one-robot replay loads policy 1's file and reproduces
    the robot's next 3 recorded periods, every field."""
    fleet = FleetInfer("flat_terrain", policy_files, N, device=gpu, randomize=7, recorder=(12, 0))
    _tables(fleet, commands(S, seed=31))
    robot = 15
    fleet.run(6)
    r = fleet.replay(robot, frame=-1)
    assert r.num_policies == 1 and r._multi_args is None and r._made_from["onnx_model_path"] == policy_files[1]
    assert r.robot_offset == robot and r.periods_done == 6
    fleet.run(3)
    mine = fleet.recorded(robot)
    assert list(mine["period"]) == list(range(1, 10))
    r.set_recorder(3)
    r.run(3)
    got = r.recorded(0)
    assert list(got["period"]) == [7, 8, 9]
    for name in fleet.frame_fields:
        np.testing.assert_array_equal(bits(got[name]), bits(mine[name][6:]), err_msg=name)
