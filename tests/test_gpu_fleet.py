"""The fleet deployment loop on the GPU (sim2sim.FleetInfer; include/duck_fleet.h): the two kernels alone
against their float32 restatements (tests/fleet_reference.py), then the loop: batch invariance, graph
replay against eager, teacher-forced against the single-robot MjInfer, falls, standing, an edited scene
and the command line."""

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native
from open_duck_playground_amd.onnx_infer import OnnxGraph, dense_policy
from open_duck_playground_amd.sim2sim import FleetInfer, MjInfer
from tests import fleet_reference as R
from tests.fleet_helpers import c_desc, commands, dev, f32_bits as bits, net_and_policy_file, stream  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PHASE_TOL = 2e-6   # three float32 roundings on an angle below 2 pi (about 1.1e-6) + 2 ulp of cosf / sinf


# --- the kernels alone --------------------------------------------------------------------
def _random_state(d, n, rng, call, fall_at, nan_robot):
    qpos = rng.normal(size=(d.nq, n)).astype(f32)
    qvel = rng.normal(size=(d.nv, n)).astype(f32)
    aux = rng.normal(size=(d.naux, n)).astype(f32)
    up = d.sens_off + d.upvector + 2
    aux[up] = np.abs(aux[up]) + f32(0.1)
    if call >= 2:
        aux[up, fall_at] = -aux[up, fall_at]          # upvector[2] goes negative on call 3
    if call == 1 and nan_robot is not None:
        qvel[0, nan_robot] = np.nan                   # (an unactuated dof: not an obs column)
    con = aux[d.con_off:d.con_off + 8]
    special = np.array([0.0, -0.0, np.nan, -1e-9, 1e-9], f32)
    pick = rng.integers(0, 12, size=con.shape)
    con[pick < 5] = special[pick[pick < 5]]
    return qpos, qvel, aux


@pytest.mark.parametrize("n,nu,standing", [(1, 14, 0), (17, 3, 0), (130, 14, 0), (17, 16, 0), (17, 14, 1)])
def test_observe_kernel_alone(gpu, n, nu, standing):
    L = native.lib()
    d = R.make_desc(nu=nu, nb=40, standing=standing)
    D = c_desc(d)
    rng = np.random.default_rng(100 + n + nu)
    F = R.ctl_fields(nu)
    O = R.obs_size(nu)
    ctl = rng.normal(size=(n, R.ctl_size(nu))).astype(f32)
    ctl[:, F["imitation_i"][0]] = rng.uniform(0, 40, n).astype(f32)
    ctl[:, F["phase_frequency_factor"][0]] = rng.uniform(0.5, 1.5, n).astype(f32)
    if n > 2:
        ctl[0, F["imitation_i"][0]], ctl[0, F["phase_frequency_factor"][0]] = 39.5, 1.0    # wraps at nb
    fall_at, nan_robot = n // 2, (n - 1 if n > 1 else None)
    acc_ref, alive_ref = torch.zeros(n, 6), torch.ones(n)
    ctl_d, obs_d = dev(ctl, gpu), torch.full((n + 1, O), 7.0, device=gpu)      # a guard row behind the last robot
    acc_d, alive_d = torch.zeros(n, 6, device=gpu), torch.ones(n, device=gpu)
    phase_err = 0.0
    for call in range(5):
        qpos, qvel, aux = _random_state(d, n, rng, call, fall_at, nan_robot)
        q_d, v_d, a_d = dev(qpos, gpu), dev(qvel, gpu), dev(aux, gpu)
        before = ctl.copy()
        obs_ref, ph64 = R.observe(d, qpos, qvel, aux, ctl, acc_ref, alive_ref)
        native.check(L.duck_fleet_observe(C.byref(D), n, q_d.data_ptr(), v_d.data_ptr(), a_d.data_ptr(),
                                          ctl_d.data_ptr(), obs_d.data_ptr(), acc_d.data_ptr(), alive_d.data_ptr(),
                                          stream(gpu)), L)
        obs, got_ctl = obs_d.cpu().numpy(), ctl_d.cpu().numpy()
        assert (obs[n] == 7.0).all()
        np.testing.assert_array_equal(bits(obs[:n, :O - 2]), bits(obs_ref[:, :O - 2]))
        ph = F["imitation_phase"][0]
        np.testing.assert_array_equal(bits(got_ctl[:, :ph]), bits(ctl[:, :ph]))      # imitation_i too
        if standing:
            np.testing.assert_array_equal(bits(got_ctl), bits(before))
            np.testing.assert_array_equal(bits(obs[:n, O - 2:]), bits(before[:, ph:ph + 2]))
        else:
            phase_err = max(phase_err, np.abs(obs[:n, O - 2:] - ph64).max())
            np.testing.assert_array_equal(bits(obs[:n, O - 2:]), bits(got_ctl[:, ph:ph + 2]))
        np.testing.assert_array_equal(bits(acc_d.cpu().numpy()), bits(acc_ref.numpy()))
        np.testing.assert_array_equal(alive_d.cpu().numpy(), alive_ref.numpy())
    print(f"observe n={n} nu={nu}: phase max |err| vs float64 {phase_err:.2e} (bound {PHASE_TOL:.0e})")
    assert phase_err <= PHASE_TOL
    # the constructed robots fell when they should, and only their accumulators stopped
    assert alive_ref[fall_at] == 0 and acc_ref[fall_at, 0] == (1 if nan_robot == fall_at else 2)
    if nan_robot is not None and nan_robot != fall_at:
        assert alive_ref[nan_robot] == 0 and acc_ref[nan_robot, 0] == 1
    if n > 2:
        assert alive_ref[0] == 1 and acc_ref[0, 0] == 5


@pytest.mark.parametrize("n,nu,limits", [(1, 14, 1), (17, 3, 1), (130, 14, 1), (17, 16, 1), (130, 14, 0)])
def test_actuate_kernel_alone(gpu, n, nu, limits):
    L = native.lib()
    d = R.make_desc(nu=nu, speed_limits=limits)
    D = c_desc(d)
    rng = np.random.default_rng(200 + n + nu)
    F = R.ctl_fields(nu)
    ctl = rng.normal(size=(n, R.ctl_size(nu))).astype(f32)
    default = np.asarray(d.act_default[:nu], f32)
    p = F["prev_motor_targets"][0]
    ctl_d = dev(ctl, gpu)
    ctrl_d = torch.full((nu + 1, n), 7.0, device=gpu)
    hit = np.zeros(3, int)
    for call in range(3):
        action = rng.uniform(-1, 1, size=(n, nu)).astype(f32)
        # rows by turns: a target far above prev (upper limit), far below (lower limit), within the step (neither)
        kind = (np.arange(n)[:, None] + np.arange(nu)[None, :] + call) % 3
        prev = default + action * f32(0.25) + np.where(kind == 0, -1.0, np.where(kind == 1, 1.0, 0.01)).astype(f32)
        ctl[:, p:p + nu] = prev.astype(f32)
        ctl_d[:, p:p + nu] = dev(ctl[:, p:p + nu], gpu)
        ctrl_ref = R.actuate(d, action, ctl)
        a_d = dev(action, gpu)
        native.check(L.duck_fleet_actuate(C.byref(D), n, a_d.data_ptr(), ctl_d.data_ptr(), ctrl_d.data_ptr(),
                                          stream(gpu)), L)
        ctrl = ctrl_d.cpu().numpy()
        assert (ctrl[nu] == 7.0).all()
        np.testing.assert_array_equal(bits(ctrl[:nu]), bits(ctrl_ref))
        np.testing.assert_array_equal(bits(ctl_d.cpu().numpy()), bits(ctl))
        mt = ctl[:, F["motor_targets"][0]:][:, :nu]
        step = f32(5.24 * 0.002 * 10)
        hit += [int((mt == (prev.astype(f32) + step).astype(f32)).sum()), int((mt == (prev.astype(f32) - step).astype(f32)).sum()),
                int((kind == 2).sum())]
    if limits:
        assert (hit > 0).all() or n * nu < 3, hit
    else:
        assert hit[0] == 0 and hit[1] == 0


# --- the loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("randomize", [None, 7])
def test_batch_invariance(policy_file, gpu, randomize):
    _, path = policy_file
    cmd = commands(33)
    big = FleetInfer("flat_terrain", path, 33, device=gpu, randomize=randomize)
    one = FleetInfer("flat_terrain", path, 1, device=gpu, randomize=randomize)
    if randomize is not None:   # duck_randomize is keyed by the global robot id: robot 20's record, copied
        one.dr.copy_(big.dr.view(-1, 33)[:, 20])
        assert not torch.equal(big.dr.view(-1, 33)[:, 20], big.dr.view(-1, 33)[:, 0])
        one.restart()
    big.set_commands(cmd)
    one.set_commands(cmd[20])
    obs_big, obs_one = big.run(10, record=True), one.run(10, record=True)
    assert obs_big.shape == (10, 33, 101) and np.isfinite(obs_big).all()
    np.testing.assert_array_equal(bits(obs_big[:, 20]), bits(obs_one[:, 0]))
    for a, b in zip(big.state(), one.state()):
        np.testing.assert_array_equal(bits(a[20]), bits(b[0]))
    assert not np.array_equal(obs_big[-1, 20], obs_big[-1, 19])      # the commands do matter
    np.testing.assert_array_equal(obs_big[:, :, 6:13], np.broadcast_to(cmd, (10, 33, 7)))


def test_graph_replay_equals_eager(policy_file, gpu, monkeypatch):
    _, path = policy_file
    monkeypatch.setattr(FleetInfer, "CHUNK", 4)
    cmd = commands(8, seed=12)
    a = FleetInfer("flat_terrain", path, 8, device=gpu)
    b = FleetInfer("flat_terrain", path, 8, device=gpu)
    a.set_commands(cmd)
    b.set_commands(cmd)
    a.run(3)      # the first call is eager
    assert a.graph is None
    a.run(8)      # two replays of the 4-period graph
    assert a.graph is not None and a.graph[1] == 4
    b.run(11)
    assert b.graph is None
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(bits(x), bits(y))
    for name in ("ctl", "obs", "acc", "alive", "warm"):
        np.testing.assert_array_equal(bits(getattr(a, name).cpu().numpy()), bits(getattr(b, name).cpu().numpy()))
    assert (a.report()["periods"] == 11).all()


def _fp64_policy(graph, x):
    """The exported graph in float64 numpy on float32 observations x [n][obs]."""
    pol = dense_policy(graph)
    h = (x.astype(f32).astype(np.float64) - graph.init["mean"].astype(np.float64)) / graph.init["std"].astype(np.float64)
    for k, (w, b) in enumerate(zip(pol["W"], pol["b"])):
        h = h @ w.astype(np.float64).T + b.astype(np.float64)
        if k < len(pol["W"]) - 1:
            h = h / (1.0 + np.exp(-h))
    return np.tanh(h[:, :pol["action_size"]])


def test_teacher_forced_against_mjinfer(policy_file, gpu):
    """Per period the 1-robot fleet takes MjInfer's state and history, then both run one control period.
    The action's bound is computed here: four times the largest error of OnnxGraph.run (numpy float32)
    against a float64 evaluation of the same graph over the 25 observations -- the margin for the MFMA
    chain's summation order and __expf. Measured on MI355X: non-phase observation error at most 0.89 of
    its bound 2^-23 max(1, |ref|), phase 4.5e-7 (bound 2e-6), action 4.50e-7 (bound 1.20e-6)."""
    _, path = policy_file
    graph = OnnxGraph(open(path, "rb").read())
    cmd = [0.1, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0]
    mj = MjInfer("flat_terrain", onnx_model_path=path, device=gpu)
    mj.commands = cmd
    fleet = FleetInfer("flat_terrain", path, 1, device=gpu)
    fleet.set_commands(cmd)
    col = lambda t: t[:, 0].cpu().numpy()  # noqa: E731
    obs_ref, obs_fleet, act_fleet = [], [], []
    for _ in range(25):
        fleet.load_state(qpos=col(mj.qpos), qvel=col(mj.qvel), ctrl=col(mj.ctrl), qacc_warmstart=col(mj.warm),
                         last_action=mj.last_action, last_last_action=mj.last_last_action,
                         last_last_last_action=mj.last_last_last_action, motor_targets=mj.motor_targets,
                         prev_motor_targets=mj.prev_motor_targets, imitation_i=[mj.imitation_i])
        o, _ = mj.control_step()
        obs_ref.append(o)
        obs_fleet.append(fleet.run(1, record=True)[0, 0])
        act_fleet.append(fleet.action.cpu().numpy()[0])
    obs_ref, obs_fleet, act_fleet = np.array(obs_ref), np.array(obs_fleet, np.float64), np.array(act_fleet, np.float64)
    err = np.abs(obs_fleet - obs_ref)
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(obs_ref))
    print("obs (non-phase) max err / tol: %.3f; phase max |err| %.2e" % ((err / tol)[:, :99].max(), err[:, 99:].max()))
    exact = _fp64_policy(graph, obs_ref)
    runtime = graph.run({"obs": obs_ref.astype(f32)})[0].astype(np.float64)
    bound = 4.0 * np.abs(runtime - exact).max()
    fleet_err = np.abs(act_fleet - exact).max()
    print("action vs float64: fleet max |err| %.3e, bound (4 x numpy float32's %.3e) %.3e"
          % (fleet_err, bound / 4, bound))
    assert (err[:, :99] <= tol[:, :99]).all()
    assert err[:, 99:].max() <= PHASE_TOL
    assert fleet_err <= bound


def test_fallen_robot_stops_counting(policy_file, gpu):
    from tests.oracle_ffi import OracleModel
    _, path = policy_file
    fleet = FleetInfer("flat_terrain", path, 3, device=gpu)
    m = fleet.model
    home = np.asarray(m.key_qpos[m.names["key"].index("home")], np.float64)
    w, x, y, z = home[3:7]
    flipped = home.copy()
    flipped[3:7] = [-x, w, -z, y]          # (0, 1, 0, 0) * q: the base turned by pi about the world's x
    om = OracleModel(m)
    d = om.new_data(qpos=flipped)
    om.forward(d)
    up = int(m.sensor_adr[m.names["sensor"].index("upvector")])
    assert d.arr("sensordata")[up + 2] < 0
    q = np.stack([home, flipped, home]).astype(f32)
    fleet.load_state(qpos=q)
    fleet.set_commands([0.1, 0.0, 0.0, 0, 0, 0, 0])
    fleet.run(5)
    rep = fleet.report()
    assert list(rep["fell"]) == [False, True, False] and list(rep["periods"]) == [5, 0, 5]
    assert np.isnan(rep["mean_vx"][1]) and np.isfinite(rep["rms_lin_err"][[0, 2]]).all()
    for a in fleet.state() + (fleet.ctl.cpu().numpy(), fleet.acc.cpu().numpy()):
        np.testing.assert_array_equal(bits(a[0]), bits(a[2]))


def test_standing_keeps_the_phase(policy_file, gpu):
    _, path = policy_file
    fleet = FleetInfer("flat_terrain", path, 2, standing=True, device=gpu)
    obs = fleet.run(5, record=True)
    assert (obs[:, :, 99:] == 0).all() and np.isfinite(obs).all()
    assert (fleet.ctl_field("imitation_phase") == 0).all() and (fleet.ctl_field("imitation_i") == 0).all()
    assert (fleet.report()["periods"] == 5).all()
    walking = FleetInfer("flat_terrain", path, 2, device=gpu)
    walking.run(5)
    assert (walking.ctl_field("imitation_i") == 5).all()


def test_edited_scene_runs_from_its_own_library(policy_file, gpu):
    _, path = policy_file
    scene = os.path.join(ROOT, "tests", "golden", "models", "flat_terrain_edited.npz")
    fleet = FleetInfer(scene, path, 3, device=gpu)
    assert fleet._lib is not native.lib()       # the symbols ship with the model's own library
    flat = FleetInfer("flat_terrain", path, 3, device=gpu)
    obs, obs_flat = fleet.run(3, record=True), flat.run(3, record=True)
    assert np.isfinite(obs).all() and (fleet.report()["periods"] == 3).all()
    np.testing.assert_array_equal(bits(obs[:, 0]), bits(obs[:, 2]))
    assert not np.array_equal(obs[-1], obs_flat[-1])      # stiffer servos, another foot: another trajectory
    d = R.desc_values(fleet.desc)
    assert d.naux == fleet.env.aux_size() and d.act_qpos[:14] == [int(fleet.model.jnt_qposadr[j]) for j in fleet.model.actuator_trnid]


def test_command_line_writes_the_grid_report(policy_file, gpu, tmp_path):
    _, path = policy_file
    out = str(tmp_path / "report.json")
    subprocess.run([sys.executable, "-m", "open_duck_playground_amd.sim2sim", "-o", path, "--num_robots", "32",
                    "--periods", "10", "--command_grid", "2x2x2", "--out", out, "--device", gpu], cwd=ROOT, check=True,
                   timeout=300)
    doc = json.load(open(out))
    cells = doc["cells"]
    assert len(cells) == 8 and sum(c["count"] for c in cells) == 32
    assert sorted({c["command"][0] for c in cells}) == pytest.approx([-0.15, 0.15])
    assert sorted({c["command"][2] for c in cells}) == pytest.approx([-1.0, 1.0])
    for c in cells:
        assert 0.0 <= c["survival_rate"] <= 1.0 and c["rms_lin_err"] is not None
