"""M's register columns in the throughput kernel: crb with an opaque lane, M x without the all-zero rows.

The throughput kernel's M x skips the rows that are zero on every lane of a column set (duck_mcols.h
zero_row; the latency kernels multiply by the loaded zeros), and its crb forms its lane masks inside the
substep. Both must leave every bit where it was. What could go wrong: a row flagged zero that is not (a wrong
M x: qacc and the line search move), a mask formed from the laundered lane that differs from the hoisted one
(a wrong or missing entry of M). Checked at 1 env and at 17 envs (one full 16-env workgroup and a workgroup
with one live team), on the four shipped scenes and two edited scenes with kernels compiled for them:
flat_terrain_edited (the shipped dof tree) and flat_terrain_head_last, the same robot with the head limb behind
both legs (dofs 16-19, so that the last column set holds a whole limb whose parent is the free joint, rows 6-15
are zero on it, and the right leg's limb ends at lane 15: another dof_parentid and another zero_row table):
  (a) physics_kernel from states three random-action env-steps after reset: the dense M of the aux record,
      qacc_smooth and qacc against the fp64 oracle at tests/test_gpu_physics.py's tolerances;
  (b) after 5 env-steps the throughput kernel equals the latency and paired kernels, and latency_x2 in the
      scenes that compile it (MODES: a plane floor and NV <= 20, LatX2::PAYS), bit for bit in every State field.
"""

import numpy as np
import pytest
import torch

from open_duck_playground_amd.joystick import Joystick
from open_duck_playground_amd.native import DuckError
from tests.helpers import parse_aux
from tests.kat_checks import model_path
from tests.oracle_ffi import OracleModel
from tests.test_gpu_step_prefetch import _assert_same_bits

pytestmark = pytest.mark.gpu

# id: (scene, the step modes it compiles besides "throughput") -- one table, so that a scene and its modes
# cannot come apart
X2, NO_X2 = ("latency", "paired", "latency_x2"), ("latency", "paired")
CASES = {
    "flat": ("flat_terrain", X2),
    "backlash": ("flat_terrain_backlash", NO_X2),
    "rough": ("rough_terrain", NO_X2),
    "rough_backlash": ("rough_terrain_backlash", NO_X2),
    "edited": (model_path("flat_terrain_edited"), X2),
    "head_last": (model_path("flat_terrain_head_last"), X2),
}
IDS = list(CASES)
SCENES = [CASES[k][0] for k in IDS]
MODES = {k: CASES[k][1] for k in IDS}
SIZES = [1, 17]


def _rollout(scene, n, gpu, mode, steps, seed=3):
    env = Joystick(scene, num_envs=n, device=gpu, use_imitation=False)
    env.set_step_mode(mode)
    assert env.step_kernel == mode
    env.lat_timeouts(reset=True)
    st = env.reset(rng=seed)
    rng = np.random.default_rng(5)
    for _ in range(steps):
        a = torch.tensor(rng.uniform(-1, 1, (n, env.action_size)).astype(np.float32), device=gpu)
        st = env.step(st, a)
    torch.cuda.synchronize()
    return env, st


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scene", SCENES, ids=IDS)
def test_mass_matrix_and_accelerations_match_oracle(scene, n, gpu):
    env, st = _rollout(scene, n, gpu, "throughput", 3)
    m = env.mj_model
    qpos = st.data.qpos.detach().cpu().numpy().astype(np.float64).reshape(n, m.nq)
    qvel = st.data.qvel.detach().cpu().numpy().astype(np.float64).reshape(n, m.nv)
    ctrl = st.data.ctrl.detach().cpu().numpy().astype(np.float64).reshape(n, m.nu)
    T = lambda a: torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float32, device=gpu)
    tq, tv, tw, tc = T(qpos), T(qvel), T(np.zeros((n, m.nv))), T(ctrl)
    aux = torch.zeros(env.aux_size() * n, dtype=torch.float32, device=gpu).view(-1, n)
    env.physics_step(tq, tv, tw, tc, 0, aux)
    torch.cuda.synchronize()
    g = parse_aux(m, aux.cpu().numpy().astype(np.float64))
    om = OracleModel(m)
    M, qs, qa, cd = [], [], [], []
    for e in range(n):
        # the oracle from the fp32 state the kernel saw
        d = om.new_data(qpos=qpos[e].astype(np.float32).astype(np.float64), qvel=qvel[e], ctrl=ctrl[e])
        om.forward(d)
        M.append(np.ctypeslib.as_array(d.qM)[:m.nv, :m.nv].copy())
        qs.append(d.arr("qacc_smooth", m.nv).copy())
        qa.append(d.arr("qacc", m.nv).copy())
        cd.append(d.arr("con_dist", 4 * m.npair).copy())
    M, qs, qa, cd = np.array(M), np.array(qs), np.array(qa), np.array(cd)
    err_m = np.abs(g["Mdense"] - M).max()
    rel = np.abs(g["qacc"] - qa).max(axis=1) / (1 + np.abs(qa).max(axis=1))
    print(f"n {n}: max |dM| {err_m:.3g}, max |d qacc_smooth| {np.abs(g['qacc_smooth'] - qs).max():.3g}, "
          f"qacc rel max {rel.max():.3g}")
    np.testing.assert_allclose(g["Mdense"], M, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(g["qacc_smooth"], qs, rtol=2e-3, atol=2e-3)
    act = (cd < 0) | (g["con_dist"] < 0)
    ok = np.all((np.abs(g["con_dist"] - cd) < 1e-5) | ~act, axis=1)
    assert ok.mean() > 0.98, ok.mean()
    assert (rel[ok] < 2e-2).mean() > 0.97, np.sort(rel)[-10:]


def test_head_last_scene_has_another_dof_tree():
    from open_duck_playground_amd import constants
    from open_duck_playground_amd.mjcf import Model
    tree = list(Model.load(model_path("flat_terrain_head_last")).arrays["dof_parentid"])
    assert tree == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 5, 11, 12, 13, 14, 5, 16, 17, 18]
    for task in (CASES[k][0] for k in IDS if k != "head_last"):
        path = task if task.endswith(".npz") else constants.task_to_xml(task)
        assert list(Model.load(path).arrays["dof_parentid"]) != tree, task


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("scene,case", list(zip(SCENES, IDS)), ids=IDS)
def test_throughput_equals_latency_kernels(scene, case, n, gpu):
    ref_env, ref = _rollout(scene, n, gpu, "throughput", 5)
    for mode in MODES[case]:
        env, st = _rollout(scene, n, gpu, mode, 5)
        _assert_same_bits(ref, st, (mode, n))
        assert env.lat_timeouts() == 0
    if "latency_x2" not in MODES[case]:
        with pytest.raises(DuckError, match="not compiled for this model"):
            ref_env.set_step_mode("latency_x2")
