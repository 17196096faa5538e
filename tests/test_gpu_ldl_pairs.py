"""The register LDL' with packed row updates (duck_ldlpairs.h, duck_team.h fac_upd) on the GPU.

Rows 2m, 2m + 1 that a pivot updates in one column set go through one packed FMA; the factor's columns are
held as those row pairs. What could go wrong: a pair whose halves are swapped or that takes a row the pivot
does not update (a wrong factor: qacc_smooth and the Newton step move), a one-row read or write of a pair
that lands in the other half, a kernel variant compiled with another pairing than the rest. Checked at 1 env
(a single team) and at 17 envs (one full workgroup and one with a single live team), on flat, flat + backlash,
rough + backlash (NV = 30: the second column set holds whole limbs) and flat_terrain_head_last (another dof
tree: the head limb is the second set's):
  (a) one physics_kernel substep from seeded non-rest states (tests/helpers.random_states) against the fp64
      oracle in qacc_smooth, qacc and the constraint force, at tests/test_gpu_physics.py::test_forward_parity's
      tolerances: qacc_smooth rtol 2e-3 / atol 2e-3; per env |d qacc| / (1 + |qacc|) < 2e-2 where the contact
      manifolds agree. The aux record has no constraint rows; the constraint force is compared in generalized
      coordinates, qfrc_constraint = M qacc - qfrc_smooth, each side from its own M, qacc and qfrc_smooth. Its
      bound follows from the three tolerances above it: row i of the difference is at most
      sum_j |M_ij| tol_qacc + sum_j tol_M_ij |qacc_j| + tol_qfrc_smooth, with tol_qacc = 2e-2 (1 + max |qacc|),
      tol_M = 1e-4 |M| + 2e-6 (test_forward_parity's) and tol_qfrc_smooth = 1e-4 |qfrc_smooth| + 1e-4 (fp32
      sums of actuator, bias and passive forces, the actuator forces' own tolerance there);
  (b) the same for one env with both feet off the ground and one with a knee past its upper limit, so that
      the one-sided contact and limit rows switch along the search line;
  (c) after 3 env-steps the throughput kernel equals the latency and paired kernels, and latency_x2 in the
      scenes that compile it, bit for bit in every State field.
"""

import numpy as np
import pytest
import torch

from open_duck_playground_amd.joystick import Joystick
from tests.helpers import parse_aux, random_states
from tests.kat_checks import model_path
from tests.oracle_ffi import OracleModel
from tests.test_gpu_mcols import _rollout
from tests.test_gpu_step_prefetch import _assert_same_bits

pytestmark = pytest.mark.gpu

X2, NO_X2 = ("latency", "paired", "latency_x2"), ("latency", "paired")
CASES = {
    "flat": ("flat_terrain", X2),
    "backlash": ("flat_terrain_backlash", NO_X2),
    "rough_backlash": ("rough_terrain_backlash", NO_X2),
    "head_last": (model_path("flat_terrain_head_last"), X2),
}
IDS = list(CASES)
SIZES = [1, 17]


def _substep(scene, qpos, qvel, ctrl, gpu):
    """One physics_kernel substep from (qpos, qvel, ctrl): the aux record of its forward pass and the oracle's."""
    n = len(qpos)
    # (the oracle starts from the fp32 state the kernel sees)
    qpos, qvel, ctrl = (a.astype(np.float32).astype(np.float64) for a in (qpos, qvel, ctrl))
    env = Joystick(scene, num_envs=1, device=gpu, use_imitation=False)
    m = env.mj_model
    T = lambda a: torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float32, device=gpu)
    tq, tv, tw, tc = T(qpos), T(qvel), T(np.zeros((n, m.nv))), T(ctrl)
    aux = torch.zeros(env.aux_size() * n, dtype=torch.float32, device=gpu).view(-1, n)
    env.physics_step(tq, tv, tw, tc, 1, aux)
    torch.cuda.synchronize()
    g = parse_aux(m, aux.cpu().numpy().astype(np.float64))
    om = OracleModel(m)
    r = {k: [] for k in ("qacc", "qacc_smooth", "qfrc_smooth", "con_dist", "M")}
    for e in range(n):
        d = om.new_data(qpos=qpos[e], qvel=qvel[e], ctrl=ctrl[e])
        om.forward(d)
        for k in ("qacc", "qacc_smooth", "qfrc_smooth"):
            r[k].append(d.arr(k, m.nv).copy())
        r["con_dist"].append(d.arr("con_dist", 4 * m.npair).copy())
        r["M"].append(np.ctypeslib.as_array(d.qM)[:m.nv, :m.nv].copy())
    return m, g, {k: np.array(v) for k, v in r.items()}


def _check(g, r, what, every_env=False):
    np.testing.assert_allclose(g["qacc_smooth"], r["qacc_smooth"], rtol=2e-3, atol=2e-3)
    act = (r["con_dist"] < 0) | (g["con_dist"] < 0)
    ok = np.all((np.abs(g["con_dist"] - r["con_dist"]) < 1e-5) | ~act, axis=1)
    amax = np.abs(r["qacc"]).max(axis=1)
    rel = np.abs(g["qacc"] - r["qacc"]).max(axis=1) / (1 + amax)
    fg = np.einsum("eij,ej->ei", g["Mdense"], g["qacc"]) - g["qfrc_smooth"]
    fr = np.einsum("eij,ej->ei", r["M"], r["qacc"]) - r["qfrc_smooth"]
    bound = (np.abs(r["M"]).sum(axis=2) * (2e-2 * (1 + amax))[:, None] +
             np.einsum("eij,ej->ei", 1e-4 * np.abs(r["M"]) + 2e-6, np.abs(r["qacc"])) +
             1e-4 * np.abs(r["qfrc_smooth"]) + 1e-4)
    fex = (np.abs(fg - fr) / bound).max(axis=1)
    print(f"{what}: manifolds agree {ok.mean():.2f}, max |d qacc_smooth| {np.abs(g['qacc_smooth'] - r['qacc_smooth']).max():.3g}, "
          f"qacc rel max {rel.max():.3g}, constraint force / bound max {fex.max():.3g}")
    assert np.isfinite(g["qacc"]).all()
    if every_env:
        assert ok.all() and (rel < 2e-2).all() and (fex < 1).all(), (ok, rel, fex)
    else:
        assert ok.mean() > 0.98, ok.mean()
        assert (rel[ok] < 2e-2).mean() > 0.97, np.sort(rel)[-10:]
        assert (fex[ok] < 1).mean() > 0.97, np.sort(fex)[-10:]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", IDS)
def test_substep_matches_oracle(case, n, gpu):
    scene = CASES[case][0]
    m0 = Joystick(scene, num_envs=1, device=gpu, use_imitation=False).mj_model
    qpos, qvel, ctrl = random_states(m0, n, seed=11)
    m, g, r = _substep(scene, qpos, qvel, ctrl, gpu)
    _check(g, r, f"{case} n {n}")


@pytest.mark.parametrize("case", IDS)
def test_feet_in_the_air_and_a_joint_past_its_limit(case, gpu):
    """Env 0: the base 0.5 m up, no floor contact (the contact rows stay off along the whole search line).
    Env 1: the same pose standing, with the first limited leg joint 0.03 rad past its upper limit and moving
    back (its limit row is active at the start and switches off along the line)."""
    scene = CASES[case][0]
    m0 = Joystick(scene, num_envs=1, device=gpu, use_imitation=False).mj_model
    qpos, qvel, ctrl = random_states(m0, 2, seed=12, vel=0.1)
    qpos[0, 2] = 0.5
    j = next(j for j in range(1, m0.njnt) if m0.jnt_limited[j])
    qpos[1, m0.jnt_qposadr[j]] = m0.jnt_range[j][1] + 0.03
    qvel[1, m0.jnt_dofadr[j]] = -0.5
    m, g, r = _substep(scene, qpos, qvel, ctrl, gpu)
    assert (r["con_dist"][0] > 0).all() and (g["con_dist"][0] > 0).all(), "env 0 is in the air"
    _check(g, r, f"{case} air/limit", every_env=True)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", IDS)
def test_three_env_steps_equal_in_every_kernel(case, n, gpu):
    scene, modes = CASES[case]
    _, ref = _rollout(scene, n, gpu, "throughput", 3)
    for mode in modes:
        env, st = _rollout(scene, n, gpu, mode, 3)
        _assert_same_bits(ref, st, (mode, n))
        assert env.lat_timeouts() == 0
