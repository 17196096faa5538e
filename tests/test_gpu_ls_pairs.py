"""The line search's paired bracket ends and its saturating activity flag on the GPU (duck_team.h quad2_pair,
duck_lspairs.h).

Each line-search iteration evaluates the rows' quadratic coefficients at the bracket ends al, ah as one pair
(packed FMAs over both points), and every one-sided row's 0/1 activity factor is one saturating multiply in
place of compare and select. What could go wrong: a coefficient that meets the other point's alpha or flag, a
friction zone taken from the other half, a flag that differs from x < 0 on some class of x (then a row's
coefficients enter or leave a point they should not), a kernel compiled with another form than the rest.

  (a) one physics_kernel substep (duck_physics_step, the same TPhys::step as the step kernels) of 32 hand-built
      envs, flat (NV 20, one limit row per lane) and rough + backlash (NV 30, two), against the fp64 oracle at
      tests/test_gpu_physics.py's tolerances: M rtol 1e-4 / atol 2e-6, qacc_smooth rtol 2e-3 / atol 2e-3,
      actuator forces 1e-4 / 1e-4, position and velocity sensors 1e-4 / 2e-4, contact distances 1e-5 where
      active, and per env |d qacc| / (1 + |qacc|) < 2e-2 for > 97 % of the envs whose manifolds agree, for qacc
      of the aux record and for the qacc_warmstart the substep writes back;
  (b) the same substep, word for word in every output (qpos, qvel, qacc_warmstart, the whole aux record),
      against the library built with -DDUCK_SCALAR_TWINS, where the two ends are two scalar quad2 calls and the
      flag is compare and select (native.debug_library "scalar_twins", built by __graft_entry__.build());
  (c) the flag's two forms (duck_debug_ls_flag) on +-0, the smallest normal and denormals of each sign, +-inf,
      NaN of each sign, +-1e-30, +-1e30, and ja + alpha v where ja = -alpha v exactly and one ulp either side:
      equal words.

The states (_states) put four kinds of team into every wave (envs 4w .. 4w + 3 are the four teams of a wave):
  0  in the air at rest: no contact or limit row is active anywhere along the line (asserted: every contact
     distance > 0), the friction rows stay in their quadratic zone, and the cost is one quadratic, so the first
     Newton point along the line ends the search (no iteration);
  1  standing with its feet through the floor (asserted: an active contact), started from qacc_smooth (zero
     qacc_warmstart, as after a reset);
  2  standing, started warm: qacc_warmstart is the oracle's qacc of the same state from a cold start (the scenes
     take one Newton step per substep, so this is that state's second step): the warm start's cost is below
     qacc_smooth's and it is chosen, beside kind 1's smooth start in the same wave;
  3  feet deeper through the floor, tilted, the first limited leg joint 0.03 rad past its upper limit and
     moving back (its row switches along the line), joint velocities of +1.5, -1.5 and 0 rad/s in turn, so that
     friction rows sit in each linear zone and in the quadratic one; many rows switch along the line, which is
     what takes the search to its iteration limit.
The iteration counts of kinds 0, 2 and 3 (none, few, up to the limit of 5) follow from that construction and
are not read back: the kernels export no per-team count.
"""

import os

import numpy as np
import pytest
import torch

from open_duck_playground_amd import joystick as jmod
from open_duck_playground_amd import native
from open_duck_playground_amd.joystick import Joystick
from open_duck_playground_amd.mjcf import axis_angle_quat, quat_mul
from tests.helpers import parse_aux
from tests.oracle_ffi import OracleModel

pytestmark = pytest.mark.gpu

SCENES = {"flat": "flat_terrain", "rough_backlash": "rough_terrain_backlash"}
N = 32  # two workgroups of the team kernels (16 envs each), eight waves of four teams
_cache = {}


def _states(m):
    rng = np.random.default_rng(5)
    key = m.key_qpos[0]
    qpos = np.tile(key, (N, 1))
    qvel = np.zeros((N, m.nv))
    ctrl = np.tile(m.key_ctrl[0], (N, 1))
    jl = next(j for j in range(1, m.njnt) if m.jnt_limited[j])
    for e in range(N):
        kind = e % 4
        yaw = axis_angle_quat([0, 0, 1], rng.uniform(-3.14, 3.14))
        qpos[e, 0:2] += rng.uniform(-0.05, 0.05, 2)
        if kind == 0:
            qpos[e, 2] = 0.5
            qpos[e, 3:7] = yaw
            continue
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        tilt = 0.15 if kind == 3 else 0.05
        qpos[e, 3:7] = quat_mul(yaw, axis_angle_quat(ax, rng.uniform(-tilt, tilt)))
        qpos[e, 2] = rng.uniform(0.13, 0.14) if kind == 3 else rng.uniform(0.145, 0.155)
        ctrl[e] += rng.uniform(-0.2, 0.2, m.nu)
        if kind == 3:
            qvel[e, :6] = rng.uniform(-0.3, 0.3, 6)
            qvel[e, 6:] = np.resize([1.5, -1.5, 0.0], m.nv - 6)
            qpos[e, m.jnt_qposadr[jl]] = m.jnt_range[jl][1] + 0.03
            qvel[e, m.jnt_dofadr[jl]] = -0.5
        else:
            qvel[e] = rng.uniform(-0.1, 0.1, m.nv)
    # (the oracle starts from the fp32 state the kernel sees)
    return tuple(a.astype(np.float32).astype(np.float64) for a in (qpos, qvel, ctrl))


def _oracle(m, qpos, qvel, ctrl, warm):
    om = OracleModel(m)
    r = {k: [] for k in ("qacc", "qacc_smooth", "sensordata", "con_dist", "M", "af")}
    for e in range(len(qpos)):
        d = om.new_data(qpos=qpos[e], qvel=qvel[e], ctrl=ctrl[e], warm=warm[e])
        om.forward(d)
        r["qacc"].append(d.arr("qacc", m.nv).copy())
        r["qacc_smooth"].append(d.arr("qacc_smooth", m.nv).copy())
        r["sensordata"].append(d.arr("sensordata", m.nsensordata).copy())
        r["con_dist"].append(d.arr("con_dist", 4 * m.npair).copy())
        r["M"].append(np.ctypeslib.as_array(d.qM)[:m.nv, :m.nv].copy())
        r["af"].append(d.arr("actuator_force", m.nu).copy())
    return {k: np.array(v) for k, v in r.items()}


def _case(scene, gpu):
    """States, warm starts and oracle results of a scene: computed once, shared by the tests, left unchanged."""
    if scene not in _cache:
        m = Joystick(scene, num_envs=1, device=gpu, use_imitation=False).mj_model
        qpos, qvel, ctrl = _states(m)
        warm = np.zeros((N, m.nv))
        cold = _oracle(m, qpos, qvel, ctrl, warm)
        warm[2::4] = cold["qacc"][2::4].astype(np.float32).astype(np.float64)
        ref = _oracle(m, qpos, qvel, ctrl, warm)
        for a in (qpos, qvel, ctrl, warm, *ref.values()):
            a.setflags(write=False)
        _cache[scene] = (m, qpos, qvel, ctrl, warm, ref)
    return _cache[scene]


def _substep(scene, gpu, qpos, qvel, ctrl, warm):
    """One physics_kernel substep through the library Joystick picks: the outputs as float32 arrays."""
    env = Joystick(scene, num_envs=1, device=gpu, use_imitation=False)
    T = lambda a: torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float32, device=gpu)
    tq, tv, tw, tc = T(qpos), T(qvel), T(warm), T(ctrl)
    aux = torch.zeros(env.aux_size() * N, dtype=torch.float32, device=gpu).view(-1, N)
    env.physics_step(tq, tv, tw, tc, 1, aux)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in (("qpos", tq), ("qvel", tv), ("qacc_warmstart", tw), ("aux", aux))}


@pytest.mark.parametrize("case", list(SCENES))
def test_substep_matches_oracle(case, gpu):
    scene = SCENES[case]
    m, qpos, qvel, ctrl, warm, r = _case(scene, gpu)
    out = _substep(scene, gpu, qpos, qvel, ctrl, warm)
    g = parse_aux(m, out["aux"].astype(np.float64))
    assert (g["con_dist"][0::4] > 0).all() and (r["con_dist"][0::4] > 0).all(), "kind 0 is in the air"
    for k in (1, 2, 3):
        assert (g["con_dist"][k::4] < 0).any(axis=1).all(), f"kind {k} stands on the floor"
    np.testing.assert_allclose(g["Mdense"], r["M"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(g["qacc_smooth"], r["qacc_smooth"], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(g["actuator_force"], r["af"], rtol=1e-4, atol=1e-4)
    act = (r["con_dist"] < 0) | (g["con_dist"] < 0)
    ok = np.all((np.abs(g["con_dist"] - r["con_dist"]) < 1e-5) | ~act, axis=1)
    pv = [k for k in range(m.nsensordata) if not (6 <= k < 9)]
    np.testing.assert_allclose(g["sensordata"][:, pv], r["sensordata"][:, pv], rtol=1e-4, atol=2e-4)
    amax = np.abs(r["qacc"]).max(axis=1)
    rel = np.abs(g["qacc"] - r["qacc"]).max(axis=1) / (1 + amax)
    relw = np.abs(out["qacc_warmstart"].T.astype(np.float64) - r["qacc"]).max(axis=1) / (1 + amax)
    print(f"{case}: manifolds agree {ok.mean():.3f}; qacc rel by kind "
          f"{[float(f'{rel[k::4].max():.2g}') for k in range(4)]}, qacc_warmstart rel max {relw.max():.3g}, "
          f"max |d qacc_smooth| {np.abs(g['qacc_smooth'] - r['qacc_smooth']).max():.3g}")
    assert np.isfinite(out["aux"]).all() and np.isfinite(out["qacc_warmstart"]).all()
    assert ok.mean() > 0.98, ok.mean()
    assert (rel[ok] < 2e-2).mean() > 0.97, np.sort(rel)[-8:]
    assert (relw[ok] < 2e-2).mean() > 0.97, np.sort(relw)[-8:]


@pytest.mark.parametrize("case", list(SCENES))
def test_pairs_equal_scalar_twins_word_for_word(case, gpu, monkeypatch):
    scene = SCENES[case]
    path = os.path.join(native.BUILD, "libduck_scalar_twins.so")
    assert os.path.exists(path), "built by __graft_entry__.build()"
    m, qpos, qvel, ctrl, warm, _ = _case(scene, gpu)
    new = _substep(scene, gpu, qpos, qvel, ctrl, warm)
    monkeypatch.setattr(jmod, "model_library", lambda m: path)
    old = _substep(scene, gpu, qpos, qvel, ctrl, warm)
    for k in new:
        a, b = new[k].view(np.int32), old[k].view(np.int32)
        assert a.shape == b.shape
        d = a != b
        assert not d.any(), (k, int(d.sum()), np.argwhere(d)[:8].tolist())
    assert np.abs(new["qacc_warmstart"]).max() > 1.0  # (the substep ran: qacc is written back)


def _flag_inputs():
    U = lambda u: np.array([u], dtype=np.uint32).view(np.float32)[0]
    xs = [0.0, -0.0, U(0x00800000), U(0x80800000), U(0x00000001), U(0x80000001), U(0x007FFFFF), U(0x807FFFFF),
          np.inf, -np.inf, U(0x7FC00000), U(0xFFC00000), U(0x7F800001), 1e-30, -1e-30, 1e30, -1e30, 1.0, -1.0,
          U(0x7F7FFFFF), U(0xFF7FFFFF)]
    # ja = -alpha v exactly, and one ulp of ja either side: x as the kernel's FMA gives it (one rounding)
    for al, v in ((0.37, 1.7), (-2.5, 0.003), (1e-3, -40.0)):
        al, v = np.float32(al), np.float32(v)
        p = np.float32(np.float64(al) * np.float64(v))
        for ja in (-p, np.nextafter(-p, np.float32(np.inf)), np.nextafter(-p, np.float32(-np.inf))):
            xs.append(np.float32(np.float64(ja) + np.float64(al) * np.float64(v)))
    return np.array(xs, dtype=np.float32)


def test_saturating_flag_equals_compare_and_select(gpu):
    x = _flag_inputs()
    n = len(x)
    tx = torch.tensor(x.view(np.int32), device=gpu).view(torch.float32)
    sel = torch.full((n,), 7.0, dtype=torch.float32, device=gpu)
    sat = torch.full((n,), 9.0, dtype=torch.float32, device=gpu)
    L = native.lib()
    native.check(L.duck_debug_ls_flag(n, tx.data_ptr(), sel.data_ptr(), sat.data_ptr(), None), L)
    torch.cuda.synchronize()
    a, b = sel.cpu().numpy().view(np.uint32), sat.cpu().numpy().view(np.uint32)
    with np.errstate(invalid="ignore"):
        want = np.where(x < 0, np.float32(1), np.float32(0)).view(np.uint32)
    # (a denormal x: the two forms must agree; which value they agree on is the device's denormal mode)
    den = (np.abs(x) < np.float32(2.0 ** -126)) & (x != 0)
    for i in range(n):
        print(f"x {x.view(np.uint32)[i]:08x}: select {a[i]:08x}  saturating {b[i]:08x}")
    assert (a == b).all(), [(hex(x.view(np.uint32)[i]), hex(a[i]), hex(b[i])) for i in np.nonzero(a != b)[0]]
    bad = (a != want) & ~den
    assert not bad.any(), [(hex(x.view(np.uint32)[i]), hex(a[i]), hex(want[i])) for i in np.nonzero(bad)[0]]
