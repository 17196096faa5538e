"""The warm start's twin chains as packed pairs (duck_team.h warm_rows_pair, spatial2_pair) and its straight-line
scalar form (warm_rows_both, contact_jx).

The solver's start evaluates every constraint row's cost at qacc_warmstart and at qacc_smooth and takes the
cheaper start. The throughput kernel and physics_kernel run the two evaluations as one pair (.x warm, .y
smooth); the latency kernels run them one after the other from the scalar statements. What could go wrong: a
half that meets the other start's word (a Huber zone, an activity flag, a foot's motion taken from the other
half), a product that contracts differently in the pair than in the scalar form, a lane past a kind's last row
whose cost or store is not dropped, a NaN of one team reaching a neighbour through a packed register.

Every test runs two physics_kernel substeps in one call (the second starts from the qacc the first wrote back
as its warm start) on 32 hand-built envs, flat (one limit row per lane) and rough + backlash (two). The six
kinds of team follow each other env by env (env e is kind e % 6), so every wave holds four different kinds side
by side:
  0  in the air, zero qacc_warmstart (as after a reset): the smooth start is chosen (asserted from the oracle's
     two start costs; standing on the floor a zero start is the cheaper one);
  1  standing with its feet through the floor, qacc_warmstart the oracle's qacc of that state from a cold
     start: the warm start is chosen (asserted likewise);
  2  joint velocities and a qacc_warmstart that put friction rows into different Huber zones at the two starts:
     each of the six ordered combinations of (lower linear, quadratic, upper linear) on some row (asserted);
  3  a limited joint past its limit whose row is active (J.x - aref < 0) at one start and inactive at the other,
     each way round on alternate teams (asserted);
  4  feet just through the floor and a qacc_warmstart that pushes the base up: at least four contact edges that
     are active at the smooth start are inactive at the warm start (asserted; on the plane floor every edge is);
  5  qacc_warmstart all NaN: the team's own words may be NaN; every other team equals, word for word, what it
     gives when this team is replaced by a finite one.
The asserted properties are read from the oracle's rows (oracle_set_hdump with oracle_set_force_start: J.x - aref
of every row and the friction band at each start), on the CPU.

  (a) against the fp64 oracle's two substeps, the criteria of tests/test_gpu_ls_pairs.py: contact distances
      within 1e-5 where active in > 98 % of the finite envs, and per env |d qacc| / (1 + |qacc|) < 2e-2 in
      > 97 % of those, for the aux record's qacc and for the written-back qacc_warmstart. On the CPU the oracle
      on the unrounded fp64 states against the oracle on their fp32 roundings stays inside the same cap;
  (b) word for word (qpos, qvel, qacc_warmstart, the whole aux record) against the library built with
      -DDUCK_SCALAR_TWINS, whose fused warm start is the scalar form;
  (c) Joystick.step from these states, the NaN teams included, in the throughput kernel against the latency and
      the paired latency kernels, word for word in every finite env.
"""

import ctypes as C
import os

import numpy as np
import pytest
import torch

from open_duck_playground_amd import joystick as jmod
from open_duck_playground_amd import native
from open_duck_playground_amd.joystick import Joystick
from open_duck_playground_amd.mjcf import JNT_HINGE, JNT_SLIDE, Model, axis_angle_quat, quat_mul
from tests import oracle_ffi
from tests.helpers import parse_aux
from tests.oracle_ffi import OracleModel

SCENES = {"flat": "flat_terrain", "rough_backlash": "rough_terrain_backlash"}
N = 32      # two workgroups of the team kernels (16 envs each), eight waves of four teams
NKIND = 6
NSUB = 2
ZONES = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if a != b]  # (zone at warm, zone at smooth)
_cache = {}


def _model(scene):
    return Model.load(os.path.join(native.HERE, "assets", f"{scene}.npz"))


def _rows(om, qpos, qvel, ctrl, warm, start):
    """The oracle's rows of one env at a start (1 qacc_warmstart, 2 qacc_smooth): J.x - aref per row, the
    friction band (R f, 0 on the one-sided rows), and the two start costs."""
    L = oracle_ffi.lib()
    buf = np.zeros(1 + oracle_ffi.MAXV * oracle_ffi.MAXV + 3 * 128)
    d = om.new_data(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm)
    L.oracle_set_force_start(start)
    L.oracle_set_hdump(buf.ctypes.data_as(C.POINTER(C.c_double)))
    try:
        om.forward(d)
    finally:
        L.oracle_set_hdump(None)
        L.oracle_set_force_start(0)
    nefc = int(buf[0])
    r = buf[1 + oracle_ffi.MAXV * oracle_ffi.MAXV:][:3 * nefc].reshape(nefc, 3)
    return r[:, 0].copy(), r[:, 2].copy(), d


def _start_costs(om, qpos, qvel, ctrl, warm):
    d = om.new_data(qpos=qpos, qvel=qvel, ctrl=ctrl, warm=warm)
    om.forward(d)
    out = (C.c_double * 2)()
    oracle_ffi.lib().oracle_last_start_costs(out)
    return float(out[0]), float(out[1])


def _zone(jx, band):
    return np.where(jx <= -band, -1, np.where(jx >= band, 1, 0))


def _nlim_active(m, qpos):
    k = 0
    for j in range(m.njnt):
        if m.jnt_limited[j] and m.jnt_type[j] in (JNT_HINGE, JNT_SLIDE):
            q = qpos[m.jnt_qposadr[j]]
            k += min(q - m.jnt_range[j][0], m.jnt_range[j][1] - q) - m.jnt_margin[j] < 0
    return int(k)


def _states(m):
    """fp64 states (qpos, qvel, ctrl) and warm starts of the N envs, and the properties read from the oracle."""
    rng = np.random.default_rng(15)
    om = OracleModel(m)
    nfric = int(np.sum(np.asarray(m.dof_frictionloss[:m.nv]) > 0))
    fdof = [i for i in range(m.nv) if m.dof_frictionloss[i] > 0]
    qpos = np.tile(m.key_qpos[0], (N, 1)).astype(np.float64)
    qvel = np.zeros((N, m.nv))
    ctrl = np.tile(m.key_ctrl[0], (N, 1)).astype(np.float64)
    warm = np.zeros((N, m.nv))
    lims = [j for j in range(1, m.njnt) if m.jnt_limited[j]]
    props = {}
    for e in range(N):
        kind = e % NKIND
        yaw = axis_angle_quat([0, 0, 1], rng.uniform(-3.14, 3.14))
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        qpos[e, 0:2] += rng.uniform(-0.05, 0.05, 2)
        qpos[e, 3:7] = quat_mul(yaw, axis_angle_quat(ax, rng.uniform(-0.05, 0.05)))
        qpos[e, 2] = rng.uniform(0.145, 0.155)
        ctrl[e] += rng.uniform(-0.2, 0.2, m.nu)
        qvel[e] = rng.uniform(-0.1, 0.1, m.nv)
        if kind == 0:
            qpos[e, 2] = 0.5
        if kind == 2:
            # every third friction row inside its quadratic zone at qacc_smooth: J.x - aref = qacc_smooth[i] +
            # b qvel[i] there, linear in qvel[i] up to the dofs' coupling, so a few secant steps on qvel put it
            # near zero; the others far out in the linear zones, one of each sign
            qvel[e, 6:] = np.resize([1.5, -1.5, 0.0], m.nv - 6)
            quad = [k for k in range(nfric) if (fdof[k] - 6) % 3 == 2]
            for _ in range(4):
                j0, _, _ = _rows(om, qpos[e], qvel[e], ctrl[e], warm[e], 2)
                dv = np.zeros(m.nv)
                dv[[fdof[k] for k in quad]] = 0.01
                j1, _, _ = _rows(om, qpos[e], qvel[e] + dv, ctrl[e], warm[e], 2)
                for k in quad:
                    qvel[e, fdof[k]] -= j0[k] * 0.01 / (j1[k] - j0[k])
        if kind == 3:
            jl = lims[(e // NKIND) % len(lims)]
            up = (e // NKIND) % 2 == 0
            qpos[e, m.jnt_qposadr[jl]] = m.jnt_range[jl][1] + 0.03 if up else m.jnt_range[jl][0] - 0.03
            # moving further out the row is active at qacc_smooth, moving back it is not (aref = -b vel - k imp pos)
            back = -1.0 if (e // (2 * NKIND)) % 2 == 0 else 0.5
            qvel[e, m.jnt_dofadr[jl]] = -back if up else back
        if kind == 4:
            qpos[e, 2] = rng.uniform(0.150, 0.154)
        # (the kernel's inputs are fp32: the properties are read at the rounded state)
        q32, v32, c32 = (a[e].astype(np.float32).astype(np.float64) for a in (qpos, qvel, ctrl))
        js, band, d = _rows(om, q32, v32, c32, warm[e], 2)
        qsm = d.arr("qacc_smooth", m.nv).copy()
        if kind == 1:
            warm[e] = d.arr("qacc", m.nv)  # (zero warm start: the smooth start, i.e. a cold start)
        elif kind == 2:
            # J = e_i on a friction row, so J.x - aref moves with qacc_warmstart[i] one for one
            warm[e] = qsm
            zs = _zone(js[:nfric], band[:nfric])
            for k, i in enumerate(fdof):
                want = [zw for zw, z in ZONES if z == zs[k]][(k + e // NKIND) % 2]
                target = (-3.0 * band[k], 0.25 * band[k] * (1 if k % 2 else -1), 3.0 * band[k])[want + 1]
                warm[e, i] += target - js[k]
        elif kind == 3:
            # the limit row's J = sgn e_dof: flip the sign of J.x - aref at the warm start
            warm[e] = qsm
            dof = m.jnt_dofadr[jl]
            sgn = -1.0 if up else 1.0
            assert _nlim_active(m, q32) == 1
            warm[e, dof] += sgn * (-2.0 * js[nfric])  # (the only active limit row follows the friction rows)
        elif kind == 4:
            warm[e] = qsm
            warm[e, 2] += 400.0
        elif kind == 5:
            warm[e] = np.nan
        props[e] = (kind, js, band)
    return qpos, qvel, ctrl, warm, props


def _oracle_steps(m, qpos, qvel, ctrl, warm):
    """NSUB oracle substeps per env: the last substep's qacc and contact distances, the state after it."""
    om = OracleModel(m)
    r = {k: [] for k in ("qacc", "con_dist", "qpos", "qvel")}
    for e in range(len(qpos)):
        d = om.new_data(qpos=qpos[e], qvel=qvel[e], ctrl=ctrl[e], warm=warm[e])
        om.step(d, NSUB)
        r["qacc"].append(d.arr("qacc", m.nv).copy())
        r["con_dist"].append(d.arr("con_dist", 4 * m.npair).copy())
        r["qpos"].append(d.arr("qpos", m.nq).copy())
        r["qvel"].append(d.arr("qvel", m.nv).copy())
    return {k: np.array(v) for k, v in r.items()}


def _case(scene):
    """States, warm starts, properties and oracle results of a scene: computed once (CPU), shared, left unchanged."""
    if scene not in _cache:
        m = _model(scene)
        qpos, qvel, ctrl, warm, props = _states(m)
        r32 = lambda a: a.astype(np.float32).astype(np.float64)
        fin = np.array([e % NKIND != 5 for e in range(N)])
        raw = _oracle_steps(m, qpos[fin], qvel[fin], ctrl[fin], warm[fin])
        q32, v32, c32, w32 = r32(qpos), r32(qvel), r32(ctrl), r32(warm)
        ref = _oracle_steps(m, q32[fin], v32[fin], c32[fin], w32[fin])
        for a in (q32, v32, c32, w32, *ref.values(), *raw.values()):
            a.setflags(write=False)
        _cache[scene] = (m, q32, v32, c32, w32, props, fin, ref, raw)
    return _cache[scene]


@pytest.mark.parametrize("case", list(SCENES))
def test_states_have_their_properties(case):
    """CPU: kinds 1-4 have the property they are built for, read from the oracle's rows at each start, and the
    oracle's result moves by less than the cap of check (a) when its inputs are rounded to fp32."""
    m, qpos, qvel, ctrl, warm, props, fin, ref, raw = _case(SCENES[case])
    om = OracleModel(m)
    nfric = int(np.sum(np.asarray(m.dof_frictionloss[:m.nv]) > 0))
    seen = set()
    for e in range(N):
        kind = e % NKIND
        if kind == 5:
            assert np.isnan(warm[e]).all()
            continue
        cw, cs = _start_costs(om, qpos[e], qvel[e], ctrl[e], warm[e])
        jw, band, _ = _rows(om, qpos[e], qvel[e], ctrl[e], warm[e], 1)
        js, _, d = _rows(om, qpos[e], qvel[e], ctrl[e], warm[e], 2)
        nl = _nlim_active(m, qpos[e])
        if kind == 0:
            assert not warm[e].any() and not cw < cs, (e, cw, cs)
        if kind == 1:
            assert cw < cs, (e, cw, cs)
        if kind in (1, 4):
            assert (d.arr("con_dist", 4 * m.npair) < 0).any(), e
        if kind == 2:
            zw, zs = _zone(jw[:nfric], band[:nfric]), _zone(js[:nfric], band[:nfric])
            assert (zw != zs).all(), (e, zw, zs)
            seen |= set(zip(zw.tolist(), zs.tolist()))
        if kind == 3:
            assert nl == 1 and (jw[nfric] < 0) != (js[nfric] < 0), (e, jw[nfric], js[nfric])
            seen.add(("lim", bool(jw[nfric] < 0)))
        if kind == 4:
            cw_, cs_ = jw[nfric + nl:], js[nfric + nl:]
            assert ((cs_ < 0) & ~(cw_ < 0)).sum() >= 4, (e, cw_, cs_)
            assert case != "flat" or not (cw_ < 0).any(), (e, cw_)
    assert seen >= set(ZONES) | {("lim", True), ("lim", False)}, seen
    amax = np.abs(ref["qacc"]).max(axis=1)
    rel = np.abs(raw["qacc"] - ref["qacc"]).max(axis=1) / (1 + amax)
    print(f"{case}: oracle, fp64 states against their fp32 roundings: qacc rel max {rel.max():.3g}")
    assert (rel < 2e-2).all(), np.sort(rel)[-8:]


def _substeps(scene, gpu, qpos, qvel, ctrl, warm):
    """NSUB physics_kernel substeps in one call through the library Joystick picks: the outputs as float32."""
    env = Joystick(scene, num_envs=1, device=gpu, use_imitation=False)
    T = lambda a: torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float32, device=gpu)
    tq, tv, tw, tc = T(qpos), T(qvel), T(warm), T(ctrl)
    aux = torch.zeros(env.aux_size() * N, dtype=torch.float32, device=gpu).view(-1, N)
    env.physics_step(tq, tv, tw, tc, NSUB, aux)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in (("qpos", tq), ("qvel", tv), ("qacc_warmstart", tw), ("aux", aux))}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SCENES))
def test_two_substeps_match_oracle(case, gpu):
    scene = SCENES[case]
    m, qpos, qvel, ctrl, warm, props, fin, r, _ = _case(scene)
    out = _substeps(scene, gpu, qpos, qvel, ctrl, warm)
    g = parse_aux(m, out["aux"].astype(np.float64))
    gd, gq = g["con_dist"][fin], g["qacc"][fin]
    gw = out["qacc_warmstart"].T.astype(np.float64)[fin]
    act = (r["con_dist"] < 0) | (gd < 0)
    ok = np.all((np.abs(gd - r["con_dist"]) < 1e-5) | ~act, axis=1)
    amax = np.abs(r["qacc"]).max(axis=1)
    rel = np.abs(gq - r["qacc"]).max(axis=1) / (1 + amax)
    relw = np.abs(gw - r["qacc"]).max(axis=1) / (1 + amax)
    kinds = np.arange(N)[fin] % NKIND
    print(f"{case}: manifolds agree {ok.mean():.3f}; qacc rel by kind "
          f"{[float(f'{rel[kinds == k].max():.2g}') for k in range(NKIND - 1)]}, qacc_warmstart rel max {relw.max():.3g}")
    assert np.isfinite(out["aux"][:, fin]).all() and np.isfinite(gw).all()
    assert ok.mean() > 0.98, ok.mean()
    assert (rel[ok] < 2e-2).mean() > 0.97, np.sort(rel)[-8:]
    assert (relw[ok] < 2e-2).mean() > 0.97, np.sort(relw)[-8:]


def _same_words(a, b, cols=None):
    for k in a:
        x, y = a[k].view(np.int32), b[k].view(np.int32)
        assert x.shape == y.shape
        d = x != y
        if cols is not None:
            d = d[:, cols]
        assert not d.any(), (k, int(d.sum()), np.argwhere(d)[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SCENES))
def test_pairs_equal_scalar_twins_word_for_word(case, gpu, monkeypatch):
    scene = SCENES[case]
    path = os.path.join(native.BUILD, "libduck_scalar_twins.so")
    assert os.path.exists(path), "built by __graft_entry__.build()"
    m, qpos, qvel, ctrl, warm, props, fin, _, _ = _case(scene)
    new = _substeps(scene, gpu, qpos, qvel, ctrl, warm)
    # the NaN teams replaced by finite ones (their zero warm start): every other team's words stay
    calm = np.where(fin[:, None], warm, 0.0)
    new_calm = _substeps(scene, gpu, qpos, qvel, ctrl, calm)
    _same_words(new, new_calm, cols=fin)
    assert np.isfinite(new_calm["aux"]).all() and np.isfinite(new["aux"][:, fin]).all()
    monkeypatch.setattr(jmod, "model_library", lambda m: path)
    old = _substeps(scene, gpu, qpos, qvel, ctrl, warm)
    _same_words(new, old, cols=fin)
    _same_words(new_calm, _substeps(scene, gpu, qpos, qvel, ctrl, calm))
    assert np.abs(new["qacc_warmstart"][:, fin]).max() > 1.0  # (the substeps ran: qacc is written back)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["latency", "paired"])
@pytest.mark.parametrize("case", list(SCENES))
def test_step_kernels_agree_on_these_states(case, mode, gpu):
    """The same states, the NaN teams among them, through Joystick.step in the throughput kernel and in a latency
    kernel. A NaN team's own words are not compared (a NaN's payload is no part of the contract, and the env is
    reset by the NaN guard); every finite env's words are, and no cross-wave wait gave up."""
    scene = SCENES[case]
    m, qpos, qvel, ctrl, warm, props, fin, _, _ = _case(scene)
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=gpu)
    outs = {}
    for md in ("throughput", mode):
        env = Joystick(scene, num_envs=N, device=gpu, use_imitation=False)
        env.set_step_mode(md)
        assert env.step_kernel == md
        env.lat_timeouts(reset=True)
        st = env.reset(rng=2)
        st.data.qpos.copy_(T(qpos))
        st.data.qvel.copy_(T(qvel))
        st.data.qacc_warmstart.copy_(T(warm))
        st = env.step(st, T(ctrl - m.key_ctrl[0]) * 0.0, inplace=True)
        torch.cuda.synchronize()
        assert env.lat_timeouts() == 0
        outs[md] = [t.cpu().numpy() for t in (st.fstate, st.istate, st.obs["state"])]

    def finite_envs(x):  # (fstate and istate are flat records of N-env columns; obs is one row per env)
        x = x.reshape(-1, N) if x.ndim == 1 else x
        ax = [i for i, n in enumerate(x.shape) if n == N]
        assert len(ax) == 1, x.shape
        return np.compress(fin, x, axis=ax[0])

    for x, y in zip(outs["throughput"], outs[mode]):
        x, y = finite_envs(x), finite_envs(y)
        d = x.view(np.int32) != y.view(np.int32)
        assert not d.any(), (int(d.sum()), np.argwhere(d)[:8].tolist())
    assert np.isfinite(finite_envs(outs["throughput"][0])).all()
