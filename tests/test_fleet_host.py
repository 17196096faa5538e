"""Host side of the fleet deployment loop (sim2sim.FleetInfer): the ONNX -> dense-policy import
(onnx_infer.dense_policy), the two C-ABI symbols, the model descriptor, and the float32 restatements
(tests/fleet_reference.py) the GPU tests compare the kernels against. No GPU."""

import os
import re

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, onnx_export, ppo
from open_duck_playground_amd.onnx_export import _bytes, _int, _key, _str, node, tensor, value_info
from open_duck_playground_amd.onnx_infer import OnnxGraph, dense_policy
from tests import fleet_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    torch.manual_seed(5)
    net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
    rng = np.random.default_rng(1)
    net.obs_norm.update(torch.tensor(rng.normal(0.3, 2.0, size=(400, 101)), dtype=torch.float32))
    path = str(tmp_path_factory.mktemp("onnx") / "policy.onnx")
    blob = onnx_export.export_onnx(net, 14, 101, output_path=path)
    return net, blob


def test_round_trip_is_exact(exported):
    net, blob = exported
    g = OnnxGraph(blob)
    pol = dense_policy(g)
    lin = [m for m in net.policy if isinstance(m, torch.nn.Linear)]
    assert pol["sizes"] == [101] + [m.out_features for m in lin[:-1]] + [28] and pol["action_size"] == 14
    for k, m in enumerate(lin):
        w, b = m.weight.detach().numpy(), m.bias.detach().numpy()
        if k == len(lin) - 1:   # the file holds the loc half; the scale half is padded with zeros
            assert pol["W"][k].shape == (28, w.shape[1]) and pol["b"][k].shape == (28,)
            assert not pol["W"][k][14:].any() and not pol["b"][k][14:].any()
            w, b = w[:14], b[:14]
            got_w, got_b = pol["W"][k][:14], pol["b"][k][:14]
        else:
            got_w, got_b = pol["W"][k], pol["b"][k]
        assert got_w.dtype == f32 and got_w.flags.c_contiguous
        assert got_w.tobytes() == np.ascontiguousarray(w, f32).tobytes()        # nn.Linear layout [out, in]
        assert got_w.tobytes() == np.ascontiguousarray(g.init[f"hidden_{k}/kernel"].T).tobytes()
        assert got_b.tobytes() == b.astype(f32).tobytes()
    assert pol["mean"].tobytes() == g.init["mean"].tobytes()
    std = g.init["std"]
    assert pol["istd"].dtype == f32 and pol["istd"].tobytes() == (1.0 / std.astype(np.float64)).astype(f32).tobytes()


def _numpy_policy(pol, x):
    h = ((x - pol["mean"]) * pol["istd"]).astype(f32) if pol["mean"] is not None else x
    for k, (w, b) in enumerate(zip(pol["W"], pol["b"])):
        h = (h @ w.T + b).astype(f32)
        if k < len(pol["W"]) - 1:
            h = (h * (1.0 / (1.0 + np.exp(-h)))).astype(f32)
    return np.tanh(h[:, :pol["action_size"]])


def test_layers_agree_with_the_runtime(exported):
    _, blob = exported
    g = OnnxGraph(blob)
    pol = dense_policy(g)
    x = np.random.default_rng(2).normal(0.3, 2.0, size=(64, 101)).astype(f32)
    ref = g.run({"obs": x})[0]
    got = _numpy_policy(pol, x)
    print("dense layers vs OnnxGraph.run: max abs diff %.3e" % np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= 1e-6


# --- hand-built graphs ------------------------------------------------------------------
def _attr_int(name, v):
    return _str(1, name) + _int(3, v) + _int(20, 2)


def _attr_float(name, v):
    return _str(1, name) + _key(2, 5) + np.float32(v).tobytes() + _int(20, 1)


def _node(op, ins, outs, attrs=()):
    return node(op, ins, outs, outs[0] + "_node") + b"".join(_bytes(5, a) for a in attrs)


def _model(nodes, inits, out="y", n_in=5, n_out=3):
    graph = (b"".join(_bytes(1, n) for n in nodes) + _str(2, "g") + b"".join(_bytes(5, tensor(k, v)) for k, v in inits)
             + _bytes(11, value_info("obs", [1, n_in])) + _bytes(12, value_info(out, [1, n_out])))
    return _int(1, 6) + _bytes(7, graph) + _bytes(8, _str(1, "") + _int(2, 11))


def _weights():
    rng = np.random.default_rng(3)
    return {"mean": rng.normal(size=5).astype(f32), "std": rng.uniform(0.5, 2, 5).astype(f32),
            "w0": rng.normal(size=(5, 8)).astype(f32), "b0": rng.normal(size=8).astype(f32),
            "w1": rng.normal(size=(8, 3)).astype(f32), "b1": rng.normal(size=3).astype(f32)}


def _gemm_graph(w, relu=False, tanh=True, alpha=None, fan_out=False, trans_b=False, matmul=False):
    inits = dict(w)
    nodes = [_node("Sub", ["obs", "mean"], ["c"]), _node("Div", ["c", "std"], ["h"])]
    if trans_b:
        inits["w0"], inits["w1"] = np.ascontiguousarray(w["w0"].T), np.ascontiguousarray(w["w1"].T)
    attrs = ([_attr_int("transB", 1)] if trans_b else []) + ([_attr_float("alpha", alpha)] if alpha is not None else [])
    if matmul:
        nodes += [_node("MatMul", ["h", "w0"], ["m0"]), _node("Add", ["m0", "b0"], ["z0"])]
    else:
        nodes.append(_node("Gemm", ["h", "w0", "b0"], ["z0"], attrs))
    if relu:
        nodes.append(_node("Relu", ["z0"], ["a0"]))
    else:
        nodes += [_node("Sigmoid", ["z0"], ["s0"]), _node("Mul", ["z0", "s0"], ["a0"])]
    if matmul:
        nodes += [_node("MatMul", ["a0", "w1"], ["m1"]), _node("Add", ["b1", "m1"], ["z1"])]   # bias first: Add commutes
    else:
        nodes.append(_node("Gemm", ["a0", "w1", "b1"], ["z1"], [_attr_int("transB", 1)] if trans_b else []))
    if fan_out:   # the hidden activation feeds a second consumer
        nodes.append(_node("Mul", ["a0", "a0"], ["side"]))
    out = "z1"
    if tanh:
        nodes.append(_node("Tanh", ["z1"], ["y"]))
        out = "y"
    return OnnxGraph(_model(nodes, list(inits.items()), out=out))


def test_equivalent_graphs_import_to_the_same_layers():
    w = _weights()
    base = dense_policy(_gemm_graph(w))
    assert base["sizes"] == [5, 8, 6]
    assert base["W"][0].tobytes() == np.ascontiguousarray(w["w0"].T).tobytes()
    x = np.random.default_rng(4).normal(size=(7, 5)).astype(f32)
    for kw in (dict(matmul=True), dict(trans_b=True)):
        g = _gemm_graph(w, **kw)
        pol = dense_policy(g)
        assert pol["sizes"] == base["sizes"]
        for key in ("W", "b"):
            for a, b in zip(pol[key], base[key]):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (kw, key)
        assert pol["mean"].tobytes() == base["mean"].tobytes() and pol["istd"].tobytes() == base["istd"].tobytes()
        np.testing.assert_allclose(_numpy_policy(pol, x), g.run({"obs": x})[0], atol=2e-6)   # the runtime reads it alike


@pytest.mark.parametrize("kw,names", [(dict(relu=True), "Relu"), (dict(tanh=False), "z1"), (dict(alpha=2.0), "z0"),
                                      (dict(fan_out=True), "a0")])
def test_other_graphs_are_rejected_by_name(kw, names):
    with pytest.raises(ValueError, match=names):
        dense_policy(_gemm_graph(_weights(), **kw))


@pytest.mark.parametrize("widths", [(101, 8, 8, 8, 8, 14), (101, 520, 14)])
def test_fleet_refuses_a_policy_outside_the_kernel_limits(tmp_path, widths):
    """More than 4 layers or wider than 512: DuckError before anything touches the device, no host fallback."""
    from open_duck_playground_amd.sim2sim import FleetInfer
    rng = np.random.default_rng(6)
    layers = [(rng.normal(size=(a, b)).astype(f32), np.zeros(b, f32)) for a, b in zip(widths, widths[1:])]
    path = str(tmp_path / "policy.onnx")
    with open(path, "wb") as f:
        f.write(onnx_export.policy_graph(layers, np.zeros(101, f32), np.ones(101, f32), 101, 14))
    assert dense_policy(OnnxGraph(open(path, "rb").read()))["sizes"] == list(widths[:-1]) + [28]
    with pytest.raises(native.DuckError, match="duck_policy_act's limits"):
        FleetInfer("flat_terrain", path, 4, device="cuda:0")


# --- the C ABI --------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_check_their_arguments():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "duck_fleet.h")).read()
    for sym in ("duck_fleet_observe", "duck_fleet_actuate"):
        assert re.search(r"^int %s\(" % sym, hdr, flags=re.M), sym
        assert sym in native.EXPORTS
    L = native.lib()
    d = native.DuckFleetDesc()
    one = C.c_void_p(16)   # (never dereferenced: the calls below are refused before any launch)
    assert L.duck_fleet_observe(None, 1, one, one, one, one, one, one, one, None) == -1
    assert L.duck_fleet_actuate(C.byref(d), 1, one, None, one, None) == -1 and b"null pointer" in L.duck_last_error()
    assert L.duck_fleet_actuate(C.byref(d), 1, one, one, one, None) == -1 and b"nu" in L.duck_last_error()   # nu = 0
    d.nq, d.nv, d.nu, d.naux = 21, 20, 14, 40
    assert L.duck_fleet_actuate(C.byref(d), -1, one, one, one, None) == -1 and b"bad size" in L.duck_last_error()
    d.sens_off, d.gyro = 38, 0      # gyro's three rows end past the record
    assert L.duck_fleet_observe(C.byref(d), 1, one, one, one, one, one, one, one, None) == -1
    assert b"outside the aux record" in L.duck_last_error()
    d.nu = 17
    assert L.duck_fleet_actuate(C.byref(d), 1, one, one, one, None) == -1
    d.nu = 14
    assert L.duck_fleet_actuate(C.byref(d), 0, one, one, one, None) == 0      # an empty fleet launches nothing


def test_descriptor_comes_from_the_model():
    from open_duck_playground_amd import constants
    from open_duck_playground_amd.mjcf import Model
    from open_duck_playground_amd.sim2sim import ctl_fields, fleet_desc
    m = Model.load(constants.task_to_xml("flat_terrain_backlash"))
    naux = 4 * m.nv + m.nu + m.nsensordata + 7 * 4 * m.npair + 999
    d = R.desc_values(fleet_desc(m, naux, 40, standing=False))
    assert (d.nq, d.nv, d.nu) == (m.nq, m.nv, m.nu) and d.sens_off == 4 * m.nv + m.nu
    assert d.con_off == d.sens_off + m.nsensordata
    names = m.names["sensor"]
    assert d.gyro == m.sensor_adr[names.index("gyro")] and d.upvector == m.sensor_adr[names.index("upvector")]
    assert d.act_qpos[:m.nu] == [int(m.jnt_qposadr[j]) for j in m.actuator_trnid]
    assert d.act_dof[:m.nu] != d.act_qpos[:m.nu]
    assert d.target_step == f32(5.24 * 0.002 * 10) and d.dof_vel_scale == f32(0.05) and d.accel_x_offset == f32(1.3)
    assert all(0 <= s <= 4 * m.npair - 4 and s % 4 == 0 for s in d.foot_con) and d.foot_con[0] != d.foot_con[1]
    assert ctl_fields(m.nu) == R.ctl_fields(m.nu)


@pytest.mark.parametrize("nu", [1, 3, 14, 16])
def test_offset_macros_are_the_control_record(nu):
    """The header's offset macros against the tests' own statement of the record, field by field; the fields
    tile [0, DUCK_FLEET_CTL_SIZE(nu)); sim2sim.ctl_fields is the same mapping."""
    from open_duck_playground_amd.cabi import HEADERS
    from open_duck_playground_amd.sim2sim import ctl_fields
    macros = {"last_action": f"ACTION({nu}, 0)", "last_last_action": f"ACTION({nu}, 1)",
              "last_last_last_action": f"ACTION({nu}, 2)", "motor_targets": f"MOTOR_TARGETS({nu})",
              "prev_motor_targets": f"PREV_MOTOR_TARGETS({nu})", "command": f"COMMAND({nu})",
              "imitation_i": f"IMITATION_I({nu})", "phase_frequency_factor": f"PHASE_FREQUENCY_FACTOR({nu})",
              "imitation_phase": f"IMITATION_PHASE({nu})"}
    want = R.ctl_fields(nu)
    assert set(macros) == set(want)
    for name, (first, _) in want.items():
        assert HEADERS.value("DUCK_FLEET_CTL_" + macros[name]) == first, name
    end = 0
    for first, width in sorted(want.values()):      # no gap, no overlap
        assert first == end and width >= 1
        end = first + width
    assert end == HEADERS.value(f"DUCK_FLEET_CTL_SIZE({nu})") == R.ctl_size(nu)
    assert ctl_fields(nu) == want


# --- the restatements on hand-written rows ----------------------------------------------
def _blank(d, n):
    C = R.ctl_size(d.nu)
    z = lambda k: np.zeros((k, n), f32)  # noqa: E731
    ctl = np.zeros((n, C), f32)
    ctl[:, R.ctl_fields(d.nu)["phase_frequency_factor"][0]] = 1.0
    return z(d.nq), z(d.nv), z(d.naux), ctl


def test_reference_clip_on_both_sides():
    d = R.make_desc(nu=3)
    _, _, _, ctl = _blank(d, 1)
    F = R.ctl_fields(3)
    default = np.asarray(d.act_default[:3], f32)
    ctl[0, F["prev_motor_targets"][0]:][:3] = default
    ctl[0, F["last_action"][0]:][:3] = [7, 8, 9]
    ctl[0, F["last_last_action"][0]:][:3] = [4, 5, 6]
    action = np.array([[1.0, -1.0, 0.1]], f32)       # 0.25, -0.25, 0.025 from default: step is 0.1048
    ctrl = R.actuate(d, action, ctl)
    step = f32(5.24 * 0.002 * 10)
    want = np.array([default[0] + step, default[1] - step, default[2] + f32(0.1) * f32(0.25)], f32)
    assert ctrl.shape == (3, 1) and ctrl[:, 0].tobytes() == want.tobytes()
    assert ctl[0, F["motor_targets"][0]:][:3].tobytes() == want.tobytes()
    assert ctl[0, F["prev_motor_targets"][0]:][:3].tobytes() == want.tobytes()
    assert list(ctl[0, :9]) == [1.0, -1.0, f32(0.1), 7, 8, 9, 4, 5, 6]
    d.speed_limits = 0
    ctl[0, F["prev_motor_targets"][0]:][:3] = default
    ctrl = R.actuate(d, action, ctl)
    assert ctrl[:, 0].tobytes() == (default + action[0] * f32(0.25)).astype(f32).tobytes()
    assert ctl[0, F["prev_motor_targets"][0]:][:3].tobytes() == default.tobytes()    # untouched without the limit


def test_reference_contacts():
    d = R.make_desc(nu=3)
    qpos, qvel, aux, ctl = _blank(d, 4)
    left, right = d.con_off + d.foot_con[0], d.con_off + d.foot_con[1]
    aux[left:left + 4] = 1.0
    aux[right:right + 4] = 1.0
    aux[left + 2, 0] = -1e-9       # robot 0: left foot touches
    aux[right + 3, 1] = 0.0        # robot 1: a zero distance is no contact
    aux[left, 2] = -0.0            # robot 2: nor is -0
    aux[right, 3] = np.nan         # robot 3: nor is NaN
    aux[left + 1, 3] = np.nan
    np.testing.assert_array_equal(R.contacts(d, aux), [[1, 0], [0, 0], [0, 0], [0, 0]])
    obs, _ = R.observe(d, qpos, qvel, aux, ctl, torch.zeros(4, 6), torch.ones(4))
    O = R.obs_size(d.nu)
    np.testing.assert_array_equal(obs[:, O - 4:O - 2], [[1, 0], [0, 0], [0, 0], [0, 0]])


def test_reference_phase_wraps_and_bookkeeping_stops():
    d = R.make_desc(nu=3, nb=40)
    qpos, qvel, aux, ctl = _blank(d, 3)
    F = R.ctl_fields(3)
    ii, fac = F["imitation_i"][0], F["phase_frequency_factor"][0]
    ctl[:, ii] = [39.0, 39.5, 0.0]
    ctl[:, fac] = [1.0, 1.0, 1.5]
    aux[d.sens_off + d.upvector + 2] = [1.0, -0.5, 1.0]       # robot 1 is upside down
    aux[d.sens_off + d.local_linvel] = 0.25
    acc, alive = torch.zeros(3, 6), torch.ones(3)
    obs, ph64 = R.observe(d, qpos, qvel, aux, ctl, acc, alive)
    assert list(ctl[:, ii]) == [0.0, 0.5, 1.5]                # wrapped at nb
    np.testing.assert_allclose(ph64[0], [1.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(ph64[2], [np.cos(1.5 / 40 * 2 * np.pi), np.sin(1.5 / 40 * 2 * np.pi)], atol=2e-7)
    assert obs[:, -2:].tobytes() == ctl[:, F["imitation_phase"][0]:][:, :2].tobytes()
    assert list(alive) == [1, 0, 1] and list(acc[:, 0]) == [1, 0, 1] and float(acc[0, 4]) == 0.0625
    qvel[5, 2] = np.nan
    R.observe(d, qpos, qvel, aux, ctl, acc, alive)
    assert list(alive) == [1, 0, 0] and list(acc[:, 0]) == [2, 0, 1]
    d.standing = 1
    before = ctl.copy()
    R.observe(d, qpos, qvel, aux, ctl, acc, alive)
    assert ctl.tobytes() == before.tobytes()
