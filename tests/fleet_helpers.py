"""What the fleet tests share (tests/test_gpu_fleet*.py, tests/test_fleet_*_host.py): bit views, the C structs
filled from plain values, device buffers with guard rows, random commands and the exported test policy. The
sizes and offsets of the records are tests/fleet_reference.py's. Test infrastructure only."""

import ctypes as C

import numpy as np
import pytest
import torch

from open_duck_playground_amd import native, onnx_export, ppo

f32 = np.float32


def bits(a):
    """The int32 view of a float32 array; any other dtype as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def f32_bits(a):
    """The int32 view of ``a`` as float32."""
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.int32)


def c_desc(d):
    """A duck_fleet_desc filled from the attributes of ``d`` (tests/fleet_reference.make_desc)."""
    out = native.DuckFleetDesc()
    for name, _ in out._fields_:
        v = getattr(d, name)
        if isinstance(v, list):
            for k, x in enumerate(v):
                getattr(out, name)[k] = x
        else:
            setattr(out, name, v)
    return out


def host_desc():
    """A valid duck_fleet_desc of the duck's sizes, for the entries' refusals (no launch reads it)."""
    d = native.DuckFleetDesc()
    d.nq, d.nv, d.nu, d.naux = 21, 20, 14, 200
    for a in range(14):
        d.act_qpos[a], d.act_dof[a] = 7 + a, 6 + a
    return d


def c_dis(seed, scale, sched=None, seg_periods=1):
    s = native.DuckFleetDisturbance()
    s.seed = seed
    for k, v in enumerate(scale):
        s.noise_scale[k] = float(v)
    if sched is not None:
        s.n_sched, s.n_seg, s.seg_periods = sched.shape[0], sched.shape[1], seg_periods
    return s


def dev(a, gpu):
    return torch.tensor(np.ascontiguousarray(a), device=gpu)


def stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(torch.device(gpu)).cuda_stream)


def guarded(a, gpu):
    """``a`` on the device with a guard row before and after it: (the whole tensor, the view of ``a``)."""
    g = np.full((1,) + a.shape[1:], 7, a.dtype)
    t = torch.tensor(np.concatenate([g, a, g]), device=gpu)
    return t, t[1:-1]


def guards_hold(t):
    t = t.cpu().numpy()
    return bool((t[0] == 7).all() and (t[-1] == 7).all())


def commands(n, seed=11):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 7), f32)
    c[:, 0], c[:, 1], c[:, 2] = rng.uniform(-0.15, 0.15, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-1, 1, n)
    return c


def _export_policy(tmp_path_factory):
    torch.manual_seed(3)
    net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
    rng = np.random.default_rng(0)
    net.obs_norm.update(torch.tensor(rng.normal(0.0, 1.0, size=(500, 101)), dtype=torch.float32))
    path = str(tmp_path_factory.mktemp("onnx") / "policy.onnx")
    onnx_export.export_onnx(net, 14, 101, output_path=path)
    return net, path


# A test module imports one of the two by name; pytest then sets it up once per importing module, each in a
# directory of its own.
@pytest.fixture(scope="module")
def policy_file(tmp_path_factory):
    """The seeded, untrained test policy exported to ONNX: its path."""
    return _export_policy(tmp_path_factory)[1]


@pytest.fixture(scope="module", name="policy_file")
def net_and_policy_file(tmp_path_factory):
    """``policy_file`` as (the network, the path)."""
    return _export_policy(tmp_path_factory)
