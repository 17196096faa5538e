"""The step kernels' stage prologues: no word may be read before its last writer.

The throughput kernel issues a stage's table words, per-env model values and older state ahead of the
stage before it (TPhys::step: com_pre, rne_pre, smooth_pre, col_pre, the warm start's and the line search's
rows ahead of their products); the latency and paired kernels load the same words right before the stage,
after their event waits. A word read too early
shows as a difference between the kernels, so every case pins the kernel with set_step_mode (AUTO takes
the latency kernel at these sizes) and compares bit for bit; the fp64 oracle guards the common value.
17 envs: one full workgroup of the throughput kernel and one with a single team.

Seeds: reset 3 and DR 8. Not test_reset_step_parity's reset seed 7: its env 4 is one of the envs that test's
5 % allowance absorbs (this file's runs from seed 7, parent library and this one alike: env 4's obs off by 2.2e-2
of 1 + |obs| at the auto-reset steps of flat_terrain, 9.8e-3 to 3.8e-2 at every step of flat_terrain_backlash,
every other env below 4e-5), and 17 envs leave no allowance (0.95 x 17 > 16). Seed 3 is the smoke run's,
whose recorded lines have all of its first 32 envs within the tolerance.
"""

import numpy as np
import pytest
import torch

from open_duck_playground_amd.joystick import Joystick, domain_randomize, wrap_for_brax_training
from tests import teacher_forcing as tf
from tests.oracle_ffi import OracleBatch, OracleModel
from tests.test_gpu_env import _compare

pytestmark = pytest.mark.gpu

N = 17
SEED = 3
KERNELS = ("throughput", "latency", "paired")


def _fields(st):
    """every tensor of a State, by name"""
    out = {"fstate": st.fstate, "istate": st.istate, "reward": st.reward, "done": st.done}
    for k in ("qpos", "qvel", "qacc_warmstart", "ctrl"):
        out["data." + k] = getattr(st.data, k)
    for group in ("obs", "metrics", "info"):
        for k, v in getattr(st, group).items():
            if torch.is_tensor(v):
                out[f"{group}.{k}"] = v
    return out


def _assert_same_bits(a, b, what):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        x, y = fa[k].contiguous(), fb[k].contiguous()
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (what, k, int((x != y).sum()))


def _make(task, imit, gpu, mode, dr, episode_length):
    env = Joystick(task, num_envs=N, device=gpu, use_imitation=imit)
    if episode_length is not None:
        env = wrap_for_brax_training(env, episode_length=episode_length,
                                     randomization_fn=domain_randomize if dr else None, rng=8)
    elif dr:
        domain_randomize(env, rng=8)
    env.set_step_mode(mode)
    assert env.step_kernel == mode
    env.lat_timeouts(reset=True)
    return env


def _oracle(env, dr):
    base = OracleModel(env.mj_model)
    models = [OracleModel(env.mj_model, dr=base.dr_sample(8, e)) for e in range(N)] if dr else base
    ob = OracleBatch(models, env._cfg_struct, N)
    ob.reset(seed=SEED)
    return ob


def _run(task, imit, gpu, kernels, dr):
    """5 env-steps with 2-step episodes (auto-reset in the run), fresh actions each step; every step is taken by
    each kernel from the throughput kernel's state"""
    envs = {m: _make(task, imit, gpu, m, dr, 2) for m in kernels}
    ref = envs["throughput"]
    st = ref.reset(rng=SEED)
    ob = _oracle(ref, dr)
    L = ref._layout
    good = _compare(ref, st, ob, L)
    rng = np.random.default_rng(0)
    off = None  # the first env-step outside the oracle tolerance (raised after the kernels were compared at every step)
    for t in range(5):
        a = rng.uniform(-1, 1, (N, ref.action_size)).astype(np.float32)
        act = torch.tensor(a, device=gpu)
        outs = {m: envs[m].step(st, act) for m in kernels}
        torch.cuda.synchronize()
        for m in kernels[1:]:
            _assert_same_bits(outs["throughput"], outs[m], (m, t))
        st = outs["throughput"]
        ob.step(a.astype(np.float64))
        try:
            good &= _compare(ref, st, ob, L)
        except AssertionError as e:
            off = off or (t, e)
    assert off is None, off
    assert good.mean() > 0.9
    for m in kernels[1:]:
        assert envs[m].lat_timeouts() == 0


@pytest.mark.parametrize("task,imit", [("flat_terrain", False), ("flat_terrain_backlash", True)])
def test_kernels_agree_over_auto_reset(task, imit, gpu):
    """Throughput, latency and paired kernels: every State field bit for bit over 5 env-steps that contain
    auto-resets; the throughput kernel against the fp64 oracle at test_reset_step_parity's tolerances."""
    _run(task, imit, gpu, KERNELS, dr=False)


def test_per_env_model_values(gpu):
    """The same with domain randomization on flat: the per-env model values (DKP, DARM, DMASS, DFRIC, DQ0,
    DIPOS) differ from env to env, so a prologue that read another env's or a stale value would show."""
    _run("flat_terrain", False, gpu, ("throughput", "latency"), dr=True)


def test_physics_kernel_chain_equals_step_kernel(gpu):
    """One env-step: physics_kernel's chain of single substeps (the out-of-line substep, through the same
    TPhys::step) against step_kernel's state, explain()'s chain_vs_step, which must be 0 for every env."""
    rep = tf.run("flat_terrain", False, N, 1, gpu, keep_states=True, step_mode="throughput")
    res = [tf.explain(rep, 0, e) for e in range(N)]
    d = np.array([r.get("chain_vs_step", np.nan) for r in res])
    print("chain_vs_step per env:", d, [r["kind"] for r in res])
    assert np.all(d == 0.0), d
