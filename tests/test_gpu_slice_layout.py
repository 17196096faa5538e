"""The env slice's LDS layout (csrc/duck_physics.h Lay, duck_team.h TLay) under every step kernel.

The layout's order, padding and per-lane record strides differ per scene (what its LDS affords), and
every step mode adds regions of its own behind the slice. 17 envs: a full 16-env throughput workgroup,
so that team 15's slice is used, plus team 0 of a second, partial one; the latency splits (4 and 8 envs
per workgroup) end on a partial workgroup too. Episodes of 2 steps and three env-steps: an auto-reset
happens on the way.

The throughput kernel is checked against the oracle (the tolerances of test_gpu_env.py::_compare); every
other step mode the scene compiles against the throughput kernel, bit for bit, each env-step taken
from the throughput kernel's state. A wide LDS access off its alignment gives the same bits, only
slower: that is what the SQ_LDS_UNALIGNED_STALL counter is for, not this test.

The GPU tests are marked `gpu`; test_reference_is_well_conditioned runs on the CPU and pins how the reset
seeds were chosen (RESET_SEEDS).
"""

import numpy as np
import pytest
import torch

from open_duck_playground_amd import constants
from open_duck_playground_amd.config import default_config, env_config_struct
from open_duck_playground_amd.joystick import Joystick, domain_randomize, wrap_for_brax_training
from open_duck_playground_amd.mjcf import Model
from tests.oracle_ffi import OracleBatch, OracleModel

N = 17
STEPS = 3
EPISODE = 2
DR_SEED = 11
ACTION_SEED = 5
# The reset seeds. The oracle can judge a kernel only where it is itself well conditioned: a contact that
# switches on under an input change the size of fp32 rounding moves an env's accelerometer reading by
# more than the tolerance in the fp64 oracle too, at a reset's closing forward as in a step
# (tests/teacher_forcing.py calls such an env "sensitive"; test_gpu_teacher_forced.py accepts it). With
# 17 envs the 0.95 share leaves room for no such env, and about one of 70 env rollouts has one, so a case's
# seed is the first of 5, 6, 7, ... at which the oracle alone stays within _compare's tolerances of its
# own unperturbed run in every env when its post-reset qpos and qvel are scaled by 1 + 1e-6 N(0, 1)
# (reference_spread, SPREAD_DRAWS draws): a property of the reference, computed on the CPU without the
# library under test, and checked by test_reference_is_well_conditioned. Seed 5 fails it for
# rough_backlash (env 13: the oracle's own obs row moves by 0.33 in its first env-step).
RESET_SEEDS = {"flat": 5, "flat_backlash": 5, "rough": 5, "rough_backlash": 6}
SPREAD_LEVEL = 1e-6
SPREAD_DRAWS = 8
# task, imitation, domain randomisation, the step modes compiled besides "throughput"
CASES = {
    "flat": ("flat_terrain", True, False, ("latency", "paired", "latency_x2")),
    "flat_backlash": ("flat_terrain_backlash", True, False, ("latency", "paired")),
    "rough": ("rough_terrain", False, True, ("latency", "paired")),
    "rough_backlash": ("rough_terrain_backlash", False, True, ("latency", "paired")),
}
MODE_CASES = [(k, m) for k, c in CASES.items() for m in c[3]]
_rollouts = {}


def _make(case, gpu, mode):
    task, imit, dr, _ = CASES[case]
    env = wrap_for_brax_training(Joystick(task, num_envs=N, device=gpu, use_imitation=imit), episode_length=EPISODE,
                                 randomization_fn=domain_randomize if dr else None, rng=DR_SEED)
    env.set_step_mode(mode)
    assert env.step_kernel == mode
    return env


def _rollout(case, gpu):
    """The throughput kernel's states (reset, then one per env-step) and the actions, once per case."""
    if case not in _rollouts:
        env = _make(case, gpu, "throughput")
        acts = _actions(env.action_size)
        states = [env.reset(rng=RESET_SEEDS[case])]
        for a in acts:
            states.append(env.step(states[-1], torch.tensor(a, device=gpu)))
        torch.cuda.synchronize()
        _rollouts[case] = (env, states, acts)
    return _rollouts[case]


def _actions(nu):
    rng = np.random.default_rng(ACTION_SEED)
    return [rng.uniform(-1, 1, (N, nu)).astype(np.float32) for _ in range(STEPS)]


def _oracle(case, m, seed):
    """The case's OracleBatch after its reset (auto-reset on, episodes of EPISODE steps)."""
    _, imit, dr, _ = CASES[case]
    config = default_config()
    config.episode_length = EPISODE
    cfg = env_config_struct(m, config, imit, True, dr)
    base = OracleModel(m)
    models = [OracleModel(m, dr=base.dr_sample(DR_SEED, e)) for e in range(N)] if dr else base
    ob = OracleBatch(models, cfg, N)
    ob.reset(seed=seed)
    return ob


def reference_spread(case, seed):
    """The oracle against itself: the largest obs / priv error (measured as in _compare) of SPREAD_DRAWS
    rollouts whose post-reset qpos and qvel are scaled by 1 + SPREAD_LEVEL N(0, 1), per env; and, for
    the reset's own rows, the same measure on the sensor values of the forward that ends the reset."""
    m = Model.load(constants.task_to_xml(CASES[case][0]))
    acts = _actions(m.nu)
    ref = _oracle(case, m, seed)
    rows = []
    for a in acts:
        ref.step(a.astype(np.float64))
        rows.append((ref.obs.copy(), ref.priv.copy()))
    rng = np.random.default_rng(seed)
    worst = np.zeros((2, N))
    off = ref.L.off
    F0 = _oracle(case, m, seed).fs.reshape(ref.L.nfloat, N)
    models = ref.models if len(ref.models) > 1 else ref.models * N

    def sensors(e, q, v):
        # the forward that ends the reset (its qacc is the accelerometer of the reset's obs rows)
        d = models[e].new_data(qpos=q, qvel=v, ctrl=F0[off["ctrl"]:off["ctrl"] + m.nu, e], warm=np.zeros(m.nv))
        models[e].forward(d)
        return d.arr("sensordata", m.nsensordata).copy()
    q0, v0 = F0[off["qpos"]:off["qpos"] + m.nq], F0[off["qvel"]:off["qvel"] + m.nv]
    s0 = [sensors(e, q0[:, e], v0[:, e]) for e in range(N)]
    for _ in range(SPREAD_DRAWS):
        ob = _oracle(case, m, seed)
        F = ob.fs.reshape(ob.L.nfloat, N)
        for name, k in (("qpos", m.nq), ("qvel", m.nv)):
            o = ob.L.off[name]
            F[o:o + k] *= 1.0 + SPREAD_LEVEL * rng.standard_normal((k, N))
        for e in range(N):
            s1 = sensors(e, F[off["qpos"]:off["qpos"] + m.nq, e], F[off["qvel"]:off["qvel"] + m.nv, e])
            worst[:, e] = np.maximum(worst[:, e], np.abs(s1 - s0[e]).max() / (1 + np.abs(s0[e]).max()))
        for a, (obs, priv) in zip(acts, rows):
            ob.step(a.astype(np.float64))
            worst[0] = np.maximum(worst[0], np.abs(ob.obs - obs).max(axis=1) / (1 + np.abs(obs).max(axis=1)))
            worst[1] = np.maximum(worst[1], np.abs(ob.priv - priv).max(axis=1) / (1 + np.abs(priv).max(axis=1)))
    return worst


@pytest.mark.parametrize("case", list(CASES))
def test_reference_is_well_conditioned(case):
    """RESET_SEEDS' criterion (above), on the CPU: the oracle's own spread under fp32-sized input changes
    stays within _compare's tolerances (2e-3 obs, 2e-2 priv) in every env at the case's seed, and at no
    smaller seed from 5 on."""
    for seed in range(5, RESET_SEEDS[case] + 1):
        worst = reference_spread(case, seed)
        assert ((worst[0] < 2e-3).all() and (worst[1] < 2e-2).all()) == (seed == RESET_SEEDS[case]), (seed, worst)


def _compare(env, st, ob, L, tol_obs=2e-3, frac=0.95):
    # tests/test_gpu_env.py::_compare, as it stands
    obs = st.obs["state"].cpu().numpy().astype(np.float64)
    priv = st.obs["privileged_state"].cpu().numpy().astype(np.float64)
    err = np.abs(obs - ob.obs).max(axis=1) / (1 + np.abs(ob.obs).max(axis=1))
    errp = np.abs(priv - ob.priv).max(axis=1) / (1 + np.abs(ob.priv).max(axis=1))
    good = (err < tol_obs) & (errp < tol_obs * 10)
    assert good.mean() >= frac, (good.mean(), np.sort(err)[-5:], np.sort(errp)[-5:])
    rew = st.reward.cpu().numpy()
    assert np.allclose(rew[good], ob.rew[good], rtol=1e-3, atol=1e-3)
    assert np.array_equal(st.done.cpu().numpy()[good], ob.done[good])
    ist = st.istate.view(L.nint, -1).cpu().numpy()
    oist = ob.is_.reshape(L.nint, -1)
    for name in ("rng_key", "rng_ctr", "push_step", "push_interval"):
        k = L.ioff[name]
        assert np.array_equal(ist[k][good], oist[k][good]), name
    return good


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_throughput_kernel_matches_oracle(case, gpu):
    """Reset and every env-step within _compare's tolerances in at least 0.95 of the 17 envs, i.e. in all."""
    env, states, acts = _rollout(case, gpu)
    ob = _oracle(case, env.mj_model, RESET_SEEDS[case])
    L = env._layout
    _compare(env, states[0], ob, L)
    resets = 0
    for a, st in zip(acts, states[1:]):
        ob.step(a.astype(np.float64))
        _compare(env, st, ob, L)
        resets += int(st.done.sum().item())
    assert resets >= N  # every env ran into its episode's end at least once


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode", MODE_CASES)
def test_step_modes_match_throughput_kernel(case, mode, gpu):
    _, states, acts = _rollout(case, gpu)
    env = _make(case, gpu, mode)
    env.lat_timeouts(reset=True)
    env.reset(rng=RESET_SEEDS[case])
    for t, a in enumerate(acts):
        s = env.step(states[t], torch.tensor(a, device=gpu))
        torch.cuda.synchronize()
        ref = states[t + 1]
        assert torch.equal(s.istate, ref.istate) and torch.equal(s.done, ref.done), t
        for name, x, y in (("fstate", s.fstate, ref.fstate), ("obs", s.obs["state"], ref.obs["state"]),
                           ("priv", s.obs["privileged_state"], ref.obs["privileged_state"]),
                           ("reward", s.reward, ref.reward)):
            assert torch.equal(x, y), (t, name, (x != y).sum().item())
    assert env.lat_timeouts() == 0
