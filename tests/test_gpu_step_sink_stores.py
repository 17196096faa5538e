"""The substep's unguarded stores: lane-guarded words through the sink, a team-uniform value from every lane.

The step kernels run the last slice of rne's FSM pass and of Euler's QVEL / WARM pass, smooth's actuator block and
the sensors' foot-contact flags on every lane and send the stores of the lanes past the end through
`ok ? addr : TLay::SINK + lane`; the free joint's integration runs on every lane of the team and every lane
stores the (same) result. No exec-masked region stands around those stores. What could go wrong: a sink slot
outside the team's own slice (the teams of a workgroup that hold no env run the same stores), a lane past the end
reading or writing a word that another lane owns, a value that is not the same on every lane after all, a store
that another wave of a latency-mode workgroup does not expect. Each shows as a difference between the kernels
or against the fp64 oracle.

17 envs: one full throughput workgroup and one that holds a single team, and partial workgroups of the
latency kernels. Seeds 3 (reset) and 8 (DR), 2-step episodes, as tests/test_gpu_step_prefetch.py, whose
helpers run the cases: every State field bit for bit between the kernels at every step, the throughput
kernel against the fp64 oracle at test_reset_step_parity's tolerances, no latency-mode wait timed out.
"""

import numpy as np
import pytest
import torch

from tests.test_gpu_env import _compare
from tests.test_gpu_step_prefetch import SEED, _make, _run

pytestmark = pytest.mark.gpu


def test_flat_every_kernel(gpu):
    """flat_terrain: throughput against latency, paired and latency_x2."""
    _run("flat_terrain", False, gpu, ("throughput", "latency", "paired", "latency_x2"), dr=False)


def test_flat_backlash_imitation(gpu):
    """flat_terrain_backlash with imitation: throughput against latency and paired."""
    _run("flat_terrain_backlash", True, gpu, ("throughput", "latency", "paired"), dr=False)


def test_rough_backlash_domain_randomized(gpu):
    """rough_terrain_backlash with DR: the slice with the fewest spare words behind the sink, and per-env
    model values that differ from env to env."""
    _run("rough_terrain_backlash", False, gpu, ("throughput", "latency", "paired"), dr=True)


def test_one_env_flat_throughput(gpu):
    """1 env on flat, throughput kernel: 15 of the workgroup's 16 teams hold no env and store into their own
    slices; the one env against the fp64 oracle over 5 env-steps with 2-step episodes."""
    from tests.oracle_ffi import OracleBatch, OracleModel
    from open_duck_playground_amd.joystick import Joystick, wrap_for_brax_training

    env = wrap_for_brax_training(Joystick("flat_terrain", num_envs=1, device=gpu, use_imitation=False),
                                 episode_length=2, randomization_fn=None, rng=8)
    env.set_step_mode("throughput")
    assert env.step_kernel == "throughput"
    st = env.reset(rng=SEED)
    ob = OracleBatch(OracleModel(env.mj_model), env._cfg_struct, 1)
    ob.reset(seed=SEED)
    good = _compare(env, st, ob, env._layout)
    rng = np.random.default_rng(0)
    for _ in range(5):
        a = rng.uniform(-1, 1, (1, env.action_size)).astype(np.float32)
        st = env.step(st, torch.tensor(a, device=gpu))
        ob.step(a.astype(np.float64))
        good &= _compare(env, st, ob, env._layout)
    torch.cuda.synchronize()
    assert good.all()
