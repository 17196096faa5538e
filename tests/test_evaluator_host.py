"""ppo.Evaluator's torch path and the episode/* host reduction, on the CPU with the toy env of test_ppo.py."""

import math

import numpy as np
import torch

from open_duck_playground_amd import ppo
from tests.test_ppo import ToyEnv, small_cfg

TIMES = ("eval/epoch_eval_time", "eval/sps")


class MetricToyEnv(ToyEnv):
    """ToyEnv whose state carries a ``metrics`` dict of two terms (plus a None slot, as the standing env
    has one). Reward and terms are rounded to multiples of 1/64 resp. 1/16, so every sum of them -- over
    steps in fp32, over envs and of squares in fp64 -- is exact in any order and the restatement below can
    ask for equality."""

    def reset(self, rng=0):
        st = super().reset(rng)
        st.metrics = {"reward/near": torch.zeros(self.num_envs), None: torch.zeros(self.num_envs),
                      "cost/far": torch.zeros(self.num_envs)}
        return st

    def step(self, state, action, inplace=True):
        err = (action - state.obs["state"]).abs()
        super().step(state, action, inplace)
        state.reward.copy_(torch.floor(state.reward * 64) / 64)
        state.metrics["reward/near"] = torch.floor((1.0 - err.min(1).values) * 16) / 16
        state.metrics["cost/far"] = -torch.floor(err.max(1).values * 16) / 16
        return state


def _net(cfg, seed=0):
    torch.manual_seed(seed)
    net = ppo.ActorCritic(3, 4, 3, cfg)
    with torch.no_grad():   # termination (|action - target| > 0.9 everywhere) needs actions far from the targets
        net.policy[-1].bias[:3] = torch.tensor([3.0, -3.0, 3.0])
    return net


def test_metric_keys_and_values_match_a_numpy_restatement():
    """Every new key is there and equals a numpy restatement that stops accumulating at the first done.
    (On the parent commit the keys do not exist.)"""
    cfg = small_cfg(episode_length=16)
    env, net = MetricToyEnv(num_envs=64, episode_length=7), _net(cfg)
    out = ppo.evaluate(net, env, cfg, rng=5)
    # the restatement: the same env and policy stepped again, the accumulation in numpy
    ref_env = MetricToyEnv(num_envs=64, episode_length=7)
    st = ref_env.reset(rng=5)
    n = 64
    acc = {k: np.zeros(n, np.float32) for k in ("reward", "reward/near", "cost/far", "length")}
    active = np.ones(n, bool)
    with torch.no_grad():
        for _ in range(16):
            ref_env.step(st, torch.tanh(net.policy_logits(st.obs["state"])[:, :3]))
            for e in range(n):
                if active[e]:
                    acc["reward"][e] += st.reward[e].item()
                    acc["reward/near"][e] += st.metrics["reward/near"][e].item()
                    acc["cost/far"][e] += st.metrics["cost/far"][e].item()
                    acc["length"][e] += 1
                    active[e] = st.done[e].item() == 0
    assert acc["length"].max() == 7 and acc["length"].min() < 7   # truncation and termination both happen

    def ms(x):
        x = x.astype(np.float64)
        mean = x.sum() / n
        return mean, math.sqrt(max(0.0, (x * x).sum() / n - mean * mean))
    want = {"eval/episode_reward": ms(acc["reward"])[0], "eval/avg_episode_length": ms(acc["length"])[0],
            "eval/std_episode_length": ms(acc["length"])[1]}
    for k in ("reward/near", "cost/far"):
        want[f"eval/episode_{k}"], want[f"eval/episode_{k}_std"] = ms(acc[k])
    assert set(out) == set(want) | {"eval/episode_reward_std"} | set(TIMES), sorted(out)
    for k, v in want.items():
        assert out[k] == v, (k, out[k], v)
    # the existing std key stays torch's fp32 std(unbiased=False): its rounding, not the restatement's
    assert abs(out["eval/episode_reward_std"] - ms(acc["reward"])[1]) <= 4 * 2.0 ** -24 * ms(acc["reward"])[1]
    assert want["eval/episode_reward/near_std"] > 0 and want["eval/episode_cost/far"] < 0
    assert out["eval/epoch_eval_time"] > 0 and out["eval/sps"] == 16 * n / out["eval/epoch_eval_time"]


def test_existing_keys_equal_the_previous_loop_bit_for_bit():
    """Plain ToyEnv (no metrics dict): the three keys evaluate() always returned, against its previous loop
    restated verbatim."""
    cfg = small_cfg()
    net = _net(cfg, seed=1)
    out = ppo.evaluate(net, ToyEnv(num_envs=48, episode_length=9), cfg, rng=11)
    eval_env = ToyEnv(num_envs=48, episode_length=9)
    with torch.no_grad():
        state = eval_env.reset(rng=11)
        n = eval_env.num_envs
        ret = torch.zeros(n, device=eval_env.device)
        length = torch.zeros(n, device=eval_env.device)
        active = torch.ones(n, device=eval_env.device)
        for _ in range(cfg.episode_length // cfg.action_repeat):
            act = ppo.NormalTanh(net.policy_logits(state.obs[cfg.policy_obs_key])).mode()
            eval_env.step(state, act, inplace=True)
            ret += state.reward * active
            length += active
            active = active * (1.0 - state.done)
    want = {"eval/episode_reward": float(ret.mean()), "eval/episode_reward_std": float(ret.std(unbiased=False)),
            "eval/avg_episode_length": float(length.mean())}
    for k, v in want.items():
        assert out[k] == v, (k, out[k], v)
    assert set(out) == set(want) | {"eval/std_episode_length"} | set(TIMES)
    assert float(length.min()) < 9 <= float(length.max())


def test_episode_report_from_hand_made_buffers():
    """episode/* from duck_episode_accumulate(TRAIN)'s fin / flag: means over the finished episodes."""
    names = ["reward/a", None, "cost/b"]            # F = 5: reward, three metric slots, steps
    fin = torch.tensor([[2.0, 1.0, 9.0, -4.0, 6.0],   # env 0: two episodes, 6 steps together
                        [0.0, 0.0, 0.0, 0.0, 0.0],    # env 1: none finished
                        [1.0, 0.5, 9.0, -1.0, 3.0]])  # env 2: one episode of 3 steps
    flag = torch.tensor([2.0, 0.0, 1.0])
    out = ppo.episode_report(fin, flag, names)
    assert out == {"episode/sum_reward": 1.0, "episode/length": 3.0, "episode/reward/a": 0.5,
                   "episode/cost/b": -5.0 / 3.0, "episode/count": 3.0}
    out = ppo.episode_report(torch.zeros(3, 5), torch.zeros(3), names)
    assert out == {"episode/sum_reward": 0.0, "episode/length": 0.0, "episode/reward/a": 0.0, "episode/cost/b": 0.0,
                   "episode/count": 0.0}


def test_config_default_keeps_old_checkpoints_loadable():
    cfg = ppo.PPOConfig()
    assert cfg.log_training_metrics is False
    old = {k: v for k, v in ppo.asdict(cfg).items() if k != "log_training_metrics"}
    assert ppo.PPOConfig(**old) == cfg
