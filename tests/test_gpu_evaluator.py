"""The evaluator on the device (DESIGN.md §8 "Evaluator"): duck_policy_act against the rollout's duck_mlp_gemm
chain bit for bit, its tanh against fp64, duck_episode_accumulate against a sequential torch restatement, and
ppo.Evaluator / the training-side episode metrics on the HIP env. Outputs of the kernels live in the NaN arena
of test_gpu_mlp_kernels.py (guards checked on fetch)."""

import ctypes as C

import pytest
import torch

from open_duck_playground_amd import ppo
from open_duck_playground_amd.cabi import METRIC_NAMES, STANDING_METRIC_NAMES
from tests.test_gpu_mlp_kernels import TINY, U24, Arena, dev

pytestmark = pytest.mark.gpu

EINVAL = -1
TIMES = ("eval/epoch_eval_time", "eval/sps")
# action = tanhf(loc) against the fp64 tanh of the kernel's own fp32 loc, in units of 2^-24 max(|value|, TINY),
# over loc = linspace(-10, 10, 4001) (test_action_is_tanh_of_loc). Measured on the MI355X: see that test's
# docstring; asserted: 4 x the measured maximum, rounded up to a power of two.
#   tanh                 measured 1.403 units  -> 8
TANH_UNITS = 8.0


def _lib():
    from open_duck_playground_amd.native import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def policy_act(N, sizes, W, b, mean, istd, obs, logits, action, nlayers=None):
    nl = len(sizes) - 1 if nlayers is None else nlayers
    return _lib().duck_policy_act(N, nl, (C.c_int * len(sizes))(*sizes), (C.c_void_p * len(W))(*[_ptr(w) for w in W]),
                                  (C.c_void_p * len(b))(*[_ptr(x) for x in b]), _ptr(mean), _ptr(istd), _ptr(obs),
                                  _ptr(logits), _ptr(action), _stream())


def gemm_chain(N, sizes, W, b, mean, istd, obs, gpu):
    """_Rollout._policy: duck_mlp_gemm mode 1 per hidden layer, then mode 0."""
    from open_duck_playground_amd.native import check
    L, inp, nl = _lib(), obs, len(sizes) - 1
    for i in range(nl):
        last = i == nl - 1
        y = torch.empty(N, sizes[i + 1], device=gpu)
        y2 = None if last else torch.empty(N, sizes[i + 1], device=gpu)
        check(L.duck_mlp_gemm(0 if last else 1, N, sizes[i], sizes[i + 1], inp.data_ptr(), W[i].data_ptr(), b[i].data_ptr(),
                              None, y.data_ptr(), _ptr(y2), _ptr(mean) if i == 0 else None,
                              _ptr(istd) if i == 0 else None, _stream()))
        inp = y2
    return y


NETS = [(101, 512, 256, 128, 28), (5, 33, 17, 6), (36, 64, 12)]
ROWS = [1, 15, 16, 17, 33, 130]


@pytest.mark.parametrize("sizes", NETS, ids=lambda s: "-".join(map(str, s)))
def test_policy_act_logits_equal_the_gemm_chain(gpu, sizes):
    """logits of duck_policy_act == the duck_mlp_gemm chain, as int32: N below, at and above the 16-row tile and
    over several workgroups, with and without the normaliser, widths off every tile multiple (5, 33, 17, 101),
    the 101-wide obs also based one float off 16-byte alignment; logits = NULL still writes the same action."""
    g = torch.Generator().manual_seed(sum(sizes))
    nl = len(sizes) - 1
    Wh = [torch.randn(sizes[i + 1], sizes[i], generator=g) / sizes[i] ** 0.5 for i in range(nl)]
    bh = [0.3 * torch.randn(sizes[i + 1], generator=g) for i in range(nl)]
    W, b = [dev(x, gpu) for x in Wh], [dev(x, gpu) for x in bh]
    mean, istd = dev(torch.randn(sizes[0], generator=g), gpu), dev(torch.rand(sizes[0], generator=g) + 0.5, gpu)
    A = sizes[-1] // 2
    for N in ROWS:
        obs_h = 2.0 * torch.randn(N, sizes[0], generator=g)
        for off in ([0, 1] if sizes[0] == 101 else [0]):
            obs = dev(obs_h, gpu, off)
            for norm in (False, True):
                mn, sd = (mean, istd) if norm else (None, None)
                want = gemm_chain(N, sizes, W, b, mn, sd, obs, gpu)
                arena = Arena()
                lg, ac, ac2 = arena.take(N, sizes[-1]), arena.take(N, A), arena.take(N, A)
                arena.alloc(gpu)
                assert policy_act(N, sizes, W, b, mn, sd, obs, arena.ptr(lg), arena.ptr(ac)) == 0
                assert policy_act(N, sizes, W, b, mn, sd, obs, None, arena.ptr(ac2)) == 0
                out = arena.fetch()
                where = f"sizes {sizes} N {N} off {off} norm {norm}"
                assert bool(torch.isfinite(out[lg]).all()), where
                assert torch.equal(out[lg].view(torch.int32), want.cpu().view(torch.int32)), where
                assert torch.equal(out[ac].view(torch.int32), out[ac2].view(torch.int32)), where
                assert bool((out[ac].double() - torch.tanh(out[lg][:, :A].double())).abs().max() < 1e-5), where


def test_policy_act_refuses_bad_shapes(gpu):
    z = torch.zeros(600, device=gpu)
    ok = [z] * 5
    for sizes in [(0, 4), (4, 0, 2), (513, 4), (4, 513, 2), (4, 3), (4, 8, 5)]:
        assert policy_act(4, sizes, ok, ok, None, None, z, z, z) == EINVAL, sizes
    assert policy_act(4, (4, 4, 4, 4, 4, 4), ok, ok, None, None, z, z, z, nlayers=5) == EINVAL
    assert policy_act(4, (4, 4), ok, ok, None, None, z, z, z, nlayers=0) == EINVAL
    assert policy_act(4, (4, 4), ok, ok, z, None, z, z, z) == EINVAL   # a mean without istd
    assert policy_act(4, (4, 4), ok, ok, None, None, z, z, None) == EINVAL
    torch.cuda.synchronize()


def test_action_is_tanh_of_loc(gpu):
    """action against the fp64 tanh of the kernel's own fp32 loc on loc = linspace(-10, 10, 4001): a one-layer
    network 1 -> 2 with W = [[1], [0]], b = 0 makes loc = obs exactly (asserted).
    Measured on the MI355X: 1.403 units (asserted 8: TANH_UNITS above)."""
    loc = torch.linspace(-10, 10, 4001)
    N = loc.numel()
    W, b, obs = dev(torch.tensor([[1.0], [0.0]]), gpu), dev(torch.zeros(2), gpu), dev(loc.view(N, 1), gpu)
    arena = Arena()
    lg, ac = arena.take(N, 2), arena.take(N, 1)
    arena.alloc(gpu)
    assert policy_act(N, (1, 2), [W], [b], None, None, obs, arena.ptr(lg), arena.ptr(ac)) == 0
    out = arena.fetch()
    assert torch.equal(out[lg][:, 0], loc) and bool((out[lg][:, 1] == 0).all())
    want = torch.tanh(loc.double())
    got = out[ac].view(-1).double()
    u = float(((got - want).abs() / (U24 * want.abs().clamp_min(TINY))).max())
    print(f"\n[measure] tanh of loc: {u:.4g} units of 2^-24 max(|value|, TINY)")
    assert bool((got.abs() <= 1).all())
    assert u <= TANH_UNITS, u


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_episode_accumulate_matches_sequential_torch(gpu, n):
    """Both modes over 7 steps of random data with done ~ Bernoulli(0.3), metrics rows at stride n + 3: run, fin
    and flag equal a sequential fp32 restatement exactly; guards intact; EVAL runs with fin = NULL."""
    from open_duck_playground_amd.native import check
    L, K, T = _lib(), 8, 7
    F_, stride = K + 2, n + 3
    g = torch.Generator().manual_seed(n)
    reward, metrics = torch.randn(T, n, generator=g), 3.0 * torch.randn(T, K, stride, generator=g)
    done = (torch.rand(T, n, generator=g) < 0.3).float()
    arena = Arena()
    h = {k: arena.take(*s) for k, s in {"run_e": (n, F_), "act": (n,), "run_t": (n, F_), "fin": (n, F_),
                                         "cnt": (n,)}.items()}
    arena.alloc(gpu)
    view = {k: arena.buf[arena.regions[i][0]:arena.regions[i][0] + arena.regions[i][1]] for k, i in h.items()}
    for k, v in view.items():
        v.fill_(1.0 if k == "act" else 0.0)
    d_r, d_m, d_d = reward.to(gpu), metrics.to(gpu), done.to(gpu)
    for t in range(T):
        for mode, run, fin, flag in ((ppo.EPISODE_EVAL, "run_e", None, "act"), (ppo.EPISODE_TRAIN, "run_t", "fin", "cnt")):
            check(L.duck_episode_accumulate(n, K, d_r[t].data_ptr(), d_d[t].data_ptr(), d_m[t].data_ptr(), stride, mode,
                                            arena.ptr(h[run]), None if fin is None else arena.ptr(h[fin]),
                                            arena.ptr(h[flag]), _stream()))
    out = arena.fetch()
    # the restatement, one env and one column at a time, fp32 adds in step order
    run_e, act = torch.zeros(n, F_), torch.ones(n)
    run_t, fin, cnt = torch.zeros(n, F_), torch.zeros(n, F_), torch.zeros(n)
    for t in range(T):
        x = torch.cat([reward[t][:, None], metrics[t][:, :n].t(), torch.ones(n, 1)], 1)
        live = act != 0
        run_e[live] = run_e[live] + x[live]
        act[live & (done[t] != 0)] = 0.0
        run_t = run_t + x
        d = done[t] != 0
        fin[d] = fin[d] + run_t[d]
        cnt[d] = cnt[d] + 1.0
        run_t[d] = 0.0
    for k, want in (("run_e", run_e), ("act", act), ("run_t", run_t), ("fin", fin), ("cnt", cnt)):
        assert torch.equal(out[h[k]], want), k
    assert L.duck_episode_accumulate(n, K, d_r[0].data_ptr(), d_d[0].data_ptr(), d_m[0].data_ptr(), stride, 1,
                                     arena.ptr(h["run_t"]), None, arena.ptr(h["cnt"]), _stream()) == EINVAL
    assert L.duck_episode_accumulate(n, K, d_r[0].data_ptr(), d_d[0].data_ptr(), d_m[0].data_ptr(), n - 1, 0,
                                     arena.ptr(h["run_e"]), None, arena.ptr(h["act"]), _stream()) == EINVAL


# ---- ppo.Evaluator on the HIP env ----------------------------------------------------------------------
def _flat_env(gpu, n, episode_length):
    from open_duck_playground_amd.joystick import Joystick, wrap_for_brax_training
    return wrap_for_brax_training(Joystick("flat_terrain", num_envs=n, device=gpu), episode_length=episode_length)


def _net_for(env, cfg, gpu, seed=0):
    torch.manual_seed(seed)
    net = ppo.ActorCritic(env.observation_size["state"][0], env.observation_size["privileged_state"][0],
                          env.action_size, cfg).to(gpu)
    net.obs_norm.update(0.3 + 2.0 * torch.randn(256, env.observation_size["state"][0], device=gpu))
    return net


def eager_reference(net, env, cfg, rng):
    """The evaluation restated: duck_policy_act and env.step launched one by one, the per-env accumulators
    [reward | metrics rows | steps] in torch fp32 with the EvalWrapper rule."""
    from open_duck_playground_amd.native import check
    n, K = env.num_envs, len(env.METRICS)
    st = env.reset(rng=rng)
    rows = st.fstate.view(env._layout.nfloat, n)[env._layout.off["metrics"]:env._layout.off["metrics"] + K]
    acc, active = torch.zeros(n, K + 2, device=env.device), torch.ones(n, device=env.device)
    action = torch.empty(n, env.action_size, device=env.device)
    args, _ = ppo.policy_act_args(net)
    for _ in range(cfg.episode_length):
        check(_lib().duck_policy_act(n, *args, st.obs["state"].data_ptr(), None, action.data_ptr(), _stream()))
        env.step(st, action, inplace=True)
        x = torch.cat([st.reward[:, None], rows.t(), torch.ones(n, 1, device=env.device)], 1)
        acc = torch.where(active[:, None] != 0, acc + x, acc)
        active = active * (1.0 - st.done)
    torch.cuda.synchronize()
    return acc.cpu()


def _no_times(d):
    return {k: v for k, v in d.items() if k not in TIMES}


@pytest.mark.parametrize("chunk", [200, 5])
def test_evaluator_graph_equals_eager_reference(gpu, monkeypatch, chunk):
    """16 flat-terrain envs wrapped with episode_length 8, evaluated for 12 steps: every env is done by step 8
    and steps 9 - 12 add nothing. The first evaluation runs eagerly, the later ones replay the captured graph
    (chunk 200: the whole episode in one graph; chunk 5: two replays and two eager steps): all equal the eager
    reference on a second identical env per env and column; the same rng gives the same dict (but for the two
    wall-time keys); an in-place parameter change shows in the next replay."""
    monkeypatch.setattr(ppo.Evaluator, "CHUNK", chunk)
    monkeypatch.delenv("DUCK_PPO_GRAPH", raising=False)
    monkeypatch.delenv("DUCK_PPO_FUSED_MLP", raising=False)
    cfg = ppo.PPOConfig(episode_length=12)
    env, ref_env = _flat_env(gpu, 16, 8), _flat_env(gpu, 16, 8)
    net = _net_for(env, cfg, gpu)
    ev = ppo.Evaluator(net, env, cfg)
    assert ev.native and ev.use_graph
    want = eager_reference(net, ref_env, cfg, rng=7)
    assert float(want[:, -1].max()) <= 8 and float(want[:, -1].min()) >= 1
    d1 = ev.run(rng=7)
    assert ev.graph is None and torch.equal(ev.acc.cpu(), want)
    d2 = ev.run(rng=7)
    assert ev.graph is not None and torch.equal(ev.acc.cpu(), want)
    d3 = ev.run(rng=7)
    assert _no_times(d1) == _no_times(d2) == _no_times(d3)
    assert d2["eval/avg_episode_length"] <= 8
    assert set(_no_times(d2)) == {"eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length",
                                  "eval/std_episode_length"} | {f"eval/episode_{k}{s}" for k in METRIC_NAMES
                                                                 for s in ("", "_std")}
    assert d2["eval/episode_reward"] == float(want[:, 0].double().sum()) / 16
    other = ev.run(rng=8)
    assert _no_times(other) != _no_times(d2)
    with torch.no_grad():
        net.policy[-1].bias.add_(0.1)   # in place: the graph reads the live parameters
    graph = ev.graph
    d4 = ev.run(rng=7)
    assert ev.graph is graph and _no_times(d4) != _no_times(d2)
    assert torch.equal(ev.acc.cpu(), eager_reference(net, ref_env, cfg, rng=7))
    # evaluate() keeps one Evaluator per (net, env, cfg)
    ppo.evaluate(net, env, cfg, rng=7)
    first = env._evaluator
    assert _no_times(ppo.evaluate(net, env, cfg, rng=7)) == _no_times(d4) and env._evaluator is first


def test_evaluator_without_graph_and_fallback(gpu, monkeypatch):
    """DUCK_PPO_GRAPH=0: the same kernels eagerly, the same numbers. DUCK_PPO_FUSED_MLP=0: the torch loop, the
    same keys."""
    cfg = ppo.PPOConfig(episode_length=6)
    env = _flat_env(gpu, 16, 4)
    net = _net_for(env, cfg, gpu)
    ev = ppo.Evaluator(net, env, cfg)
    ev.run(rng=3)
    d = ev.run(rng=3)
    monkeypatch.setenv("DUCK_PPO_GRAPH", "0")
    ev0 = ppo.Evaluator(net, env, cfg)
    assert ev0.native and not ev0.use_graph
    ev0.run(rng=3)
    assert _no_times(ev0.run(rng=3)) == _no_times(d) and ev0.graph is None
    monkeypatch.setenv("DUCK_PPO_FUSED_MLP", "0")
    evt = ppo.Evaluator(net, env, cfg)
    assert not evt.native
    dt = evt.run(rng=3)
    assert set(dt) == set(d) and dt["eval/avg_episode_length"] <= 4


def test_standing_env_key_set(gpu):
    from open_duck_playground_amd.joystick import wrap_for_brax_training
    from open_duck_playground_amd.standing import Standing
    cfg = ppo.PPOConfig(episode_length=4)
    env = wrap_for_brax_training(Standing("flat_terrain", num_envs=8, device=gpu), episode_length=4)
    net = _net_for(env, cfg, gpu)
    ev = ppo.Evaluator(net, env, cfg)
    assert ev.native
    out = ev.run(rng=2)
    names = [k for k in STANDING_METRIC_NAMES if k]
    assert len(names) == 7 and "eval/episode_cost/head_pos" in out and not any("None" in k for k in out)
    assert set(_no_times(out)) == {"eval/episode_reward", "eval/episode_reward_std", "eval/avg_episode_length",
                                   "eval/std_episode_length"} | {f"eval/episode_{k}{s}" for k in names
                                                                  for s in ("", "_std")}
    assert all(v == v and abs(v) < float("inf") for v in out.values())


def test_training_episode_metrics_leave_training_untouched(gpu):
    """ppo.train on 64 HIP envs (episode_length 6, unroll 4, 3 updates) with and without log_training_metrics:
    every train/* value and the final state_dict agree bit for bit; the episode/* records are consistent."""
    runs = []
    for flag in (False, True):
        env = _flat_env(gpu, 64, 6)
        cfg = ppo.PPOConfig(num_envs=64, batch_size=2, num_minibatches=32, num_evals=0, episode_length=6,
                            unroll_length=4, log_training_metrics=flag)
        runs.append(ppo.train(env, cfg, max_updates=3))
    off, on = runs
    assert len(on.metrics) == len(off.metrics) == 3
    for a, b in zip(off.metrics, on.metrics):
        assert not any(k.startswith("episode/") for k in a)
        assert {k: v for k, v in a.items() if k.startswith("train/")} == \
               {k: v for k, v in b.items() if k.startswith("train/")}
        assert {"episode/sum_reward", "episode/length", "episode/count"} | \
               {f"episode/{k}" for k in METRIC_NAMES} <= set(b)
        if b["episode/count"] > 0:
            assert 1 <= b["episode/length"] <= 6
        else:
            assert b["episode/length"] == 0 and b["episode/sum_reward"] == 0
    assert sum(m["episode/count"] for m in on.metrics) >= 2 * 64
    sa, sb = off.net.state_dict(), on.net.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
