"""PPO outer loop on the HIP env: rollouts through libduck, learner in torch."""

import json
import os

import numpy as np
import pytest
import torch

from open_duck_playground_amd import ppo, runner
from open_duck_playground_amd.joystick import Joystick, domain_randomize, wrap_for_brax_training

pytestmark = pytest.mark.gpu


def test_ppo_updates_on_hip_env(gpu):
    n = 512
    env = wrap_for_brax_training(Joystick("flat_terrain", num_envs=n, device=gpu), episode_length=1000,
                                 randomization_fn=domain_randomize, rng=3)
    cfg = ppo.PPOConfig(num_envs=n, batch_size=16, num_minibatches=32, num_evals=0)
    res = ppo.train(env, cfg, max_updates=3)
    assert len(res.metrics) == 3 and res.env_steps == 3 * 20 * n
    for m in res.metrics:
        assert all(np.isfinite(v) for v in m.values())
    assert int(res.net.obs_norm.count) == 3 * 20 * n
    # the normaliser follows the obs: home-pose joint offsets (state[13:27]) stay near 0
    assert float(res.net.obs_norm.mean[13:27].abs().max()) < 0.5
    ev = ppo.evaluate(res.net, wrap_for_brax_training(Joystick("flat_terrain", num_envs=32, device=gpu),
                                                      episode_length=50), ppo.PPOConfig(episode_length=50), rng=1)
    assert np.isfinite(ev["eval/episode_reward"]) and 1 <= ev["eval/avg_episode_length"] <= 50


def test_runner_cli_one_update(gpu, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(runner.BaseRunner, "make_ppo_params",
                        lambda self: ppo.PPOConfig(num_timesteps=self.num_timesteps, num_envs=256, batch_size=8,
                                                   num_minibatches=32, episode_length=40, num_evals=2))
    runner.main(["--output_dir", "ck", "--num_timesteps", str(2 * 20 * 256), "--num_eval_envs", "16"])
    lines = [json.loads(x) for x in open(tmp_path / "ck" / "metrics.jsonl")]
    assert lines[0]["step"] == 0 and "eval/episode_reward" in lines[0]
    assert lines[-1]["step"] == 2 * 20 * 256
    cks = sorted(p for p in os.listdir(tmp_path / "ck") if p.endswith(".pt"))
    assert cks, os.listdir(tmp_path / "ck")
    assert os.path.exists(tmp_path / "ck" / cks[-1].replace(".pt", ".onnx"))
    net = ppo.load_checkpoint(str(tmp_path / "ck" / cks[-1]), device=gpu)
    assert net.policy_logits(torch.zeros(2, 101, device=gpu)).shape == (2, 28)
    # resume from it
    runner.main(["--output_dir", "ck2", "--num_timesteps", str(20 * 256), "--num_eval_envs", "16",
                 "--restore_checkpoint_path", str(tmp_path / "ck" / cks[-1])])


def test_train_surfaces_latency_timeout(gpu, monkeypatch):
    """The graph-captured rollout with the force_timeout test build (its latency-kernel waits in
    workgroup 1 give up, which sets the device error word and NaN-s that workgroup's qpos): train()
    raises DuckError instead of learning from the corrupted transitions."""
    from open_duck_playground_amd import joystick as jmod
    from open_duck_playground_amd.native import BUILD, DuckError
    path = os.path.join(BUILD, "libduck_force_timeout.so")
    assert os.path.exists(path), "built by __graft_entry__.build()"
    monkeypatch.setattr(jmod, "model_library", lambda m: path)
    n = 64
    env = wrap_for_brax_training(Joystick("flat_terrain", num_envs=n, device=gpu), episode_length=1000)
    env.set_step_mode("latency")
    cfg = ppo.PPOConfig(num_envs=n, batch_size=2, num_minibatches=32, num_evals=0)
    with pytest.raises(DuckError, match="device error word"):
        ppo.train(env, cfg, max_updates=3, use_graph=True)
    assert env.device_error(clear=True) == 1


def test_graph_learner_matches_eager(gpu):
    """The HIP-graph learner replays the same update sequence as the eager one.

    entropy_cost = 0 takes the learner's only random draw (the entropy sample) out of the
    gradients, so both paths see identical numbers and differ only if the graph is wrong.
    """
    out = []
    for use_graph in (False, True):
        env = wrap_for_brax_training(Joystick("flat_terrain", num_envs=256, device=gpu), episode_length=1000)
        cfg = ppo.PPOConfig(num_envs=256, batch_size=8, num_minibatches=32, num_evals=0, entropy_cost=0.0)
        res = ppo.train(env, cfg, max_updates=2, use_graph=use_graph)
        out.append(torch.cat([p.detach().reshape(-1) for p in res.net.parameters()]))
    err = (out[0] - out[1]).abs().max().item()
    assert err < 1e-5, err


@pytest.mark.parametrize("T,B", [(20, 5120), (7, 1000), (1, 3), (0, 4), (5, 0)])
def test_gae_kernel_matches_restatement(gpu, T, B):
    from tests.test_ppo import gae_numpy
    rng = np.random.default_rng(T * 1000 + B)
    r, v, boot = rng.normal(size=(T, B)), rng.normal(size=(T, B)), rng.normal(size=B)
    done = (rng.random((T, B)) < 0.1).astype(np.float64)
    trunc = done * (rng.random((T, B)) < 0.5)
    term = done * (1 - trunc)
    f32 = [x.astype(np.float32).astype(np.float64) for x in (trunc, term, r, v, boot)]
    ins = [torch.tensor(x, dtype=torch.float32, device=gpu) for x in f32]
    vs, adv = ppo.compute_gae(*ins, 0.95, 0.97)
    vs_n, adv_n = gae_numpy(*f32, 0.95, 0.97)
    np.testing.assert_allclose(vs.cpu().numpy(), vs_n, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(adv.cpu().numpy(), adv_n, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("T,B,normalize", [(20, 256, True), (7, 1000, True), (3, 5, False), (1, 1024, True),
                                              (24, 256, True), (25, 256, False)])
def test_gae_stats_kernel_matches_torch(gpu, T, B, normalize):
    """duck_gae_stats (one launch: termination = done (1 - truncation), reward scaling, GAE, the advantage
    mean / 1 / (std + 1e-8)) against the torch expressions FusedGrad used and duck_gae, then
    duck_ppo_loss_stats with those statistics against duck_ppo_loss computing its own."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=gpu).manual_seed(T * 7 + B)
    r, v = torch.randn(T, B, device=gpu, generator=g), torch.randn(T, B, device=gpu, generator=g)
    boot = torch.randn(B, device=gpu, generator=g)
    done = (torch.rand(T, B, device=gpu, generator=g) < 0.1).float()
    trunc = done * (torch.rand(T, B, device=gpu, generator=g) < 0.5).float()
    vs_ref, adv_ref = ppo.compute_gae(trunc, done * (1.0 - trunc), r * 0.7, v, boot, 0.95, 0.97)
    vs, adv, stats = torch.empty(T, B, device=gpu), torch.empty(T, B, device=gpu), torch.empty(2, device=gpu)
    check(L.duck_gae_stats(T, B, trunc.data_ptr(), done.data_ptr(), r.data_ptr(), 0.7, v.data_ptr(), boot.data_ptr(),
                           0.95, 0.97, vs.data_ptr(), adv.data_ptr(), int(normalize), stats.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(vs, vs_ref) and torch.equal(adv, adv_ref)      # the same fp32 expressions, in order
    a64 = adv_ref.double()
    want = (a64.mean(), 1 / (a64.std(unbiased=False) + 1e-8)) if normalize else (0.0, 1.0)
    assert abs(float(stats[0]) - float(want[0])) <= 1e-5 and abs(float(stats[1]) / float(want[1]) - 1) <= 1e-5
    assert L.duck_gae_stats(T, 1025, trunc.data_ptr(), done.data_ptr(), r.data_ptr(), 0.7, v.data_ptr(),
                            boot.data_ptr(), 0.95, 0.97, vs.data_ptr(), adv.data_ptr(), 1, stats.data_ptr(), st) < 0
    if not normalize:
        return
    A, N = 14, T * B
    logits, ra = torch.randn(N, 2 * A, device=gpu, generator=g), torch.randn(N, A, device=gpu, generator=g)
    olp, base, eps = torch.randn(N, device=gpu, generator=g), torch.randn(N, device=gpu, generator=g), \
        torch.randn(N, A, device=gpu, generator=g)
    res = []
    for fn in ("duck_ppo_loss", "duck_ppo_loss_stats"):
        out = torch.empty(L.duck_ppo_loss_out_size(N), device=gpu)
        gl, gb = torch.empty(N, 2 * A, device=gpu), torch.empty(N, device=gpu)
        args = [N, A, logits.data_ptr(), ra.data_ptr(), olp.data_ptr(), adv.data_ptr(), vs.data_ptr(), base.data_ptr(),
                eps.data_ptr(), 0.2, 0.005]
        args += [1] if fn == "duck_ppo_loss" else [stats.data_ptr()]
        check(getattr(L, fn)(*args, out.data_ptr(), gl.data_ptr(), gb.data_ptr(), st))
        torch.cuda.synchronize()
        res.append((out[:4].clone(), gl, gb))
    (o0, g0, b0), (o1, g1, b1) = res
    assert torch.allclose(o0, o1, rtol=1e-5, atol=1e-7) and torch.allclose(g0, g1, rtol=1e-4, atol=1e-9)
    assert torch.equal(b0, b1)


@pytest.mark.parametrize("N,F", [(163840, 101), (163840, 172), (1000, 65), (3, 1), (0, 7)])
def test_column_stats_kernel_matches_torch(gpu, N, F):
    """duck_column_stats (the batch moments of RunningStatistics.update) against torch's fp64 column sums
    (the same sums in another order: fp64 rounding apart), the same bits on a second run, and
    RunningStatistics.update on the GPU against the same update on the CPU."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=gpu).manual_seed(N + F)
    x = torch.randn(N, F, device=gpu, generator=g) * 3.0 + 0.5
    scratch = torch.empty(max(1, L.duck_column_stats_scratch(N, F)), dtype=torch.float64, device=gpu)
    outs = []
    for _ in range(2):
        out = torch.full((2 * F,), float("nan"), dtype=torch.float64, device=gpu)
        check(L.duck_column_stats(N, F, x.data_ptr(), out.data_ptr(), scratch.data_ptr(), st))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    x64 = x.double()
    want = torch.cat([x64.sum(0), (x64 * x64).sum(0)])
    assert torch.allclose(outs[0], want, rtol=1e-12, atol=1e-9)
    assert L.duck_column_stats(N, 0, x.data_ptr(), outs[0].data_ptr(), scratch.data_ptr(), st) < 0
    if N == 0:
        return
    rs_gpu, rs_cpu = ppo.RunningStatistics(F).to(gpu), ppo.RunningStatistics(F)
    for k in range(2):
        xb = x[k::2]
        rs_gpu.update(xb)
        rs_cpu.update(xb.cpu())
    for name in ("count", "mean", "summed_var", "std"):
        assert torch.allclose(getattr(rs_gpu, name).cpu(), getattr(rs_cpu, name), rtol=1e-10, atol=1e-12), name


def test_runner_standing_env(gpu, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(runner.BaseRunner, "make_ppo_params",
                        lambda self: ppo.PPOConfig(num_timesteps=self.num_timesteps, num_envs=256, batch_size=8,
                                                   num_minibatches=32, episode_length=40, num_evals=0))
    runner.main(["--output_dir", "ck", "--env", "standing", "--num_timesteps", str(20 * 256)])
    line = json.loads(open(tmp_path / "ck" / "metrics.jsonl").readline())
    assert line["step"] == 20 * 256 and np.isfinite(line["train/loss"])


@pytest.mark.parametrize("normalize", [True, False])
def test_fused_loss_matches_torch(gpu, normalize):
    """duck_ppo_loss (one HIP launch) against the torch expression of ppo_loss on the same minibatch:
    loss, the three metrics and every parameter gradient, with the entropy sample drawn from the same
    generator state; ratios pushed across the clip range on some samples (both sides of the clamp,
    and exact ties where rho is inside it)."""
    torch.manual_seed(0)
    T, B, A = 20, 64, 14
    cfg = ppo.PPOConfig(normalize_advantage=normalize)
    net = ppo.ActorCritic(101, 172, A, cfg).to(gpu)
    g = torch.Generator(device="cpu").manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu)
    batch = {"obs": r(T, B, 101), "priv": r(T, B, 172), "next_priv": r(T, B, 172),
             "reward": r(T, B), "truncation": (torch.rand(T, B, generator=g) < 0.05).float().to(gpu),
             "done": (torch.rand(T, B, generator=g) < 0.1).float().to(gpu), "raw_action": 1.5 * r(T, B, A)}
    with torch.no_grad():
        lp = ppo.NormalTanh(net.policy_logits(batch["obs"])).log_prob(batch["raw_action"])
    # old log-probs: the current ones shifted so that rho spans [0.5, 1.6] (clip range 0.8 .. 1.2)
    batch["log_prob"] = lp - torch.log(torch.linspace(0.5, 1.6, T * B, device=gpu)).view(T, B)
    res = []
    for fused in (False, True):
        net.zero_grad(set_to_none=True)
        gen = torch.Generator(device=gpu).manual_seed(7)
        loss, m = ppo.ppo_loss(net, batch, cfg, gen, fused=fused)
        loss.backward()
        res.append((float(loss), {k: float(v) for k, v in m.items()},
                    [p.grad.detach().clone() for p in net.parameters()]))
    (l0, m0, g0), (l1, m1, g1) = res
    assert abs(l1 - l0) <= 1e-5 * (1 + abs(l0)), (l0, l1)
    for k in m0:
        assert abs(m1[k] - m0[k]) <= 1e-5 * (1 + abs(m0[k])), (k, m0[k], m1[k])
    for a, b in zip(g0, g1):
        err = float((a - b).abs().max()) / (1e-6 + float(a.abs().max()))
        assert err < 1e-4, err


@pytest.mark.parametrize("normalize_obs", [True, False])
def test_fused_mlp_grads_match_autograd(gpu, normalize_obs):
    """FusedGrad (both MLPs forward and backward through the duck_mlp_* fp32 MFMA kernels, no
    autograd) against ppo_loss(fused=True) + loss.backward() on the same minibatch: the loss, the
    three metrics and every parameter gradient to 1e-4 (relative to the gradient's largest entry),
    with a fitted observation normaliser (op(X) = (X - mean) / std fused into the first layer's
    loads) and without one; sizes off the 64-row / 64-column tiles (T x B = 140 rows, obs 101)."""
    torch.manual_seed(0)
    T, B, A = 20, 7, 14
    cfg = ppo.PPOConfig(normalize_observations=normalize_obs)
    net = ppo.ActorCritic(101, 172, A, cfg).to(gpu)
    g = torch.Generator(device="cpu").manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(gpu)
    # raw observations off-centre when the normaliser is fitted (it brings them to N(0, 1)); centred
    # without one (un-normalised inputs of mean 2, std 3 make the problem ill-conditioned in fp32:
    # torch's own fp32 gradients then differ from fp64 by 3e-3)
    obs = 2 + 3 * r(T, B, 101) if normalize_obs else r(T, B, 101)
    batch = {"obs": obs, "priv": r(T, B, 172) - (1 if normalize_obs else 0), "next_priv": r(T, B, 172),
             "reward": r(T, B), "truncation": (torch.rand(T, B, generator=g) < 0.05).float().to(gpu),
             "done": (torch.rand(T, B, generator=g) < 0.1).float().to(gpu), "raw_action": 1.5 * r(T, B, A)}
    if normalize_obs:
        net.obs_norm.update(batch["obs"])
        net.priv_norm.update(batch["priv"])
    with torch.no_grad():
        lp = ppo.NormalTanh(net.policy_logits(batch["obs"])).log_prob(batch["raw_action"])
    batch["log_prob"] = lp - torch.log(torch.linspace(0.5, 1.6, T * B, device=gpu)).view(T, B)
    net.zero_grad(set_to_none=True)
    loss, m = ppo.ppo_loss(net, batch, cfg, torch.Generator(device=gpu).manual_seed(7), fused=True)
    loss.backward()
    ref = [p.grad.detach().clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    fg = ppo.FusedGrad(net, T * B, B, gpu)
    out = fg(batch, cfg, torch.Generator(device=gpu).manual_seed(7))
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(loss)) <= 1e-5 * (1 + abs(float(loss)))
    for k in m:
        assert abs(float(out[k]) - float(m[k])) <= 1e-5 * (1 + abs(float(m[k]))), k
    for (name, p), a in zip(net.named_parameters(), ref):
        err = float((p.grad - a).abs().max()) / (1e-6 + float(a.abs().max()))
        assert err < 1e-4, (name, err)


def test_fused_mlp_gemm_shapes(gpu):
    """duck_mlp_gemm modes 0 / 1 / 2 against torch at the learner's shapes (5120 x 101 -> 512 ..)."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(1)
    for (n, k, m) in [(5120, 101, 512), (5376, 512, 256), (5120, 128, 28), (130, 70, 1)]:
        x, w, b = torch.randn(n, k, device=gpu), torch.randn(m, k, device=gpu) / k ** 0.5, torch.randn(m, device=gpu)
        mean, std = torch.randn(k, device=gpu), torch.rand(k, device=gpu) + 0.5
        z, h = torch.empty(n, m, device=gpu), torch.empty(n, m, device=gpu)
        check(L.duck_mlp_gemm(1, n, k, m, x.data_ptr(), w.data_ptr(), b.data_ptr(), None, z.data_ptr(), h.data_ptr(),
                              mean.data_ptr(), (1 / std).data_ptr(), st))
        zr = torch.addmm(b, (x - mean) / std, w.t())
        torch.cuda.synchronize()
        assert float((z - zr).abs().max()) <= 1e-4 * float(zr.abs().max()), (n, k, m)
        assert float((h - torch.nn.functional.silu(zr)).abs().max()) <= 1e-4 * float(zr.abs().max())
        # the data gradient through this layer: (dY W) * silu'(zp)
        dy, zp = torch.randn(n, m, device=gpu), torch.randn(n, k, device=gpu)
        dx = torch.empty(n, k, device=gpu)
        check(L.duck_mlp_gemm(2, n, m, k, dy.data_ptr(), w.data_ptr(), None, zp.data_ptr(), dx.data_ptr(), None, None,
                              None, st))
        s = torch.sigmoid(zp)
        dxr = (dy @ w) * (s * (1 + zp * (1 - s)))
        torch.cuda.synchronize()
        assert float((dx - dxr).abs().max()) <= 1e-4 * float(dxr.abs().max()), (n, k, m)


def test_policy_sample_kernel(gpu):
    """duck_policy_sample: action = tanh(raw), log_prob = NormalTanh(logits).log_prob(raw) (the torch
    expression), the implied draws eps = (raw - loc) / scale standard normal, and the device counter
    advancing (a second call draws other noise)."""
    from open_duck_playground_amd.native import check, lib
    n, A = 8192, 14
    torch.manual_seed(2)
    logits = torch.randn(n, 2 * A, device=gpu)
    ctr = torch.zeros(1, dtype=torch.int32, device=gpu)
    outs = []
    for _ in range(2):
        raw, lp, act = torch.empty(n, A, device=gpu), torch.empty(n, device=gpu), torch.empty(n, A, device=gpu)
        check(lib().duck_policy_sample(n, A, logits.data_ptr(), 12345, ctr.data_ptr(), raw.data_ptr(), lp.data_ptr(),
                                       act.data_ptr(), torch.cuda.current_stream().cuda_stream))
        outs.append((raw, lp, act))
    torch.cuda.synchronize()
    assert int(ctr.item()) == 2
    d = ppo.NormalTanh(logits)
    for raw, lp, act in outs:
        assert torch.allclose(act, torch.tanh(raw), atol=1e-6)
        ref = d.log_prob(raw)
        assert float((lp - ref).abs().max()) <= 1e-4 * (1 + float(ref.abs().max()))
        eps = ((raw - d.loc) / d.scale).reshape(-1)
        assert abs(float(eps.mean())) < 0.01 and abs(float(eps.std()) - 1) < 0.01
    assert not torch.equal(outs[0][0], outs[1][0])


def test_clip_adam_matches_torch(gpu):
    """duck_clip_adam (flat clip_grad_norm_ + Adam, two launches) against torch's clip_grad_norm_ and
    Adam over 5 steps of random gradients, with clipping active (large gradients) and inactive."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    torch.manual_seed(4)
    P = 300_001
    p0 = torch.randn(P, device=gpu)
    for scale, max_norm in ((10.0, 1.0), (1e-4, 1.0)):
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([ref], lr=3e-4)
        p = p0.clone()
        m, v = torch.zeros(P, device=gpu), torch.zeros(P, device=gpu)
        step = torch.zeros(1, dtype=torch.int32, device=gpu)
        scratch = torch.zeros(L.duck_clip_adam_scratch_size(P), device=gpu)
        for _ in range(5):
            g = scale * torch.randn(P, device=gpu)
            ref.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
            opt.step()
            check(L.duck_clip_adam(P, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), scratch.data_ptr(),
                                   step.data_ptr(), 3e-4, 0.9, 0.999, 1e-8, max_norm,
                                   torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert int(step.item()) == 5
        err = float((p - ref.detach()).abs().max())
        assert err <= 1e-6, (scale, err)


@pytest.mark.parametrize("P", [1, 2047, 2048, 2049, 526_337])
def test_clip_adam_matches_torch_sizes(gpu, P):
    """test_clip_adam_matches_torch at the sizes where the launch geometry changes: one entry, one workgroup
    (2048 entries) less one / exactly / plus one, and 257 workgroups, where the update's strided sum of the
    norm partials (thread t: partials t, t + 256, ..) makes a second trip. The same comparison and 1e-6, and
    the first moment against torch's to 1e-5 of its largest entry; two steps for the large size."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    torch.manual_seed(4 + P)
    assert L.duck_clip_adam_scratch_size(P) == -(-P // 2048)
    p0 = torch.randn(P, device=gpu)
    steps = 2 if P > 100_000 else 5
    for scale, max_norm in ((10.0, 1.0), (1e-4, 1.0)):
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([ref], lr=3e-4)
        p = p0.clone()
        m, v = torch.zeros(P, device=gpu), torch.zeros(P, device=gpu)
        step = torch.zeros(1, dtype=torch.int32, device=gpu)
        scratch = torch.zeros(L.duck_clip_adam_scratch_size(P), device=gpu)
        for _ in range(steps):
            g = scale * torch.randn(P, device=gpu)
            ref.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
            opt.step()
            check(L.duck_clip_adam(P, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), scratch.data_ptr(),
                                   step.data_ptr(), 3e-4, 0.9, 0.999, 1e-8, max_norm,
                                   torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert int(step.item()) == steps
        err = float((p - ref.detach()).abs().max())
        assert err <= 1e-6, (scale, err)
        # Adam's step is invariant to the gradient's scale, so the parameters hardly see a wrong clip norm; the
        # first moment is linear in it. fp32 sums of the squares agree to ~1e-6; a norm partial left out of
        # 257 is 2e-3.
        m_ref = opt.state[ref]["exp_avg"]
        err = float((m - m_ref).abs().max()) / float(m_ref.abs().max())
        assert err <= 1e-5, (scale, err)


def test_clip_adam_reduce_equals_reduce_then_clip_adam(gpu):
    """duck_clip_adam_reduce (the weight-gradient partials summed by the update's first launch, one rank)
    gives the same bits as duck_mlp_wgrad_reduce + duck_clip_adam: gradient, moments, parameters, step."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=gpu).manual_seed(11)
    P, S = 300_001, 8
    p0 = torch.randn(P, device=gpu, generator=g)
    runs = []
    for fused in (False, True):
        p, grad = p0.clone(), torch.zeros(P, device=gpu)
        m, v = torch.zeros(P, device=gpu), torch.zeros(P, device=gpu)
        step = torch.zeros(1, dtype=torch.int32, device=gpu)
        scratch = torch.zeros(L.duck_clip_adam_scratch_size(P), device=gpu)
        g.manual_seed(12)
        for k in range(4):
            part = torch.randn(S * P, device=gpu, generator=g) * (3.0 if k % 2 else 1e-3)
            if fused:
                check(L.duck_clip_adam_reduce(P, S, part.data_ptr(), p.data_ptr(), grad.data_ptr(), m.data_ptr(),
                                              v.data_ptr(), scratch.data_ptr(), step.data_ptr(), 3e-4, 0.9, 0.999,
                                              1e-8, 1.0, st))
            else:
                check(L.duck_mlp_wgrad_reduce(P, S, part.data_ptr(), grad.data_ptr(), st))
                check(L.duck_clip_adam(P, p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                       scratch.data_ptr(), step.data_ptr(), 3e-4, 0.9, 0.999, 1e-8, 1.0, st))
        torch.cuda.synchronize()
        runs.append((p, grad, m, v, step))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert L.duck_clip_adam_reduce(P, 0, part.data_ptr(), p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                   scratch.data_ptr(), step.data_ptr(), 3e-4, 0.9, 0.999, 1e-8, 1.0, st) < 0


def test_ppo_loss_grad_then_sums_equals_loss_stats(gpu):
    """duck_ppo_loss_grad (gradients and partial sums, no loss sums) + duck_ppo_loss_sums == duck_ppo_loss_stats,
    bit for bit: the learner's epoch graph skips the sums for every minibatch but the reported one."""
    from open_duck_playground_amd.native import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=gpu).manual_seed(5)
    N, A = 5120, 14
    ins = [torch.randn(N, 2 * A, device=gpu, generator=g), torch.randn(N, A, device=gpu, generator=g)] + \
        [torch.randn(N, device=gpu, generator=g) for _ in range(4)] + [torch.randn(N, A, device=gpu, generator=g)]
    stats = torch.tensor([0.1, 1.3], device=gpu)
    res = []
    for split in (False, True):
        out = torch.empty(L.duck_ppo_loss_out_size(N), device=gpu)
        gl, gb = torch.empty(N, 2 * A, device=gpu), torch.empty(N, device=gpu)
        args = [N, A] + [t.data_ptr() for t in ins] + [0.2, 0.005, stats.data_ptr(), out.data_ptr(), gl.data_ptr(),
                                                       gb.data_ptr(), st]
        if split:
            check(L.duck_ppo_loss_grad(*args))
            check(L.duck_ppo_loss_sums(N, A, 0.005, out.data_ptr(), st))
        else:
            check(L.duck_ppo_loss_stats(*args))
        torch.cuda.synchronize()
        res.append((out[:4].clone(), gl, gb))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert L.duck_ppo_loss_sums(N, 17, 0.005, out.data_ptr(), st) < 0


def test_gather_columns_matches_index_select(gpu):
    """duck_gather_columns (one launch for every field of a minibatch) == torch.index_select per field,
    including a one-row field (the bootstrap observation) and a field of width 1."""
    import ctypes
    import ctypes as C
    from open_duck_playground_amd.native import DuckGatherField, check, lib
    g = torch.Generator(device=gpu)
    g.manual_seed(3)
    T, B, m = 20, 300, 37
    src = {"obs": torch.rand(T, B, 101, device=gpu, generator=g), "r": torch.rand(T, B, device=gpu, generator=g),
           "a": torch.rand(T, B, 14, device=gpu, generator=g), "np": torch.rand(T, B, 172, device=gpu, generator=g)}
    idx = torch.randperm(B, device=gpu, generator=g)[:m]
    dst = {"obs": torch.empty(T, m, 101, device=gpu), "r": torch.empty(T, m, device=gpu),
           "a": torch.empty(T, m, 14, device=gpu), "np": torch.empty(m, 172, device=gpu)}
    f = [DuckGatherField(src[k].data_ptr(), dst[k].data_ptr(), T, B, w) for k, w in (("obs", 101), ("r", 1), ("a", 14))]
    f.append(DuckGatherField(src["np"][-1].data_ptr(), dst["np"].data_ptr(), 1, B, 172))
    arr = (DuckGatherField * len(f))(*f)
    check(lib().duck_gather_columns(len(f), arr, idx.data_ptr(), m, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k in ("obs", "r", "a"):
        assert torch.equal(dst[k], torch.index_select(src[k], 1, idx)), k
    assert torch.equal(dst["np"], torch.index_select(src["np"][-1], 0, idx))
    assert lib().duck_gather_columns(9, arr, idx.data_ptr(), m, None) < 0
    # duck_gather_columns_norm: fields 0 (obs) and 3 (the bootstrap row) through a normaliser, the rest copied
    mo, io = torch.randn(101, device=gpu, generator=g), torch.rand(101, device=gpu, generator=g) + 0.5
    mp, ip = torch.randn(172, device=gpu, generator=g), torch.rand(172, device=gpu, generator=g) + 0.5
    norm = (ctypes.c_void_p * 8)(mo.data_ptr(), io.data_ptr(), None, None, None, None, mp.data_ptr(), ip.data_ptr())
    for v in dst.values():
        v.fill_(float("nan"))
    check(lib().duck_gather_columns_norm(len(f), arr, norm, idx.data_ptr(), m, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(dst["obs"], (torch.index_select(src["obs"], 1, idx) - mo) * io)
    assert torch.equal(dst["np"], (torch.index_select(src["np"][-1], 0, idx) - mp) * ip)
    for k in ("r", "a"):
        assert torch.equal(dst[k], torch.index_select(src[k], 1, idx)), k


def test_mlp_group_equals_separate_launches(gpu):
    """duck_mlp_group (several layer problems in one launch) writes what the separate duck_mlp_gemm /
    duck_mlp_wgrad calls write, bit for bit: a forward layer with the normaliser, a data gradient and a
    weight gradient side by side."""
    from open_duck_playground_amd.native import DuckMlpProblem, check, lib
    L = lib()
    g = torch.Generator(device=gpu)
    g.manual_seed(5)
    st = torch.cuda.current_stream().cuda_stream
    N, R, M = 700, 101, 96
    x = torch.randn(N, R, device=gpu, generator=g)
    W = torch.randn(M, R, device=gpu, generator=g) * 0.1
    bias = torch.randn(M, device=gpu, generator=g)
    mean, istd = torch.randn(R, device=gpu, generator=g), torch.rand(R, device=gpu, generator=g) + 0.5
    dZ = torch.randn(N, M, device=gpu, generator=g)
    Zp = torch.randn(N, R, device=gpu, generator=g)
    P = M * R + M + 16
    outs = {}
    for how in ("separate", "group"):
        Y, Y2, dX = torch.empty(N, M, device=gpu), torch.empty(N, M, device=gpu), torch.empty(N, R, device=gpu)
        part = torch.zeros(3 * P, device=gpu)
        if how == "separate":
            check(L.duck_mlp_gemm(1, N, R, M, x.data_ptr(), W.data_ptr(), bias.data_ptr(), None, Y.data_ptr(),
                                  Y2.data_ptr(), mean.data_ptr(), istd.data_ptr(), st))
            check(L.duck_mlp_gemm(2, N, M, R, dZ.data_ptr(), W.data_ptr(), None, Zp.data_ptr(), dX.data_ptr(),
                                  None, None, None, st))
            check(L.duck_mlp_wgrad(N, M, R, dZ.data_ptr(), x.data_ptr(), mean.data_ptr(), istd.data_ptr(), 3,
                                   part.data_ptr(), P, M, 0, st))
        else:
            probs = [DuckMlpProblem(1, N, R, M, x.data_ptr(), W.data_ptr(), bias.data_ptr(), None, Y.data_ptr(),
                                    Y2.data_ptr(), mean.data_ptr(), istd.data_ptr(), 0, 0, 0, 0, None),
                     DuckMlpProblem(2, N, M, R, dZ.data_ptr(), W.data_ptr(), None, Zp.data_ptr(), dX.data_ptr(),
                                    None, None, None, 0, 0, 0, 0, None),
                     DuckMlpProblem(3, N, R, M, dZ.data_ptr(), x.data_ptr(), None, None, None, None,
                                    mean.data_ptr(), istd.data_ptr(), 3, P, M, 0, part.data_ptr())]
            check(L.duck_mlp_group(3, (DuckMlpProblem * 3)(*probs), st))
        torch.cuda.synchronize()
        outs[how] = (Y, Y2, dX, part)
        if how == "group":   # 64-wide output tiles: the same reduction order per element, the same bits
            Y, Y2, dX = torch.empty(N, M, device=gpu), torch.empty(N, M, device=gpu), torch.empty(N, R, device=gpu)
            part = torch.zeros(3 * P, device=gpu)
            probs[0].Y, probs[0].Y2, probs[1].Y, probs[2].partial = Y.data_ptr(), Y2.data_ptr(), dX.data_ptr(), \
                part.data_ptr()
            check(L.duck_mlp_group_bn(3, (DuckMlpProblem * 3)(*probs), 64, st))
            torch.cuda.synchronize()
            outs["group64"] = (Y, Y2, dX, part)
            # 32-row tiles (duck_mlp_group_tiles): the same bits again
            Y, Y2, dX = torch.empty(N, M, device=gpu), torch.empty(N, M, device=gpu), torch.empty(N, R, device=gpu)
            part = torch.zeros(3 * P, device=gpu)
            probs[0].Y, probs[0].Y2, probs[1].Y, probs[2].partial = Y.data_ptr(), Y2.data_ptr(), dX.data_ptr(), \
                part.data_ptr()
            check(L.duck_mlp_group_tiles(3, (DuckMlpProblem * 3)(*probs), 32, 32, st))
            torch.cuda.synchronize()
            outs["group32rows"] = (Y, Y2, dX, part)
    for key in ("group64", "group32rows"):
        for a, b in zip(outs["separate"], outs[key]):
            assert torch.equal(a, b), key
    assert L.duck_mlp_group_bn(1, (DuckMlpProblem * 1)(probs[0]), 48, st) < 0
    assert L.duck_mlp_group_tiles(1, (DuckMlpProblem * 1)(probs[0]), 32, 64, st) < 0
    assert L.duck_mlp_group_tiles(1, (DuckMlpProblem * 1)(probs[0]), 16, 32, st) < 0
    for a, b in zip(outs["separate"], outs["group"]):
        assert torch.equal(a, b)
    assert L.duck_mlp_group(5, (DuckMlpProblem * 5)(), st) < 0
