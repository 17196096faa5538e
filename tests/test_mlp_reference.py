"""The references of tests/mlp_reference.py checked on the host (no GPU): the fp64 GEMM / data-gradient /
weight-gradient references against torch.autograd on a two-layer fp64 MLP, the loss reference against
ppo.ppo_loss(fused=False) in fp64, the threefry restatement against the Random123 vectors, the Box-Muller
draws' layout and moments, and the a-priori fp32 chain bound against a numpy fp32 chain."""

import numpy as np
import pytest
import torch

from open_duck_playground_amd import ppo
from tests import mlp_reference as ref


def _f32(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("splits", [1, 3, 40])
def test_layer_references_equal_autograd(normalise, splits):
    """Z1 = op(X) W1^T + b1, H1 = silu(Z1), Z2 = H1 W2^T + b2, loss = sum(G Z2): every gradient autograd
    forms in fp64 equals the reference of the kernel that would compute it (to fp64 rounding)."""
    g = torch.Generator().manual_seed(3)
    N, K, M1, M2, P = 37, 19, 23, 5, 700
    X, W1, b1, W2, b2, G = _f32(g, N, K), _f32(g, M1, K), _f32(g, M1), _f32(g, M2, M1), _f32(g, M2), _f32(g, N, M2)
    mean, istd = (_f32(g, K), torch.rand(K, generator=g) + 0.5) if normalise else (None, None)
    Xn = ref.op_norm(X, mean, istd)
    if normalise:
        assert torch.equal(Xn, ((X - mean) * istd).double()) and not torch.equal(Xn, (X.double() - mean.double()) * istd.double())
    w1, B1, w2, B2 = (t.double().requires_grad_(True) for t in (W1, b1, W2, b2))
    Z1 = Xn @ w1.t() + B1
    Z1.retain_grad()
    H1 = torch.nn.functional.silu(Z1)
    Z2 = H1 @ w2.t() + B2
    (G.double() * Z2).sum().backward()
    tol = dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref.gemm_ref(X, W1, b1, mean, istd), Z1.detach(), **tol)
    assert torch.allclose(ref.silu(Z1.detach()), H1.detach(), **tol)
    # the data gradient through the hidden layer; fp32 operands for the reference's signature
    dZ1 = ref.dgrad_ref(G, W2, Z1.detach().float())
    Z1f = Z1.detach().float().double().requires_grad_(True)
    (torch.nn.functional.silu(Z1f) * (G.double() @ W2.double())).sum().backward()
    assert torch.allclose(dZ1, Z1f.grad, **tol)
    assert torch.allclose(ref.dgrad_ref(G, W2, Z1.detach().float()) / ref.dsilu(Z1.detach().float()), G.double() @ W2.double(), **tol)
    # the weight gradients: the partials' sum over the splits, scattered at the offsets
    off_w, off_b = 5, 5 + M2 * M1 + 7
    part, mag, mask = ref.wgrad_ref(G, H1.detach().float(), None, None, splits, P, off_w, off_b)
    H1f = H1.detach().float().double()
    assert torch.allclose(part.sum(0)[off_w:off_w + M2 * M1].view(M2, M1), G.double().t() @ H1f, **tol)
    assert torch.allclose(G.double().t() @ H1f, w2.grad, rtol=1e-6, atol=1e-6)    # (H1f is H1 rounded to fp32)
    assert torch.allclose(part.sum(0)[off_b:off_b + M2], B2.grad, **tol)
    assert int(mask.sum()) == M2 * M1 + M2 and not part[:, ~mask].any() and (mag >= part.abs() - 1e-12).all()
    # the first layer, with the normaliser on its loads; dZ1 from autograd, rounded to fp32 as the kernel's input
    d1 = Z1.grad.float()
    part, _, _ = ref.wgrad_ref(d1, X, mean, istd, splits, P, 0, M1 * K)
    assert torch.allclose(part.sum(0)[:M1 * K].view(M1, K), d1.double().t() @ Xn, **tol)
    assert torch.allclose(d1.double().t() @ Xn, w1.grad, rtol=1e-5, atol=1e-5)     # (d1 is Z1.grad rounded to fp32)
    rps = -(-N // splits)
    for s in range(splits):   # every block on its own, empty ones included
        blk = slice(min(N, s * rps), min(N, (s + 1) * rps))
        assert torch.allclose(part[s, :M1 * K].view(M1, K), d1[blk].double().t() @ Xn[blk], **tol)
        assert torch.allclose(part[s, M1 * K:M1 * K + M1], d1[blk].double().sum(0), **tol)


@pytest.mark.parametrize("normalize", [True, False])
def test_loss_reference_equals_ppo_loss_fp64(normalize):
    """ppo_loss_ref == ppo.ppo_loss(fused=False) run in fp64: the loss, the three metrics, and every
    parameter gradient when the reference's logits / baseline gradients are pushed through the networks."""
    torch.manual_seed(0)
    T, B, A = 6, 9, 5
    cfg = ppo.PPOConfig(normalize_advantage=normalize, normalize_observations=False)
    net = ppo.ActorCritic(11, 13, A, cfg).double()
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    batch = {"obs": r(T, B, 11), "priv": r(T, B, 13), "next_priv": r(T, B, 13), "reward": r(T, B),
             "truncation": (torch.rand(T, B, generator=g) < 0.05).double(),
             "done": (torch.rand(T, B, generator=g) < 0.1).double(), "raw_action": 1.5 * r(T, B, A)}
    with torch.no_grad():
        lp = ppo.NormalTanh(net.policy_logits(batch["obs"])).log_prob(batch["raw_action"])
    assert torch.allclose(lp.reshape(-1), ref.normal_tanh_log_prob(net.policy_logits(batch["obs"]).reshape(-1, 2 * A).detach(),
                                                                   batch["raw_action"].reshape(-1, A)), rtol=1e-12, atol=1e-12)
    batch["log_prob"] = lp - torch.log(torch.linspace(0.5, 1.6, T * B, dtype=torch.float64)).view(T, B)
    loss, m = ppo.ppo_loss(net, batch, cfg, torch.Generator().manual_seed(7), fused=False)
    loss.backward()
    want = [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    # the same quantities the loss kernel is given
    logits = net.policy_logits(batch["obs"])
    priv, nxt = batch["priv"], batch["next_priv"][-1]
    v_all = net.value_of(torch.cat([priv.reshape(-1, 13), nxt], 0))
    baseline, boot = v_all[:T * B].view(T, B), v_all[T * B:]
    trunc = batch["truncation"]
    vs, adv = ppo.compute_gae(trunc, batch["done"] * (1 - trunc), batch["reward"] * cfg.reward_scaling, baseline.detach(),
                              boot.detach(), cfg.gae_lambda, cfg.discounting)
    eps = torch.randn(T, B, A, generator=torch.Generator().manual_seed(7))    # as NormalTanh.sample_raw draws it
    out = ref.ppo_loss_ref(logits.reshape(-1, 2 * A), batch["raw_action"].reshape(-1, A), batch["log_prob"].reshape(-1),
                           adv.reshape(-1), vs.reshape(-1), baseline.reshape(-1), eps.reshape(-1, A),
                           cfg.clipping_epsilon, cfg.entropy_cost, normalize)
    got = out["out"]
    assert abs(float(got[0]) - float(loss.detach())) <= 1e-12 * (1 + abs(float(loss.detach())))
    for k, name in ((1, "policy_loss"), (2, "v_loss"), (3, "entropy")):
        assert abs(float(got[k]) - float(m[name])) <= 1e-12 * (1 + abs(float(m[name]))), name
    torch.autograd.backward([logits, baseline], [out["grad_logits"].view_as(logits), out["grad_baseline"].view_as(baseline)])
    for p, w in zip(net.parameters(), want):
        assert torch.allclose(p.grad, w, rtol=1e-10, atol=1e-13)
    # both sides of the clip and the interior are present, so the clip classification is exercised
    rho = out["rho"]
    assert (rho < 0.8).any() and (rho > 1.2).any() and ((rho > 0.8) & (rho < 1.2)).any()


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0), (0, 0), (0x6B200159, 0x99BA4EFE)),
    ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x1CB996FC, 0xBB002BE7)),
    ((0x243F6A88, 0x85A308D3), (0x13198A2E, 0x03707344), (0xC4923A9C, 0x483DF7A0)),
])
def test_threefry_restatement_kat(ctr, key, out):
    """Random123 kat_vectors, threefry2x32 with 20 rounds (the vectors of test_oracle_physics.py)."""
    a, b = ref.threefry2x32(key[0], key[1], np.array([ctr[0]] * 3), np.array([ctr[1]] * 3))
    assert a.dtype == np.uint32 and [(int(x), int(y)) for x, y in zip(a, b)] == [out] * 3


def test_sampler_restatement_layout_and_moments():
    """sample_eps_ref: element 2 pair / 2 pair + 1 are the cosine / sine draws of counter (row, 8 ctr + pair),
    an odd A drops the last sine draw, counters 8 apart continue the stream, and the draws are standard
    normal (mean and variance of 160 k draws within 4 standard errors)."""
    seed = 0x9E3779B97F4A7C15
    e = ref.sample_eps_ref(5, 16, seed, 3)
    a, b = ref.threefry2x32(seed & 0xFFFFFFFF, seed >> 32, np.array([4]), np.array([8 * 3 + 6]))
    u1, u2 = ((int(a[0]) >> 9) + 1) / 2 ** 23, (int(b[0]) >> 9) / 2 ** 23
    r = np.sqrt(-2 * np.log(u1))
    assert e[4, 12] == r * np.cos(2 * np.pi * u2) and e[4, 13] == r * np.sin(2 * np.pi * u2)
    assert np.array_equal(ref.sample_eps_ref(5, 13, seed, 3), e[:, :13])
    assert not np.array_equal(ref.sample_eps_ref(5, 16, seed & 0xFFFFFFFF, 3), e)      # the high word is part of the key
    assert not np.array_equal(ref.sample_eps_ref(5, 16, seed, 4), e)
    big = ref.sample_eps_ref(10000, 16, 12345, 0).reshape(-1)
    n = big.size
    assert abs(big.mean()) < 4 / np.sqrt(n) and abs(big.var() - 1) < 4 * np.sqrt(2 / n)
    assert np.abs(big).max() <= np.sqrt(-2 * np.log(2.0 ** -23)) and np.isfinite(big).all()


@pytest.mark.parametrize("N,R,M", [(65, 101, 33), (33, 36, 65), (64, 512, 64), (16, 1, 16), (65, 129, 17)])
def test_chain_bound_holds_for_fp32_chain(N, R, M):
    """A k-ordered fp32 multiply-add chain (numpy, products rounded: the unfused case) stays within half of
    chain_bound, i.e. within the bound without its factor 2, on N(0, 1) inputs with W / sqrt(R); and small-
    integer data of the exact tests gives the fp64 product bit for bit."""
    g = torch.Generator().manual_seed(N + R + M)
    A, W, b = _f32(g, N, R), _f32(g, M, R) / R ** 0.5, _f32(g, M)
    mean, istd = _f32(g, R), torch.rand(R, generator=g) + 0.5
    x, w = ((A - mean) * istd).numpy(), W.numpy()
    acc = np.zeros((N, M), dtype=np.float32)
    for k in range(R):
        acc = acc + x[:, k:k + 1] * w[None, :, k]
    acc = acc + b.numpy()[None]
    assert acc.dtype == np.float32
    err = (torch.from_numpy(acc).double() - ref.gemm_ref(A, W, b, mean, istd)).abs()
    assert (err <= 0.5 * ref.chain_bound(R, ref.gemm_mag(A, W, b, mean, istd))).all()
    Ai, Wi = torch.randint(-3, 4, (N, R), generator=g).float(), torch.randint(-3, 4, (M, R), generator=g).float()
    mi = torch.randint(-2, 3, (R,), generator=g).float()
    si = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (R,), generator=g)]
    bi = torch.randint(-3, 4, (M,), generator=g).float()
    x, w = ((Ai - mi) * si).numpy(), Wi.numpy()
    acc = np.zeros((N, M), dtype=np.float32)
    for k in range(R):
        acc = acc + x[:, k:k + 1] * w[None, :, k]
    acc = acc + bi.numpy()[None]
    assert torch.equal(torch.from_numpy(acc).double(), ref.gemm_ref(Ai, Wi, bi, mi, si))
