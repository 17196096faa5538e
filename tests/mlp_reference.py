"""fp64 references of the learner kernels (csrc/duck_mlp.hip, csrc/duck_ppo.hip; include/duck_ppo.h), in
plain torch / numpy on the host. The GPU tests (test_gpu_mlp_kernels.py) compare the kernels with these;
test_mlp_reference.py checks the references themselves against torch.autograd, ppo.ppo_loss and the
Random123 vectors, so they are validated on a machine with no GPU.

Inputs are the fp32 host tensors the kernels are given. The only fp32 arithmetic here is op(A): the
normaliser is evaluated with the kernel's expression in fp32 (IEEE subtraction and multiplication give the
same bits on the host), then everything is widened to fp64.
"""

import math

import numpy as np
import torch

U24 = 2.0 ** -24     # the unit roundoff of fp32
MIN_STD = 1e-3       # ppo.MIN_STD: scale = softplus(pre) + MIN_STD


# ---- the MLP layers -----------------------------------------------------------------------------------
def op_norm(A: torch.Tensor, mean=None, istd=None) -> torch.Tensor:
    """op(A) = (A - mean) * istd per column in fp32 (the kernel's expression), widened to fp64."""
    assert A.dtype == torch.float32
    if mean is None:
        return A.double()
    return ((A - mean) * istd).double()


def gemm_ref(A, W, bias=None, mean=None, istd=None) -> torch.Tensor:
    """Z [N][M] = op(A) [N][R] W^T + b, W [M][R] (modes 0 and 1)."""
    Z = op_norm(A, mean, istd) @ W.double().t()
    return Z if bias is None else Z + bias.double()


def gemm_mag(A, W, bias=None, mean=None, istd=None) -> torch.Tensor:
    """|op(A)| |W|^T + |b|: the magnitude the a-priori error bound of the fp32 chain scales with."""
    Z = op_norm(A, mean, istd).abs() @ W.double().abs().t()
    return Z if bias is None else Z + bias.double().abs()


def chain_bound(L: int, mag: torch.Tensor) -> torch.Tensor:
    """2 (L + 2) 2^-24 mag: the a-priori bound of an fp32 multiply-add chain of length L (the factor 2
    covers an unfused product), per element."""
    return 2.0 * (L + 2) * U24 * mag


def silu(z: torch.Tensor) -> torch.Tensor:
    z = z.double()
    return z * torch.sigmoid(z)


def dsilu(z: torch.Tensor) -> torch.Tensor:
    """silu'(z) = s (1 + z (1 - s)), s = sigmoid(z)"""
    z = z.double()
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def dsilu_mag(z: torch.Tensor) -> torch.Tensor:
    """s (1 + |z| (1 - s)) >= |silu'(z)|: the magnitude of the terms silu' sums. For z < 0 they cancel (silu' has
    a root at z = -1.2785), so an fp32 evaluation's error scales with this, not with the value."""
    z = z.double()
    s = torch.sigmoid(z)
    return s * (1.0 + z.abs() * (1.0 - s))


def dgrad_ref(dZ, W, aux) -> torch.Tensor:
    """(dZ [N][R] W [R][M]) * silu'(aux [N][M]) (mode 2)."""
    return (dZ.double() @ W.double()) * dsilu(aux)


def wgrad_blocks(dZ, H, mean, istd, splits: int):
    """dW [splits][M][K], db [splits][M] of the row blocks of rps = ceil(N / splits) rows (blocks past the
    batch are zero), and the magnitudes |dZ|^T |op(H)|, sum |dZ| of the same blocks."""
    N, M = dZ.shape
    K = H.shape[1]
    rps = -(-N // splits)
    pad = splits * rps - N
    d = torch.cat([dZ.double(), torch.zeros(pad, M, dtype=torch.float64)]).view(splits, rps, M)
    h = torch.cat([op_norm(H, mean, istd), torch.zeros(pad, K, dtype=torch.float64)]).view(splits, rps, K)
    dW = torch.einsum("srm,srk->smk", d, h)
    mW = torch.einsum("srm,srk->smk", d.abs(), h.abs())
    return dW, d.sum(1), mW, d.abs().sum(1)


def wgrad_ref(dZ, H, mean, istd, splits: int, P: int, off_w: int, off_b: int):
    """The partial array duck_mlp_wgrad writes: part [splits][P] (zero outside the layer), the magnitude
    array of the same layout, and the boolean mask [P] of the layer's M K + M entries."""
    M, K = dZ.shape[1], H.shape[1]
    dW, db, mW, mb = wgrad_blocks(dZ, H, mean, istd, splits)
    part = torch.zeros(splits, P, dtype=torch.float64)
    mag = torch.zeros(splits, P, dtype=torch.float64)
    mask = torch.zeros(P, dtype=torch.bool)
    part[:, off_w:off_w + M * K], mag[:, off_w:off_w + M * K] = dW.reshape(splits, -1), mW.reshape(splits, -1)
    part[:, off_b:off_b + M], mag[:, off_b:off_b + M] = db, mb
    mask[off_w:off_w + M * K] = True
    mask[off_b:off_b + M] = True
    return part, mag, mask


# ---- the PPO loss ----------------------------------------------------------------------------------------
def _ldj(x):
    return 2.0 * (math.log(2.0) - x - torch.nn.functional.softplus(-2.0 * x))


def normal_tanh_log_prob(logits, raw, dtype=torch.float64) -> torch.Tensor:
    """brax NormalTanhDistribution.log_prob of pre-tanh actions raw [N][A] under logits [N][2A]."""
    logits, raw = logits.to(dtype), raw.to(dtype)
    A = raw.shape[-1]
    loc, scale = logits[..., :A], torch.nn.functional.softplus(logits[..., A:]) + MIN_STD
    z = (raw - loc) / scale
    return (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2 * math.pi) - _ldj(raw)).sum(-1)


def ppo_loss_ref(logits, raw_action, old_logprob, advantage, value_target, baseline, eps, clip_eps, entropy_cost,
                 normalize, dtype=torch.float64):
    """include/duck_ppo.h duck_ppo_loss in `dtype` torch with autograd. Returns a dict: out [4] = {loss,
    policy, value, entropy}, grad_logits [N][2A], grad_baseline [N] (d out[0] / d .), and rho [N], adv_n [N]
    (the probability ratio and the normalised advantage, for the clip classification), terms [3][N] (the
    per-sample terms whose means are policy, value, entropy)."""
    lg = logits.detach().to(dtype).clone().requires_grad_(True)
    bl = baseline.detach().to(dtype).clone().requires_grad_(True)
    ra, olp, adv, vs, ep = (t.detach().to(dtype) for t in (raw_action, old_logprob, advantage, value_target, eps))
    A = ra.shape[-1]
    loc, scale = lg[:, :A], torch.nn.functional.softplus(lg[:, A:]) + MIN_STD
    z = (ra - loc) / scale
    lp = (-0.5 * z * z - torch.log(scale) - 0.5 * math.log(2 * math.pi) - _ldj(ra)).sum(-1)
    if normalize:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    rho = torch.exp(lp - olp)
    s1, s2 = rho * adv, torch.clamp(rho, 1.0 - clip_eps, 1.0 + clip_eps) * adv
    t_policy, t_value = -torch.minimum(s1, s2), 0.25 * (vs - bl) ** 2
    t_entropy = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(scale) + _ldj(loc + scale * ep)).sum(-1)
    policy, value, entropy = t_policy.mean(), t_value.mean(), t_entropy.mean()
    loss = policy + value - entropy_cost * entropy
    loss.backward()
    return {"out": torch.stack([loss, policy, value, entropy]).detach(), "grad_logits": lg.grad, "grad_baseline": bl.grad,
            "rho": rho.detach(), "adv_n": adv.detach(), "terms": torch.stack([t_policy, t_value, t_entropy]).detach()}


# ---- the sampler's stream -----------------------------------------------------------------------------
_ROT = (13, 15, 26, 6, 17, 29, 16, 24)


def threefry2x32(k0, k1, c0, c1):
    """threefry2x32 with 20 rounds (Salmon et al. 2011, Random123), vectorised over uint32 numpy arrays."""
    M32 = np.uint64(0xFFFFFFFF)
    k0, k1, x0, x1 = (np.asarray(v, dtype=np.uint64) & M32 for v in (k0, k1, c0, c1))
    ks = (k0, k1, np.uint64(0x1BD11BDA) ^ k0 ^ k1)
    x0, x1 = (x0 + ks[0]) & M32, (x1 + ks[1]) & M32
    for r in range(20):
        x0 = (x0 + x1) & M32
        rot = np.uint64(_ROT[r % 8])
        x1 = ((x1 << rot) | (x1 >> (np.uint64(32) - rot))) & M32
        x1 = x1 ^ x0
        if r % 4 == 3:
            s = r // 4 + 1
            x0 = (x0 + ks[s % 3]) & M32
            x1 = (x1 + ks[(s + 1) % 3] + np.uint64(s)) & M32
    return x0.astype(np.uint32), x1.astype(np.uint32)


def sample_eps_ref(N: int, A: int, seed: int, ctr: int) -> np.ndarray:
    """The standard normal draws eps [N][A] (fp64) of duck_policy_sample: threefry2x32 keyed by the seed's
    (low, high) words at counter (row, 8 ctr + pair); Box-Muller with u1 = ((a >> 9) + 1) / 2^23 in (0, 1],
    u2 = (b >> 9) / 2^23; element 2 pair is the cosine draw and 2 pair + 1 the sine draw."""
    npair = (A + 1) // 2
    row = np.repeat(np.arange(N, dtype=np.uint64), npair)
    pair = np.tile(np.arange(npair, dtype=np.uint64), N)
    a, b = threefry2x32(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, row, (np.uint64(8 * ctr) + pair))
    u1 = ((a >> np.uint32(9)).astype(np.float64) + 1.0) / 2.0 ** 23
    u2 = (b >> np.uint32(9)).astype(np.float64) / 2.0 ** 23
    r = np.sqrt(-2.0 * np.log(u1))
    e = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=-1)  # [N npair][2]
    return e.reshape(N, 2 * npair)[:, :A]
