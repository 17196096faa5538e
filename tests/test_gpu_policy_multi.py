"""duck_policy_act_multi (include/duck_ppo.h; DESIGN.md §9 "Policies"): K policies in one launch, a policy per
16-row tile. The contract is bit identity with duck_policy_act called per segment with that segment's parameters
alone, so every comparison is of int32 views. Outputs live in the NaN arena of test_gpu_mlp_kernels.py (guards
checked on fetch): a row outside a segment, or a word outside [0, N) rows, that was written shows there."""

import ctypes as C

import pytest
import torch

from tests.test_gpu_evaluator import EINVAL, _lib, _ptr, _stream, policy_act
from tests.test_gpu_mlp_kernels import Arena, dev

pytestmark = pytest.mark.gpu

NETS = [(101, 512, 256, 128, 28), (5, 33, 17, 6)]
# an empty segment, one shorter than a tile, exactly a tile, one row over, and boundaries off multiples of 16 (a
# tile's padding rows are a neighbour's real rows); then the same with the empty segment last
LAYOUTS = [(0, 1, 15, 16, 17, 33), (1, 15, 16, 17, 33, 0)]
ORDERS = (0, 1)   # policy-major, dealt over the XCDs


def policy_act_multi(N, seg, sizes, W, b, mean, istd, obs, logits, action, K=None):
    K = len(seg) - 1 if K is None else K
    return _lib().duck_policy_act_multi(N, K, (C.c_int * len(seg))(*seg), len(sizes) - 1, (C.c_int * len(sizes))(*sizes),
                                        (C.c_void_p * len(W))(*[_ptr(w) for w in W]),
                                        (C.c_void_p * len(b))(*[_ptr(x) for x in b]), _ptr(mean), _ptr(istd), _ptr(obs),
                                        _ptr(logits), _ptr(action), _stream())


@pytest.fixture
def order():
    """Sets the block order for a test and puts back the one that held."""
    was = _lib().duck_policy_multi_order(-1)
    yield lambda o: _lib().duck_policy_multi_order(o)
    _lib().duck_policy_multi_order(was)


def _params(sizes, K, g, gpu):
    """K distinct policies stacked [K][...]: weights, biases, normalisers."""
    nl = len(sizes) - 1
    W = [dev(torch.randn(K, sizes[i + 1], sizes[i], generator=g) / sizes[i] ** 0.5, gpu) for i in range(nl)]
    b = [dev(0.3 * torch.randn(K, sizes[i + 1], generator=g), gpu) for i in range(nl)]
    mean = dev(torch.randn(K, sizes[0], generator=g), gpu)
    istd = dev(torch.rand(K, sizes[0], generator=g) + 0.5, gpu)
    return W, b, mean, istd


def _per_segment(seg, sizes, W, b, mean, istd, obs, gpu):
    """duck_policy_act per segment with that policy's parameters alone: (logits [N][M], action [N][A])."""
    N, M = seg[-1], sizes[-1]
    logits, action = torch.zeros(N, M, device=gpu), torch.zeros(N, M // 2, device=gpu)
    for k in range(len(seg) - 1):
        n = seg[k + 1] - seg[k]
        if n == 0:
            continue
        lg, ac = torch.empty(n, M, device=gpu), torch.empty(n, M // 2, device=gpu)
        assert policy_act(n, sizes, [w[k] for w in W], [x[k] for x in b], None if mean is None else mean[k],
                          None if istd is None else istd[k], obs[seg[k]:seg[k + 1]].contiguous(), lg, ac) == 0
        logits[seg[k]:seg[k + 1]], action[seg[k]:seg[k + 1]] = lg, ac
    return logits.cpu(), action.cpu()


@pytest.mark.parametrize("lengths", LAYOUTS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("sizes", NETS, ids=lambda s: "-".join(map(str, s)))
def test_segments_equal_policy_act_bit_for_bit(gpu, order, sizes, lengths):
    """Six policies with distinct weights and normalisers over segments of 0, 1, 15, 16, 17 and 33 rows: every row
    carries the bits duck_policy_act gives it with its own policy alone, with and without the normaliser, under
    both block orders (which give identical bits), and logits = NULL writes the same actions."""
    g = torch.Generator().manual_seed(sum(sizes) + lengths[0])
    K, A = len(lengths), sizes[-1] // 2
    seg = [0]
    for n in lengths:
        seg.append(seg[-1] + n)
    N = seg[-1]
    W, b, mean, istd = _params(sizes, K, g, gpu)
    obs = dev(2.0 * torch.randn(N, sizes[0], generator=g), gpu)
    for norm in (False, True):
        mn, sd = (mean, istd) if norm else (None, None)
        want_lg, want_ac = _per_segment(seg, sizes, W, b, mn, sd, obs, gpu)
        for o in ORDERS:
            order(o)
            arena = Arena()
            lg, ac, ac2 = arena.take(N, sizes[-1]), arena.take(N, A), arena.take(N, A)
            arena.alloc(gpu)
            assert policy_act_multi(N, seg, sizes, W, b, mn, sd, obs, arena.ptr(lg), arena.ptr(ac)) == 0
            assert policy_act_multi(N, seg, sizes, W, b, mn, sd, obs, None, arena.ptr(ac2)) == 0
            out = arena.fetch()
            where = f"sizes {sizes} lengths {lengths} norm {norm} order {o}"
            assert bool(torch.isfinite(out[lg]).all()) and bool(torch.isfinite(out[ac]).all()), where
            assert torch.equal(out[lg].view(torch.int32), want_lg.view(torch.int32)), where
            assert torch.equal(out[ac].view(torch.int32), want_ac.view(torch.int32)), where
            assert torch.equal(out[ac2].view(torch.int32), want_ac.view(torch.int32)), where
    # the policies are distinct: policy 0's parameters on another segment's rows give other bits
    k = max(range(K), key=lambda j: lengths[j])
    if k != 0:
        n = lengths[k]
        lg0, ac0 = torch.empty(n, sizes[-1], device=gpu), torch.empty(n, A, device=gpu)
        assert policy_act(n, sizes, [w[0] for w in W], [x[0] for x in b], mean[0], istd[0],
                          obs[seg[k]:seg[k + 1]].contiguous(), lg0, ac0) == 0
        assert not torch.equal(lg0.cpu().view(torch.int32), want_lg[seg[k]:seg[k + 1]].view(torch.int32))


@pytest.mark.parametrize("N", [1, 16, 17, 130])
def test_one_policy_equals_policy_act(gpu, order, N):
    sizes = NETS[0]
    g = torch.Generator().manual_seed(N)
    W, b, mean, istd = _params(sizes, 1, g, gpu)
    obs = dev(2.0 * torch.randn(N, sizes[0], generator=g), gpu)
    want_lg, want_ac = _per_segment([0, N], sizes, W, b, mean, istd, obs, gpu)
    for o in ORDERS:
        order(o)
        arena = Arena()
        lg, ac = arena.take(N, sizes[-1]), arena.take(N, sizes[-1] // 2)
        arena.alloc(gpu)
        assert policy_act_multi(N, [0, N], sizes, W, b, mean, istd, obs, arena.ptr(lg), arena.ptr(ac)) == 0
        out = arena.fetch()
        assert torch.equal(out[lg].view(torch.int32), want_lg.view(torch.int32)), (N, o)
        assert torch.equal(out[ac].view(torch.int32), want_ac.view(torch.int32)), (N, o)


def test_many_policies_of_a_few_rows(gpu, order):
    """64 policies (the limit) of 3 rows each, and 9 policies of 20: more policies than lanes in the dealt order, a
    lane holding several policies, every tile a part tile."""
    sizes = NETS[1]
    for K, n in ((64, 3), (9, 20)):
        g = torch.Generator().manual_seed(K)
        seg = [n * k for k in range(K + 1)]
        N = seg[-1]
        W, b, mean, istd = _params(sizes, K, g, gpu)
        obs = dev(2.0 * torch.randn(N, sizes[0], generator=g), gpu)
        want_lg, want_ac = _per_segment(seg, sizes, W, b, mean, istd, obs, gpu)
        for o in ORDERS:
            order(o)
            arena = Arena()
            lg, ac = arena.take(N, sizes[-1]), arena.take(N, sizes[-1] // 2)
            arena.alloc(gpu)
            assert policy_act_multi(N, seg, sizes, W, b, mean, istd, obs, arena.ptr(lg), arena.ptr(ac)) == 0
            out = arena.fetch()
            assert torch.equal(out[lg].view(torch.int32), want_lg.view(torch.int32)), (K, o)
            assert torch.equal(out[ac].view(torch.int32), want_ac.view(torch.int32)), (K, o)


def test_refusals_leave_a_canary_untouched(gpu):
    """Every refused call returns DUCK_EINVAL with a message and launches nothing: the output buffers, NaN canaries
    of the arena, keep every word. N == 0 is accepted and launches nothing either."""
    sizes, N = (4, 8, 4), 4
    z = torch.zeros(3 * 8 * 8, device=gpu)
    ok = [z, z]
    arena = Arena()
    lg, ac = arena.take(N, 4, canary=True), arena.take(N, 2, canary=True)
    arena.alloc(gpu)
    L = _lib()

    def refused(seg, K=None, W=ok, b=ok, mean=None, istd=None, sizes=sizes, n=N):
        rc = policy_act_multi(n, seg, sizes, W, b, mean, istd, z, arena.ptr(lg), arena.ptr(ac), K=K)
        return rc == EINVAL and b"duck_policy_act_multi" in L.duck_last_error()
    assert refused([0, 4], K=0)
    assert refused([0] * 65 + [4], K=65)
    assert refused([1, 4])                      # seg[0] != 0
    assert refused([0, 3, 2, 4])                # decreasing
    assert refused([0, 2, 3])                   # seg[K] != N
    assert refused([0, 2, 5])
    assert refused([0, 4], W=[z, None])         # a null layer pointer
    assert refused([0, 4], b=[None, z])
    assert refused([0, 4], mean=z)              # mean without istd
    assert refused([0, 4], sizes=(4, 513, 4))   # duck_policy_act's own refusals
    assert refused([0, 4], sizes=(4, 8, 3))
    assert policy_act_multi(0, [0, 0, 0], sizes, ok, ok, None, None, z, arena.ptr(lg), arena.ptr(ac)) == 0
    out = arena.fetch()   # (the canary regions are checked with the guards: all NaN)
    assert bool(out[lg].isnan().all()) and bool(out[ac].isnan().all())
