"""The learner kernels (csrc/duck_mlp.hip, csrc/duck_ppo.hip) against the fp64 references of
tests/mlp_reference.py at the shapes where each code path can go wrong (DESIGN.md §8 "Learner kernel tests").

Every GEMM case is compared twice: with small-integer data, for which every product and partial sum is
exactly representable, so the kernel must EQUAL the fp64 reference (a misplaced, dropped or duplicated
element shows whatever its size); and with N(0, 1) data against the a-priori bound of an fp32 chain,
|Y - ref| <= 2 (L + 2) 2^-24 (|op(A)| |W|^T + |b|) per element (mlp_reference.chain_bound: derived, not tuned).
Every output lives in a NaN-filled arena with at least 64 guard floats on both sides, checked after the
launches. Each test prints its measured figures ("[measure] ...") before it asserts.
"""

import math

import pytest
import torch

from tests import mlp_reference as ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
U24 = ref.U24
# Activation epilogues (Y2 = silu(Z), the silu' factor of mode 2; both through __expf): error against the fp64
# function of the kernel's own fp32 Z / aux, in units of 2^-24 max(|value|, TINY). Below TINY the comparison is
# absolute: a subnormal sigmoid (< 2^-126) flushed to zero times |z| <= 2^8 is an absolute error below
# 2^-118 = 2^-24 2^-94. Measured on the MI355X over z = linspace(-30, 30, 6001) and +-88
# (test_activation_epilogues); asserted: 4 x the measured maximum, rounded up to a power of two.
#   silu                 measured 28.9 units   -> 128   (__expf's relative error grows with |z|: the argument
#                                                        z log2(e) is rounded before exp2; 56 units at z ~ -60)
#   silu'                measured 109.5 units  -> 512   (on the grid only: silu' = s (1 + z (1 - s)) has a root at
#                                                        z = -1.2785 where the two terms cancel, so the error in
#                                                        units of the VALUE is unbounded next to it and is only
#                                                        meaningful on fixed points)
#   silu', conditioned   measured 27.06 units  -> 128   (in units of 2^-24 s (1 + |z| (1 - s)), the magnitude of the
#                                                        terms summed: bounded everywhere, used for random aux)
TINY = 2.0 ** -90
SILU_UNITS, DSILU_UNITS, DSILU_COND_UNITS = 128.0, 512.0, 128.0

ENTRIES = ("direct", (64, 32), (64, 64), (32, 32))   # duck_mlp_gemm / duck_mlp_wgrad, or duck_mlp_group_tiles(bm, bn)
ANCHORS = [(65, 101, 33), (33, 36, 65)]              # (N, R, M)
DIM_LISTS = {"N": [1, 31, 32, 33, 63, 64, 65, 97],
             "R": [1, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65, 96, 97, 100, 101, 129],
             "M": [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]}
W_ANCHORS = [(65, 33, 101), (33, 65, 32)]            # weight gradient: (batch rows, M, K)
W_DIM_LISTS = {"rows": [1, 31, 32, 33, 64, 65, 97, 130], "M": [1, 31, 32, 33, 64, 65],
               "K": [1, 3, 4, 31, 32, 33, 63, 64, 65, 101]}


class Arena:
    """Outputs planned first (take), then one NaN-filled device buffer (alloc), then one copy back (fetch) that
    checks every float outside the taken regions -- at least GUARD on both sides of each -- is still NaN."""

    def __init__(self):
        self.pos, self.regions, self.buf = 0, [], None

    def take(self, *shape, off=0, canary=False):
        n = math.prod(shape)
        start = self.pos + GUARD + off
        self.pos = -(-(start + n) // GUARD) * GUARD
        self.regions.append((start, n, shape, canary))
        return len(self.regions) - 1

    def alloc(self, gpu):
        self.buf = torch.full((self.pos + 2 * GUARD,), NAN, dtype=torch.float32, device=gpu)
        return self

    def ptr(self, h):
        return self.buf.data_ptr() + 4 * self.regions[h][0]

    def fetch(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        guard = torch.ones(host.numel(), dtype=torch.bool)
        for start, n, _, canary in self.regions:
            if not canary:
                guard[start:start + n] = False
        assert bool(host[guard].isnan().all()), "a guard float next to an output was written"
        return [host[s:s + n].view(shape) for s, n, shape, _ in self.regions]


def dev(t, gpu, off=0):
    """A host tensor on the device, at element offset `off` of its buffer (off = 1: base off 16-byte alignment)."""
    if t is None:
        return None
    if t.dtype != torch.float32 or off == 0:
        return t.to(gpu)
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=gpu)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _p(x):
    return None if x is None else (x if isinstance(x, int) else x.data_ptr())


def problem(kind, N, R, M, A, W, bias=None, aux=None, Y=None, Y2=None, mean=None, istd=None, splits=0, P=0, off_w=0,
            off_b=0, partial=None):
    from open_duck_playground_amd.native import DuckMlpProblem
    return DuckMlpProblem(kind, N, R, M, _p(A), _p(W), _p(bias), _p(aux), _p(Y), _p(Y2), _p(mean), _p(istd), splits, P,
                          off_w, off_b, _p(partial))


def launch(entry, probs):
    """The problems through the separate entry points, or as one group launch with the tile shape `entry`."""
    from open_duck_playground_amd.native import DuckMlpProblem, check, lib
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    if entry == "direct":
        for p in probs:
            if p.kind < 3:
                check(L.duck_mlp_gemm(p.kind, p.N, p.R, p.M, p.A, p.W, p.bias, p.aux, p.Y, p.Y2, p.mean, p.istd, st))
            else:
                check(L.duck_mlp_wgrad(p.N, p.M, p.R, p.A, p.W, p.mean, p.istd, p.splits, p.partial, p.P, p.off_w,
                                       p.off_b, st))
    else:
        check(L.duck_mlp_group_tiles(len(probs), (DuckMlpProblem * len(probs))(*probs), entry[0], entry[1], st))


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def istd_exact(g, n):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]


def units(got, want, mag=None):
    """max |got - want| in units of 2^-24 max(|want|, TINY) (or of 2^-24 max(mag, TINY))"""
    if got.numel() == 0:
        return 0.0
    return float(((got.double() - want).abs() / (U24 * (want.abs() if mag is None else mag).clamp_min(TINY))).max())


class Measure:
    def __init__(self):
        self.v = {}

    def add(self, key, x):
        self.v[key] = max(self.v.get(key, 0.0), float(x))

    def report(self, what):
        print(f"\n[measure] {what}: " + ", ".join(f"{k} = {v:.4g}" for k, v in sorted(self.v.items())))


# ---- forward and data-gradient GEMMs ---------------------------------------------------------------------
def gemm_inputs(g, N, R, M, exact):
    """Host operands of the six variants of one shape: forward A [N][R], W [M][R]; data gradient dZ [N][R],
    W2 [R][M], aux [N][M]."""
    if exact:
        d = {"A": ints(g, -3, 3, N, R), "W": ints(g, -3, 3, M, R), "b": ints(g, -3, 3, M), "mean": ints(g, -2, 2, R),
             "istd": istd_exact(g, R), "dZ": ints(g, -3, 3, N, R), "W2": ints(g, -3, 3, R, M)}
    else:
        rn = lambda *s: torch.randn(*s, generator=g)
        d = {"A": rn(N, R), "W": rn(M, R) / R ** 0.5, "b": rn(M), "mean": rn(R), "istd": torch.rand(R, generator=g) + 0.5,
             "dZ": rn(N, R), "W2": rn(R, M) / R ** 0.5}
    d["aux"] = 3.0 * torch.randn(N, M, generator=g)
    d["aux0"] = torch.zeros(N, M)
    return d


# (name, mode, normaliser, aux)
VARIANTS = [("m0", 0, False, None), ("m0n", 0, True, None), ("m1", 1, False, None), ("m1n", 1, True, None),
            ("m2z", 2, False, "aux0"), ("m2", 2, False, "aux")]


def run_gemm_shape(gpu, g, N, R, M, exact, meas, off=0):
    """All variants x entry points of one shape; checks against the references; returns the outputs of the
    "direct" entry (for the alignment comparison)."""
    h = gemm_inputs(g, N, R, M, exact)
    d = {k: dev(v, gpu, off) for k, v in h.items()}
    arena, plan = Arena(), {}
    for name, mode, _, _ in VARIANTS:
        for e in ENTRIES:
            plan[name, e] = (arena.take(N, M, off=off), arena.take(N, M, off=off) if mode == 1 else None)
    arena.alloc(gpu)
    for e in ENTRIES:
        probs = []
        for name, mode, norm, aux in VARIANTS:
            y, y2 = plan[name, e]
            mean, istd = (d["mean"], d["istd"]) if norm else (None, None)
            if mode == 2:
                probs.append(problem(2, N, R, M, d["dZ"], d["W2"], aux=d[aux], Y=arena.ptr(y)))
            else:
                probs.append(problem(mode, N, R, M, d["A"], d["W"], bias=d["b"], Y=arena.ptr(y),
                                     Y2=None if y2 is None else arena.ptr(y2), mean=mean, istd=istd))
        if e == "direct":
            launch(e, probs)
        else:   # at most DUCK_MLP_GROUP_MAX problems per launch
            launch(e, probs[:4])
            launch(e, probs[4:])
    out = arena.fetch()
    tag = f"(N, R, M) = {(N, R, M)} exact = {exact} off = {off}"
    direct = {}
    for name, mode, norm, aux in VARIANTS:
        mean, istd = (h["mean"], h["istd"]) if norm else (None, None)
        for e in ENTRIES:
            y, y2 = plan[name, e]
            Y = out[y]
            where = f"{tag} variant {name} entry {e}"
            assert bool(torch.isfinite(Y).all()), where
            if e == "direct":
                direct[name] = (Y, None if y2 is None else out[y2])
            else:   # the tile shapes agree bit for bit with each other and with the separate entry points
                assert torch.equal(Y, direct[name][0]), where
                if y2 is not None:
                    assert torch.equal(out[y2], direct[name][1]), where
            if mode != 2:
                want = ref.gemm_ref(h["A"], h["W"], h["b"], mean, istd)
                if exact:
                    assert torch.equal(Y.double(), want), where
                else:
                    bound = ref.chain_bound(R, ref.gemm_mag(h["A"], h["W"], h["b"], mean, istd))
                    meas.add("gemm err / bound", ((Y.double() - want).abs() / bound).max())
                    assert bool(((Y.double() - want).abs() <= bound).all()), where
                if mode == 1:   # the epilogue against the fp64 function of the kernel's own fp32 Z
                    u = units(out[y2], ref.silu(Y))
                    meas.add("silu units", u)
                    assert SILU_UNITS is None or u <= SILU_UNITS, (where, u)
            elif aux == "aux0":   # silu'(0) = 0.5 exactly: the GEMM factor alone
                want = 0.5 * (h["dZ"].double() @ h["W2"].double())
                if exact:
                    assert torch.equal(Y.double(), want), where
                else:
                    bound = 0.5 * ref.chain_bound(R, h["dZ"].double().abs() @ h["W2"].double().abs())
                    meas.add("dgrad err / bound", ((Y.double() - want).abs() / bound).max())
                    assert bool(((Y.double() - want).abs() <= bound).all()), where
            elif exact:   # the silu' factor: the exact integer GEMM factor divided out
                G = h["dZ"].double() @ h["W2"].double()
                nz = G != 0
                assert bool((Y[~nz] == 0).all()), where
                u = units(Y.double()[nz] / G[nz], ref.dsilu(h["aux"])[nz], ref.dsilu_mag(h["aux"])[nz])
                meas.add("silu' conditioned units", u)
                assert DSILU_COND_UNITS is None or u <= DSILU_COND_UNITS, (where, u)
    return direct


@pytest.mark.parametrize("anchor", [0, 1])
@pytest.mark.parametrize("dim", ["N", "R", "M"])
def test_gemm_edges(gpu, dim, anchor):
    """Modes 0, 1 (with and without the normaliser) and 2 through duck_mlp_gemm and the three tile shapes of
    duck_mlp_group_tiles, one dimension varied over its edge list at an awkward anchor: exact equality on
    integer data, the a-priori chain bound on N(0, 1) data, the tile shapes bit-identical, guards intact.
    R runs 1 .. 5 reduction chunks (odd / even counts, the c + 2 < nch prefetch), R % 4 in {0, 1, 3} (the
    scalar loads), 36 and 100 a vector load followed by a tail; M % 4 != 0 the scalar ColTile path of mode 2.
    Measured on the MI355X: the forward GEMM reaches 0.24 of the bound, the data gradient 0.20."""
    meas = Measure()
    g = torch.Generator().manual_seed(100 * anchor + len(dim) + ord(dim[0]))
    for x in DIM_LISTS[dim]:
        shape = dict(zip("NRM", ANCHORS[anchor]))
        shape[dim] = x
        for exact in (True, False):
            run_gemm_shape(gpu, g, shape["N"], shape["R"], shape["M"], exact, meas)
    meas.report(f"gemm edges {dim} at {ANCHORS[anchor]}")


def test_activation_epilogues(gpu):
    """Y2 = silu(Z) of mode 1 and the silu' factor of mode 2 (both through __expf) against the fp64 functions
    on z = linspace(-30, 30, 6001) and +-88, in units of 2^-24 max(|value|, TINY); at +-100 and +-200 the
    results are finite and equal the limits (silu -> 0 / z, silu' -> 0 / 1). R = 1 with W = 1 makes Z = z
    exactly (asserted), and the mode-2 GEMM factor a small integer that is divided out.
    Measured on the MI355X: silu 28.9 units (asserted 128), silu' 109.5 units (asserted 512), silu' in units
    of its summed terms' magnitude 27.06 (asserted 128): see SILU_UNITS above."""
    grid = torch.cat([torch.linspace(-30, 30, 6001), torch.tensor([88.0, -88.0])])
    lim = torch.tensor([100.0, -100.0, 200.0, -200.0])
    z = torch.cat([grid, lim])
    N = z.numel()
    G = torch.tensor([1.0, 2.0, 3.0, -1.0, -2.0, -3.0]).repeat(N // 6 + 1)[:N]
    one = torch.ones(1, 1)
    d = {k: dev(v, gpu) for k, v in {"z": z.view(N, 1), "G": G.view(N, 1), "one": one}.items()}
    arena, plan = Arena(), {}
    for e in ENTRIES:
        plan[e] = [arena.take(N, 1) for _ in range(3)]
    arena.alloc(gpu)
    for e in ENTRIES:
        zz, y2, dy = (arena.ptr(x) for x in plan[e])
        launch(e, [problem(1, N, 1, 1, d["z"], d["one"], Y=zz, Y2=y2),
                   problem(2, N, 1, 1, d["G"], d["one"], aux=d["z"], Y=dy)])
    out = arena.fetch()
    meas = Measure()
    for e in ENTRIES:
        zz, y2, dy = (out[x].view(-1) for x in plan[e])
        assert torch.equal(zz, z), e
        for a, b in zip(plan[e], plan["direct"]):
            assert torch.equal(out[a], out[b]), e
        assert bool(torch.isfinite(y2).all() and torch.isfinite(dy).all()), e
        n = grid.numel()
        us, ud = units(y2[:n], ref.silu(grid)), units(dy[:n].double() / G[:n].double(), ref.dsilu(grid))
        meas.add("silu units", us)
        meas.add("silu' units", ud)
        meas.add("silu' conditioned units", units(dy[:n].double() / G[:n].double(), ref.dsilu(grid), ref.dsilu_mag(grid)))
        assert torch.equal(y2[n:], torch.tensor([100.0, 0.0, 200.0, 0.0])), (e, y2[n:])
        assert torch.equal(dy[n:] / G[n:], torch.tensor([1.0, 0.0, 1.0, 0.0])), (e, dy[n:])
    meas.report("activation epilogues")
    assert SILU_UNITS is None or meas.v["silu units"] <= SILU_UNITS
    assert DSILU_UNITS is None or meas.v["silu' units"] <= DSILU_UNITS
    assert DSILU_COND_UNITS is None or meas.v["silu' conditioned units"] <= DSILU_COND_UNITS


# ---- the weight gradient -------------------------------------------------------------------------------------
def run_wgrad_case(gpu, g, rows, M, K, splits, norm, exact, meas, off=0):
    """duck_mlp_wgrad and kind 3 of the three tile shapes into NaN-filled partials of splits + 2 rows, P larger
    than the layer (off_w = 5, off_b after a gap), then duck_mlp_wgrad_reduce over the written rows."""
    from open_duck_playground_amd.native import check, lib
    if exact:
        dZ, H = ints(g, -3, 3, rows, M), ints(g, -3, 3, rows, K)
        mean, istd = (ints(g, -2, 2, K), istd_exact(g, K)) if norm else (None, None)
    else:
        dZ, H = torch.randn(rows, M, generator=g), torch.randn(rows, K, generator=g)
        mean, istd = (torch.randn(K, generator=g), torch.rand(K, generator=g) + 0.5) if norm else (None, None)
    off_w, off_b = 5, 5 + M * K + 7
    P = off_b + M + 3
    d = [dev(t, gpu, off) for t in (dZ, H, mean, istd)]
    arena = Arena()
    parts = [arena.take(splits + 2, P, off=off) for _ in ENTRIES]
    grad = arena.take(P, off=off)
    arena.alloc(gpu)
    for e, part in zip(ENTRIES, parts):
        launch(e, [problem(3, rows, K, M, d[0], d[1], mean=d[2], istd=d[3], splits=splits, P=P, off_w=off_w, off_b=off_b,
                           partial=arena.ptr(part))])
    check(lib().duck_mlp_wgrad_reduce(P, splits, arena.ptr(parts[0]), arena.ptr(grad),
                                      torch.cuda.current_stream().cuda_stream))
    out = arena.fetch()
    want, mag, mask = ref.wgrad_ref(dZ, H, mean, istd, splits, P, off_w, off_b)
    rps = -(-rows // splits)
    where = f"(rows, M, K) = {(rows, M, K)} splits = {splits} norm = {norm} exact = {exact} off = {off}"
    for e, part in zip(ENTRIES, parts):
        got = out[part]
        # every float of the buffer outside the layer's entries of rows s < splits is still NaN
        assert bool(got[splits:].isnan().all()) and bool(got[:splits][:, ~mask].isnan().all()), (where, e)
        layer = got[:splits][:, mask]
        assert bool(torch.isfinite(layer).all()), (where, e)     # nothing the kernel failed to write
        assert torch.equal(layer, out[parts[0]][:splits][:, mask]), (where, e)
        if exact:
            assert torch.equal(layer.double(), want[:, mask]), (where, e)
        else:
            bound = ref.chain_bound(rps, mag[:, mask])
            err = (layer.double() - want[:, mask]).abs()
            assert bool((err <= bound).all()), (where, e)
            meas.add("wgrad err / bound", (err / bound.clamp_min(1e-300)).max())
    gr = out[grad][mask].double()
    if exact:
        assert torch.equal(gr, want.sum(0)[mask]), where
    else:
        bound = ref.chain_bound(rps + splits, mag.sum(0)[mask])
        err = (gr - want.sum(0)[mask]).abs()
        assert bool((err <= bound).all()), where
        meas.add("reduced err / bound", (err / bound.clamp_min(1e-300)).max())
    return out[parts[0]][:splits][:, mask], out[grad][mask]


@pytest.mark.parametrize("anchor", [0, 1])
@pytest.mark.parametrize("dim", ["rows", "M", "K"])
def test_wgrad_edges(gpu, dim, anchor):
    """duck_mlp_wgrad and kind 3 of every tile shape against the fp64 per-split reference: equality on integer
    data, the chain bound (L = rows per split; L = rps + splits after duck_mlp_wgrad_reduce) on N(0, 1) data,
    splits 1, 2, 3, 16 and rows + 3 (blocks that are empty or start past the batch write zeros), with and
    without the normaliser, off_w = 5 (not a multiple of 4). K = 31 / 63 put the bias column last in a tile,
    K = 32 / 64 alone in the next one (both tile widths). Unwritten elements cannot hide: the partials start
    as NaN and everything outside the layer's entries must still be NaN afterwards.
    Measured on the MI355X: the partials reach 0.26 of the bound, the reduced gradient 0.12."""
    meas = Measure()
    g = torch.Generator().manual_seed(200 * anchor + len(dim) + ord(dim[0]))
    for x in W_DIM_LISTS[dim]:
        shape = dict(zip(("rows", "M", "K"), W_ANCHORS[anchor]))
        shape[dim] = x
        rows = shape["rows"]
        for splits in (1, 2, 3, 16, rows + 3):
            for norm in (False, True):
                for exact in (True, False):
                    run_wgrad_case(gpu, g, rows, shape["M"], shape["K"], splits, norm, exact, meas)
    meas.report(f"wgrad edges {dim} at {W_ANCHORS[anchor]}")


def test_misaligned_bases_give_the_same_bits(gpu):
    """Every input and output base pointer one float off 16-byte alignment (leading dimensions still multiples
    of 4, so only the base-alignment test of the loads' vector path decides): the scalar fall-back loads give
    the same bits as the aligned run, for each kind and entry point, and the references still hold."""
    meas = Measure()
    for exact in (True, False):
        runs = []
        for off in (0, 1):
            g = torch.Generator().manual_seed(31)
            a = run_gemm_shape(gpu, g, 33, 36, 64, exact, meas, off=off)
            b = run_wgrad_case(gpu, g, 33, 64, 36, 3, True, exact, meas, off=off)
            runs.append((a, b))
        (a0, b0), (a1, b1) = runs
        for name in a0:
            for x, y in zip(a0[name], a1[name]):
                assert (x is None and y is None) or torch.equal(x, y), name
        assert torch.equal(b0[0], b1[0]) and torch.equal(b0[1], b1[1])
    meas.report("misaligned bases")


@pytest.mark.parametrize("empty_at", [None, 0, 2, 3])
def test_group_of_four_kinds(gpu, empty_at):
    """Kinds 1, 2, 3 and 0 with four different shapes in one launch, for each tile shape, equal to the fp64
    references on integer data; and the group with an N = 0 forward problem first, in the middle and last (a
    zero-tile problem makes equal entries in start[]): every output matches and the empty problem's outputs
    stay NaN. A group holds at most DUCK_MLP_GROUP_MAX = 4 problems, so the empty problem takes the place of
    the kind-0 one."""
    g = torch.Generator().manual_seed(77)
    h1 = gemm_inputs(g, 65, 101, 33, True)
    h2 = gemm_inputs(g, 33, 36, 65, True)
    h0 = gemm_inputs(g, 31, 5, 17, True)
    rows, M, K, splits = 97, 33, 31, 3
    dZ, H, mean, istd = ints(g, -3, 3, rows, M), ints(g, -3, 3, rows, K), ints(g, -2, 2, K), istd_exact(g, K)
    off_w, off_b = 5, 5 + M * K + 7
    P = off_b + M + 3
    d1, d2, d0 = ({k: dev(v, gpu) for k, v in h.items()} for h in (h1, h2, h0))
    dw = [dev(t, gpu) for t in (dZ, H, mean, istd)]
    want3, _, mask = ref.wgrad_ref(dZ, H, mean, istd, splits, P, off_w, off_b)
    for e in ENTRIES[1:]:
        arena = Arena()
        z1, y1, y2, part = arena.take(65, 33), arena.take(65, 33), arena.take(33, 65), arena.take(splits + 2, P)
        y0 = arena.take(31, 17)
        ye, ye2 = arena.take(1, 8, canary=True), arena.take(1, 8, canary=True)
        arena.alloc(gpu)
        probs = [problem(1, 65, 101, 33, d1["A"], d1["W"], bias=d1["b"], Y=arena.ptr(z1), Y2=arena.ptr(y1),
                         mean=d1["mean"], istd=d1["istd"]),
                 problem(2, 33, 36, 65, d2["dZ"], d2["W2"], aux=d2["aux0"], Y=arena.ptr(y2)),
                 problem(3, rows, K, M, dw[0], dw[1], mean=dw[2], istd=dw[3], splits=splits, P=P, off_w=off_w,
                         off_b=off_b, partial=arena.ptr(part))]
        if empty_at is None:
            probs.append(problem(0, 31, 5, 17, d0["A"], d0["W"], bias=d0["b"], Y=arena.ptr(y0)))
        else:
            probs.insert(empty_at, problem(1, 0, 5, 8, d0["A"], d0["W"], bias=d0["b"], Y=arena.ptr(ye), Y2=arena.ptr(ye2)))
        launch(e, probs)
        out = arena.fetch()
        Z1 = ref.gemm_ref(h1["A"], h1["W"], h1["b"], h1["mean"], h1["istd"])
        assert torch.equal(out[z1].double(), Z1), e
        u = units(out[y1], ref.silu(out[z1]))
        assert SILU_UNITS is None or u <= SILU_UNITS, (e, u)
        assert torch.equal(out[y2].double(), 0.5 * (h2["dZ"].double() @ h2["W2"].double())), e
        assert torch.equal(out[part][:splits][:, mask].double(), want3[:, mask]), e
        assert bool(out[part][splits:].isnan().all()) and bool(out[part][:splits][:, ~mask].isnan().all()), e
        if empty_at is None:
            assert torch.equal(out[y0].double(), ref.gemm_ref(h0["A"], h0["W"], h0["b"])), e
        else:
            assert bool(out[y0].isnan().all() and out[ye].isnan().all() and out[ye2].isnan().all()), e


# ---- the loss kernels ------------------------------------------------------------------------------------
def loss_inputs(g, N, A):
    """A minibatch whose ratios rho span [0.5, 1.6] (clip range 0.8 .. 1.2), with a few pre-softplus logits
    above 20 (the softplus branch) and a few raw actions at +-9 (tanh saturation in the log-det-Jacobian).
    The raw actions are loc + scale e, e ~ 1.5 N(0, 1), as a rollout produces them (the saturated ones around a
    loc near +-9): the log-probability stays O(A), so fp32 can represent rho. (raw independent of the logits
    puts |z| = |raw - loc| / scale near 100 on some entries, the log-probability in the thousands and 1e-4 of
    rounding into rho: two equivalent fp32 evaluations then differ by luck, not by correctness.)"""
    rn = lambda *s: torch.randn(*s, generator=g)
    logits = rn(N, 2 * A)
    logits[::7, A] = 22.5
    logits[2::13, 2 * A - 1] = 31.0
    sat = torch.zeros(N, A, dtype=torch.bool)
    sat[::5, 0] = True
    sat[3::11, A - 1] = True
    sign = torch.where(torch.arange(N)[:, None] % 2 == 0, 1.0, -1.0).expand(N, A)
    loc, pre = logits[:, :A], logits[:, A:]
    loc[sat] = (9.0 * sign + 0.3 * rn(N, A))[sat]
    pre[sat & (pre < 20)] = 0.5
    scale = torch.nn.functional.softplus(pre.double()) + ref.MIN_STD
    raw = (loc.double() + scale * 1.5 * rn(N, A).double()).float()
    raw[sat] = (9.0 * sign)[sat]
    lp = ref.normal_tanh_log_prob(logits, raw)
    olp = (lp - torch.log(torch.linspace(0.5, 1.6, N, dtype=torch.float64))).float()
    return [logits, raw, olp, rn(N), rn(N), rn(N), rn(N, A)]   # .., advantage, value_target, baseline, eps


def run_loss(gpu, ins, N, A, clip, ent_cost, normalize):
    from open_duck_playground_amd.native import check, lib
    L = lib()
    d = [t.to(gpu) for t in ins]
    arena = Arena()
    o, gl, gb = arena.take(L.duck_ppo_loss_out_size(N)), arena.take(N, 2 * A), arena.take(N)
    arena.alloc(gpu)
    check(L.duck_ppo_loss(N, A, *(t.data_ptr() for t in d), clip, ent_cost, int(normalize), arena.ptr(o), arena.ptr(gl),
                          arena.ptr(gb), torch.cuda.current_stream().cuda_stream))
    out = arena.fetch()
    return out[o][:4], out[gl], out[gb]


@pytest.mark.parametrize("A", [1, 13, 16, 17, 31])
def test_ppo_loss_matches_fp64_autograd(gpu, A):
    """duck_ppo_loss -- the team kernel for A <= 16, the one-thread-per-sample kernel (dynamic LDS, in-place
    gradient rows) for 16 < A <= 31 -- against the fp64 autograd reference: out[0..3], grad_logits and
    grad_baseline, N in {1, 15, 16, 17, 127, 128, 129, 300}, normalize_advantage 0 and 1.

    Tolerance: the same torch expression evaluated in fp32 on the host gives each output's fp32 noise floor,
    and the kernel may be 8 x that away (another, equivalent fp32 evaluation order; fast expf / log1pf).
    Gradients, per element: |gpu - ref| <= 8 (floor + 2^-24 |ref|), floor = the largest distance of the host's
    fp32 gradient from the fp64 one over the tensor. The four scalars: the same form, with floor = the larger
    of |fp32 - fp64| of the scalar itself and the RMS sum of the per-sample terms' fp32 errors,
    sqrt(sum_i (t32_i - t64_i)^2) / N. The distance of ONE fp32 evaluation of a mean from fp64 is a single
    draw of that noise and lands near zero by chance (measured: 1.4e-9 for a loss whose terms carry 1e-5 of
    rho's rounding each, against which a correct kernel's 5.4e-7 would "fail" 8 x floor by a factor 49); the
    RMS of the terms' errors is the scale those draws come from.

    Measured on the MI355X, largest over N and normalize (floor | GPU error | error / allowed):
      A = 13 (team)    loss 2.8e-6 | 1.9e-6 | 0.30   entropy 1.6e-6 | 2.2e-6 | 0.16   grad_logits 2.1e-5 | 1.3e-5 | 0.42
      A = 16 (team)    loss 3.5e-7 | 5.4e-7 | 0.21   entropy 2.5e-6 | 2.9e-6 | 0.17   grad_logits 4.3e-6 | 3.5e-6 | 0.69
      A = 17 (thread)  loss 1.4e-6 | 1.6e-6 | 0.24   entropy 2.4e-6 | 3.9e-6 | 0.27   grad_logits 1.6e-5 | 2.0e-5 | 0.34
      A = 31 (thread)  loss 2.0e-6 | 2.0e-6 | 0.25   entropy 2.1e-6 | 8.2e-6 | 0.15   grad_logits 3.0e-5 | 2.1e-5 | 0.28
      grad_baseline: floor 1.5e-8 .. 6.0e-8, the same as the GPU error (0.11 of the allowed error)."""
    meas = Measure()
    g = torch.Generator().manual_seed(1000 + A)
    bad = []
    for N in (1, 15, 16, 17, 127, 128, 129, 300):
        for normalize in (0, 1):
            ins = loss_inputs(g, N, A)
            r64 = ref.ppo_loss_ref(*ins, 0.2, 0.005, normalize)
            r32 = ref.ppo_loss_ref(*ins, 0.2, 0.005, normalize, dtype=torch.float32)
            o, gl, gb = run_loss(gpu, ins, N, A, 0.2, 0.005, normalize)
            rms = ((r32["terms"].double() - r64["terms"]) ** 2).sum(1).sqrt() / N
            rms = [float(rms[0] + rms[1] + 0.005 * rms[2])] + [float(x) for x in rms]
            for k, name in enumerate(("loss", "policy", "value", "entropy")):
                floor = max(abs(float(r32["out"][k]) - float(r64["out"][k])), rms[k])
                err = abs(float(o[k]) - float(r64["out"][k]))
                meas.add(f"{name} floor", floor)
                meas.add(f"{name} err", err)
                allowed = 8 * (floor + U24 * abs(float(r64["out"][k])))
                meas.add(f"{name} err / allowed", err / allowed if allowed > 0 else (0.0 if err == 0 else float("inf")))
                if not err <= allowed:
                    bad.append((N, normalize, name, err, floor))
            for name, got in (("grad_logits", gl), ("grad_baseline", gb)):
                w = r64[name]
                floor = float((r32[name].double() - w).abs().max())
                allowed = 8 * (floor + U24 * w.abs())
                err = (got.double() - w).abs()
                ok = allowed > 0
                ratio = float((err[ok] / allowed[ok]).max()) if bool(ok.any()) else 0.0
                meas.add(f"{name} floor", floor)
                meas.add(f"{name} err", err.max())
                meas.add(f"{name} err / allowed", ratio)
                if not bool((err <= allowed).all()):
                    bad.append((N, normalize, name, float(err.max()), floor))
    meas.report(f"ppo loss A = {A}")
    assert not bad, bad


@pytest.mark.parametrize("A", [13, 31])
@pytest.mark.parametrize("normalize", [0, 1])
def test_ppo_loss_clipped_rows_are_exactly_zero(gpu, A, normalize):
    """With entropy_cost = 0 every sample the surrogate clips (rho > 1 + eps with positive normalised
    advantage, rho < 1 - eps with negative) has an exactly zero grad_logits row, and no unclipped sample with
    a non-zero advantage has one; both kernels. Samples within 1e-3 of a clip edge or with |advantage| < 1e-3
    are left unclassified (fp32 rho carries ~1e-5 of error there)."""
    N, clip = 300, 0.2
    ins = loss_inputs(torch.Generator().manual_seed(5 + A), N, A)
    r64 = ref.ppo_loss_ref(*ins, clip, 0.0, normalize)
    _, gl, _ = run_loss(gpu, ins, N, A, clip, 0.0, normalize)
    rho, an = r64["rho"], r64["adv_n"]
    sure = ((rho - (1 + clip)).abs() > 1e-3) & ((rho - (1 - clip)).abs() > 1e-3) & (an.abs() > 1e-3)
    clipped = ((rho > 1 + clip) & (an > 0)) | ((rho < 1 - clip) & (an < 0))
    zero_row = (gl == 0).all(1)
    assert int((sure & clipped).sum()) > 20 and int((sure & ~clipped).sum()) > 20
    assert bool(zero_row[sure & clipped].all())
    assert not bool(zero_row[sure & ~clipped].any())
    assert bool((r64["grad_logits"][sure & clipped] == 0).all())     # the reference agrees on which rows vanish


def test_ppo_loss_rejects_action_size_32(gpu):
    from open_duck_playground_amd.native import lib
    L = lib()
    N, A = 16, 32
    ins = [t.to(gpu) for t in loss_inputs(torch.Generator().manual_seed(1), N, A)]
    out = torch.full((L.duck_ppo_loss_out_size(N),), NAN, device=gpu)
    gl, gb = torch.full((N, 2 * A), NAN, device=gpu), torch.full((N,), NAN, device=gpu)
    assert L.duck_ppo_loss(N, A, *(t.data_ptr() for t in ins), 0.2, 0.005, 1, out.data_ptr(), gl.data_ptr(),
                           gb.data_ptr(), torch.cuda.current_stream().cuda_stream) < 0
    torch.cuda.synchronize()
    assert bool(out.isnan().all() and gl.isnan().all() and gb.isnan().all())


# ---- the sampler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [12345, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("ctr0", [0, 3])
def test_policy_sample_stream_is_pinned(gpu, ctr0, seed):
    """duck_policy_sample draws eps from threefry2x32 keyed by the seed's two words at counter (row,
    8 ctr + pair), Box-Muller, element 2 pair the cosine draw and 2 pair + 1 the sine draw: eps recovered as
    (raw - loc) / scale with fp64 loc / scale equals the host restatement to 2e-5 (derived: the fp32 argument
    2 pi u2 carries 2 pi 2^-24 of rounding, times r <= 5.7 is 2.1e-6; logf, sqrtf, sincosf add ~1e-6; 2e-5 is
    ~6 x that, and a wrong counter or a swapped draw misses by O(1)), scaled by 1 / scale where scale < 1
    (the subtraction raw - loc cancels). log-prob against the fp64 NormalTanh log-probability of the returned
    raw within 8 (floor + 2^-24 |ref|), floor = the largest distance of the fp32 host expression from fp64;
    the counter advances by exactly 1; rows >= N of the outputs stay untouched (NaN guards).
    Measured on the MI355X: eps err 0.052 of the allowed 2e-5 (1.0e-6); log-prob floor 1.6e-5, GPU error 2.1e-5,
    0.18 of the allowed error."""
    from open_duck_playground_amd.native import check, lib
    meas = Measure()
    for N, A in ((1, 1), (257, 13), (300, 16), (64, 14)):
        g = torch.Generator().manual_seed(N + A)
        logits = torch.randn(N, 2 * A, generator=g)
        logits[::9, A] = 21.5             # pre > 20: the softplus branch
        logits[1::17, 2 * A - 1] = 25.0
        dl = logits.to(gpu)
        ctr = torch.tensor([ctr0], dtype=torch.int32, device=gpu)
        arena = Arena()
        raw, lp, act = arena.take(N, A), arena.take(N), arena.take(N, A)
        arena.alloc(gpu)
        check(lib().duck_policy_sample(N, A, dl.data_ptr(), seed, ctr.data_ptr(), arena.ptr(raw), arena.ptr(lp),
                                       arena.ptr(act), torch.cuda.current_stream().cuda_stream))
        out = arena.fetch()
        assert int(ctr.item()) == ctr0 + 1
        raw, lp, act = out[raw], out[lp], out[act]
        loc = logits[:, :A].double()
        scale = torch.nn.functional.softplus(logits[:, A:].double()) + ref.MIN_STD
        eps = (raw.double() - loc) / scale
        want = torch.from_numpy(ref.sample_eps_ref(N, A, seed, ctr0))
        allowed = 2e-5 / scale.clamp(max=1.0)
        err = (eps - want).abs()
        meas.add("eps err / allowed", (err / allowed).max())
        assert bool((err <= allowed).all()), (N, A, float((err / allowed).max()))
        assert float((act.double() - torch.tanh(raw.double())).abs().max()) <= 1e-6
        l64 = ref.normal_tanh_log_prob(logits, raw)
        floor = float((ref.normal_tanh_log_prob(logits, raw, dtype=torch.float32).double() - l64).abs().max())
        allowed = 8 * (floor + U24 * l64.abs())
        err = (lp.double() - l64).abs()
        meas.add("logprob floor", floor)
        meas.add("logprob err", err.max())
        meas.add("logprob err / allowed", (err / allowed).max())
        assert bool((err <= allowed).all()), (N, A, float((err / allowed).max()))
    meas.report(f"policy sample seed {seed:#x} ctr {ctr0}")
