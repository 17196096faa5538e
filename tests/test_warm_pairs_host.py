"""The warm start's pair logic on the host (CPU): a float32 restatement of duck_team.h's scalar row costs
(fric_cost, side_cost, the limit row's J.x - aref) against one of their pair forms in warm_rows_pair (.x at
qacc_warmstart, .y at qacc_smooth), statement by statement as the device code has them.

The device helpers are members of the step kernel's template and use the device reciprocal, so they do not
compile on the host; this restates them, as tests/test_ls_pairs_host.py does for the line search. Both sides are
restatements in Python: the test checks the pairing as a piece of logic (which start's word meets which half, the
Huber zone and the activity test per half, a lane past the last row whose cost is dropped), on random and edge
inputs. It does not run the device code and cannot see its operand order or its contractions; those are held by
tests/test_gpu_warm_pairs.py, word for word against the scalar build on the GPU. An FMA is the exact product and
sum in float64 rounded once to float32 (exact for float32 operands up to double rounding, which both
restatements share)."""

import numpy as np

F = np.float32
U = lambda u: np.array([u], dtype=np.uint32).view(F)[0]


def fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def fric_cost(D, x, f):
    """duck_team.h fric_cost as the parent compiles it (profiles/r15_contraction_points.txt)."""
    rf = F(f * (F(1) / D))
    t = F(F(F(0.5) * rf) * f)
    lo, hi, qd = fma(x, -f, -t), fma(f, x, -t), F(F(F(F(0.5) * D) * x) * x)
    r = hi if x >= rf else qd
    return lo if x <= -rf else r


def side_cost(D, jx):
    return F(F(F(F(0.5) * D) * jx) * jx) if jx < 0 else F(0.0)


def rows_scalar(row, x):
    """One start: the friction row and one limit row at qacc x (the lane's dof value), summed in order."""
    D, f, ar, lD, sg, lar, ok = row
    c = fric_cost(D, F(x - ar), f)
    jl = fma(sg, x, -lar)
    return F(c + (side_cost(lD, jl) if ok else F(0.0))), F(x - ar), jl


def rows_pair(row, w, q):
    """warm_rows_pair: every statement over the pair (w, q); the rows' words are the same in both halves."""
    D, f, ar, lD, sg, lar, ok = row
    x = np.array([w, q], dtype=F)
    j = (x - ar).astype(F)
    rf = F(f * (F(1) / D))
    t = F(F(F(0.5) * rf) * f)
    hD = F(F(0.5) * D)
    lo = np.array([fma(j[h], -f, -t) for h in range(2)])
    hi = np.array([fma(f, j[h], -t) for h in range(2)])
    qd = ((hD * j).astype(F) * j).astype(F)
    c = np.zeros(2, dtype=F)
    for h in range(2):
        r = hi[h] if j[h] >= rf else qd[h]
        c[h] = lo[h] if j[h] <= -rf else r
    jl = np.array([fma(x[h], sg, -lar) for h in range(2)])
    ql = ((F(F(0.5) * lD) * jl).astype(F) * jl).astype(F)
    c = (c + np.array([ql[h] if ok and jl[h] < 0 else F(0.0) for h in range(2)], dtype=F)).astype(F)
    return c, j, jl


def _same(a, b):
    return np.array(a, dtype=F).view(np.uint32) == np.array(b, dtype=F).view(np.uint32)


def test_pair_equals_two_scalar_evaluations():
    rng = np.random.default_rng(15)
    edge = [F(0.0), F(-0.0), F(np.inf), F(-np.inf), F(np.nan), U(0x00800000), U(0x80800000), F(1e30), F(-1e30)]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for trial in range(400):
            D, f = F(rng.uniform(0.5, 50)), F(rng.uniform(0.01, 2))
            ar, lar = F(rng.normal()), F(rng.normal() * 10)
            row = (D, f, ar, F(rng.uniform(0, 100)), F(rng.choice([-1.0, 1.0])), lar, bool(trial % 3))
            rf = F(f * (F(1) / D))
            # the zone boundaries x - ar = +-rf and one ulp either side, the limit row's switch, random and edge values
            xs = [F(rng.normal() * 3), F(rng.normal() * 0.1)]
            for b in (F(ar + rf), F(ar - rf), F(row[4] * lar)):
                xs += [b, np.nextafter(b, F(np.inf)), np.nextafter(b, F(-np.inf))]
            xs += [edge[trial % len(edge)]]
            for w in xs:
                for q in (xs[0], xs[(trial + 3) % len(xs)]):
                    cw, jw, lw = rows_scalar(row, F(w))
                    cs, js, ls = rows_scalar(row, F(q))
                    c, j, jl = rows_pair(row, F(w), F(q))
                    assert _same(c, [cw, cs]).all(), (trial, w, q, c, cw, cs)
                    assert _same(j, [jw, js]).all() and _same(jl, [lw, ls]).all(), (trial, w, q)


def test_pair_halves_are_not_swapped():
    """A limit row active at the warm start only: its cost is in the first half and not in the second."""
    row = (F(1.0), F(100.0), F(0.0), F(2.0), F(1.0), F(0.0), True)  # (a wide quadratic zone: the Huber cost is 0.5 D x^2)
    c, j, jl = rows_pair(row, F(-3.0), F(4.0))
    assert c.tolist() == [4.5 + 9.0, 8.0] and jl.tolist() == [-3.0, 4.0]
    c, _, _ = rows_pair(row, F(4.0), F(-3.0))
    assert c.tolist() == [8.0, 4.5 + 9.0]
    c, _, _ = rows_pair(row[:6] + (False,), F(-3.0), F(-3.0))  # a lane past the last limit row: its cost is dropped
    assert c.tolist() == [4.5, 4.5]


def test_nan_start_stays_in_its_half():
    row = (F(2.0), F(0.5), F(0.1), F(3.0), F(-1.0), F(0.2), True)
    with np.errstate(invalid="ignore"):
        c, j, jl = rows_pair(row, F(np.nan), F(0.7))
        cs, js, ls = rows_scalar(row, F(0.7))
    assert np.isnan(c[0]) and np.isnan(j[0]) and np.isnan(jl[0])
    assert _same([c[1], j[1], jl[1]], [cs, js, ls]).all()
