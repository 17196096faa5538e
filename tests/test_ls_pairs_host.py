"""The line search's pair logic on the host (CPU): a float32 restatement of duck_team.h's quad2 (one alpha)
against one of quad2_pair (the bracket ends al, ah as a pair), statement by statement as the device code has
them, on random and edge rows.

It guards what the pairing can get wrong without a GPU: which row coefficient meets which alpha and which
flag, the friction (Huber) row's zone per half, the order in which the rows are added (one chain per point, as
the scalar form), and the saturating flag's arithmetic (duck_lspairs.h) against x < 0 on the classes the GPU
test feeds the device. An FMA is restated as the exact product and sum in float64 rounded once to float32
(exact for float32 operands up to double rounding, which both restatements share)."""

import numpy as np
import pytest

F = np.float32


def fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def ftz(x):
    x = F(x)
    return F(0.0) * np.sign(x) if x != 0 and abs(x) < F(2.0 ** -126) else x


def flag_select(x):
    return F(1.0) if ftz(x) < 0 else F(0.0)


def flag_sat(x):
    """x times -2^127, clamped to [0, 1], NaN to 0 (the device's clamp), denormal inputs read as 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = ftz(x) * F(-2.0 ** 127)
    if np.isnan(y):
        return F(0.0)
    return F(min(max(y, F(0.0)), F(1.0))) + F(0.0)


def quad2(R, alpha, nrow):
    """duck_team.h quad2 from (0, 0, 0): the friction row's zone, then the one-sided rows in order."""
    alpha = F(alpha)
    x = fma(alpha, R["fv"], R["fja"])
    lo, hi = x <= -R["frf"], x >= R["frf"]
    quad = not (lo or hi)
    sg = F(-1.0) if lo else F(1.0)
    q0 = R["fQ0"] if quad else fma(sg, R["ffja"], R["flin0"])
    q1 = R["fQ1"] if quad else F(sg * R["ffv"])
    q2 = R["fQ2"] if quad else F(0.0)
    for k in range(nrow):
        on = flag_select(fma(alpha, R["v"][k], R["ja"][k]))
        q0, q1, q2 = fma(on, R["Q0"][k], q0), fma(on, R["Q1"][k], q1), fma(on, R["Q2"][k], q2)
    return q0, q1, q2


def quad2_pair(R, alphas, nrow):
    """duck_team.h quad2_pair: every statement over the pair (al, ah); a row's word is the same in both halves."""
    al = np.array(alphas, dtype=F)
    x = np.array([fma(al[h], R["fv"], R["fja"]) for h in range(2)])
    t = np.zeros((3, 2), dtype=F)
    for h in range(2):
        lo, hi = x[h] <= -R["frf"], x[h] >= R["frf"]
        quad = not (lo or hi)
        sg = F(-1.0) if lo else F(1.0)
        t[0, h] = R["fQ0"] if quad else fma(sg, R["ffja"], R["flin0"])
        t[1, h] = R["fQ1"] if quad else F(sg * R["ffv"])
        t[2, h] = R["fQ2"] if quad else F(0.0)
    q = t.copy()
    for k in range(nrow):
        xk = [fma(al[h], R["v"][k], R["ja"][k]) for h in range(2)]
        on = [flag_sat(xk[h]) for h in range(2)]
        for c, Q in enumerate(("Q0", "Q1", "Q2")):
            q[c] = [fma(on[h], R[Q][k], q[c, h]) for h in range(2)]
    return q


def _rows(rng, nrow, edge):
    """Rows2 as set_fric / set_row fill it (float32 statements), from random D, ja, v, f; `edge`: some rows
    exactly at their switch (ja = -alpha v), some with zero or huge entries."""
    D, f = F(rng.uniform(0.5, 50)), F(rng.uniform(0.01, 2))
    ja, v = F(rng.normal()), F(rng.normal())
    rf = F(f * (F(1) / D))
    R = {"fja": ja, "fv": v, "frf": rf, "flin0": F(F(-0.5) * rf * f), "ffja": F(f * ja), "ffv": F(f * v),
         "fQ0": F(F(0.5) * D * ja * ja), "fQ1": F(D * v * ja), "fQ2": F(F(0.5) * D * v * v)}
    Dk = rng.uniform(0, 100, nrow).astype(F)
    jak, vk = rng.normal(size=nrow).astype(F), rng.normal(size=nrow).astype(F)
    if edge:
        jak[0], vk[0] = F(0), F(0)            # a padded row: never active
        jak[1] = F(-F(0.5) * vk[1])           # switches exactly at alpha = 0.5
        jak[2], vk[2] = F(1e30), F(-1e30)
        Dk[3] = F(0)
    with np.errstate(over="ignore"):
        R.update(ja=jak, v=vk, Q0=(F(0.5) * Dk * jak * jak).astype(F), Q1=(Dk * vk * jak).astype(F),
                 Q2=(F(0.5) * Dk * vk * vk).astype(F))
    return R


@pytest.mark.parametrize("nrow", [5, 6])  # NLR + 4: the flat scenes, the scenes with backlash
def test_pair_equals_two_scalar_evaluations(nrow):
    rng = np.random.default_rng(nrow)
    alphas = [(0.0, 1.0), (0.5, 0.25), (-0.3, 2.0), (1e-3, 1e3), (0.5, 0.5)]
    for trial in range(200):
        R = _rows(rng, nrow, edge=trial % 4 == 0)
        pairs = alphas + [tuple(rng.normal(size=2) * 10 ** rng.uniform(-3, 1))]
        # the friction row's switches: x = +-rf exactly on one half, just inside on the other
        if R["fv"] != 0:
            a = F((R["frf"] - R["fja"]) / R["fv"])
            pairs.append((a, F(-a)))
        for al, ah in pairs:
            with np.errstate(over="ignore", invalid="ignore"):
                lo, hi, p = quad2(R, al, nrow), quad2(R, ah, nrow), quad2_pair(R, (al, ah), nrow)
            got = np.array(p, dtype=F).view(np.uint32)
            want = np.array([[lo[c], hi[c]] for c in range(3)], dtype=F).view(np.uint32)
            assert (got == want).all(), (trial, al, ah, got, want)


def test_pair_halves_are_not_swapped():
    """Rows active at al only: their coefficients are in the first half and not in the second."""
    R = _rows(np.random.default_rng(0), 5, edge=False)
    for k in ("fja", "fv", "flin0", "ffja", "ffv", "fQ0", "fQ1", "fQ2"):
        R[k] = F(0.0)                            # (the friction row: quadratic zone, no contribution)
    R["ja"][:], R["v"][:] = F(1.0), F(-1.0)      # x = 1 - alpha: active for alpha > 1
    R["Q0"][:], R["Q1"][:], R["Q2"][:] = F(2.0), F(3.0), F(5.0)
    q = quad2_pair(R, (2.0, 0.5), 5)
    assert q[:, 0].tolist() == [10.0, 15.0, 25.0] and q[:, 1].tolist() == [0.0, 0.0, 0.0]
    q = quad2_pair(R, (0.5, 2.0), 5)
    assert q[:, 1].tolist() == [10.0, 15.0, 25.0] and q[:, 0].tolist() == [0.0, 0.0, 0.0]


def test_saturating_flag_is_x_below_zero():
    U = lambda u: np.array([u], dtype=np.uint32).view(F)[0]
    xs = [0.0, -0.0, U(0x00800000), U(0x80800000), U(1), U(0x80000001), U(0x007FFFFF), U(0x807FFFFF), np.inf, -np.inf,
          np.nan, U(0xFFC00000), 1e-30, -1e-30, 1e30, -1e30, 1.0, -1.0, U(0x7F7FFFFF), U(0xFF7FFFFF)]
    rng = np.random.default_rng(1)
    with np.errstate(over="ignore", under="ignore"):
        xs += list((rng.normal(size=200) * 10.0 ** rng.uniform(-46, 39, 200)).astype(F))
    for x in xs:
        a, b = flag_select(F(x)), flag_sat(F(x))
        assert np.array(a).view(np.uint32) == np.array(b).view(np.uint32), (x, a, b)
