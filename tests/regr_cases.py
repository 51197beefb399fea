"""Oracle and tolerance of the regr_* tests (tests/test_regr.py,
tests/test_regr_gpu.py).

The oracle is exact rational arithmetic (``fractions.Fraction``) over the
exact binary values of the inputs, rounded to double at the end; it shares
nothing with either engine path.

Tolerance, for groups of at most ``MAX_PAIRS`` = 2048 pairs. The GPU kernel sums
values shifted by K, a sample of the group, so (K - mean)^2 <= sum((x -
mean)^2) and the condition number of M2 = Sxx - Sx^2 / n against the
well-conditioned centred sum is at most 1 + n. With u = 2^-53 and any
summation order a sum of n terms carries a relative error of at most n u, so
M2x, M2y and Cxy are within about n (1 + n) u of the exact values: below 5e-10
for n <= 2048. ``RTOL`` = 1e-9 is about twice that, for the finaliser's few
extra operations. Cxy may legitimately be near 0 (its terms cancel), so it
also gets 1e-9 * sum(|x - mx| |y - my|) as an absolute bound. regr_slope and
regr_r2 are quotients of those moments: the same RTOL. regr_intercept = my -
slope * mx gets RTOL * (|my| + |slope * mx|) as an absolute bound. A mean is K
+ S / n with |x - K| <= 2 max|x - mean|, so its error is at most 2 u |mean| +
2 n u max|x - mean|: RTOL * (|mean| + max|x - mean|) covers it by orders of
magnitude. The CPU engine's two-pass sums are better conditioned still and
are held to the same bounds.
"""
import math
from fractions import Fraction

RTOL = 1e-9
MAX_PAIRS = 2048
FUNCS = ("regr_count", "regr_avgx", "regr_avgy", "regr_sxx", "regr_syy", "regr_sxy", "regr_slope",
         "regr_intercept", "regr_r2")


def oracle(ys, xs):
    """{function: (exact value as a Fraction or None for NULL, absolute bound)}
    over the pairs of ``ys`` / ``xs`` (floats or None) with neither side None."""
    pairs = [(Fraction(x), Fraction(y)) for y, x in zip(ys, xs) if x is not None and y is not None]
    n = len(pairs)
    assert n <= MAX_PAIRS, "the tolerance is derived for groups of at most 2048 pairs"
    out = {"regr_count": (Fraction(n), 0.0)}
    if n == 0:
        out.update({f: (None, 0.0) for f in FUNCS[1:]})
        return out
    mx = sum(x for x, _ in pairs) / n
    my = sum(y for _, y in pairs) / n
    m2x = sum((x - mx) ** 2 for x, _ in pairs)
    m2y = sum((y - my) ** 2 for _, y in pairs)
    cxy = sum((x - mx) * (y - my) for x, y in pairs)
    devx = max(abs(x - mx) for x, _ in pairs)
    devy = max(abs(y - my) for _, y in pairs)
    out["regr_avgx"] = (mx, RTOL * float(abs(mx) + devx))
    out["regr_avgy"] = (my, RTOL * float(abs(my) + devy))
    out["regr_sxx"] = (m2x, RTOL * float(m2x))
    out["regr_syy"] = (m2y, RTOL * float(m2y))
    out["regr_sxy"] = (cxy, RTOL * float(abs(cxy)) + RTOL * float(sum(abs(x - mx) * abs(y - my) for x, y in pairs)))
    if n < 2 or m2x == 0:
        out.update({f: (None, 0.0) for f in ("regr_slope", "regr_intercept", "regr_r2")})
        return out
    slope = cxy / m2x
    out["regr_slope"] = (slope, RTOL * float(abs(slope)))
    out["regr_intercept"] = (my - slope * mx, RTOL * float(abs(my) + abs(slope * mx)))
    r2 = Fraction(1) if m2y == 0 else cxy * cxy / (m2x * m2y)
    out["regr_r2"] = (r2, RTOL * float(r2))
    return out


def mismatches(got: dict, want: dict, where="") -> list:
    """Messages for every function of ``got`` ({function: value or None})
    outside its bound of ``want`` (an ``oracle`` result)."""
    bad = []
    for f, v in got.items():
        exact, bound = want[f]
        if exact is None or v is None:
            if exact is not None or v is not None:
                bad.append(f"{where}{f}: got {v!r}, want {None if exact is None else float(exact)!r}")
            continue
        if f == "regr_count":
            if int(v) != exact:
                bad.append(f"{where}{f}: got {v!r}, want {int(exact)}")
            continue
        err = abs(Fraction(float(v)) - exact) if math.isfinite(float(v)) else math.inf
        if not err <= bound:
            bad.append(f"{where}{f}: got {v!r}, want {float(exact)!r} (error {float(err):.3g} > bound {bound:.3g})")
    return bad


def select_list(y="y", x="x", funcs=FUNCS) -> str:
    return ", ".join(f"{f}({y}, {x}) as {f}" for f in funcs)
