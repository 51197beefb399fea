"""Independent references for the relational core: GROUP BY encoding, equi-join
matching and the grouped aggregates. Plain Python ints and floats, written from
the SQL definitions, importing nothing from the code under test.

Conventions shared with the code under test, and only these:
* the operator names of ``ops/agg.py`` (sum_int, sum_f64, count, min_int,
  max_int, min_f64, max_f64, and_int, or_int, xor_int);
* a group without a (non-NULL) row keeps the operator's identity: 0 for the
  sums and COUNT, INT64_MAX / INT64_MIN for integer MIN / MAX, +inf / -inf for
  f64 MIN / MAX, -1 / 0 / 0 for AND / OR / XOR;
* f64 MIN / MAX use the total order -inf < ... < +inf < NaN, a NaN of either
  sign and any payload being the one greatest value;
* rows whose group id lies outside [0, ngroups) belong to no group;
* NULL join keys match nothing.
"""
import math

from window_ref import fkey, same_f64, U  # noqa: F401  (re-exported for the tests)

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
OPS = ("sum_int", "sum_f64", "count", "min_int", "max_int", "min_f64", "max_f64", "and_int", "or_int", "xor_int")


def group_ref(keys):
    """(groups, first): ``groups`` lists, in order of first occurrence, the rows
    (ascending) of every distinct key; ``first`` is each group's first row."""
    rows = {}
    for i, k in enumerate(keys):
        rows.setdefault(int(k), []).append(i)
    groups = list(rows.values())          # dicts keep insertion order: first occurrence
    return groups, [g[0] for g in groups]


def join_ref(build, bvalid, probe, pvalid):
    """(counts, pairs, matched): matches per probe row, the set of (probe row,
    build row) pairs with equal non-NULL keys, and the set of build rows some
    probe row matched."""
    rows = {}
    for r, k in enumerate(build):
        if bvalid is None or bvalid[r]:
            rows.setdefault(int(k), []).append(r)
    counts, pairs, matched = [0] * len(probe), set(), set()
    for j, k in enumerate(probe):
        if pvalid is not None and not pvalid[j]:
            continue
        hit = rows.get(int(k), ())
        counts[j] = len(hit)
        for r in hit:
            pairs.add((j, r))
        matched.update(hit)
    return counts, pairs, matched


def _fsum(xs):
    """math.fsum extended to the non-finite sums IEEE addition defines."""
    if any(x != x for x in xs):
        return math.nan
    pos, neg = math.inf in xs, -math.inf in xs
    if pos or neg:
        return math.nan if pos and neg else (math.inf if pos else -math.inf)
    return math.fsum(xs)


def agg_ref(gid, ngroups, op, vals, valid, n=None):
    """Per-group state of one aggregate over the rows with a group id in
    [0, ngroups) and (for every operator, COUNT included) a true ``valid``.
    ``gid`` None: one group of every row. Integer results are exact Python
    ints (a SUM may exceed 64 bits; bit operations work on the value as a
    signed 64-bit integer, i.e. an int32 source sign-extended). sum_f64
    returns ``(fsum, sum of |x|, terms)`` lists for the error bound. ``n``:
    the row count, needed only when gid, vals and valid are all None."""
    g = max(ngroups, 1)
    if n is None:
        n = len(next(a for a in (gid, vals, valid) if a is not None))
    per = [[] for _ in range(g)]
    for i in range(n):
        k = 0 if gid is None else int(gid[i])
        if gid is not None and not 0 <= k < ngroups:
            continue
        if valid is not None and not valid[i]:
            continue
        per[k].append(1 if vals is None else vals[i])
    if op == "count":
        return [len(p) for p in per]
    if op == "sum_f64":
        per = [[float(x) for x in p] for p in per]
        return ([_fsum(p) if p else 0.0 for p in per],
                [math.fsum(abs(x) for x in p) if all(math.isfinite(x) for x in p) else math.inf for p in per],
                [len(p) for p in per])
    if op in ("min_f64", "max_f64"):
        pick, ident = (min, math.inf) if op == "min_f64" else (max, -math.inf)
        out = []
        for p in per:
            x = pick((float(x) for x in p), key=fkey, default=ident)
            out.append(math.nan if x != x else x)
        return out
    per = [[int(x) for x in p] for p in per]
    if op == "sum_int":
        return [sum(p) for p in per]
    if op == "min_int":
        return [min(p, default=I64_MAX) for p in per]
    if op == "max_int":
        return [max(p, default=I64_MIN) for p in per]
    out = []
    for p in per:      # Python's bit operators act on the infinite two's complement: exact for int64 values
        acc = -1 if op == "and_int" else 0
        for x in p:
            acc = acc & x if op == "and_int" else (acc | x if op == "or_int" else acc ^ x)
        out.append(acc)
    return out


def sum_bound(absum, terms):
    """Largest |computed - exact| of a float64 sum of ``terms`` values taken in
    ANY order (Higham, Accuracy and Stability, eq. 4.4): gamma_(t-1) * sum|x|."""
    t = max(terms - 1, 0)
    return t * U / (1.0 - t * U) * absum
