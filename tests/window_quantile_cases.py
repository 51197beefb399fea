"""Shared cases of the framed order statistics (median / percentile_cont /
percentile_disc / approx_* OVER a frame): the table, the statements and a
plain-Python oracle that sorts every frame. tests/test_window_quantile.py runs
them on the CPU engine, tests/test_window_quantile_gpu.py on the device."""
import bisect
import math
import random
import struct
from decimal import Decimal

import pyarrow as pa

NAN, INF = float("nan"), float("inf")


def make_rows(n_small=300, long_part=0, seed=11):
    """Rows (dicts): id unique; k the partition (never NULL); o an int order key
    with ties; xi / xd / xf int64 / decimal(12,2) / float64 values with NULLs, xf
    also NaN, +-inf and -0.0; g a flag for FILTER. ``long_part`` rows more in one
    extra partition (k = 9)."""
    rng = random.Random(seed)
    rows = []
    for i in range(n_small + long_part):
        k = rng.randrange(5) if i < n_small else 9
        xi = rng.randrange(-50, 50) if rng.random() > 0.2 else None
        xd = Decimal(rng.randrange(-99999, 99999)).scaleb(-2) if rng.random() > 0.2 else None
        r = rng.random()
        xf = None if r < 0.2 else NAN if r < 0.25 else INF if r < 0.28 else -INF if r < 0.31 else \
            -0.0 if r < 0.35 else 0.0 if r < 0.39 else round(rng.uniform(-100, 100), 3)
        rows.append({"id": i, "k": k, "o": rng.randrange(0, 40) if i < n_small else rng.randrange(0, long_part // 3 + 1),
                     "xi": xi, "xd": xd, "xf": xf, "g": rng.randrange(3)})
    # partition 4 starts with a stretch of NULLs in every value column: frames wholly inside it are empty of values
    for r in rows:
        if r["k"] == 4 and r["o"] < 8:
            r["xi"] = r["xd"] = r["xf"] = None
    rng.shuffle(rows)
    return rows


def table(rows):
    return pa.table({"id": pa.array([r["id"] for r in rows], pa.int64()),
                     "k": pa.array([r["k"] for r in rows], pa.int32()),
                     "o": pa.array([r["o"] for r in rows], pa.int64()),
                     "xi": pa.array([r["xi"] for r in rows], pa.int64()),
                     "xd": pa.array([r["xd"] for r in rows], pa.decimal128(12, 2)),
                     "xf": pa.array([r["xf"] for r in rows], pa.float64()),
                     "g": pa.array([r["g"] for r in rows], pa.int32())})


# ------------------------------------------------------------------ statements
#: (unit, start, end): a bound is "up" / "uf" / "cur" / ("p", k) / ("f", k)
FRAMES = [
    ("rows", "up", "cur"), ("rows", ("p", 2), ("f", 3)), ("rows", "cur", "uf"), ("rows", "up", "uf"),
    ("rows", ("p", 40), "cur"), ("rows", ("p", 3), ("p", 1)), ("rows", ("f", 1), ("f", 2)), ("rows", "cur", "cur"),
    ("rows", ("p", 16), ("f", 15)), ("rows", ("p", 16), ("f", 16)),
    ("range", "up", "cur"), ("range", ("p", 5), ("f", 5)), ("range", "cur", "uf"), ("range", ("p", 3), "cur"),
    ("range", "cur", ("f", 4)), ("range", ("p", 6), ("p", 2)), ("range", "up", "uf"),
    ("groups", ("p", 1), ("f", 1)), ("groups", "up", "cur"), ("groups", "cur", "uf"), ("groups", ("p", 2), "cur"),
    ("groups", "cur", ("f", 1)), ("groups", ("p", 2), ("p", 1)), ("groups", ("f", 1), "uf"),
]
#: (function, column, q)
CALLS = [("median", "xi", None), ("median", "xd", None), ("median", "xf", None), ("approx_median", "xf", None),
         ("percentile_cont", "xf", 0.25), ("percentile_cont", "xi", 0.5), ("percentile_cont", "xd", 1),
         ("approx_percentile_cont", "xf", 0), ("approx_percentile_cont", "xd", 0.25),
         ("percentile_disc", "xi", 0.25), ("percentile_disc", "xf", 0.5), ("percentile_disc", "xd", 1),
         ("percentile_disc", "xf", 0)]


def _bound(b):
    if isinstance(b, tuple):
        return f"{b[1]} {'preceding' if b[0] == 'p' else 'following'}"
    return {"up": "unbounded preceding", "uf": "unbounded following", "cur": "current row"}[b]


def frame_sql(fr):
    unit, s, e = fr
    return f"{unit} between {_bound(s)} and {_bound(e)}"


def call_sql(fn, col, q, flt=None):
    args = col if q is None else f"{col}, {q}"
    return f"{fn}({args})" + (f" filter (where {flt})" if flt else "")


def over_sql(fr, partition=True, order=True):
    """ROWS frames order by (o, id) so the row order is fixed; RANGE and GROUPS
    frames hold whole peer groups, so ORDER BY o is enough."""
    p = "partition by k " if partition else ""
    if not order:
        return f"over ({p})"
    o = "order by o, id " if fr[0] == "rows" else "order by o "
    return f"over ({p}{o}{frame_sql(fr)})"


def statement(fr, calls=CALLS, partition=True, flt=None):
    sel = ", ".join(f"{call_sql(fn, col, q, flt)} {over_sql(fr, partition)} as c{j}"
                    for j, (fn, col, q) in enumerate(calls))
    return f"select id, {sel} from t"


# ------------------------------------------------------------------ oracle
def f64_key(x: float) -> int:
    """The total order of the window MIN / MAX: -inf < .. < -0.0 < +0.0 < .. < +inf < NaN."""
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else b ^ (2**63 - 1)


def _trunc_half(s: int) -> int:
    return abs(s) // 2 * (1 if s >= 0 else -1)


def stat(fn, q, vals):
    """vals: the frame's non-NULL values (int, Decimal or float), unsorted."""
    c = len(vals)
    if c == 0:
        return None
    fl = isinstance(vals[0], float)
    dec = isinstance(vals[0], Decimal)
    vs = sorted(vals, key=f64_key) if fl else sorted(vals)
    if fn in ("median", "approx_median"):
        a, b = vs[(c - 1) // 2], vs[c // 2]
        if fl:
            return (a + b) / 2
        if dec:
            ex = a.as_tuple().exponent
            return Decimal(_trunc_half(int(a.scaleb(-ex)) + int(b.scaleb(-ex)))).scaleb(ex)
        return _trunc_half(a + b)
    if fn in ("percentile_cont", "approx_percentile_cont"):
        pos = (c - 1) * float(q)
        k0 = math.floor(pos)
        k1 = min(k0 + 1, c - 1)
        v0, v1 = float(vs[k0]), float(vs[k1])
        return v0 + (v1 - v0) * (pos - k0)
    assert fn == "percentile_disc"
    return vs[max(math.ceil(c * float(q)) - 1, 0)]


def frames_of(rows, fr, partition=True, order=True):
    """{id: (sorted partition, a, z)}: the frame of row id is partition[a:z]."""
    unit, s, e = fr if order else (None, None, None)      # no ORDER BY: the frame is the partition
    parts = {}
    for r in rows:
        parts.setdefault(r["k"] if partition else 0, []).append(r)
    out = {}
    for part in parts.values():
        if not order:
            for r in part:
                out[r["id"]] = (part, 0, len(part))
            continue
        part = sorted(part, key=lambda r: (r["o"], r["id"]))
        if unit == "rows":
            key = list(range(len(part)))
        elif unit == "range":
            key = [r["o"] for r in part]
        else:
            distinct = sorted({r["o"] for r in part})
            key = [distinct.index(r["o"]) for r in part]

        def edge(b, me, low):
            if b == "up":
                return -math.inf
            if b == "uf":
                return math.inf
            if b == "cur":
                return me
            return me - b[1] if b[0] == "p" else me + b[1]
        for i, r in enumerate(part):
            # the keys ascend along the sorted partition, so the rows with a <= key <= z are one slice
            a, z = edge(s, key[i], True), edge(e, key[i], False)
            out[r["id"]] = (part, bisect.bisect_left(key, a), bisect.bisect_right(key, z))
    return out


def expected(rows, fr, calls=CALLS, partition=True, order=True, keep=lambda r: True):
    """{id: [value per call]}"""
    fm = frames_of(rows, fr, partition, order)
    out, seen = {}, {}
    for r in rows:
        part, a, z = fm[r["id"]]
        at = (id(part), a, z)           # rows sharing a frame (a whole partition) share its statistics
        if at not in seen:
            frame = part[a:z]
            seen[at] = [stat(fn, q, [x[col] for x in frame if x[col] is not None and keep(x)]) for fn, col, q in calls]
        out[r["id"]] = seen[at]
    return out


def same(a, b) -> bool:
    """Exact equality: NaN equals NaN, -0.0 differs from +0.0, a type never equals another."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        if not (isinstance(a, float) and isinstance(b, float)):
            return False
        return (a != a and b != b) or struct.pack("<d", a) == struct.pack("<d", b)
    return type(a) is type(b) and a == b


def mismatches(got_rows, want, what=""):
    """got_rows: the statement's to_pylist(); want: expected()."""
    bad = []
    assert sorted(r["id"] for r in got_rows) == sorted(want)
    for r in got_rows:
        for j, w in enumerate(want[r["id"]]):
            if not same(r[f"c{j}"], w):
                bad.append(f"{what}id={r['id']} c{j}: got {r[f'c{j}']!r} want {w!r}")
    return bad
