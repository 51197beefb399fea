"""Times of the two-operand string kernels (csrc/kernels/strpair.hip),
BASELINE.md's "String pair functions" table.

    python scripts/strpair_bench.py [--rows 4000000] [--reps 9] [--device cuda:0]

The table holds ``rows`` rows built on the device: two plain string columns
``c1`` / ``c2`` of TPC-H-comment-like text (lower-case words, 10 to 117
bytes), a plain column ``nd`` of three-letter needles and a dictionary column
``d`` over 25 one-letter entries. Each case sums its result, so the output is
one row and the time is the kernel's, not the export's:

    (a) sum(levenshtein(c1, c2))          edit distance, both sides per row
    (b) sum(strpos(c1, nd))               per-row needle (strpair.hip)
    (c) sum(strpos(c1, 'lit'))            literal needle (strfunc.hip, the yardstick of (b))
    (d) sum(find_in_set(d, 'a,b,c'))      dictionary column against a constant set

Every statement runs 2 untimed and ``reps`` timed executions; the time is
taken with device events around ``engine.sql`` and ends in a synchronise.
Prints one JSON line: per case the result, median / min / max milliseconds
and the host steps per execution, the (b)/(c) ratio and the effective GB/s of
(a) (offsets and bytes of both operands read plus the int32 results written)."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rows", type=int, default=4_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
sys.path.insert(0, a.tree)

import pyarrow as pa  # noqa: E402
import torch  # noqa: E402
import igloo_amd as ig  # noqa: E402
from igloo_amd import types as T  # noqa: E402
from igloo_amd.columnar import Column  # noqa: E402
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS  # noqa: E402

if a.device != "cpu" and not torch.cuda.is_available():
    sys.exit("no GPU: a time taken elsewhere says nothing about the device path")
dev = torch.device(a.device)
WARMUP = 2
n = a.rows
g = torch.Generator(device=dev)
g.manual_seed(7)


def text(lo: int, hi: int, space_every: int) -> Column:
    """Plain string column of ``n`` rows, lo..hi random lower-case bytes each,
    about one space per ``space_every`` bytes."""
    lens = torch.randint(lo, hi + 1, (n,), generator=g, device=dev, dtype=torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    chars = torch.randint(ord("a"), ord("z") + 1, (total,), generator=g, device=dev, dtype=torch.int64)
    if space_every:
        gap = torch.randint(0, space_every, (total,), generator=g, device=dev)
        chars = torch.where(gap == 0, torch.full_like(chars, ord(" ")), chars)
    return Column(T.UTF8, chars.to(torch.uint8), None, offsets=off)


c1, c2, nd = text(10, 117, 6), text(10, 117, 6), text(3, 3, 0)
entries = Column.from_arrow(pa.array([chr(ord("a") + i) for i in range(25)], pa.large_string()), device=dev,
                            dict_encode=False)
d = Column(T.UTF8, torch.randint(0, 25, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.int32), None,
           dictionary=entries)
e = ig.QueryEngine(device=a.device)
e.register_table("t", {"c1": c1, "c2": c2, "nd": nd, "d": d})
CASES = {
    "a_levenshtein": ("sum(levenshtein(c1, c2))", "str_lev"),
    "b_strpos_per_row": ("sum(strpos(c1, nd))", "str_pair"),
    "c_strpos_literal": ("sum(strpos(c1, 'lit'))", "str_fn_int"),
    "d_find_in_set_dict": ("sum(find_in_set(d, 'a,b,c'))", None),
}


def timed(sql):
    h0, times, res = sum(HOST_STEPS.values()), [], None
    for i in range(WARMUP + a.reps):
        if dev.type == "cuda":
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            res = e.sql(sql).table.to_pylist()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1)
        else:
            import time
            w0 = time.perf_counter()
            res = e.sql(sql).table.to_pylist()
            ms = (time.perf_counter() - w0) * 1e3
        if i >= WARMUP:
            times.append(ms)
    return {"result": res[0]["s"], "ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
            "ms_max": round(max(times), 3), "host_steps_per_run": (sum(HOST_STEPS.values()) - h0) / (WARMUP + a.reps)}


out = {"package": ig.__file__, "rows": n, "reps": a.reps, "device": a.device}
for name, (expr, kernel) in CASES.items():
    calls = KERNEL_CALLS[kernel] if kernel else 0
    out[name] = timed(f"select {expr} s from t")
    assert kernel is None or dev.type != "cuda" or KERNEL_CALLS[kernel] > calls, name
traffic = 2 * (n + 1) * 8 + c1.data.numel() + c2.data.numel() + 4 * n
out["a_bytes"] = traffic
out["a_gb_per_s"] = round(traffic / (out["a_levenshtein"]["ms_median"] * 1e-3) / 1e9, 2)
out["a_dp_cells"] = int(((c1.offsets[1:] - c1.offsets[:-1]) * (c2.offsets[1:] - c2.offsets[:-1])).sum())
out["b_over_c"] = round(out["b_strpos_per_row"]["ms_median"] / out["c_strpos_literal"]["ms_median"], 3)
print(json.dumps(out))
