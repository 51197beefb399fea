"""regr_slope(y, x) on the shifted-moments kernel against corr(y, x) on the
five-sum path, over float64 pairs resident in HBM: grouped by a key of
``--groups`` values and global.
   python scripts/bench_regr.py [--rows 100000000] [--groups 1000] [--reps 10] [--only NAME]
Prints the mean wall time per statement (host clock around a device
synchronise) after warm-up, the statements alternating. Query graphs are off so
a kernel trace of the same command (rocprofv3 --kernel-trace --stats) lists
each path's kernels; ``--only`` runs one statement for such a trace.
Bytes the aggregate itself moves per row: regr_* 16 B read (x, y); corr 40 B
read (x, y, x*y, x*x, y*y) + 24 B written (the three products) + the
products' own 48 B of reads; both also read 4 B of group id when grouped."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("IGLOO_GRAPHS", "0")     # (read when the package is imported)

import torch  # noqa: E402

import igloo_amd as ig  # noqa: E402
from igloo_amd import types as T  # noqa: E402
from igloo_amd.catalog import MemoryTable  # noqa: E402
from igloo_amd.columnar import Column  # noqa: E402
from igloo_amd.ops._lib import KERNEL_CALLS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    n = a.rows
    x = torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * 1000.0
    y = 3.0 * x - 7.0 + torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
    k = torch.randint(0, a.groups, (n,), device=dev, generator=gen, dtype=torch.int64)
    e = ig.QueryEngine(device=dev)
    e.register_table("t", MemoryTable({"k": Column(T.INT64, k), "x": Column(T.FLOAT64, x), "y": Column(T.FLOAT64, y)}, n))
    stmts = {
        "regr_slope grouped": "select k, regr_slope(y, x) as v from t group by k",
        "corr grouped": "select k, corr(y, x) as v from t group by k",
        "regr_slope global": "select regr_slope(y, x) as v from t",
        "corr global": "select corr(y, x) as v from t",
    }
    if a.only:
        stmts = {a.only: stmts[a.only]}
    for name, sql in stmts.items():          # warm-up: plans, recordings, code objects
        for _ in range(3):
            e.sql(sql)
    torch.cuda.synchronize()
    if os.environ.get("IGLOO_PROF_GAP") == "1":
        time.sleep(1.0)      # scripts/kernel_summary.py drops everything before the last long idle gap
    total = {name: 0.0 for name in stmts}
    for _ in range(a.reps):
        for name, sql in stmts.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.sql(sql)
            torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
    for name in stmts:
        print(f"rows={n} groups={a.groups} {name}: {total[name] / a.reps * 1e3:.3f} ms "
              f"(mode {e.last_metrics['speculation']})", flush=True)
    print("launches:", {k: v for k, v in KERNEL_CALLS.items() if k in ("agg_moments2", "agg_update", "agg_partitioned")})


if __name__ == "__main__":
    main()
