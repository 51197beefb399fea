"""Order statistics over window frames against max(x) OVER the identical frame
(the sparse-table / scan path, unchanged by this work: the yardstick), over
float64 values resident in HBM, in ``--parts`` partitions and unpartitioned.
   python scripts/bench_window_select.py [--rows 10000000] [--parts 1000] [--reps 10] [--only NAME]
Statements (each a reduction over the window column, so the result path moves
one row and the window operator is what is timed):
   loop    median(x)                 ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING
   tree    median(x)                 ROWS BETWEEN 100000 PRECEDING AND CURRENT ROW
   whole   percentile_cont(x, 0.95)  over the whole partition
and ``max(x)`` with the same OVER clause. Prints the mean wall time per
statement (host clock around a device synchronise) after 3 warm-up executions,
the statements alternating, the HBM high-water mark of one execution and the
bytes of the merge-sort tree (ceil(log2 m) * 4 B per valid row, computed from
the shape). Query graphs are off so a kernel trace of the same command
(rocprofv3 --kernel-trace, then scripts/kernel_summary.py) splits a statement
into sort / tree build (select_tile_kernel, select_merge_kernel) / query
(select_query_kernel, frame_kth_kernel); ``--only`` runs one statement for such
a trace."""
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

FRAMES = {
    "loop": "rows between 3 preceding and 3 following",
    "tree": "rows between 100000 preceding and current row",
    "whole": "rows between unbounded preceding and unbounded following",
}


def statements(partitioned: bool):
    p = "partition by k " if partitioned else ""
    tag = "parts" if partitioned else "flat"
    out = {}
    for name, frame in FRAMES.items():
        stat = "percentile_cont(x, 0.95)" if name == "whole" else "median(x)"
        for fn, call in (("stat", stat), ("max", "max(x)")):
            out[f"{name} {tag} {fn}"] = f"select max(v) as v from (select {call} over ({p}order by o {frame}) as v from t)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--parts", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, help="a statement name, or a prefix such as 'tree parts'")
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    n = a.rows
    x = torch.randn(n, device=dev, generator=gen, dtype=torch.float64)
    k = torch.randint(0, a.parts, (n,), device=dev, generator=gen, dtype=torch.int64)
    o = torch.randperm(n, device=dev, generator=gen)
    e = ig.QueryEngine(device=dev)
    e.register_table("t", MemoryTable({"k": Column(T.INT64, k), "o": Column(T.INT64, o), "x": Column(T.FLOAT64, x)}, n))
    stmts = {**statements(True), **statements(False)}
    if a.only:
        stmts = {name: sql for name, sql in stmts.items() if name.startswith(a.only)}
        assert stmts, a.only
    peak = {}
    for name, sql in stmts.items():          # warm-up: plans, recordings, code objects
        for _ in range(3):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e.sql(sql)
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
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
    levels = max(n - 1, 1).bit_length()
    for name in stmts:
        print(f"rows={n} parts={a.parts} {name}: {total[name] / a.reps * 1e3:.3f} ms "
              f"(mode {e.last_metrics['speculation']}; HBM above the table {peak[name] / 2**20:.0f} MiB)", flush=True)
    print(f"tree: {levels} levels x {n} rows x 4 B = {levels * n * 4 / 2**20:.0f} MiB")
    print("launches:", {k: v for k, v in KERNEL_CALLS.items() if k in ("win_frame_kth", "win_select", "win_sparse",
                                                                      "win_frame_minmax", "win_seg_scan")})


if __name__ == "__main__":
    main()
