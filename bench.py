"""Headline benchmark: TPC-H SF100 total query time (22 queries) + scan rows/s.

BASELINE.json metric: "TPC-H SF100 total query time (s) + rows/sec scan,
1/2/4/8 MI355X", on synthetic TPC-H-shaped Parquet data. One step = one run
of the full 22-query suite.

Data path of a ``--full`` run (``--source parquet``, its default):
  1. each rank generates its hash partition of the SF tables on the GPU
     (spec distributions, models/tpch/datagen.py) and writes it as snappy
     Parquet files with a parallel writer (models/tpch/parquet_gen.py); a
     complete dataset from an earlier run with the same parameters is reused.
     Generation/write time is reported separately (``datagen_s``/``write_s``).
  2. a fresh engine registers the files. ``cold_s`` = the FIRST suite run:
     native pread of the column chunks + H2D + gfx950 page decode into the
     HBM cache tier + every derived structure the queries build (sortedness
     flags, range/secondary indexes, HLL sketches, narrow copies) + the
     queries themselves.
     Scan shapes get query-specialised kernels (igloo_amd/ops/jit.py):
     hiprtc compiles them on host threads during the cold suite, which runs
     the interpreted kernels; remaining compile time is ``jit.wait_s``.
     Repeated queries over unchanged data replay their host readbacks
     (sizes, ranges) and validate them on the device at the end of each query
     (``speculation`` counts, engine.py); every kernel still runs every step.
  3. ``--warmup`` untimed suites, then ``--steps`` timed suites over the
     cached columns (bracketed by barrier + device sync, max over ranks):
     ``value`` is seconds per warm suite.
Every result of every run is digested (row count, exact sums of numeric
columns, order-independent hash of the rest); all runs must agree with the
cold run (``verified``), and at ``--sf <= 1`` the digests are also checked
against the CPU engine over the same files (``cpu_check``).
``scan_rows_per_s`` counts base-table rows the queries actually read (each
table once per query; index / range searches count only the rows touched).
``--source hbm`` runs on tables generated straight into HBM (no Parquet).

A plain run (no ``--full``) does only what the headline figure needs: it
generates the tables straight into HBM (``--source`` defaults to ``hbm``),
runs the first (cold) suite that builds the derived structures, the
``--warmup`` suites and the ``--steps`` timed suites, and prints the result
line. ``--full`` adds everything else, as described above: the Parquet data
path (``--source`` defaults to ``parquet``: dataset write, cold file read +
GPU decode), the eager and ad-hoc suites (``--eager-steps``,
``--vary-params``), the digest verification of every timed result against the
cold run and the CPU-engine check at ``--sf <= 1``.

``--dump-outputs DIR`` writes what the last timed step returned to the caller
(one Arrow table per query) as ``DIR/q<NN>.<II>_<column>.npy`` in float64
(integers, dates, decimals and booleans as their float64 value; strings as the
float64 value of a CRC-32 of their UTF-8 bytes; NULL as NaN), with the column
order in ``DIR/manifest.json``. The generated data and the validation
parameters are fixed, so two builds run with the same arguments dump the same
arrays.

Single GPU:  python bench.py --gpus 1 --steps 3 --warmup 1
N GPUs:      python bench.py --gpus N ...   (launches N rank processes itself), or
             python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
                 --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
With ``--gpus N > 1`` and no launcher environment (no WORLD_SIZE), this
process starts ``torch.distributed.run`` with N ranks as a CHILD process
before anything touches the GPU (it only counts devices), and exits with the
child's code; rank 0 prints the JSON line. A world that does not equal
``--gpus``, or more ranks than visible GPUs, is an error (exit 2).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "TPC-H SF100 total query time (s) + rows/sec scan, 1/2/4/8 MI355X"


def parse_queries(s: str):
    out = []
    for part in s.split(","):
        if "-" in part:
            a, b = part.split("-")
            out += list(range(int(a), int(b) + 1))
        elif part:
            out.append(int(part))
    return out


DUMP_BUDGET_BYTES = 64 << 20


def _as_float_array(col):
    """One result column as a float64 numpy array: numbers, decimals, dates
    and booleans by value, strings by the CRC-32 of their UTF-8 bytes, NULL as
    NaN."""
    import zlib
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    t = arr.type
    if pa.types.is_dictionary(t):
        arr = arr.cast(t.value_type)
        t = arr.type
    if pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t):
        vals = [float("nan") if v is None else float(zlib.crc32(v if isinstance(v, bytes) else v.encode()))
                for v in arr.to_pylist()]
        return np.asarray(vals, dtype=np.float64)
    if pa.types.is_date32(t):
        arr = arr.cast(pa.int32())
    elif pa.types.is_date64(t) or pa.types.is_timestamp(t) or pa.types.is_time(t) or pa.types.is_duration(t):
        arr = arr.cast(pa.int64())
    elif pa.types.is_boolean(t):
        arr = arr.cast(pa.int8())
    elif not (pa.types.is_integer(t) or pa.types.is_floating(t) or pa.types.is_decimal(t)):
        # nested / other types: by the CRC-32 of their printed value
        vals = [float("nan") if v is None else float(zlib.crc32(repr(v).encode())) for v in arr.to_pylist()]
        return np.asarray(vals, dtype=np.float64)
    out = pc.cast(arr, pa.float64(), safe=False)
    return np.asarray(out.to_numpy(zero_copy_only=False), dtype=np.float64)


def dump_outputs(out_dir: str, results: dict) -> None:
    """Write one timed step's results (query number -> Arrow table) as
    ``q<NN>.<II>_<column>.npy`` float64 arrays plus ``manifest.json``. Results past
    DUMP_BUDGET_BYTES in all are cut to a fixed, seeded sample of their rows
    (the same rows for the same result sizes)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(8 * t.num_rows * t.num_columns for t in results.values())
    keep = min(1.0, DUMP_BUDGET_BYTES / total) if total else 1.0
    manifest = {}
    for q in sorted(results):
        t = results[q]
        rows = None
        if keep < 1.0 and t.num_rows > 1:
            n = max(1, int(t.num_rows * keep))
            rows = np.sort(np.random.default_rng(1234 + q).choice(t.num_rows, size=n, replace=False))
        cols = []
        for i, name in enumerate(t.column_names):
            v = _as_float_array(t.column(i))
            if rows is not None:
                v = v[rows]
            fname = f"q{q:02d}.{i:02d}_{''.join(c if c.isalnum() else '_' for c in name)}"
            np.save(os.path.join(out_dir, fname + ".npy"), v)
            cols.append({"name": name, "file": fname + ".npy", "type": str(t.schema.field(i).type)})
        manifest[f"q{q:02d}"] = {"rows": t.num_rows, "rows_written": t.num_rows if rows is None else len(rows),
                                 "columns": cols}
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


_MODE_TAG = {"recorded": "R", "replayed": "P", "graph": "G", "partial": "x"}


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(a, argv) -> int:
    """``--gpus N`` without a launcher: run N ranks under torch.distributed.run
    as a child process (never exec: the GPU may not be touched by a process
    that later replaces itself) and return its exit code. Only the device
    COUNT is read here (torch.cuda.device_count does not initialise HIP)."""
    shared = os.environ.get("IGLOO_BENCH_SHARE_GPU") == "1"
    if not a.cpu and not shared:
        import torch
        ngpu = torch.cuda.device_count()
        if ngpu < a.gpus:
            print(f"[bench] error: --gpus {a.gpus} but only {ngpu} GPU(s) visible; one rank per GPU is required "
                  f"(IGLOO_BENCH_SHARE_GPU=1 rehearses several ranks on one GPU over gloo)", file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__)] + list(argv)
    print(f"[bench] launching {a.gpus} ranks: {' '.join(cmd[1:6])} ...", file=sys.stderr, flush=True)
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--queries", default="1-22")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: the Parquet data path (cold read + GPU "
                         "decode), the eager and ad-hoc suites, digest verification, the CPU check at sf <= 1")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's query results to DIR as float64 .npy arrays")
    ap.add_argument("--source", choices=["parquet", "hbm"], default=None,
                    help="where the tables come from (default: parquet with --full, else hbm)")
    ap.add_argument("--data-dir", default=os.environ.get("IGLOO_BENCH_DIR", "/tmp/igloo_tpch"))
    ap.add_argument("--lean", action="store_true", help="skip comment columns no query reads")
    ap.add_argument("--parquet-codec", choices=["snappy", "zstd", "none"], default="snappy",
                    help="codec of the generated Parquet files (--source parquet)")
    ap.add_argument("--cpu-check", choices=["auto", "on", "off"], default="auto",
                    help="check result digests against the CPU engine (auto: sf <= 1)")
    ap.add_argument("--per-query", action="store_true", help="print per-query times to stderr")
    ap.add_argument("--digests-out", default="", help="write the cold run's result digests (JSON) here")
    ap.add_argument("--cpu", action="store_true", help="run on CPU (debug)")
    ap.add_argument("--eager-steps", type=int, default=2,
                    help="with --full: suites timed with query graphs off (warm_eager_s), after the headline steps")
    ap.add_argument("--profile-adhoc", type=float, default=0.0, metavar="MS",
                    help="diagnostics: cProfile every ad-hoc statement, print those slower than MS")
    ap.add_argument("--param-seed", type=int, default=1000,
                    help="seed of the first ad-hoc parameter stream (stream k uses seed + k)")
    ap.add_argument("--vary-params", type=int, default=2, metavar="STREAMS",
                    help="with --full: suites with fresh TPC-H substitution parameters per query (adhoc_s; 0 = skip)")
    a = ap.parse_args()
    if a.source is None:
        a.source = "parquet" if a.full else "hbm"
    if not a.full:
        # a plain run times the headline steps only
        a.eager_steps = a.vary_params = 0
        a.cpu_check = "off"

    if a.gpus < 1:
        print(f"[bench] error: --gpus {a.gpus}", file=sys.stderr)
        sys.exit(2)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        print(f"[bench] error: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks", file=sys.stderr)
        sys.exit(2)

    import torch
    import igloo_amd as ig
    from igloo_amd.models.tpch import datagen, parquet_gen, queries
    from igloo_amd.utils.digest import digest
    # IGLOO_BENCH_SHARE_GPU=1: every rank on cuda:0 with host-staged gloo
    # collectives — a rehearsal of the multi-rank path on a one-GPU box
    shared = os.environ.get("IGLOO_BENCH_SHARE_GPU") == "1"
    device = "cpu" if a.cpu else ("cuda:0" if shared else f"cuda:{local}")
    if not a.cpu and not shared and local >= torch.cuda.device_count():
        print(f"[bench] error: rank {rank} (local {local}) has no GPU: {torch.cuda.device_count()} visible",
              file=sys.stderr)
        sys.exit(2)
    if not a.cpu:
        torch.cuda.set_device(torch.device(device))
    comm = None
    # IGLOO_FORCE_SPMD=1 on one GPU: the multi-GPU code path with a world of
    # one (every exchange and collective runs, RCCL; parallel/comm.py)
    force_spmd = os.environ.get("IGLOO_FORCE_SPMD") == "1"
    if world > 1 or force_spmd:
        from igloo_amd.parallel.comm import Communicator
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", str(world))
        comm = Communicator.init(backend="gloo" if (a.cpu or shared) else "nccl", device=device,
                                 force_spmd=force_spmd)
        if comm.world_size != world:
            print(f"[bench] error: the process group has {comm.world_size} ranks, expected {world}", file=sys.stderr)
            sys.exit(2)
    spmd = comm is not None

    def barrier():
        if comm is not None:
            comm.barrier()
        if not a.cpu:
            torch.cuda.synchronize()

    def log(msg):
        if rank == 0:
            print(msg, file=sys.stderr, flush=True)

    qs = parse_queries(a.queries)
    from igloo_amd.models.tpch import params as _params
    # the spec's validation parameters, Q11's FRACTION scaled to the SF
    SQL = {q: _params.validation(q, a.sf) for q in qs}
    load = {"source": a.source}
    t0 = time.perf_counter()
    if a.source == "parquet":
        man = parquet_gen.write_dataset(a.sf, a.data_dir, device=device, rank=rank, world=world, lean=a.lean,
                                        log=log, compression=a.parquet_codec)
        if not a.cpu:
            torch.cuda.empty_cache()
        barrier()
        load.update(datagen_s=man["gen_s"], write_s=man["write_s"], dataset_bytes=man["bytes"],
                    files=man["files"], dataset_reused=man["reused"], compression=man["compression"])
        rows = dict(man["rows"])
        eng = ig.QueryEngine(device=device, comm=comm)
        parquet_gen.register_dataset(eng, a.data_dir, a.sf, rank, world, lean=a.lean, spmd=spmd)
    else:
        eng = ig.QueryEngine(device=device, comm=comm)
        tabs = datagen.generate(a.sf, device, rank, world, lean=a.lean, spmd=spmd)
        for name, t in tabs.items():
            eng.register_table(name, t)
        barrier()
        load["datagen_s"] = round(time.perf_counter() - t0, 2)
        rows = {k: v.num_rows() for k, v in tabs.items()}
        del tabs
    if comm is not None:
        # fact tables are partitioned over ranks; dimension tables replicated
        for k in rows:
            if parquet_gen.PARTITION_KEY[k] is not None:
                rows[k] = comm.allreduce_int(rows[k])
    log(f"[bench] sf={a.sf} world={world} source={a.source} load={load} rows={rows}")

    spec_modes = {}

    def suite(record=None, results=None, scanned=None):
        modes = []
        for q in qs:
            tq = time.perf_counter()
            r = eng.sql(SQL[q])
            m = eng.last_metrics.get("speculation")
            spec_modes[m] = spec_modes.get(m, 0) + 1
            modes.append(f"{q}:{_MODE_TAG.get(m, '-')}")
            if results is not None:
                results[q] = r.table
            if scanned is not None:
                scanned[q] = eng.last_metrics.get("rows_scanned", 0)
            if record is not None:
                barrier()
                record[q] = record.get(q, 0.0) + (time.perf_counter() - tq)
        if a.per_query:
            log("[bench] modes " + " ".join(modes))

    # ---- cold: first touch of every column (Parquet read + GPU decode) and structure
    from igloo_amd.connectors import gpu_parquet as _gpq
    for k in _gpq.TOTALS:
        _gpq.TOTALS[k] = 0
    barrier()
    tc = time.perf_counter()
    cold_res, cold_scanned = {}, {}
    cold_per_q = {} if a.per_query else None
    suite(cold_per_q, cold_res, cold_scanned)
    barrier()
    cold_s = time.perf_counter() - tc
    if comm is not None:
        cold_s = comm.allreduce_max_float(cold_s)
    log(f"[bench] cold suite: {cold_s:.3f}s")
    if cold_per_q:
        log("[bench] cold per query (ms): " + " ".join(f"Q{q}={cold_per_q[q] * 1e3:.1f}" for q in qs))
    ref = {q: digest(t) for q, t in cold_res.items()} if (a.full or a.digests_out) else {}
    del cold_res
    if a.digests_out and rank == 0:
        with open(a.digests_out, "w") as f:
            json.dump({str(q): repr(d) for q, d in ref.items()}, f, indent=1, sort_keys=True)
    # generated scan kernels (ops/jit.py) compile on host threads while the
    # cold suite runs on the interpreted ones; whatever is still compiling is
    # waited for here and reported (not hidden in the warm steps)
    from igloo_amd.ops import jit as _jit
    tj = time.perf_counter()
    _jit.wait_all(timeout=120)
    jit_wait_s = time.perf_counter() - tj
    log(f"[bench] jit: {_jit.STATS} wait {jit_wait_s:.3f}s")

    for w in range(a.warmup):
        tw = time.perf_counter()
        suite()
        barrier()
        log(f"[bench] warmup {w}: {time.perf_counter() - tw:.3f}s")
    # like a serving process after startup: the loaded catalog, caches and
    # plans move to the permanent GC generation, so a full collection (it
    # struck the first fresh statements at ~90 ms) no longer walks them
    import gc
    gc.collect()
    gc.freeze()
    per_q = {} if a.per_query else None
    step_results = []
    barrier()
    if os.environ.get("IGLOO_PROF_GAP"):
        time.sleep(1.0)   # idle gap that scripts/kernel_summary.py uses to isolate the timed steps in a trace
    spec_modes.clear()
    t1 = time.perf_counter()
    for s in range(a.steps):
        res = {}
        suite(per_q, res)
        if a.full:
            step_results.append(res)     # every step's results are digested after the timed region
        else:
            step_results[:] = [res]      # only what --dump-outputs writes
        if rank == 0:
            print(f"[bench] step {s}: {time.perf_counter() - t1:.3f}s cumulative", file=sys.stderr, flush=True)
    barrier()
    elapsed = time.perf_counter() - t1
    timed_modes = dict(spec_modes)
    rank_info = None
    if comm is not None:
        # per-rank timed region and data-plane traffic (outside the timed region)
        rank_info = comm.allgather_object({"rank": comm.rank, "world": comm.world_size, "device": device,
                                           "backend": comm.backend, "timed_region_s": round(elapsed, 4),
                                           "collectives": comm.calls, "bytes_sent": comm.bytes_sent})
        elapsed = comm.allreduce_max_float(elapsed)
    step_s = elapsed / max(a.steps, 1)

    # ---- secondary measurements (after the headline steps, not part of ``value``):
    # warm_eager_s — the same SQL with query graphs off (replayed readbacks,
    # Python operator dispatch); adhoc_s — every statement new SQL text
    # (TPC-H substitution parameters, models/tpch/params.py): nothing keyed
    # on the SQL text (plans, readbacks, graphs) applies
    from igloo_amd.exec import graphs as _graphs_mod
    eager_s = adhoc_s = None
    adhoc_streams, adhoc_readbacks, adhoc_modes, adhoc_plans = [], [], {}, {}
    if a.eager_steps > 0:
        saved = _graphs_mod.GRAPHS
        _graphs_mod.GRAPHS = False
        try:
            suite()          # first eager pass re-records readbacks without graphs
            barrier()
            te = time.perf_counter()
            for _ in range(a.eager_steps):
                suite()
            barrier()
            eager_s = (time.perf_counter() - te) / a.eager_steps
        finally:
            _graphs_mod.GRAPHS = saved
        if comm is not None:
            eager_s = comm.allreduce_max_float(eager_s)
        log(f"[bench] warm eager (graphs off): {eager_s:.4f}s per suite")
    if a.vary_params > 0:
        streams = [_params.stream(qs, a.param_seed + k, a.sf) for k in range(a.vary_params)]
        barrier()
        ta = time.perf_counter()
        for k, st_sql in enumerate(streams):
            ts = time.perf_counter()
            nrb = 0
            qtimes = []
            for q in qs:
                tq = time.perf_counter()
                if a.profile_adhoc:
                    # diagnostics: where does a slow fresh statement spend its time
                    import cProfile
                    import io
                    import pstats
                    pr = cProfile.Profile()
                    pr.enable()
                    eng.sql(st_sql[q])
                    pr.disable()
                    if time.perf_counter() - tq > a.profile_adhoc / 1e3:
                        buf = io.StringIO()
                        pstats.Stats(pr, stream=buf).sort_stats("cumulative").print_stats(25)
                        log(f"[bench] ad-hoc stream {k} Q{q} took {(time.perf_counter() - tq) * 1e3:.1f} ms:\n"
                            + buf.getvalue())
                else:
                    eng.sql(st_sql[q])
                qtimes.append(f"Q{q}={(time.perf_counter() - tq) * 1e3:.1f}")
                nrb += eng.last_metrics.get("readbacks", 0)
                m = eng.last_metrics.get("speculation")
                adhoc_modes[m] = adhoc_modes.get(m, 0) + 1
                ps = eng.last_metrics.get("plan_source")
                adhoc_plans[ps] = adhoc_plans.get(ps, 0) + 1
            barrier()
            adhoc_streams.append(time.perf_counter() - ts)
            adhoc_readbacks.append(nrb)
            log(f"[bench] ad-hoc stream {k} per query (ms): {' '.join(qtimes)}")
        barrier()
        adhoc_s = (time.perf_counter() - ta) / a.vary_params
        if comm is not None:
            adhoc_s = comm.allreduce_max_float(adhoc_s)
            adhoc_streams = [comm.allreduce_max_float(x) for x in adhoc_streams]
        log(f"[bench] ad-hoc (fresh substitution parameters): {adhoc_s:.4f}s per suite; per stream "
            f"{[round(x, 4) for x in adhoc_streams]} s, blocking readbacks {adhoc_readbacks}, modes {adhoc_modes}, "
            f"plans {adhoc_plans}, templates {eng.template_stats}")

    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, step_results[-1] if step_results else {})

    # ---- verification (outside the timed region; --full)
    mismatches = [(i, q) for i, res in enumerate(step_results) for q, t in res.items() if digest(t) != ref[q]] \
        if a.full else []
    del step_results
    cpu_check = None
    if rank == 0 and (a.cpu_check == "on" or (a.cpu_check == "auto" and a.sf <= 1 and world == 1)) and not a.cpu:
        ce = ig.QueryEngine(device="cpu")
        if a.source == "parquet":
            parquet_gen.register_dataset(ce, a.data_dir, a.sf, rank, world, lean=a.lean)
        else:
            datagen.register(ce, a.sf, lean=a.lean)
        bad = [q for q in qs if digest(ce.sql(SQL[q]).table) != ref[q]]
        cpu_check = {"queries": len(qs), "mismatched": bad}
        if bad:
            log(f"[bench] CPU check mismatches: {bad}")
    # None: a plain run does not digest its results (--full does)
    verified = (not mismatches and (cpu_check is None or not cpu_check["mismatched"])) if a.full else None
    if mismatches:
        log(f"[bench] result digests differ from the cold run: {mismatches[:10]}")
    scanned = sum(cold_scanned.values())
    if comm is not None:
        scanned = comm.allreduce_int(int(scanned))
    if rank == 0:
        if a.per_query:
            from igloo_amd.exec import graphs as _graphs
            log(f"[bench] graphs: {_graphs.STATS}; engine graphs {len(eng._graphs)} holding "
                f"{eng.graph_bytes / 2**30:.1f} GiB, {eng.graph_stats}; cache tier {eng.cache.hbm_used / 2**30:.1f} GiB; "
                f"HBM reserved {torch.cuda.memory_reserved() / 2**30:.1f} GiB, "
                f"peak allocated {eng.hbm_peak_bytes / 2**30:.1f} GiB (max per-query high-water mark)")
            for msg in _graphs.LAST_ERROR:
                log("[bench] graph not captured: " + msg.strip().replace("\n", " | ")[-600:])
        if per_q:
            for q in qs:
                print(f"[bench] Q{q:02d} {per_q[q] / a.steps * 1e3:9.2f} ms", file=sys.stderr)
        src_txt = (f"synthetic TPC-H-shaped Parquet (spec distributions, {a.parquet_codec}, dictionary pages) generated on "
                   "the device; GPU-decoded into the HBM cache tier; value = warm suite over the cached columns, "
                   "cold_s = first suite incl. file read + GPU decode + index builds"
                   if a.source == "parquet" else
                   "synthetic TPC-H-shaped (spec distributions), generated in HBM; no Parquet")
        out = {
            "metric": METRIC,
            "value": round(step_s, 4),
            "unit": "s (22-query suite, lower is better)",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "full": a.full,
            "ms_per_step": round(step_s * 1e3, 2),
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "exact decimal(15,2) int64 fixed-point / int32 keys",
            "data": src_txt,
            "config": {"model": f"TPC-H SF{a.sf:g} queries {a.queries}", "global_batch": sum(rows.values()),
                       "seq_len": None,
                       "parallelism": (f"dp{world}" if world > 1 else ("spmd-world1-rehearsal" if spmd else "single-gpu")),
                       "layout": ("fact tables (lineitem, orders) hash-partitioned by order key, dimension tables "
                                  "replicated" if spmd else "single rank"),
                       "sf": a.sf, "queries": qs},
            "world": world,
            # one entry per rank: the process-group size it saw, its own timed
            # region (``value`` uses the max), collectives issued over the run
            "ranks": rank_info,
            "warm_s": round(step_s, 4),
            "warm_graph_s": round(step_s, 4),
            "warm_eager_s": round(eager_s, 4) if eager_s is not None else None,
            "adhoc_s": round(adhoc_s, 4) if adhoc_s is not None else None,
            # per ad-hoc stream: wall seconds and blocking host readbacks
            "adhoc_streams_s": [round(x, 4) for x in adhoc_streams],
            "adhoc_readbacks": adhoc_readbacks,
            # how the fresh statements were planned: "template" = a verified
            # statement template of the validation text (sql/template.py),
            # "planned" = parse + bind + optimize
            "adhoc_plans": adhoc_plans,
            "cold_s": round(cold_s, 4),
            # timed-step queries whose host readbacks were replayed and validated
            # on the device (engine.QueryEngine._execute_speculative)
            "speculation": {str(k): v for k, v in timed_modes.items()},
            "jit": {"wait_s": round(jit_wait_s, 3), "kernels_compiled": _jit.STATS["compiled"],
                    "disk_hits": _jit.STATS["disk_hits"], "failed": _jit.STATS["failed"]},
            "load": load,
            "verified": verified,
            "cpu_check": cpu_check,
            "scan_rows_per_s": round(scanned / step_s, 1),
            "rows_read_per_suite": int(scanned),
            # cold-run Parquet decode alone (file bytes through read + H2D + GPU
            # decode, index builds excluded): rank 0's reader
            "parquet_decode_gbps": (round(_gpq.TOTALS["file_bytes"] / _gpq.TOTALS["seconds"] / 1e9, 2)
                                    if _gpq.TOTALS["seconds"] else None),
            "parquet_decode": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in _gpq.TOTALS.items()},
        }
        print(json.dumps(out), flush=True)
    eng.close()              # query graphs hold RCCL resources (Communicator.shutdown)
    if comm is not None:
        comm.shutdown()


if __name__ == "__main__":
    main()
