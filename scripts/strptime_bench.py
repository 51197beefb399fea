"""to_timestamp(s, fmt) on the device (BASELINE.md "strptime on the device"): 4,000,000 rows of
'%Y-%m-%d %H:%M:%S' text and of '%d/%b/%Y:%I:%M:%S %p %z' text, each as a plain column and as a
1,000-entry dictionary column, against the two ways the same ISO bytes were read before:
try_parse(..., TIMESTAMP) (the fixed-grammar device kernel) and _parse_ts_host (the host round trip).
Kernel times are device events around the launch alone, end-to-end times the host clock around the
operator and a synchronise (the error-cell readback included). Warmed; prints one JSON line.

Usage: python scripts/strptime_bench.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from igloo_amd import types as T
from igloo_amd.columnar import Column
from igloo_amd.exec.expr_eval import _parse_ts_host
from igloo_amd.ops import digest as DG, strptime as SP, trycast as TC
from igloo_amd.ops._lib import native, ptr, stream
from igloo_amd.ops.gather import take

dev = "cuda:0"
N_ROWS, N_DICT, REPS = 4_000_000, 1000, 20
ISO, LOG = "%Y-%m-%d %H:%M:%S", "%d/%b/%Y:%I:%M:%S %p %z"


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def measure(fn, timer, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = [timer(fn) for _ in range(reps)]
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


g = torch.Generator(device=dev); g.manual_seed(7)
lo, hi = -2208988800, 4102444800          # 1900 .. 2100
secs = torch.randint(lo, hi, (N_ROWS,), dtype=torch.int64, device=dev, generator=g)
offs = (torch.randint(-14 * 60, 14 * 60 + 1, (N_ROWS,), dtype=torch.int64, device=dev, generator=g) * 60).to(torch.int32)
iso = DG.to_char(Column(T.TIMESTAMP, secs * 1_000_000, None), ISO)
log = DG.to_char(Column(T.TIMESTAMP, (secs + offs) * 1_000_000, None), LOG, offs)
codes = torch.randint(0, N_DICT, (N_ROWS,), dtype=torch.int32, device=dev, generator=g)
first = torch.arange(N_DICT, dtype=torch.int64, device=dev)
iso_dict = Column(T.UTF8, codes, None, dictionary=take(iso, first))
log_dict = Column(T.UTF8, codes, None, dictionary=take(log, first))
want = secs * 1_000_000
assert torch.equal(SP.strptime(iso, (ISO,)).data, want) and torch.equal(SP.strptime(log, (LOG,)).data, want)
assert torch.equal(SP.strptime(iso_dict, (ISO,)).data, want[:N_DICT][codes.long()])
assert torch.equal(TC.try_parse(iso, T.TIMESTAMP).data, want)
assert torch.equal(_parse_ts_host(iso).data, want)

N = native()
out = torch.empty(N_ROWS, dtype=torch.int64, device=dev)
ok = torch.empty(N_ROWS, dtype=torch.uint8, device=dev)
err = torch.full((1,), N_ROWS, dtype=torch.int64, device=dev)


def kernel(col, fmt):
    p = SP.compile_formats((fmt,))
    h = torch.frombuffer(bytearray(p), dtype=torch.uint8)
    return lambda: N.strptime(ptr(h), len(p), 0, ptr(col.offsets), ptr(col.data), col.data.numel(), 0, N_ROWS, ptr(out),
                              ptr(err), stream(out))


res = {"rows": N_ROWS, "iso_text_bytes": iso.data.numel(), "log_text_bytes": log.data.numel()}
res["strptime_iso_kernel"] = measure(kernel(iso, ISO), events)
res["strptime_log_kernel"] = measure(kernel(log, LOG), events)
res["try_parse_iso_kernel"] = measure(lambda: N.try_parse(ptr(iso.offsets), ptr(iso.data), N_ROWS, 0, 9, 0, 0, ptr(out), ptr(ok),
                                                          stream(out)), events)
res["strptime_iso_op"] = measure(lambda: SP.strptime(iso, (ISO,)), wall)
res["strptime_log_op"] = measure(lambda: SP.strptime(log, (LOG,)), wall)
res["strptime_iso_dict_op"] = measure(lambda: SP.strptime(iso_dict, (ISO,)), wall)
res["strptime_log_dict_op"] = measure(lambda: SP.strptime(log_dict, (LOG,)), wall)
res["try_parse_iso_op"] = measure(lambda: TC.try_parse(iso, T.TIMESTAMP), wall)
res["try_parse_iso_dict_op"] = measure(lambda: TC.try_parse(iso_dict, T.TIMESTAMP), wall)
res["parse_ts_host_iso"] = measure(lambda: _parse_ts_host(iso), wall, reps=3, warm=1)
k, tp = res["strptime_iso_kernel"]["median_ms"], res["try_parse_iso_kernel"]["median_ms"]
res["ratio_kernel_strptime_to_try_parse"] = round(k / tp, 3)
res["ratio_op_strptime_to_host_round_trip"] = round(res["strptime_iso_op"]["median_ms"] / res["parse_ts_host_iso"]["median_ms"], 5)
res["iso_text_GBps"] = round(iso.data.numel() / (k * 1e-3) / 1e9, 1)
res["log_text_GBps"] = round(log.data.numel() / (res["strptime_log_kernel"]["median_ms"] * 1e-3) / 1e9, 1)
res["iso_moved_GBps"] = round((iso.data.numel() + 16 * N_ROWS) / (k * 1e-3) / 1e9, 1)      # text + offsets + values
print(json.dumps(res), flush=True)
