"""TRY_CAST kernels against what plain CAST runs (BASELINE.md "TRY_CAST"): cast_checked INT64 -> INT32 over 64 Mi
rows against the ATen copy of _convert_tensor, and try_parse to INT64 over 16 Mi rows of 6-12 byte text against
str_parse, kernel alone (device events) and end to end with str_parse's flag readback (host clock around a
synchronise). Warmed, old and new alternating in one process; prints one JSON line per pair.

Usage: python scripts/trycast_bench.py"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from igloo_amd import types as T
from igloo_amd.columnar import Column
from igloo_amd.ops import strings as S, trycast as TC
from igloo_amd.ops._lib import native, ptr, stream

dev = "cuda:0"
REPS = 30


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def ab(old, new, warm=5):
    for _ in range(warm):
        old(); new()
    torch.cuda.synchronize()
    to, tn = [], []
    for _ in range(REPS):
        to.append(timed(old)); tn.append(timed(new))
    return to, tn


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


out = {}
# 1. INT64 -> INT32, 64 M rows: ATen copy (what _convert_tensor calls) vs cast_checked
n = 64 << 20
g = torch.Generator(device=dev); g.manual_seed(1)
x = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device=dev, generator=g)
col = Column(T.INT64, x, None)
N = native()
dst = torch.empty(n, dtype=torch.int32, device=dev); ok = torch.empty(n, dtype=torch.uint8, device=dev)
old = lambda: x.to(torch.int32)
new = lambda: N.cast_checked(ptr(x), 3, 0, n, 0, 2, 0, 0, ptr(dst), ptr(ok), stream(x))
to, tn = ab(old, new)
assert bool((dst == x.to(torch.int32)).all()) and bool(ok.all())
op = lambda: TC.cast_checked(col, T.INT32)
to2, tn2 = ab(old, op)
out["int64_to_int32"] = {"rows": n, "aten_copy": summary(to), "cast_checked_kernel": summary(tn),
                         "aten_copy_b": summary(to2), "cast_checked_op_with_alloc": summary(tn2),
                         "ratio_kernel": round(statistics.median(tn) / statistics.median(to), 4),
                         "ratio_op": round(statistics.median(tn2) / statistics.median(to2), 4),
                         "bytes_per_s_new": round(13 * n / (statistics.median(tn) * 1e-3) / 1e12, 3),
                         "bytes_per_s_old": round(12 * n / (statistics.median(to) * 1e-3) / 1e12, 3)}
print(json.dumps(out["int64_to_int32"]), flush=True)
del x, dst, ok, col
torch.cuda.empty_cache()

# 2. text -> INT64, 16 M rows of 6-12 byte text, all valid: str_parse vs try_parse
n = 16 << 20
u = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
v = torch.floor(torch.pow(10.0, 5.0 + 7.0 * u)).to(torch.int64).clamp_(10**5, 10**12 - 1)
text = S.to_string(Column(T.INT64, v, None))
lens = text.offsets[1:] - text.offsets[:-1]
nbytes = int(text.offsets[-1])
print("text rows", n, "bytes", nbytes, "len min/max", int(lens.min()), int(lens.max()), flush=True)
o = torch.empty(n, dtype=torch.int64, device=dev); err = torch.zeros(1, dtype=torch.int32, device=dev)
ok = torch.empty(n, dtype=torch.uint8, device=dev)
old = lambda: N.str_parse(ptr(text.offsets), ptr(text.data), n, 0, 0, 0, ptr(o), ptr(err), stream(o))
new = lambda: N.try_parse(ptr(text.offsets), ptr(text.data), n, 0, 0, 0, 0, ptr(o), ptr(ok), stream(o))
to, tn = ab(old, new)
assert bool((o == v).all()) and bool(ok.all()) and int(err) == 0


def wall(fn):
    torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


eo, en = [], []
for i in range(5 + REPS):
    a = wall(lambda: S.parse(text, T.INT64)); b = wall(lambda: TC.try_parse(text, T.INT64))
    if i >= 5:
        eo.append(a); en.append(b)
moved_old = 16 * n + nbytes            # offsets (8) + values (8) + text
out["text_to_int64"] = {"rows": n, "text_bytes": nbytes, "str_parse_kernel": summary(to), "try_parse_kernel": summary(tn),
                        "ratio_kernel": round(statistics.median(tn) / statistics.median(to), 4),
                        "end_to_end_parse_with_readback": summary(eo), "end_to_end_try_parse": summary(en),
                        "ratio_end_to_end": round(statistics.median(en) / statistics.median(eo), 4),
                        "bytes_per_s_new": round((moved_old + n) / (statistics.median(tn) * 1e-3) / 1e12, 3),
                        "bytes_per_s_old": round(moved_old / (statistics.median(to) * 1e-3) / 1e12, 3)}
print(json.dumps(out["text_to_int64"]), flush=True)
