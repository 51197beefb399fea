"""Time of a MAP lookup against the expression it replaces, BASELINE.md's
"MAP lookup" table.

    python scripts/map_lookup_bench.py [--rows 4000000] [--entries 8] [--reps 9] [--device cuda:0]

The table holds ``rows`` maps of ``entries`` entries each, built on the device:
a plain-string-keyed map (keys 'k0'..'k7', rotated per row so the match sits
at every position), an int64-keyed map over the same key numbers, and the same
data as two LIST columns per map. Each case sums the looked-up values, so the
result is one row and the time is the lookup's, not the export's:

    sum(ms['k3'])   against   sum(array_element(sv, array_position(sk, 'k3')))

with a constant needle and with a per-row needle column, for both key types.
Every statement runs 2 untimed and ``reps`` timed executions; the time is
taken with device events around ``engine.sql`` and ends in a synchronise.
Prints one JSON line: per case the result of both sides (they must agree),
median / min / max milliseconds of each, and the host steps per execution."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rows", type=int, default=4_000_000)
ap.add_argument("--entries", type=int, default=8)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--device", default="cuda:0")
a = ap.parse_args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402
import igloo_amd as ig  # noqa: E402
from igloo_amd import types as T  # noqa: E402
from igloo_amd.columnar import Column, Nested  # noqa: E402
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS  # noqa: E402

if a.device != "cpu" and not torch.cuda.is_available():
    sys.exit("no GPU: a time taken elsewhere says nothing about the device path")
if not 1 <= a.entries <= 10:
    sys.exit("--entries: 1 to 10 (keys are 'k' + one digit)")
dev = torch.device(a.device)
WARMUP = 2
n, k = a.rows, a.entries


def plain_strings(num: torch.Tensor) -> Column:
    """'k<digit>' per element of ``num`` as a plain string column."""
    chars = torch.stack([torch.full_like(num, ord("k")), num + ord("0")], 1).to(torch.uint8).reshape(-1)
    return Column(T.UTF8, chars, None, offsets=torch.arange(num.numel() + 1, dtype=torch.int64, device=dev) * 2)


r = torch.arange(n, dtype=torch.int64, device=dev)
t = torch.arange(k, dtype=torch.int64, device=dev)
key_num = ((r.view(n, 1) + t.view(1, k)) % k).reshape(-1)          # entry t of row r holds key (r + t) % k
values = torch.arange(n * k, dtype=torch.int64, device=dev) % 1000
se = torch.stack([r * k, torch.full_like(r, k)], 1).contiguous()
kstr, kint, vals = plain_strings(key_num), Column(T.INT64, key_num), Column(T.INT64, values)
needle_num = (r * 7 + 3) % (k + 1)                                   # k itself: a needle no row holds


def lst(child):
    return Column(T.LIST(child.dtype), se, None, dictionary=Nested(child=child))


def mp(keys):
    return Column(T.MAP(keys.dtype, T.INT64), se, None, dictionary=Nested(children={"key": keys, "value": vals}))


e = ig.QueryEngine(device=a.device)
e.register_table("t", {"ms": mp(kstr), "mi": mp(kint), "sk": lst(kstr), "ik": lst(kint), "sv": lst(vals),
                       "ns": plain_strings(needle_num), "ni": Column(T.INT64, needle_num)})
CASES = {
    "string keys, constant": ("ms['k3']", "array_element(sv, array_position(sk, 'k3'))"),
    "int64 keys, constant": ("mi[3]", "array_element(sv, array_position(ik, 3))"),
    "string keys, per-row needle": ("ms[ns]", "array_element(sv, array_position(sk, ns))"),
    "int64 keys, per-row needle": ("mi[ni]", "array_element(sv, array_position(ik, ni))"),
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
            c0 = time.perf_counter()
            res = e.sql(sql).table.to_pylist()
            ms = (time.perf_counter() - c0) * 1e3
        if i >= WARMUP:
            times.append(ms)
    return {"result": res[0]["s"], "ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
            "ms_max": round(max(times), 3), "host_steps_per_run": (sum(HOST_STEPS.values()) - h0) / (WARMUP + a.reps)}


out = {"package": ig.__file__, "rows": n, "entries": k, "reps": a.reps, "device": a.device}
for name, (lookup, composed) in CASES.items():
    calls = KERNEL_CALLS["map_lookup_idx"]
    # the two sides alternate inside one process: composed, lookup, composed, lookup
    c1, l1 = timed(f"select sum({composed}) s from t"), timed(f"select sum({lookup}) s from t")
    c2, l2 = timed(f"select sum({composed}) s from t"), timed(f"select sum({lookup}) s from t")
    assert l1["result"] == c1["result"] == l2["result"] == c2["result"], (name, l1, c1)
    assert dev.type != "cuda" or KERNEL_CALLS["map_lookup_idx"] > calls, name
    out[name] = {"map_lookup": [l1, l2], "composed": [c1, c2]}
print(json.dumps(out))
