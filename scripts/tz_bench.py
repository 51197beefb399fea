"""Throughput of the tz kernels (csrc/kernels/tz.hip) beside the naive date_trunc('hour') pass.

64 Mi rows of America/New_York timestamps, once in random order and once sorted. Each case is timed
with device events around 200 calls after 3 warm-ups, in two alternating rounds. GB/s counts the
bytes a single pass has to move: the input read plus the output written. The naive yardstick is two
ATen launches with an intermediate tensor, so it moves more than it is credited with; its column
compares whole passes, not kernels. Every timed output is compared with the CPU twin on a 1 Mi-row
sample.

Usage: python scripts/tz_bench.py [OUT.json]   (one MI355X)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from igloo_amd.exec.expr_eval import trunc_ts  # noqa: E402
from igloo_amd.ops import timezone as TZ  # noqa: E402
from igloo_amd.utils import tzdb  # noqa: E402

N = 64 * 1024 * 1024
ZONE = "America/New_York"
DEVICE = "cuda:0"
REPS = 200
WARMUP = 3

CASES = {
    "tz_to_local": lambda x: TZ.to_local(x, ZONE),
    "tz_trunc_day": lambda x: TZ.trunc(x, ZONE, "day"),
    "tz_part_hour": lambda x: TZ.part(x, ZONE, "hour"),
    "tz_to_utc": lambda x: TZ.to_utc(x, ZONE),
    "tz_to_local_fixed": lambda x: TZ.to_local(x, "+05:30"),
    "naive_trunc_hour": lambda x: trunc_ts(x, "hour"),
}


def timed(fn, x):
    """Mean milliseconds per call and the last output."""
    for _ in range(WARMUP):
        fn(x)
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        out = fn(x)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / REPS, out


def main():
    tzdb.set_tz_dir(os.path.join(ROOT, "tests", "golden", "tz"))
    gen = torch.Generator(device=DEVICE)
    gen.manual_seed(7)
    rand = torch.randint(0, 2_208_988_800_000_000, (N,), dtype=torch.int64, device=DEVICE, generator=gen)   # 1970 .. 2040
    inputs = (("random", rand), ("sorted", torch.sort(rand).values))
    sample = torch.arange(0, N, 64, device=DEVICE) + 1
    results, same = {}, True
    for _ in range(2):
        for name, fn in CASES.items():
            for label, x in inputs:
                ms, out = timed(fn, x)
                moved = N * (8 + out.element_size())
                results.setdefault(f"{name}/{label}", []).append({"ms": round(ms, 4), "GBps": round(moved / ms / 1e6, 1)})
                same = same and bool((out[sample].cpu() == fn(x[sample].cpu())).all())
    report = {"rows": N, "zone": ZONE, "device": torch.cuda.get_device_name(0), "sample_equals_cpu": same,
              "results": results}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
