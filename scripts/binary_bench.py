"""Kernel times of the BINARY functions (csrc/kernels/binary.hip, blake2 in
digest.hip), BASELINE.md's "Binary functions" table.

    python scripts/binary_bench.py [--rounds 3] [--launches 30] [--device cuda:0]

Two shapes of random bytes built on the device: 4M rows of 8..64 bytes and
64K rows of 4 KiB. Per shape and round every kernel is timed alone with
device events: 3 warm-up launches, then the median of ``launches`` launches.
The existing ``str_case`` (upper) kernel over the same column, in the same
process and alternating with the others in every round, is the memory-bound
yardstick (one byte read, one written per byte). GB/s is bytes read plus
written (offsets included where the kernel reads them) over the median.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--device", default="cuda:0")
ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (a quick look: 0.01)")
a = ap.parse_args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402
import igloo_amd as ig  # noqa: E402
from igloo_amd import types as T  # noqa: E402
from igloo_amd.columnar import Column  # noqa: E402
from igloo_amd.ops import binary as BN  # noqa: E402
from igloo_amd.ops._lib import native, ptr, stream  # noqa: E402
from igloo_amd.ops.select import offsets_from_lengths  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("no GPU: a time taken elsewhere says nothing about the device path")
dev = torch.device(a.device)
N = native()
g = torch.Generator(device=dev)
g.manual_seed(11)


def column(n, lo, hi, kind="bytes") -> Column:
    lens = torch.randint(lo, hi + 1, (n,), generator=g, device=dev, dtype=torch.int64)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    if kind == "bytes":
        data = torch.randint(0, 256, (total,), generator=g, device=dev, dtype=torch.int64).to(torch.uint8)
    else:
        data = torch.randint(97, 123, (total,), generator=g, device=dev, dtype=torch.int64).to(torch.uint8)
        if kind == "two_byte":       # 10 % of the positions start a two-byte character (C3 A9), rows kept whole
            pos = torch.nonzero(torch.rand(total, generator=g, device=dev) < 0.05).flatten()
            last = off[1:] - 1
            pos = pos[~torch.isin(pos, last)]
            pos = pos[~torch.isin(pos - 1, pos)]
            data[pos] = 0xC3
            data[pos + 1] = 0xA9
    return Column(T.BINARY, data, None, offsets=off)


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(a.launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    return statistics.median(ts)


def shape(name, n, lo, hi):
    c = column(n, lo, hi)
    asc, two = column(n, lo, hi, "ascii"), column(n, lo, hi, "two_byte")
    assert BN.utf8_validate(asc) is None and BN.utf8_validate(two) is None
    s = stream(c.data)
    nb, offb = c.data.numel(), (n + 1) * 8
    hx, b64 = BN.encode(c, "hex"), BN.encode(c, "base64")
    out_case = torch.empty_like(c.data)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out_hex = torch.empty(2 * nb, dtype=torch.uint8, device=dev)
    out_bin = torch.empty(nb, dtype=torch.uint8, device=dev)
    err = torch.tensor([n, 0], dtype=torch.int64, device=dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    out_b64 = torch.empty(b64.data.numel(), dtype=torch.uint8, device=dev)
    dec_off, _ = offsets_from_lengths(c.offsets[1:] - c.offsets[:-1])
    flags = torch.empty(N.utf8_num_tiles(nb), dtype=torch.uint8, device=dev)
    dig = torch.empty(n * 128, dtype=torch.uint8, device=dev)
    nb64 = b64.data.numel()
    cases = {
        "str_case": (lambda: N.str_case(ptr(c.data), nb, True, ptr(out_case), ptr(flag), s), 2 * nb),
        "hex_encode": (lambda: N.bin_hex_encode(ptr(c.data), nb, ptr(out_hex), s), 3 * nb),
        "hex_validate": (lambda: N.bin_hex_validate(ptr(hx.offsets), ptr(hx.data), 0, n, 2 * nb, ptr(err), s),
                         2 * nb + offb),
        "hex_decode": (lambda: N.bin_hex_decode(ptr(hx.offsets), n, ptr(hx.data), nb, ptr(out_bin), s), 3 * nb),
        "b64_enc_lengths": (lambda: N.bin_b64_enc_lengths(ptr(c.offsets), 0, n, ptr(lens), s), 2 * offb),
        "b64_encode": (lambda: N.bin_b64_write(True, ptr(c.offsets), ptr(c.data), ptr(b64.offsets), n, nb64,
                                               ptr(out_b64), s), nb + nb64 + 2 * offb),
        "b64_dec_lengths": (lambda: N.bin_b64_dec_lengths(ptr(b64.offsets), ptr(b64.data), 0, n, nb64, ptr(lens),
                                                          ptr(err), s), nb64 + 2 * offb),
        "b64_decode": (lambda: N.bin_b64_write(False, ptr(b64.offsets), ptr(b64.data), ptr(dec_off), n, nb,
                                               ptr(out_bin), s), nb + nb64 + 2 * offb),
        "utf8_validate_ascii": (lambda: N.utf8_validate(ptr(asc.offsets), ptr(asc.data), 0, n, asc.data.numel(),
                                                        ptr(flags), ptr(err), s), asc.data.numel() + offb),
        "utf8_validate_two_byte": (lambda: N.utf8_validate(ptr(two.offsets), ptr(two.data), 0, n, two.data.numel(),
                                                           ptr(flags), ptr(err), s), 2 * two.data.numel() + offb),
        "blake2b": (lambda: N.digest_hex(5, ptr(c.offsets), ptr(c.data), n, ptr(dig), s), nb + offb + 128 * n),
    }
    rounds = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, (fn, _b) in cases.items():       # str_case first in every round, the others after it
            rounds[k].append(timed(fn))
    assert torch.equal(out_bin, c.data) and int(err[0]) == n      # the last decode gave the bytes back
    res = {"rows": n, "bytes": nb}
    base = statistics.median(rounds["str_case"])
    for k, (_fn, nbytes) in cases.items():
        ms = statistics.median(rounds[k])
        gbs = nbytes / (ms * 1e-3) / 1e9
        res[k] = {"ms": round(ms, 4), "gb_per_s": round(gbs, 1), "bytes": nbytes,
                  "ratio_to_str_case": round(gbs / (2 * nb / (base * 1e-3) / 1e9), 3),
                  "rounds_ms": [round(x, 4) for x in rounds[k]],
                  "spread_pct": round(100 * (max(rounds[k]) - min(rounds[k])) / ms, 1)}
    return name, res


out = {"package": ig.__file__, "device": torch.cuda.get_device_name(dev), "launches": a.launches, "rounds": a.rounds}
for nm, n, lo, hi in (("short_rows", int(4_000_000 * a.scale), 8, 64), ("long_rows", int(65_536 * a.scale), 4096, 4096)):
    k, v = shape(nm, max(n, 1), lo, hi)
    out[k] = v
print(json.dumps(out))
