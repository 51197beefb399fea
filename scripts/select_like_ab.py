"""A/B timing of the compaction (select.hip tile_write) and segment-LIKE
(strings.hip like_stream / like_seg) kernels between two builds of the native
extension.

    python scripts/select_like_ab.py --so _ab/native_old.so --tag old
    python scripts/select_like_ab.py --tag new        (the in-tree build)
    python scripts/select_like_ab.py --like-only --rounds 3 --so _ab/a.so --so _ab/b.so

Times mask_to_indices over 600M / 60M-row masks at several selectivities and
LIKE '%special%requests%' over SF10 o_comment (15M strings), CUDA events,
median of 15 runs. --like-only times only LIKE, at the sizes of the SF100
suite: o_comment of SF100 (150M strings) and '%green%' over its p_name (20M).
Several --so (``tree`` = the in-tree build) are timed in one command, one
fresh process each, alternating for --rounds rounds."""
import argparse
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", action="append", default=None)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--like-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=1)
    a = ap.parse_args()
    sos = a.so or ["tree"]
    if len(sos) > 1 or a.rounds > 1:
        # one build per process (an extension module loads once), alternating
        import subprocess
        for rnd in range(a.rounds):
            for so in sos:
                tag = f"{os.path.basename(so)} r{rnd}"
                cmd = [sys.executable, os.path.abspath(__file__), "--so", so, "--tag", tag]
                subprocess.run(cmd + (["--like-only"] if a.like_only else []), check=True)
        return
    a.so = None if sos[0] == "tree" else sos[0]
    a.tag = a.tag or ("new" if a.so is None else os.path.basename(a.so))
    import torch
    if a.so:
        spec = importlib.util.spec_from_file_location("igloo_amd._native", a.so)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        sys.modules["igloo_amd._native"] = m
    import igloo_amd as ig
    from igloo_amd.ops import _lib
    from igloo_amd.ops import strings as S
    from igloo_amd.ops.select import mask_to_indices
    if a.so:
        _lib._native = sys.modules["igloo_amd._native"]
    dev = "cuda:0"

    def timed(fn, reps=15):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]
    from igloo_amd.models.tpch import datagen, schema

    def time_like(col, pats):
        for pat in pats:
            r = S.like(col, pat)
            ms = timed(lambda: S.like(col, pat))
            gbs = (col.data.numel() + 8 * len(col) + len(col)) / ms / 1e6
            print(f"[{a.tag}] like {pat} n={len(col)} bytes={col.data.numel()} hits={int(r.sum())}: "
                  f"{ms:.3f} ms ({gbs:.0f} GB/s of chars + offsets + result)", flush=True)
    if a.like_only:
        # the two columns as datagen makes them at SF100, without the other tables
        col = datagen.gen_text("words", torch.arange(150_000_000, device=dev), 6, 3, 12, dev, schema.WORDS)
        time_like(col, ("%special%requests%", "%Customer%Complaints%", "%requests"))
        del col
        torch.cuda.empty_cache()
        k = torch.arange(1, 20_000_001, device=dev, dtype=torch.int64)
        time_like(datagen.gen_text("distinct_words", k, 32, 5, 5, dev, schema.COLORS), ("%green%", "forest%"))
        return
    g = torch.Generator(device=dev).manual_seed(1)
    for n in (600_000_000, 60_000_000):
        u = torch.rand(n, device=dev, generator=g)
        for sel in (0.5, 0.1, 0.01):
            mask = u < sel
            ref = torch.nonzero(mask).flatten().to(torch.int32)
            got = mask_to_indices(mask)
            assert torch.equal(got, ref), "compaction mismatch"
            ms = timed(lambda: mask_to_indices(mask, total=ref.numel()))
            print(f"[{a.tag}] select n={n} sel={sel}: {ms:.3f} ms", flush=True)
        del u
    from igloo_amd.ops.select import exclusive_scan
    for n in (100_000_000, 10_000_000):
        c = torch.randint(0, 4, (n,), device=dev, dtype=torch.int32, generator=g)
        ex, tot = exclusive_scan(c)
        assert tot == int(c.sum()) and int(ex[-1]) == tot - int(c[-1]), "scan mismatch"
        ms = timed(lambda: exclusive_scan(c, host_total=False))
        print(f"[{a.tag}] scan n={n}: {ms:.3f} ms", flush=True)
    torch.cuda.empty_cache()
    e = ig.QueryEngine(device=dev)
    datagen.register(e, 10)
    time_like(e.sql_device("SELECT o_comment FROM orders").columns["o_comment"], ("%special%requests%", "%pending%"))


if __name__ == "__main__":
    main()
