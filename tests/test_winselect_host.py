"""The routines of the framed order statistics (csrc/kernels/window_select.h: the merge-sort
tree's placement step, its descent, and the narrow-frame loop) compiled as host C++ into a
stand-alone program under AddressSanitizer / UBSan (csrc/tools/winselect_host.cpp) and fed random
arrays and frames, malformed ones included: every answer equals a brute-force sort of the frame
and the sanitizers stay silent. The same header compiles into the gfx950 kernels, which
tests/test_window_quantile_gpu.py runs."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")

I64MIN, I64MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("winselect_host")
    t = os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), d / "common.h")
    shutil.copy(os.path.join(t, "winselect_host.cpp"), d / "main.cpp")
    out = str(d / "winselect_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{d}", f"-I{os.path.join(ROOT, 'csrc', 'kernels')}", "-x", "c++", str(d / "main.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    return out


def brute(vals, ok, n, lo, hi, k):
    """The row holding rank k of the frame's valid (value, position) pairs, or -1."""
    if lo < 0 or hi >= n or hi < lo:
        return -1
    rows = sorted((vals[j], j) for j in range(lo, hi + 1) if ok[j])
    return rows[k][1] if 0 <= k < len(rows) else -1


def run(exe, cases):
    """cases: [(T, vals, ok, [(lo, hi, k0, k1, two)])] -> per case a list of (a, b, c, d), c = d = None
    where the loop was not run."""
    text = []
    for T, vals, ok, qs in cases:
        text.append(f"{T} {len(vals)} {len(qs)}")
        text.append(" ".join(map(str, vals)))
        text.append(" ".join(str(int(b)) for b in ok))
        text += [" ".join(map(str, q)) for q in qs]
    r = subprocess.run([exe], input="\n".join(text).encode() + b"\n", capture_output=True, timeout=600)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, err[-4000:]
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    nq = sum(len(c[3]) for c in cases)
    assert f"{len(cases)} cases, {nq} queries, no sanitizer report" in err
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == nq
    out, at = [], 0
    for c in cases:
        got = []
        for ln in lines[at:at + len(c[3])]:
            a, b, x, y = ln.split()
            got.append((int(a), int(b), None if x == "x" else int(x), None if y == "x" else int(y)))
        out.append(got)
        at += len(c[3])
    return out


def check(cases, results):
    bad = []
    for (T, vals, ok, qs), got in zip(cases, results):
        n = len(vals)
        for (lo, hi, k0, k1, two), (a, b, c, d) in zip(qs, got):
            w0 = brute(vals, ok, n, lo, hi, k0)
            w1 = brute(vals, ok, n, lo, hi, k1) if two else -1
            if (a, b) != (w0, w1) or (c is not None and (c, d) != (w0, w1)):
                bad.append((T, n, (lo, hi, k0, k1, two), (w0, w1), (a, b, c, d)))
    assert not bad, f"{len(bad)} differ (T, n, query, want, got): {bad[:10]}"


def values(rng, n, kind):
    if kind == "equal":
        return [7] * n
    if kind == "up":
        return list(range(-(n // 2), n - n // 2))
    if kind == "down":
        return list(range(n, 0, -1))
    if kind == "ties":
        return [rng.randrange(5) for _ in range(n)]
    if kind == "extreme":
        return [rng.choice((I64MIN, I64MIN + 1, -1, 0, 1, I64MAX - 1, I64MAX)) for _ in range(n)]
    return [rng.randrange(-1000, 1000) for _ in range(n)]


def validity(rng, n, kind):
    if kind == "all":
        return [1] * n
    if kind == "none":
        return [0] * n
    if kind == "last":
        return [0] * (n - 1) + [1] * min(n, 1)
    return [int(rng.random() > 0.3) for _ in range(n)]


def frames(rng, vals, ok, n, count):
    qs = []
    for _ in range(count):
        how = rng.randrange(8)
        if n == 0 or how == 0:        # malformed: outside [0, n), reversed, far away
            lo, hi = rng.choice(((-1, n - 1), (0, n), (-5, -2), (n, n + 3), (3, 1), (I64MIN, I64MAX), (I64MAX, I64MAX),
                                 (0, I64MAX), (I64MIN, 0), (n - 1, n - 2)))
        elif how == 1:
            lo, hi = 0, n - 1
        elif how == 2:
            lo = rng.randrange(n)
            hi = lo - 1
        elif how == 3:
            lo = rng.randrange(n)
            hi = min(n - 1, lo + rng.choice((0, 31, 32, 63, 64)))
        else:
            lo = rng.randrange(n)
            hi = rng.randrange(lo, n)
        c = sum(ok[lo:hi + 1]) if 0 <= lo <= hi < n else 0
        k0 = rng.choice((0, c - 1, (c - 1) // 2, c, -1, rng.randrange(-2, c + 3), I64MAX, I64MIN))
        k1 = rng.choice((c // 2, min(k0 + 1, max(c - 1, 0)), k0, c, -1, rng.randrange(-2, c + 3)))
        qs.append((lo, hi, k0, k1, int(rng.randrange(4) != 0)))
    return qs


def test_random_arrays_and_frames(exe):
    rng = random.Random(20240)
    cases = []
    for T in (1, 2, 8, 64, 2048):
        sizes = {0, 1, 2, 3, 5, 33, 64, 65, T - 1, T, T + 1, 2 * T + 3, 4 * T + 1} - {-1}
        for n in sorted(sizes):
            if n > 600 and T != 2048:
                continue
            for vk in ("equal", "up", "down", "ties", "extreme", "random"):
                for ok_kind in ("all", "some", "none", "last"):
                    if n > 600 and (vk, ok_kind) not in (("ties", "some"), ("random", "all"), ("down", "all"),
                                                         ("extreme", "some"), ("equal", "last")):
                        continue
                    vals = values(rng, n, vk)
                    ok = validity(rng, n, ok_kind)
                    cases.append((T, vals, ok, frames(rng, vals, ok, n, 40 if n <= 600 else 25)))
    print(f"{len(cases)} cases, {sum(len(c[3]) for c in cases)} queries")
    check(cases, run(exe, cases))


def test_frames_inside_a_null_stretch_and_the_loop_switch(exe):
    n = 200
    vals = [(i * 37) % 101 for i in range(n)]
    ok = [0 if 50 <= i < 120 else 1 for i in range(n)]
    qs = [(60, 100, 0, 0, 1), (50, 119, 0, 1, 1), (49, 119, 0, 1, 1), (50, 120, 0, 0, 1), (49, 120, 1, 2, 1)]
    for w in (1, 32, 33):
        for lo in (0, 17, 40, 119, n - w):
            c = sum(ok[lo:lo + w])
            qs += [(lo, lo + w - 1, 0, c - 1, 1), (lo, lo + w - 1, (c - 1) // 2, c // 2, 1), (lo, lo + w - 1, c, -1, 1)]
    cases = [(T, vals, ok, qs) for T in (4, 16, 2048)]
    check(cases, run(exe, cases))
