"""The TRY_CAST element routines (parse_timestamp of csrc/kernels/textparse.h, the
checked conversions of csrc/kernels/castcheck.h) compiled as host C++ into a
stand-alone program under AddressSanitizer / UBSan (csrc/tools/trycast_host.cpp)
and fed the timestamp cases, every cast_checked edge case and one million random
(source, target, value) triples of tests/trycast_cases.py: each result equals the
Python expectation exactly and the sanitizers stay silent. The same code compiles
into the gfx950 kernels, which tests/test_try_cast_gpu.py runs on the same cases."""
import os
import shutil
import struct
import subprocess

import pytest

import trycast_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")

KIND = {"int8": 0, "int16": 1, "int32": 2, "int64": 3, "float32": 4, "float64": 5, "decimal": 6, "wide": 7}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("trycast_host")
    t = os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), d / "common.h")
    shutil.copy(os.path.join(t, "trycast_host.cpp"), d / "main.cpp")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n")
    out = str(d / "trycast_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{d}", f"-I{os.path.join(ROOT, 'csrc', 'kernels')}", "-x", "c++", str(d / "main.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    return out


def run(exe, lines):
    """lines: [(kind, spec, text)] -> one result per line: the integer, or None for a rejection."""
    data = "".join(f"{k}\t{s}\t{t}\n" for k, s, t in lines).encode("utf-8")
    r = subprocess.run([exe], input=data, capture_output=True, timeout=600)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, err[-4000:]
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert f"{len(lines)} cases, no sanitizer report" in err
    out = r.stdout.decode("utf-8").split("\n")[:-1]
    assert len(out) == len(lines)
    return [int(ln[3:]) if ln.startswith("ok\t") else None for ln in out]


def check(what, lines, want, got):
    bad = [(ln[1], ln[2][:60], w, g) for ln, w, g in zip(lines, want, got) if w != g]
    print(f"{what}: {len(lines)} cases, {len(bad)} mismatches")
    assert not bad, f"{what}: {len(bad)} of {len(lines)} differ (spec, input, want, got): {bad[:10]}"


def convert_line(src, dst, v):
    s_scale = src[2] if src[0] == "decimal" else src[1] if src[0] == "wide" else 0
    d_scale, d_prec = (dst[2], dst[1]) if dst[0] == "decimal" else (0, 0)
    if src[0] == "float64":
        text = "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]
    elif src[0] == "float32":
        text = "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    else:
        text = str(v)
    return "C", f"{KIND[src[0]]},{s_scale},{KIND[dst[0]]},{d_scale},{d_prec}", text


def test_timestamp_cases(exe):
    cases = K.timestamp_cases()
    # the multi-byte digit of the rejected list, and texts one byte short of each accepted form
    cases = list(cases) + [(t[:-1], None) for t, v in cases[:200] if v is not None and len(t) in (10, 16, 19)]
    lines = [("T", 0, t) for t, _ in cases if "\n" not in t and "\t" not in t]
    check("timestamp", lines, [v for _, v in cases], run(exe, lines))


def test_every_cast_checked_edge(exe):
    lines, want = [], []
    for src, dst, vals in K.convert_cases():
        for v in vals:
            lines.append(convert_line(src, dst, v))
            want.append(K.expect_convert(v, src, dst))
    assert None in want and len(want) > 5000
    check("cast_checked edges", lines, want, run(exe, lines))


def test_one_million_random_triples(exe):
    total = 0
    for chunk in range(4):
        triples = K.random_convert_triples(250_000, 900 + chunk)
        lines = [convert_line(*t) for t in triples]
        want = [K.expect_convert(v, src, dst) for src, dst, v in triples]
        K.assert_quarters(want, f"random triples {chunk}")
        check(f"random triples {chunk}", lines, want, run(exe, lines))
        total += len(lines)
    assert total >= 1_000_000
