"""The format-program parser (parse_by_program of csrc/kernels/strptime.h) compiled as host C++
into a stand-alone program under AddressSanitizer / UBSan (csrc/tools/strptime_host.cpp) and fed
every case of tests/strptime_cases.py plus 100,000 random (program, text) pairs, half of them
valid texts and half with one byte changed, deleted or inserted: every line equals the Python
twin py_strptime and the sanitizers stay silent. The kernel's row guard (a byte range that is
negative, reversed or past the buffer) is exercised here only. The same header compiles into the
gfx950 kernel, which tests/test_strptime_gpu.py runs on the same cases."""
import os
import shutil
import subprocess

import pytest

import strptime_cases as K
from igloo_amd.ops import strptime as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("strptime_host")
    t = os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), d / "common.h")
    shutil.copy(os.path.join(t, "strptime_host.cpp"), d / "main.cpp")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n")
    out = str(d / "strptime_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{d}", f"-I{os.path.join(ROOT, 'csrc', 'kernels')}", "-x", "c++", str(d / "main.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    return out


def run(exe, lines):
    """lines: [(program, spec, text bytes)] -> one result per line: the integer, or None for 'bad'."""
    data = b"".join(p.hex().encode() + b"\t" + str(s).encode() + b"\t" + t + b"\n" for p, s, t in lines)
    r = subprocess.run([exe], input=data, capture_output=True, timeout=600)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, err[-4000:]
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert f"{len(lines)} cases, no sanitizer report" in err
    out = r.stdout.decode("utf-8").split("\n")[:-1]
    assert len(out) == len(lines)
    assert all(ln == "bad" or ln.startswith("ok\t") for ln in out)
    return [int(ln[3:]) if ln.startswith("ok\t") else None for ln in out]


def check(what, lines, want, got):
    bad = [(ln[0].hex(), ln[1], ln[2][:60], w, g) for ln, w, g in zip(lines, want, got) if w != g]
    print(f"{what}: {len(lines)} cases, {len(bad)} mismatches")
    assert not bad, f"{what}: {len(bad)} of {len(lines)} differ (program, unit, text, want, got): {bad[:10]}"


_PROGRAMS = {}


def program(formats):
    p = _PROGRAMS.get(formats)
    if p is None:
        p = _PROGRAMS[formats] = SP.compile_formats(formats)
    return p


def test_every_case_in_every_unit(exe):
    cases = [c for c in K.all_cases() if b"\n" not in c[1]]
    assert len(cases) == len(K.all_cases())
    lines, want = [], []
    generated = len(cases) - len(K.table_cases())
    for k, (formats, text, v) in enumerate(cases):
        # the table and a sample of the generated cases in all four units; the rest in one each, round robin
        for unit in (range(4) if k >= generated or k % 97 == 0 else (k % 4,)):
            lines.append((program(formats), unit, text))
            want.append(SP.py_strptime(text, program(formats), unit))
            name = ("micros", "millis", "seconds", "date")[unit]
            assert want[-1] == K.expect_unit(v, name), (formats, text, name)      # the twin is right about it
    assert None in want and len(lines) > len(cases)
    check("cases", lines, want, run(exe, lines))


def test_100000_random_pairs(exe):
    pairs = K.random_pairs(100_000, 4242)
    lines = [(program(f), k % 4, t) for k, (f, t) in enumerate(pairs)]
    want = [SP.py_strptime(t, p, u) for p, u, t in lines]
    n_ok = sum(w is not None for w in want)
    print(f"random pairs: {n_ok} match, {len(want) - n_ok} do not")
    assert n_ok >= 50_000 and len(want) - n_ok >= 25_000      # the valid half, and most mutations break the text
    check("random pairs", lines, want, run(exe, lines))


def test_row_guard_and_malformed_programs(exe):
    """A row outside the buffer is a failed row whose bytes are not read; a program that runs past
    its end (no END, a literal longer than what is left, an unknown op) matches nothing."""
    p = program(("%Y-%m-%d",))
    text = b"xx2024-04-03yy"
    v = K.us(2024, 4, 3)
    lines = [(p, "0:2:12:14", text), (p, "0:2:12:12", text), (p, "0:-1:12:14", text), (p, "0:12:2:14", text),
             (p, "0:2:15:14", text), (p, "0:2:1000000:14", text), (p, "0:-5:-2:14", text), (p, "0:14:14:14", text),
             (p, "0:2:12:11", text), (p, f"0:{1 << 40}:{(1 << 40) + 10}:14", text), (p, "3:2:12:14", text)]
    want = [v, v, None, None, None, None, None, None, None, None, v // K.US_DAY]
    broken = [p[:-1], p[:1], bytes([SP.OP_LIT]), bytes([SP.OP_LIT, 200, 0x32]), bytes([SP.OP_YEAR, 99, SP.OP_END]),
              b"", p + bytes([SP.OP_LIT, 5])]
    lines += [(b, 0, b"2024-04-03") for b in broken]
    want += [None, None, None, None, None, None, v]         # the last: the first format matched before the broken tail
    check("guards", lines, want, run(exe, lines))
