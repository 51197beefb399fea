"""csrc/kernels/textparse.h compiled as host C++ into a stand-alone program
under AddressSanitizer / UBSan (csrc/tools/textparse_host.cpp) and fed every
case of tests/text_cases.py plus two million random float texts: each result
equals the Python expectation exactly (bits for doubles), each text that must
be rejected is, and the sanitizers stay silent. The float slow path is integer
only, so what is proven here holds bit for bit on the device, where
tests/test_text_values_gpu.py runs the same cases through the kernels."""
import os
import shutil
import subprocess

import pytest

import text_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("textparse_host")
    t = os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), d / "common.h")
    shutil.copy(os.path.join(t, "textparse_host.cpp"), d / "main.cpp")
    (d / "hip").mkdir()
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n")
    out = str(d / "textparse_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{d}", f"-I{os.path.join(ROOT, 'csrc', 'kernels')}", "-x", "c++", str(d / "main.cpp"), "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    return out


def run(exe, cases):
    """cases: [(kind, scale, text)] -> one result per case: the value text, or None for a rejection."""
    data = "".join(f"{k}\t{s}\t{t}\n" for k, s, t in cases).encode("utf-8")
    r = subprocess.run([exe], input=data, capture_output=True, timeout=600)
    err = r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, err[-4000:]
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert f"{len(cases)} cases, no sanitizer report" in err
    lines = r.stdout.decode("utf-8").split("\n")[:-1]
    assert len(lines) == len(cases)
    return [ln[3:] if ln.startswith("ok\t") else None for ln in lines]


def check(what, cases, want, got):
    bad = [(c[2][:80], w, g) for c, w, g in zip(cases, want, got) if w != g]
    print(f"{what}: {len(cases)} cases, {len(bad)} mismatches")
    assert not bad, f"{what}: {len(bad)} of {len(cases)} differ (text, want, got): {bad[:10]}"


def _hex(v):
    return None if v is None else "%016x" % C.bits(v)


def test_power_of_five_table_is_what_the_script_writes():
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_pow5_table.py"), "--check"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_float_cases(exe):
    cases = C.float_cases()
    inp = [("f", 0, t) for t, _ in cases]
    check("float", inp, [_hex(v) for _, v in cases], run(exe, inp))


def test_two_million_random_floats(exe):
    total = 0
    for chunk in range(4):
        texts = C.random_float_texts(500_000, 1000 + chunk)
        inp = [("f", 0, t) for t in texts]
        check(f"random floats {chunk}", inp, [_hex(float(t)) for t in texts], run(exe, inp))
        total += len(texts)
    assert total >= 2_000_000


def test_int_cases(exe):
    cases = C.int_cases()
    texts = [t for t, _ in cases] + C.random_int_texts(20_000, 21)
    inp = [("i", 0, t) for t in texts]
    want = [None if v is None else str(v) for v in map(C.expect_int, texts)]
    assert want[:len(cases)] == [None if v is None else str(v) for _, v in cases]
    check("int", inp, want, run(exe, inp))


def test_decimal_cases(exe):
    cases = [(t, s) for t, s, _ in C.decimal_cases()]
    for s in C.DECIMAL_SCALES:
        cases += [(t, s) for t in C.random_decimal_texts(10_000, s, 30 + s)]
    inp = [("d", s, t) for t, s in cases]
    want = [None if v is None else str(v) for v in (C.expect_decimal(t, s) for t, s in cases)]
    check("decimal", inp, want, run(exe, inp))


def test_date_cases(exe):
    cases = C.date_cases()
    texts = [t for t, _ in cases] + C.random_date_texts(20_000, 41)
    inp = [("t", 0, t) for t in texts]
    want = [None if v is None else str(v) for v in map(C.expect_date, texts)]
    check("date", inp, want, run(exe, inp))


def test_format_fixed(exe):
    cases = C.fixed_format_cases()
    inp = [("F", s, str(v)) for v, s, _ in cases]
    check("format_fixed", inp, [t for _, _, t in cases], run(exe, inp))


def test_format_date(exe):
    cases = C.date_format_cases()
    inp = [("D", 0, str(v)) for v, _ in cases]
    check("format_date", inp, [t for _, t in cases], run(exe, inp))


def test_parsed_text_round_trips(exe):
    """format -> parse gives the value back, for both inverse pairs."""
    fixed = C.fixed_format_cases()
    got = run(exe, [("d", s, t) for _, s, t in fixed])
    assert got == [str(v) for v, _, _ in fixed]
    dates = [(v, t) for v, t in C.date_format_cases() if len(t) == 10 and t[0] != "-" and not t.startswith("0000")]
    got = run(exe, [("t", 0, t) for _, t in dates])
    assert got == [str(v) for v, _ in dates]
