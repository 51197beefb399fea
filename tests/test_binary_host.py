"""The device routines of csrc/kernels/binary.hip (hex / base64 validators and
writers, the UTF-8 automaton) and the blake2 compressors of digest.hip,
compiled as host C++ into a stand-alone program under AddressSanitizer /
UBSan (csrc/tools/binary_host.cpp). The program runs as its own process with
nothing preloaded and checks the cases of tests/binary_cases.py plus a few
thousand random rows against a table written here from Python's binascii /
base64 / hashlib / bytes.decode. GPU ASan is not available on the pool."""
import os
import random
import shutil
import subprocess

import pytest

import binary_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _hx(b: bytes) -> str:
    return b.hex() or "-"


def _table(path):
    rnd = random.Random(11)
    alpha = [b"a", b"Z", b"0", b"\x00", b"\xff", "é".encode(), "€".encode(), "\U0001F600".encode(), b"\xc3", b"\x80", b"="]
    vals = BC.base_values() + BC.alignment_rows() + BC.UTF8_VALID + BC.UTF8_INVALID + BC.UTF8_SPLIT
    vals += [rnd.randbytes(rnd.randrange(0, 80)) for _ in range(2000)]
    vals += [b"".join(rnd.choice(alpha) for _ in range(rnd.randrange(0, 30))) for _ in range(1000)]
    vals += [bytes(rnd.randrange(32, 127) for _ in range(rnd.randrange(4000, 9000))) for _ in range(3)]   # ASCII tiles
    with open(path, "w") as f:
        for v in vals:
            f.write(f"R {_hx(v)} {BC.b64_of(v) or '-'} {BC.blake2(v, 'blake2b')} {BC.blake2(v, 'blake2s')} "
                    f"{int(BC.utf8_ok(v))}\n")
        for v in BC.HEX_INVALID:
            f.write(f"XH {_hx(v)}\n")
        for v in BC.B64_INVALID:
            assert BC.b64_strict(v) is None, v
            f.write(f"XB {_hx(v)}\n")
        for v in BC.B64_VALID:
            f.write(f"VB {_hx(v)} {_hx(BC.b64_strict(v))}\n")
    return len(vals)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")
def test_binary_routines_sanitizer_clean(tmp_path):
    k, t = os.path.join(ROOT, "csrc", "kernels"), os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(k, "binary.hip"), tmp_path / "binary.inc")
    shutil.copy(os.path.join(k, "digest.hip"), tmp_path / "digest.inc")
    shutil.copy(os.path.join(k, "kernels.h"), tmp_path / "kernels.h")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), tmp_path / "common.h")
    shutil.copy(os.path.join(t, "binary_host.cpp"), tmp_path / "main.cpp")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("#pragma once\n")
    n = _table(tmp_path / "table.txt")
    assert n > 3000
    exe = str(tmp_path / "binary_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{tmp_path}", "-x", "c++", str(tmp_path / "main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe, str(tmp_path / "table.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no sanitizer report" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
