"""The device routines of csrc/kernels/strpair.hip and the substr_index case
of strfunc.hip, compiled as host C++ into a stand-alone program under
AddressSanitizer / UBSan (csrc/tools/strpair_host.cpp): no access outside a
row, the result, the long-row counter or the scratch slab, and every distance
equal to a full-matrix oracle. GPU ASan is not available on the pool."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang")
def test_string_pair_routines_sanitizer_clean(tmp_path):
    k, t = os.path.join(ROOT, "csrc", "kernels"), os.path.join(ROOT, "csrc", "tools")
    shutil.copy(os.path.join(k, "strpair.hip"), tmp_path / "strpair.inc")
    shutil.copy(os.path.join(k, "strfunc.hip"), tmp_path / "strfunc.inc")
    shutil.copy(os.path.join(k, "kernels.h"), tmp_path / "kernels.h")
    shutil.copy(os.path.join(t, "strpair_host_shim.h"), tmp_path / "common.h")
    shutil.copy(os.path.join(t, "strpair_host.cpp"), tmp_path / "main.cpp")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("#pragma once\n")
    exe = str(tmp_path / "strpair_host")
    c = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{tmp_path}", "-x", "c++", str(tmp_path / "main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no sanitizer report" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
