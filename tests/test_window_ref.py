"""The torch CPU path of igloo_amd/ops/window.py (the oracle of older GPU
tests) against the independent references of tests/window_ref.py, over the
case lists of tests/window_cases.py: the same lists
tests/test_window_kernels_gpu.py runs on the gfx950 kernels (all but its
4.2M-row carry-chunk case).
"""
import numpy as np
import pytest
import torch

import window_cases as C
import window_ref as R
from igloo_amd.ops import window as W

CPU = "cpu"


@pytest.mark.parametrize("n", C.SCAN_SIZES)
def test_seg_scan(n):
    for layout in C.LAYOUTS:
        C.check_scan(n, layout, CPU)


def test_seg_scan_overflow_flag():
    C.check_overflow(CPU)


def test_numpy_reference_matches_walker():
    """The vectorised per-segment reference (used for the one large GPU case)
    equals the Python walker at n = 5000."""
    n = 5000
    rng = np.random.default_rng(1)
    ids = C.layout_ids("geometric", n, rng)
    ids[:2300] = ids[0]
    ints = rng.integers(-1000, 1000, n, dtype=np.int64)
    full = C.scan_values(R.V_I64, R.MIN_I, n, rng)
    flt = C.scan_values(R.V_F64, R.MAX_F, n, rng)
    for vals, vkind, op in ((ints, R.V_I64, R.SUM_I), (full, R.V_I64, R.MIN_I), (full, R.V_I64, R.MAX_I),
                            (flt, R.V_F64, R.MIN_F), (flt, R.V_F64, R.MAX_F)):
        for rev in (False, True):
            want, _ = R.seg_scan_ref(ids, vals, vkind, op, n, None, None, rev)
            got = R.seg_scan_np(ids, vals, op, rev).tolist()
            assert all(R.same_f64(a, b) for a, b in zip(got, want)), (op, rev)


def test_findings_of_the_old_cpu_path():
    """The three edges at which the torch path used to differ from the kernels."""
    k = torch.tensor([2**63 - 10, 2**63 - 5, 2**63 - 1])
    z, last, r = torch.zeros(3, dtype=torch.int64), torch.full((3,), 2), torch.arange(3)
    lo, hi = W.bounds(3, z, last, r, r, "range", "current", None, "following", 100, key=k)
    assert (lo.tolist(), hi.tolist()) == ([0, 1, 2], [2, 2, 2])          # wrapped to hi = -1
    lo, hi = W.bounds(3, z, last, None, None, "rows", "preceding", 2**63 - 1, "following", 2**63 - 1)
    assert (lo.tolist(), hi.tolist()) == ([0, 0, 0], [2, 2, 2])          # wrapped to hi = -2**63
    x = torch.tensor([1.0, float("nan"), 0.5, 2.0], dtype=torch.float64)
    mn = W.seg_scan(None, x, W.V_F64, W.MIN_F, 4).tolist()
    mx = W.seg_scan(None, x, W.V_F64, W.MAX_F, 4).tolist()
    assert mn == [1.0, 1.0, 0.5, 0.5]                                    # NaN is the greatest value
    assert mx[0] == 1.0 and all(v != v for v in mx[1:])


@pytest.mark.parametrize("unit", ["rows", "groups"])
def test_bounds(unit):
    C.check_bounds(unit, "i64", False, "none", CPU)


@pytest.mark.parametrize("nulls", ["none", "first", "last"])
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_bounds_range(kind, desc, nulls):
    C.check_bounds("range", kind, desc, nulls, CPU)


def test_frame_sum():
    C.check_frame_sum(CPU)


@pytest.mark.parametrize("width", C.WIDTHS + ["mixed32", "mixed33"])
def test_frame_minmax(width):
    C.check_minmax(width, CPU)


@pytest.mark.parametrize("fn", [R.ROW_NUMBER, R.RANK, R.DENSE_RANK, R.PERCENT_RANK, R.CUME_DIST])
def test_rank(fn):
    C.check_rank(fn, 0, CPU)


@pytest.mark.parametrize("arg", [1, 2, 3, 7, C.RANK_PSIZE, C.RANK_PSIZE + 1, 10**6])
def test_ntile(arg):
    C.check_rank(R.NTILE, arg, CPU)


def test_index():
    C.check_index(CPU)


def test_sql_nan_order():
    C.check_sql_nan(CPU)


def test_sql_sum_overflow_contract():
    C.check_sql_overflow(CPU)
