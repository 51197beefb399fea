"""The torch CPU paths of ORDER BY, top-k and the key-bit pair sort against the
independent reference of tests/sort_ref.py, over the case sets the GPU test
runs (tests/sort_cases.py), and the reference itself against hand-written
literal cases. Runs without a GPU."""
import math

import pytest

import sort_cases as C
import sort_ref as R

NAN = math.nan
NEG_NAN = float(C.F64_NAN[1])


# ------------------------------------------------- the reference, pinned
def test_argsort_ref_literal_floats():
    v = [2.0, NAN, -math.inf, 0.0, NEG_NAN, -0.0, math.inf, 5e-324, -5e-324, 2.0]
    assert math.copysign(1.0, NEG_NAN) < 0 and NEG_NAN != NEG_NAN
    # -inf < -denormal < -0.0 = 0.0 < denormal < 2.0 = 2.0 < inf < NaN = NaN; ties in row order
    assert R.argsort_ref([(v, False, False, None)], 10) == [2, 8, 3, 5, 7, 0, 9, 6, 1, 4]
    # DESC reverses the values, not the tied rows
    assert R.argsort_ref([(v, True, False, None)], 10) == [1, 4, 6, 0, 9, 7, 3, 5, 8, 2]


def test_argsort_ref_literal_nulls():
    v = [3, 1, 99, 2, -99, 1]
    ok = [True, True, False, True, False, True]        # the values under the NULL slots never matter
    assert R.argsort_ref([(v, False, True, ok)], 6) == [2, 4, 1, 5, 3, 0]
    assert R.argsort_ref([(v, False, False, ok)], 6) == [1, 5, 3, 0, 2, 4]
    assert R.argsort_ref([(v, True, True, ok)], 6) == [2, 4, 0, 3, 1, 5]      # NULLS FIRST whatever DESC says
    assert R.argsort_ref([(v, True, False, ok)], 6) == [0, 3, 1, 5, 2, 4]
    # most significant column first; the second one breaks the ties of the first, NULLs included
    w = [0, 1, 5, 0, 4, 0]
    assert R.argsort_ref([(v, False, True, ok), (w, True, False, None)], 6) == [2, 4, 1, 5, 3, 0]
    assert R.argsort_ref([(v, False, True, ok), (w, False, False, None)], 6) == [4, 2, 5, 1, 3, 0]
    assert R.argsort_ref([], 3) == [0, 1, 2]
    assert R.topk_ref([(v, False, True, ok)], 6, 3) == [2, 4, 1]
    assert R.topk_ref([(v, False, True, ok)], 6, 9) == [2, 4, 1, 5, 3, 0]
    assert R.argsort_ref([([True, False, True], False, False, None)], 3) == [1, 0, 2]
    assert R.argsort_ref([([C.I64_MAX, C.I64_MIN, 0], True, False, None)], 3) == [0, 2, 1]


def test_sort_pairs_ref_literal():
    keys = [0x1F3, -1, 0x0F0, 0x2F1, 0x003]
    # bits [4, 8): 0xF, 0xF, 0xF, 0xF, 0x0 -- everything else is ignored
    assert R.sort_pairs_ref(keys, [10, 11, 12, 13, 14], 4, 8, 32) == \
        ([0x003, 0x1F3, -1, 0x0F0, 0x2F1], [14, 10, 11, 12, 13])
    # all 32 / 64 bits: -1 is the greatest unsigned key
    assert R.sort_pairs_ref(keys, [0, 1, 2, 3, 4], 0, 32, 32)[1] == [4, 2, 0, 3, 1]
    assert R.sort_pairs_ref([-1, C.I64_MIN, C.I64_MAX, 0], [0, 1, 2, 3], 0, 64, 64)[1] == [3, 2, 1, 0]
    assert R.sort_pairs_ref([-1, C.I64_MIN, C.I64_MAX, 0], [0, 1, 2, 3], 63, 64, 64)[1] == [2, 3, 0, 1]


# ------------------------------------- the CPU paths over the shared cases
@pytest.mark.parametrize("n", C.ARGSORT_ROWS)
@pytest.mark.parametrize("name", sorted(C.ARGSORT_CASES))
def test_argsort_cpu(name, n):
    C.check_argsort(name, n, "cpu")


@pytest.mark.parametrize("n", C.PAIR_ROWS)
@pytest.mark.parametrize("kdt,begin,end", [(k, b, e) for k in sorted(C.PAIR_RANGES) for b, e in C.PAIR_RANGES[k]])
def test_sort_pairs_cpu(kdt, begin, end, n):
    C.check_sort_pairs(kdt, begin, end, n, "cpu")


@pytest.mark.parametrize("n", C.PAIR_ROWS)
def test_sort_pairs_single_digit_cpu(n):
    C.check_sort_pairs_single_digit(n, "cpu")


@pytest.mark.parametrize("k", C.TOPK_KS)
@pytest.mark.parametrize("name", sorted(C.TOPK_CASES))
def test_topk_cpu(name, k):
    C.check_topk(name, k, "cpu")
    C.check_topk_candidates(name, k, "cpu")


def test_topk_refinement_cpu():
    C.check_topk_refinement("cpu")


def test_sql_order_by_nullable_double_cpu():
    C.check_sql_order_by("cpu")
