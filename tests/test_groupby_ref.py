"""The torch CPU paths of the hash tables and grouped aggregates against the
independent references of tests/groupby_ref.py, over the case sets the GPU
tests run (tests/groupby_cases.py), and the references themselves against
hand-written literal cases. Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

import groupby_cases as C
import groupby_ref as R
from igloo_amd.ops import agg as A

NAN = math.nan
I64_MIN, I64_MAX = R.I64_MIN, R.I64_MAX


# ------------------------------------------------- the references, pinned
def test_group_ref_literal():
    groups, first = R.group_ref([5, I64_MIN, 5, -1, I64_MIN, I64_MAX, 5])
    assert groups == [[0, 2, 6], [1, 4], [3], [5]] and first == [0, 1, 3, 5]
    assert R.group_ref([]) == ([], [])


def test_join_ref_literal():
    build, bvalid = [7, I64_MIN, 7, 9, I64_MIN, 3], [True, True, True, False, True, True]
    probe, pvalid = [I64_MIN, 9, 7, 7, 4, 3], [True, True, True, False, True, True]
    counts, pairs, matched = R.join_ref(build, bvalid, probe, pvalid)
    assert counts == [2, 0, 2, 0, 0, 1]          # 9 is NULL on the build side, the second 7 on the probe side
    assert pairs == {(0, 1), (0, 4), (2, 0), (2, 2), (5, 5)}
    assert matched == {0, 1, 2, 4, 5}
    assert R.join_ref([1, 2], None, [I64_MIN], None) == ([0], set(), set())
    assert R.join_ref([], None, [1], None) == ([0], set(), set())


def test_agg_ref_literal_integers():
    gid = [0, 0, 1, -1, 1, 7, 0, 3]             # -1 and 7 lie outside [0, 4); group 2 has no row
    v = [I64_MAX, I64_MAX, I64_MIN, 99, I64_MIN, 99, 2, -6]
    ok = [True, True, True, True, True, True, True, False]      # group 3: a NULL row only
    assert R.agg_ref(gid, 4, "sum_int", v, None) == [2**64, -2**64, 0, -6]
    assert R.agg_ref(gid, 4, "sum_int", v, ok) == [2**64, -2**64, 0, 0]
    assert R.agg_ref(gid, 4, "count", None, ok) == [3, 2, 0, 0]
    assert R.agg_ref(gid, 4, "count", None, None) == [3, 2, 0, 1]
    assert R.agg_ref(gid, 4, "min_int", v, ok) == [2, I64_MIN, I64_MAX, I64_MAX]
    assert R.agg_ref(gid, 4, "max_int", v, ok) == [I64_MAX, I64_MIN, I64_MIN, I64_MIN]
    b = [-4, 6, 1, 0, -2, 0, 12, 5]             # -4 = ...11100, 6 = 00110, 12 = 01100
    assert R.agg_ref(gid, 4, "and_int", b, ok) == [4, 0, -1, -1]
    assert R.agg_ref(gid, 4, "or_int", b, ok) == [-2, -1, 0, 0]
    assert R.agg_ref(gid, 4, "xor_int", b, ok) == [-4 ^ 6 ^ 12, 1 ^ -2, 0, 0]
    assert -4 ^ 6 ^ 12 == -10 and 1 ^ -2 == -1
    assert R.agg_ref(None, 1, "sum_int", [1, 2, 3], [True, False, True]) == [4]
    assert R.agg_ref(None, 1, "count", None, None, n=5) == [5]


def test_agg_ref_literal_floats():
    gid = [0, 0, 0, 1, 1, 2, 2, 2, 3]
    x = [1.0, C.NAN_NEG, -2.0, C.NAN_POS, C.NAN_NEG, math.inf, -math.inf, -0.0, 5.0]
    mn = R.agg_ref(gid, 5, "min_f64", x, None)
    mx = R.agg_ref(gid, 5, "max_f64", x, None)
    # one NaN among numbers: MIN skips it, MAX is NaN; all NaN: both NaN; no row: the identities
    assert mn[0] == -2.0 and mn[1] != mn[1] and mn[2] == -math.inf and mn[3:] == [5.0, math.inf]
    assert mx[0] != mx[0] and mx[1] != mx[1] and mx[2] == math.inf and mx[3:] == [5.0, -math.inf]
    s, a, t = R.agg_ref(gid, 5, "sum_f64", [1e16, 1.0, -1e16, 0.5, 0.25, math.inf, -math.inf, 1.0, C.DENORM], None)
    assert s[0] == 1.0 and s[1] == 0.75 and s[2] != s[2] and s[3:] == [C.DENORM, 0.0]      # fsum: exact
    assert a[:2] == [2e16 + 1.0, 0.75] and a[2] == math.inf and t == [3, 2, 3, 1, 0]
    assert R.sum_bound(10.0, 1) == 0.0 and R.sum_bound(10.0, 0) == 0.0
    assert R.sum_bound(1.0, 3) == 2 * R.U / (1 - 2 * R.U)
    assert R.same_f64(C.NAN_NEG, NAN) and R.same_f64(-0.0, 0.0) and not R.same_f64(NAN, math.inf)


def test_cpu_min_max_f64_nan_order():
    """-inf < ... < +inf < NaN for a NaN of either sign (literal expectations)."""
    x = torch.from_numpy(np.array([1.0, C.NAN_NEG, 2.0, C.NAN_POS, -math.inf, 3.0]))
    assert x.view(torch.int64)[1] < 0 < x.view(torch.int64)[3]      # the sign bits survive
    gid = torch.tensor([0, 0, 1, 1, 2, 2], dtype=torch.int32)
    mn, mx = A.grouped_aggregate(gid, 4, [("min_f64", x, None), ("max_f64", x, None)], 6, "cpu")
    assert mn.tolist()[:1] == [1.0] and mn.tolist()[1:3] == [2.0, -math.inf] and mn.tolist()[3] == math.inf
    assert mx[0] != mx[0] and mx[1] != mx[1] and mx.tolist()[2:] == [3.0, -math.inf]
    only = A.grouped_aggregate(None, 1, [("min_f64", x[1:2].contiguous(), None)], 1, "cpu")[0]
    assert only[0] != only[0]       # nothing but a NaN: NaN


# ------------------------------------- the CPU paths over the shared cases
@pytest.mark.parametrize("name", sorted(C.join_cases()))
def test_join_table_cpu(name):
    C.check_join(name, "cpu")


@pytest.mark.parametrize("name", sorted(C.group_cases()))
def test_group_ids_cpu(name):
    C.check_group(name, "cpu")


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_sorted_runs_cpu(dtype, monkeypatch):
    C.check_sorted_runs(dtype, "cpu", monkeypatch)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("nagg", [8, 1])
@pytest.mark.parametrize("regime", C.REGIMES)
def test_grouped_aggregate_cpu(regime, nagg, masked, monkeypatch):
    C.check_agg(regime, nagg, masked, "cpu", monkeypatch)
