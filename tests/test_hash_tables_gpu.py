"""The join and GROUP BY hash tables (csrc/kernels/hashtable.hip) at key and
shape edges against the independent references of tests/groupby_ref.py: a live
key equal to the empty-slot sentinel (twelve key sets, hashed tables at load
factor 0.5), int32 keys in hashed tables, direct tables at both ends of int64
probed from far outside, mixed key widths, a skewed build side, empty /
all-NULL / single-row sides, probe sizes off the 8192-row tile, and the sorted
run path. Cases and checkers live in tests/groupby_cases.py
(tests/test_groupby_ref.py runs them on the torch CPU paths); every checker
also asserts which table mode ran. Runs on a real MI355X."""
import pytest

import groupby_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(C.join_cases()))
def test_join_table_edges(gpu_device, name):
    C.check_join(name, gpu_device)


@pytest.mark.parametrize("name", sorted(C.group_cases()))
def test_group_ids_edges(gpu_device, name):
    C.check_group(name, gpu_device)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_sorted_run_path(gpu_device, dtype, monkeypatch):
    C.check_sorted_runs(dtype, gpu_device, monkeypatch)
