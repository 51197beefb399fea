"""ORDER BY, ORDER BY ... LIMIT k and the key-bit pair sort
(csrc/kernels/sort.hip, igloo_amd/ops/sort.py) against tests/sort_ref.py at
float, NULL and width edges: NaN of either sign and any payload, +-inf, signed
zeros and denormals (also hidden under NULL slots), all-NaN and all-NULL
columns, int64 over its whole range and at exactly +-2^62 with a NULL flag (a
65-bit field), the narrow integer types at their extremes, constant columns,
key sets of exactly 64 and 65 bits, of three 64-bit groups and of 9 and 17
narrow columns; pair sorts with noise below ``begin_bit`` and at or above
``end_bit``; top-k cutting through ties and NULL runs, with the select's
refinement pass, and its candidate sets. Row counts sit on both sides of the
rank sort (512 rows), the one-workgroup sort (4096) and the tile edges. Every
comparison is exact equality of row ids; the checkers assert the path from the
thresholds and the launch counters. Cases live in tests/sort_cases.py
(tests/test_sort_ref.py runs them on the torch CPU path). Runs on a real
MI355X."""
import pytest

import sort_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", C.ARGSORT_ROWS)
@pytest.mark.parametrize("name", sorted(C.ARGSORT_CASES))
def test_argsort_edges(gpu_device, name, n):
    C.check_argsort(name, n, gpu_device)


@pytest.mark.parametrize("name", C.PACK_PERM_CASES)
def test_key_pack_perm_widths(gpu_device, name):
    C.check_pack_perm_widths(name, 4097, gpu_device)


@pytest.mark.parametrize("n", C.PAIR_ROWS)
@pytest.mark.parametrize("kdt,begin,end", [(k, b, e) for k in sorted(C.PAIR_RANGES) for b, e in C.PAIR_RANGES[k]])
def test_sort_pairs_bit_range(gpu_device, kdt, begin, end, n):
    C.check_sort_pairs(kdt, begin, end, n, gpu_device)


@pytest.mark.parametrize("n", C.PAIR_ROWS)
def test_sort_pairs_single_digit(gpu_device, n):
    C.check_sort_pairs_single_digit(n, gpu_device)


@pytest.mark.parametrize("k", C.TOPK_KS)
@pytest.mark.parametrize("name", sorted(C.TOPK_CASES))
def test_topk_edges(gpu_device, name, k):
    C.check_topk(name, k, gpu_device)


@pytest.mark.parametrize("k", C.TOPK_KS)
@pytest.mark.parametrize("name", sorted(C.TOPK_CASES))
def test_topk_candidates(gpu_device, name, k):
    C.check_topk_candidates(name, k, gpu_device)


def test_topk_refinement_pass(gpu_device):
    C.check_topk_refinement(gpu_device)


def test_sql_order_by_nullable_double(gpu_device):
    C.check_sql_order_by(gpu_device)
