"""Form choice and byte accounting of the sorted-key index (ops/hashing.py
rank_index_form / rank_index_nbytes / dense_form; utils/memory.py charges the
DENSE tag's tensors). No GPU: the tuples are set by hand."""
import torch

from igloo_amd.ops import hashing as H
from igloo_amd.utils import tags
from igloo_amd.utils.memory import derived_nbytes


def test_form_follows_distinct_count_and_span(monkeypatch):
    # nb rows, ndistinct keys, span key values
    assert H.rank_index_form(1000, 1000, 1000) == H.IDENTITY       # distinct, no holes: no table
    assert H.rank_index_form(1000, 1000, 4000) == H.RANK           # distinct, holes: rank level only
    assert H.rank_index_form(4000, 1000, 1000) == H.FLAT           # repeats, no holes: the flat table
    assert H.rank_index_form(4000, 1000, 1001) == H.RANK_STARTS    # repeats and one hole: both levels
    assert H.rank_index_form(1, 1, 1) == H.IDENTITY
    # distinct keys of which some lie outside the recorded range count as repeats: rows differ from ranks
    assert H.rank_index_form(1000, 900, 2000) == H.RANK_STARTS
    monkeypatch.setattr(H, "RANK_INDEX_STARTS", False)
    assert H.rank_index_form(4000, 1000, 1001) == H.FLAT
    assert H.rank_index_form(1000, 1000, 4000) == H.RANK
    assert H.RANK_INDEX_MIN_ENTRIES >= 1 << 16


def test_bytes_of_each_form(monkeypatch):
    # TPC-H SF100: orders.o_orderkey (150M distinct keys over 600M values), lineitem.l_orderkey (600M rows)
    span = 600_000_000
    flat = 4 * (span + 1)
    assert H.rank_index_nbytes(H.FLAT, 150_000_000, 150_000_000, span) == flat
    assert H.rank_index_nbytes(H.RANK, 150_000_000, 150_000_000, span) == 16 * (span // 64) == 150_000_000
    assert H.rank_index_nbytes(H.RANK_STARTS, 600_000_000, 150_000_000, span) == 150_000_000 + 4 * 150_000_001
    assert H.rank_index_nbytes(H.IDENTITY, 15_000_000, 15_000_000, 15_000_000) == 0
    assert H.rank_index_nbytes(H.RANK, 65, 65, 65 + 64) == 16 * 3      # a partly used last word
    monkeypatch.setattr(H, "INT32_MAX", 0)       # rows that need int64
    assert H.rank_index_nbytes(H.RANK_STARTS, 4000, 1000, 1001) == 16 * 16 + 8 * 1001
    assert H.rank_index_nbytes(H.FLAT, 4000, 1000, 1000) == 8 * 1001


def test_derived_bytes_charge_both_levels():
    """The index lives in the DENSE tag as ints, tensors and None: memory.py
    charges exactly its tensors, and dense_form reads the form back."""
    nb, nd, span = 4000, 1000, 1001
    nw = (span + 63) // 64
    entries = torch.zeros(2 * nw, dtype=torch.int64)
    starts = torch.zeros(nd + 1, dtype=torch.int32)
    for idx, form in (((0, span - 1, torch.zeros(span + 1, dtype=torch.int32)), H.FLAT),
                      ((0, span - 1, None, None, span), H.IDENTITY),
                      ((0, span - 1, None, entries, nd), H.RANK),
                      ((0, span - 1, starts, entries, nd), H.RANK_STARTS)):
        col = torch.zeros(8, dtype=torch.int32)
        tags.DENSE.set(col, idx)
        assert H.dense_form(idx) == form
        n = span if form == H.IDENTITY else nd
        rows = n if form in (H.IDENTITY, H.RANK) else nb
        assert derived_nbytes(col) == H.rank_index_nbytes(form, rows, n, span)
