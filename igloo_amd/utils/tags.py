"""Registry of the facts and derived buffers the engine remembers on tensors.

Operators avoid device-to-host readbacks by keeping what they learnt about a
tensor on the tensor object, as ``_igloo_*`` attributes. Each is declared here
with its meaning and read and written through its ``Tag`` only, so a misspelt
name fails at once instead of reading as "no fact". A tag never set reads None.
"""
from __future__ import annotations

from typing import Optional

import torch

FACT, LINEAGE, DERIVED_KIND, MEMO = "fact", "lineage", "derived", "memo"


class Tag:
    __slots__ = ("attr", "kind", "doc")

    def __init__(self, attr: str, kind: str, doc: str):
        self.attr, self.kind, self.doc = attr, kind, doc

    def get(self, t, default=None):
        return getattr(t, self.attr, default)

    def set(self, t, v) -> bool:
        """False when ``t`` takes no attributes (None, a slotted object): the caller goes without the tag."""
        try:
            setattr(t, self.attr, v)
        except (AttributeError, RuntimeError):
            return False
        return True

    def clear(self, t) -> None:
        if hasattr(t, self.attr):
            delattr(t, self.attr)


# ---- facts about the values; no device memory held
RESIDENT = Tag("_igloo_resident", FACT, "True: a table column that outlives the query (catalog._mark_resident)")
INCR = Tag("_igloo_incr", FACT, "True: a strictly increasing row index (ops/select.py mask rows, ops/hashing.py probe hits)")
DISTINCT = Tag("_igloo_distinct", FACT, "True: no value twice (exec/aggregate.py lone GROUP BY key; kept by inherit_take)")
SORTED = Tag("_igloo_sorted", FACT, "None: unchecked; True / False: non-decreasing or not (is_sorted; True kept by inherit_take)")
UNIQUE = Tag("_igloo_unique", FACT, "None: unchecked; True / False: a resident column's values all differ (key_unique)")
BOUND = Tag("_igloo_bound", FACT, "(lo, hi) holding every value, set by the producer: group ids, dictionary codes, JIT results")
STATS = Tag("_igloo_stats", FACT, "((min, max) or None, non-decreasing?) of a NULL-free key tensor (ops/hashing.py column_stats)")
RANGE = Tag("_igloo_range", FACT, "(first, last) key of a sorted tensor, read back once (ops/hashing.py _dense_index_build)")
HASHED = Tag("_igloo_hashed", FACT, "True: 64-bit hashes, so group_ids reads no key range (ops/strings.py)")
INDEX_KEYS = Tag("_igloo_index_keys", FACT, "True: the sorted keys of a resident column's perm index, as long-lived as the column")
NDV = Tag("_igloo_ndv", FACT, "estimated number of distinct values, sketched once (exec/joins.py)")
# ---- lineage: which resident column the values came from
BASE = Tag("_igloo_base", LINEAGE, "(source Column, its rows): rows of the source in row order (exec/scan.py _tag_base)")
ORIGIN = Tag("_igloo_origin", LINEAGE, "the resident column every value was gathered from (inherit_take)")
# ---- derived: device buffers built once on a resident column and charged to it (utils/memory.py)
NARROW = Tag("_igloo_narrow", DERIVED_KIND, "narrowest integer copy, or the column itself when none is narrower (exec/fused.py)")
PERM = Tag("_igloo_perm", DERIVED_KIND, "(keys in sorted order, int32 row permutation) (ops/hashing.py perm_index)")
DENSE = Tag("_igloo_dense", DERIVED_KIND, "None: not tried; False: too sparse; (kmin, kmax, first) lower-bound table, or a large resident column's "
            "(kmin, kmax, starts | None, entries | None, ndistinct) rank index (dense_index)")
HLL = Tag("_igloo_hll", DERIVED_KIND, "HyperLogLog registers, uint8 [4096] (ops/hashing.py hll_sketch)")
FENCE = Tag("_igloo_fence", DERIVED_KIND, "every 256th key of a sorted column (ops/hashing.py search_fence)")
PACKED = Tag("_igloo_packed", DERIVED_KIND, "row-packed copies of column sets, on a set's first column (ops/packed_gather.py)")
# ---- memo: remembered results that the cache budget does NOT see
KEY_HIST = Tag("_igloo_key_hist", MEMO, "(kmin, span, rows-per-key device histogram), not charged (exec/aggregate.py)")
SLICES = Tag("_igloo_slices", MEMO, "dict of a rank's slice plans and column views, not charged (parallel/slicing.py)")
TC = Tag("_igloo_tc", MEMO, "(per-tile set-row counts, mask._version); consumed (set to None) by the next count (ops/select.py)")

#: the structures charged to their column (every tag of kind "derived"), in accounting order, and their attribute names
CHARGED = (NARROW, PERM, DENSE, HLL, FENCE, PACKED)
DERIVED = tuple(t.attr for t in CHARGED)


def base_column(t: torch.Tensor) -> Optional[torch.Tensor]:
    """A filtered scan's source tensor, when ``t`` still holds its values as they are (same dtype)."""
    base = BASE.get(t)
    return base[0].data if base is not None and base[0].data.dtype == t.dtype else None


def origin(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The resident table column every value of ``t`` was gathered from (no
    negative rows), or None: ``t`` itself, the origin a gather inherited, or a
    filtered scan's source. ops/hashing.py key_bound takes key ranges from it."""
    if RESIDENT.get(t, False):
        return t
    o = ORIGIN.get(t)
    if o is None and (b := base_column(t)) is not None:
        o = origin(b)
    return o


def inherit_take(dst: torch.Tensor, src: torch.Tensor, idx, sorted: bool = True, distinct: bool = True) -> None:
    """Tags of ``dst = src[idx]`` (no negative rows). ``idx``: the index
    tensor, or True for rows kept in order without one (mask compaction). The
    origin carries over; through a strictly increasing index a sorted source
    stays sorted and a distinct one distinct, unless the caller turns that off."""
    if (o := origin(src)) is not None:
        ORIGIN.set(dst, o)
    if idx is True or INCR.get(idx, False):
        if sorted and SORTED.get(src) is True:
            SORTED.set(dst, True)
        if distinct and DISTINCT.get(src, False):
            DISTINCT.set(dst, True)
