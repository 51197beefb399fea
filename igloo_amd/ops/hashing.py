"""Hash-join tables and GROUP BY encoding (csrc/kernels/hashtable.hip).

``JoinTable`` builds once on the (smaller) build side and supports the probe
shapes the join operator needs: full pair expansion (inner / outer), first
match (unique build keys, semi/anti), and build-side "matched" flags (right /
full outer). ``group_ids`` maps int64 group keys to dense group ids.

CPU tensors use a sort + searchsorted reference implementation.
"""
from __future__ import annotations

from ..utils import switches as _sw
import contextvars
from typing import List, Optional, Sequence, Tuple

import torch

from ..utils import tags
from .gather import origin as _origin
from ._lib import capturing, check_not_capturing, is_gpu, launch, native, ptr, stream, to_host_f64s, to_host_int, to_host_ints, unlogged
from .select import exclusive_scan, mask_to_indices

EMPTY_KEY = -(2**63)
INT32_MAX = 2**31 - 1
BLOOM_MAX_KEYS = 4 << 20   # build sides up to this size get a Bloom filter
BLOOM_MIN_RATIO = 4        # ... used when probe rows >= ratio x build rows
EXACT_BITMAP = True
EXACT_BITMAP_MAX_SPAN = 1 << 25   # direct tables up to this key span use an exact bitmap instead
#: join build keys whose [min, max] span is at most this use the direct-mapped
#: table (one random read per probe) whatever the build size: 2^26 slots is a
#: 256 MB head array, small next to 288 GB of HBM
DIRECT_JOIN_MAX_SPAN = 1 << 26

#: bytes one join table may take under an engine device budget (set around a
#: query's execution by engine.py); None = unbounded. A direct-mapped table is
#: sized by the key span, not the build rows: a grace partition or a streamed
#: semi-join build side keeps the whole span of its keys
TABLE_BYTES_LIMIT: "contextvars.ContextVar[Optional[int]]" = contextvars.ContextVar("igloo_table_bytes", default=None)
#: first-match probes that only select rows use the two-pass hit-bit kernels
PROBE_SELECT = True


def _next_pow2(x: int) -> int:
    p = 1
    while p < x:
        p <<= 1
    return p


def column_stats(keys: torch.Tensor, valid: Optional[torch.Tensor] = None) -> Tuple[Optional[Tuple[int, int]], bool]:
    """((min, max) of the non-NULL keys or None, non-decreasing?) — one pass of
    csrc/kernels/util.hip and one host sync on the GPU. Remembered on resident
    key columns (no validity)."""
    if valid is None:
        hit = tags.STATS.get(keys)
        if hit is not None:
            return hit
    n = keys.numel()
    if not is_gpu(keys) or keys.dtype not in (torch.int32, torch.int64):
        k = keys if valid is None else keys[valid]
        if k.numel() == 0:
            return None, True
        mn, mx = torch.aminmax(k)
        srt = True if k.numel() < 2 else bool((k[1:] >= k[:-1]).all().item())
        return (int(mn.item()), int(mx.item())), srt
    N = launch("column_stats")
    buf = torch.empty(N.STATS_SLOTS, dtype=torch.int64, device=keys.device)   # result + per-block partials
    N.column_stats(ptr(keys.contiguous()), keys.dtype == torch.int64,
                   ptr(valid.contiguous() if valid is not None else None), n, ptr(buf), stream(keys))
    out = buf[:3]
    if valid is None and tags.RESIDENT.get(keys, False):
        with unlogged():      # remembered below: a one-time build (ops/_lib.py unlogged)
            mn, mx, bad = to_host_ints(out)
    else:
        mn, mx, bad = to_host_ints(out)
    res = ((mn, mx) if mn <= mx else None), (bad == 0 and valid is None)
    if valid is None:
        # remembered on any key tensor (like is_sorted's flag): a sortedness
        # check followed by a range lookup of the same keys (group_ids_ex ->
        # group_ids, inner_pairs -> JoinTable) reads the stats back once
        if tags.STATS.set(keys, res) and tags.RESIDENT.get(keys, False):
            tags.SORTED.set(keys, res[1])
    return res


def key_range(keys: torch.Tensor, valid: Optional[torch.Tensor] = None) -> Optional[Tuple[int, int]]:
    return column_stats(keys, valid)[0]


#: below this many keys a readback-free bound that rules out the direct table
#: is trusted (hash table, no range readback); above it the exact range is read,
#: since a filtered subset may still fit a direct table (far cheaper at size)
BOUND_TRUST_ROWS = 1 << 20


#: IGLOO_DEBUG=key_tags (tests set CHECK_KEY_TAGS directly): verify every
#: readback-free key fact (key_unique tags, key_bound intervals) against the
#: data it describes, one readback each
CHECK_KEY_TAGS = _sw.debug("key_tags")


def _check_bound(keys: torch.Tensor, b: Tuple[int, int]) -> Tuple[int, int]:
    if CHECK_KEY_TAGS and keys.numel() and not capturing():
        lo, hi = to_host_ints(torch.stack([keys.min().to(torch.int64), keys.max().to(torch.int64)]))
        if lo < b[0] or hi > b[1]:
            raise AssertionError(f"key_bound {b} does not hold the keys' range [{lo}, {hi}]")
    return b


def key_bound(keys: torch.Tensor) -> Optional[Tuple[int, int]]:
    """An interval holding every key, known without a readback in steady
    state: the (remembered) range of the resident column the keys were
    gathered from, or a bound its producer attached (``_igloo_bound``:
    dictionary codes lie in [0, dictionary size)). Looser than ``key_range``
    for a filtered subset; callers use it where a bound suffices
    (direct-mapped table spans, bit widths, overflow-free sums)."""
    b = tags.BOUND.get(keys)
    if b is not None:
        return _check_bound(keys, b)
    o = _origin(keys)
    if o is None or o.dtype != keys.dtype or o.dim() != 1:
        return None
    st = tags.STATS.get(o)
    if st is None:
        if capturing():
            return None
        st = column_stats(o)
    return _check_bound(keys, st[0]) if st[0] is not None else None


#: unsorted resident key columns up to this many rows get a one-time
#: uniqueness check (sorted ones: one adjacent-difference pass at any size)
UNIQUE_CHECK_MAX_ROWS = 1 << 27


def _check_unique(keys: torch.Tensor, why: str) -> bool:
    """IGLOO_DEBUG=key_tags: a tag-derived uniqueness must hold on the data."""
    if CHECK_KEY_TAGS and keys.numel() > 1 and not capturing():
        n = keys.numel()
        u = torch.unique(keys.to(torch.int64)).numel()
        if u != n:
            raise AssertionError(f"key_unique() trusted {why} on {n} keys with {n - u} duplicates")
    return True


def key_unique(keys: torch.Tensor) -> bool:
    """True only when the keys are known distinct with no readback in steady
    state: a single GROUP BY key (``_igloo_distinct``, kept through filters
    that select rows in order, ops/gather.py take_many), distinct rows (a resident column, or a filtered scan's rows of one,
    in row order) of a resident column whose values are unique (checked once
    and remembered on it)."""
    if tags.DISTINCT.get(keys, False):
        return _check_unique(keys, "a distinct tag")
    o = keys if tags.RESIDENT.get(keys, False) else tags.base_column(keys)
    if o is None or not tags.RESIDENT.get(o, False):
        return False
    u = tags.UNIQUE.get(o)
    if u is None:
        if capturing() or not is_gpu(o) or o.dim() != 1:
            return False
        if TABLE_BYTES_LIMIT.get() is not None or (o.numel() > UNIQUE_CHECK_MAX_ROWS and not is_sorted(o)):
            # under a device budget, or an unsorted column too large for a
            # one-time group-by pass: not known unique (the build's own
            # duplicate check decides)
            return False
        with unlogged():     # one-time check of a resident column (ops/_lib.py unlogged)
            n = o.numel()
            if n < 2:
                u = True
            elif column_stats(o)[1]:
                u = to_host_int((o[1:] == o[:-1]).any().to(torch.int64)) == 0
            else:
                u = group_ids(o)[1] == n
        if not tags.UNIQUE.set(o, u):
            return False
    return u and _check_unique(keys, "the resident base column's uniqueness" if o is not keys else
                               "a resident column's uniqueness")


def _keys_ok(k: torch.Tensor) -> torch.Tensor:
    assert k.dim() == 1 and k.dtype in (torch.int32, torch.int64), f"join keys must be int32/int64, got {k.dtype}"
    return k.contiguous()


def _key_column(keys: torch.Tensor, valid: Optional[torch.Tensor] = None):
    """A build or probe key column (``_keys_ok`` keys, optional validity mask)
    as the native join entry points take it (csrc/kernels/kernels.h KeyColumn)."""
    return native().KeyColumn(ptr(keys), keys.dtype == torch.int64, ptr(valid), keys.numel())


class JoinTable:
    """Hash table over build-side keys (int32/int64; NULL keys never match)."""

    def __init__(self, keys: torch.Tensor, valid: Optional[torch.Tensor] = None, defer_unique: bool = False):
        """``defer_unique``: the build's duplicate count is read back only when
        ``unique`` is first asked -- or together with the first
        ``probe_select``'s hit total (one readback for both)."""
        keys = _keys_ok(keys)
        self.n = n = keys.numel()
        self._dups = None
        self.device = keys.device
        self.gpu = is_gpu(keys)
        self.valid = valid
        rng = None
        if valid is None and self.gpu:
            # a resident-derived bound that already selects the direct table
            # (the exact range could only narrow it): no range readback
            bnd = key_bound(keys)
            if bnd is not None and (self._direct_for(bnd[1] - bnd[0] + 1, n) or n < BOUND_TRUST_ROWS):
                rng = bnd
        if rng is None:
            rng = key_range(keys, valid)
        self.empty = rng is None
        if self.empty:
            self.unique = True
            return
        self.kmin, kmax = rng
        span = kmax - self.kmin + 1
        self.direct = self._direct_for(span, n)
        if not self.gpu:
            # NULL rows leave before the sort (no key value is free to park
            # them behind the others: the keys may reach INT64_MAX)
            rows = None if valid is None else torch.nonzero(valid).reshape(-1)
            k = keys if rows is None else keys.index_select(0, rows)
            sk, order = torch.sort(k.to(torch.int64), stable=True)
            if rows is not None:
                order = rows.index_select(0, order)
            self.sorted_keys, self.order = sk, order
            self.unique = bool((sk[1:] != sk[:-1]).all().item()) if sk.numel() > 1 else True
            return
        known_unique = valid is None and key_unique(keys)
        N = launch("join_build")
        self.cap = span if self.direct else _next_pow2(2 * n)
        # entries of every per-slot array: a hashed table keeps one reserved
        # slot past its cap probed ones for the key equal to EMPTY_KEY
        # (csrc/kernels/hashtable.hip home_slot)
        self.slots = self.cap if self.direct else self.cap + 1
        # Bloom filter for selective probes: ~8 bits per key, at most 4 MB (L2-resident)
        self.bits, self.bmask, self._fold = None, 0, None
        if self.direct and EXACT_BITMAP and span <= EXACT_BITMAP_MAX_SPAN:
            # exact membership bitmap over the key span (<= 4 MB, L2-resident):
            # no false positives (csrc/kernels/hashtable.hip kExactBits)
            self.bits = torch.empty((span + 31) // 32, dtype=torch.int32, device=self.device)
            self.bmask = 1 << 63
        elif n <= BLOOM_MAX_KEYS:
            nbits = min(max(_next_pow2(8 * n), 1 << 15), 1 << 25)
            self.bits = torch.empty(nbits // 32, dtype=torch.int32, device=self.device)
            self.bmask = nbits - 1
        # row ids: int32 below 2^31 build rows, int64 above
        self.rid = torch.int32 if n < INT32_MAX else torch.int64
        self.rid64 = self.rid == torch.int64
        self.thead = torch.empty(self.slots, dtype=self.rid, device=self.device)
        self.tkeys = torch.empty(1 if self.direct else self.slots, dtype=torch.int64, device=self.device)
        dups = torch.empty(1, dtype=torch.int64, device=self.device)
        st = stream(keys)
        # thead = -1, tkeys = EMPTY_KEY (hashed), bits = 0, dups = 0: one launch
        N.join_table_init(ptr(self.thead), self.rid64, self.slots, 0 if self.direct else ptr(self.tkeys),
                          ptr(self.bits), 0 if self.bits is None else self.bits.numel(), ptr(dups), st)
        self.cstart = self.crows = None
        self._set_ref()
        N.join_build(self._ref, _key_column(keys, valid), ptr(dups), st)
        if known_unique and CHECK_KEY_TAGS and not capturing():
            # debug / test mode: the tag-derived uniqueness must match the build's own duplicate count
            if to_host_int(dups) != 0:
                raise AssertionError("key_unique() trusted a key tag on keys that hold duplicates")
        self._csr_src = (keys, valid)
        if known_unique:
            self._unique = True
        elif defer_unique:
            self._unique, self._dups = None, dups
        else:
            self._set_unique(to_host_int(dups) == 0)

    @property
    def unique(self) -> bool:
        if self._unique is None:
            self._set_unique(to_host_int(self._dups) == 0)
        return self._unique

    @unique.setter
    def unique(self, v: bool) -> None:
        self._unique = v

    def _set_unique(self, u: bool) -> None:
        """Record the build's uniqueness; duplicate keys get CSR runs (count ->
        exclusive scan -> scatter), so a multi-match probe reads one
        contiguous run of build rows."""
        self._unique, self._dups = u, None
        if not u:
            keys, valid = self._csr_src
            col = _key_column(keys, valid)
            st = stream(keys)
            cnt = torch.zeros(self.slots + 1, dtype=self.rid, device=self.device)
            launch("join_csr_count").join_csr_count(self._ref, col, ptr(cnt), st)
            self.cstart = torch.zeros(self.slots + 1, dtype=self.rid, device=self.device)
            torch.cumsum(cnt[:-1], 0, dtype=self.rid, out=self.cstart[1:])
            self.crows = torch.empty(self.n, dtype=self.rid, device=self.device)
            self._set_ref()
            launch("join_csr_scatter").join_csr_scatter(self._ref, col, ptr(cnt), st)

    def _set_ref(self) -> None:
        """The table as the native entry points take it (csrc/kernels/kernels.h
        JoinTableRef): made after the build's buffers exist, and again when
        the CSR runs or the fold scratch are added."""
        self._ref = native().JoinTableRef(
            tkeys=ptr(self.tkeys), thead=ptr(self.thead), cstart=ptr(self.cstart), crows=ptr(self.crows),
            rid64=self.rid64, cap=self.cap, kmin=self.kmin, direct=self.direct, bits=ptr(self.bits),
            bmask=self.bmask, fold=ptr(self._fold), n_build=self.n)

    @staticmethod
    def _direct_for(span: int, n: int) -> bool:
        lim = TABLE_BYTES_LIMIT.get()
        # (head + CSR start/count arrays: up to 3 int32 words per slot)
        wide_ok = span <= DIRECT_JOIN_MAX_SPAN and (lim is None or 12 * span <= lim)
        return span < 2**31 - 1 and (span <= 4 * n + 4096 or wide_ok)

    # ----------------------------------------------------------------- probes
    def probe_first(self, pkeys: torch.Tensor, pvalid: Optional[torch.Tensor] = None,
                    build_matched: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One matching build row per probe row (-1 if none). Exact for unique builds;
        with duplicates it returns an arbitrary match (enough for semi/anti joins)."""
        self.unique      # a deferred duplicate count is read now (CSR runs built if any)
        pkeys = _keys_ok(pkeys)
        m = pkeys.numel()
        if self.empty or m == 0:
            return torch.full((m,), -1, dtype=torch.int32, device=pkeys.device)
        if not self.gpu:
            cnt, lo = self._cpu_ranges(pkeys, pvalid)
            first = torch.where(cnt > 0, self.order.index_select(0, lo.clamp(max=max(self.order.numel() - 1, 0))),
                                torch.full_like(lo, -1)).to(torch.int32)
            if build_matched is not None:
                self._cpu_mark(cnt, lo, build_matched)
            return first
        first = torch.empty(m, dtype=self.rid, device=pkeys.device)
        launch("join_probe").join_probe(self._ref, _key_column(pkeys, pvalid), self._use_filter(m), 0, ptr(first),
                                        ptr(build_matched), stream(pkeys))
        return first

    def probe_select(self, pkeys: torch.Tensor, pvalid: Optional[torch.Tensor] = None, negate: bool = False,
                     want_build: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Probe rows with a match (``negate``: without one), in row order, and
        for matches their (first) build row — what ``probe_first`` + compaction
        give, in two passes that never write a per-row result (GPU)."""
        pkeys = _keys_ok(pkeys)
        m = pkeys.numel()
        dev = pkeys.device
        if not self.gpu or self.empty or m == 0 or not PROBE_SELECT:
            first = self.probe_first(pkeys, pvalid)      # resolves a deferred ``unique``
            if not self.unique and want_build and not negate:
                return None     # duplicate build keys: the caller takes the multi-match probe (as the GPU path)
            sel = mask_to_indices(first < 0 if negate else first >= 0)
            return sel, (first.index_select(0, sel.long()) if want_build and not negate else None)
        N = launch("probe_hits")
        st = stream(pkeys)
        col = _key_column(pkeys, pvalid)
        tiles = N.probe_hit_tiles(m)
        words = torch.empty(tiles * 128, dtype=torch.int64, device=dev)
        tcount = torch.empty(tiles, dtype=torch.int64, device=dev)
        use_filter = self._use_filter(m)
        if use_filter:
            self._fold_scratch(m, st)
        N.probe_hits(self._ref, col, use_filter, negate, ptr(words), ptr(tcount), st)
        if self._unique is None:
            # deferred duplicate count: read back with the hit total (one sync);
            # duplicate build keys leave the pairs to the multi-match probe
            toff, tdev = exclusive_scan(tcount, host_total=False)
            dups, total = to_host_ints(torch.cat([self._dups.reshape(-1)[:1], tdev.reshape(-1)[:1]]))
            self._set_unique(dups == 0)
            if dups and want_build and not negate:
                return None
        else:
            toff, total = exclusive_scan(tcount)
        it = torch.int32 if m < INT32_MAX else torch.int64
        pidx = torch.empty(total, dtype=it, device=dev)
        bidx = torch.empty(total, dtype=self.rid, device=dev) if want_build and not negate else None
        if total:
            N.probe_write(self._ref, col, ptr(words), ptr(toff), ptr(pidx), it == torch.int64, ptr(bidx),
                          pidx.numel(), st)
        tags.INCR.set(pidx, True)    # hit rows in row order
        return pidx, bidx

    def probe_pairs(self, pkeys: torch.Tensor, pvalid: Optional[torch.Tensor] = None,
                    build_matched: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """All (probe_row, build_row) matches, grouped by probe row.
        Returns (probe_idx int32, build_idx (int32 below 2^31 build rows, else int64),
        counts int32 per probe row)."""
        self.unique      # a deferred duplicate count is read now (CSR runs built if any)
        pkeys = _keys_ok(pkeys)
        m = pkeys.numel()
        dev = pkeys.device
        if self.empty or m == 0:
            z = torch.zeros(0, dtype=torch.int32, device=dev)
            return z, z, torch.zeros(m, dtype=torch.int32, device=dev)
        if not self.gpu:
            cnt, lo = self._cpu_ranges(pkeys, pvalid)
            if build_matched is not None:
                self._cpu_mark(cnt, lo, build_matched)
            total = int(cnt.sum().item())
            pidx = torch.repeat_interleave(torch.arange(m), cnt)
            starts = torch.cumsum(cnt, 0) - cnt
            within = torch.arange(total) - starts.index_select(0, pidx)
            bpos = lo.index_select(0, pidx) + within
            bidx = self.order.index_select(0, bpos)
            return pidx.to(torch.int32), bidx.to(torch.int32), cnt.to(torch.int32)
        if m >= INT32_MAX:
            raise ValueError(f"probe_pairs: {m} probe rows exceed int32 probe ids; split the probe side")
        N = launch("join_probe")
        s = stream(pkeys)
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        col = _key_column(pkeys, pvalid)
        use_filter = self._use_filter(m)
        N.join_probe(self._ref, col, use_filter, ptr(counts), 0, ptr(build_matched), s)
        offsets, total = exclusive_scan(counts)
        pidx = torch.empty(total, dtype=torch.int32, device=dev)
        bidx = torch.empty(total, dtype=self.rid, device=dev)
        if total:
            launch("join_expand")
            N.join_expand(self._ref, col, use_filter, ptr(offsets), ptr(pidx), ptr(bidx), pidx.numel(), s)
        return pidx, bidx, counts

    def _use_filter(self, m: int) -> bool:
        """Use the Bloom filter only when the probe side is much larger than the
        build side (then most probes are expected to miss)."""
        return self.bits is not None and m >= BLOOM_MIN_RATIO * self.n

    def _bloom(self, m: int) -> Tuple[int, int]:
        """(filter words, bmask) a probe of ``m`` rows consults; (0, 0): none."""
        return (ptr(self.bits), self.bmask) if self._use_filter(m) else (0, 0)

    def _fold_scratch(self, m: int, st: int) -> None:
        """The exact bitmap folded to the 64 KiB that probe_hits' fold kernels
        keep in LDS, for bitmaps wider than that: computed by the first probe
        that uses the filter and takes one of them, and kept with the table."""
        N = native()
        if self._fold is None and self.direct and self.bmask >> 63 and N.probe_fold_needed(m, self.cap):
            self._fold = torch.empty(N.kFoldWords, dtype=torch.int32, device=self.device)
            N.probe_fold_build(ptr(self.bits), self.cap, ptr(self._fold), st)
            self._set_ref()

    # ------------------------------------------------------------ cpu helpers
    def _cpu_ranges(self, pkeys, pvalid):
        pk = pkeys.to(torch.int64)
        lo = torch.searchsorted(self.sorted_keys, pk, right=False)
        hi = torch.searchsorted(self.sorted_keys, pk, right=True)
        cnt = hi - lo
        if pvalid is not None:
            cnt = torch.where(pvalid, cnt, torch.zeros_like(cnt))
        return cnt, lo

    def _cpu_mark(self, cnt, lo, build_matched):
        total = int(cnt.sum().item())
        if total == 0:
            return
        pidx = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
        starts = torch.cumsum(cnt, 0) - cnt
        bpos = lo.index_select(0, pidx) + torch.arange(total) - starts.index_select(0, pidx)
        build_matched.index_fill_(0, self.order.index_select(0, bpos).long(), True)


#: inputs at least this large are checked for sorted (clustered) keys first
SORTED_CHECK_ROWS = 1 << 20

def is_sorted(keys: torch.Tensor) -> bool:
    """Non-decreasing check (one pass; remembered on the tensor object, so the
    resident key columns of a table are checked once)."""
    hit = tags.SORTED.get(keys)
    if hit is not None:
        if hit and CHECK_KEY_TAGS and not capturing() and not tags.RESIDENT.get(keys, False) \
                and keys.numel() > 1 and keys.is_cuda:
            # test mode: a sortedness tag inferred through gathers must hold
            if to_host_int((keys[1:] < keys[:-1]).any().to(torch.int64)):
                raise AssertionError("an inferred sorted tag does not hold")
        return hit
    base = tags.base_column(keys)
    if base is not None and is_sorted(base):
        # a filtered scan's rows of a sorted source column, in row order
        # (exec/scan.py _tag_base): sorted without another pass (the
        # source's flag is computed once and remembered on it)
        return True
    r = keys.numel() < 2 or column_stats(keys)[1]
    tags.SORTED.set(keys, r)
    return r


DENSE_INDEX = True
DENSE_INDEX_MIN_QUERIES = 1 << 20   # below this a binary search per query is cheaper than building
DENSE_INDEX_MAX_SPAN_RATIO = 4      # table entries per indexed row (orders: 1 of 4 key values used)


def dense_index(big: torch.Tensor, build: bool = True, queries: Optional[int] = None):
    """Key-value index of a sorted key column (csrc/kernels/ranges.hip), or
    None when the key span is too sparse. Remembered on the tensor object
    (resident table columns build it once). Its form (``dense_form``):

    * ``(kmin, kmax, first)``: the flat lower-bound table, first[k - kmin] =
      first row whose key >= k. Every index of fewer than
      ``RANK_INDEX_MIN_ENTRIES`` entries, every intermediate's, and large
      resident columns whose keys repeat and leave no hole.
    * ``(kmin, kmax, starts, entries, ndistinct)``: a large resident column's
      two-level index (``rank_index_form``). ``entries`` holds per 64 key
      values a presence word and the distinct keys before it, ``starts`` the
      first row of each distinct key (``ndistinct + 1`` rows). Distinct keys
      need no ``starts`` (None: row = rank); distinct keys without holes no
      ``entries`` either (None: row = k - kmin)."""
    hit = tags.DENSE.get(big)
    # (the sorted keys of a resident column's secondary index live as long as
    # the column: their table is built once too -- Q9's 1.1M green parts
    # searched 600M l_partkey keys by bisection, 0.93 ms per query)
    resident = tags.RESIDENT.get(big, False) or tags.INDEX_KEYS.get(big, False)
    if hit or (hit is False and (queries is None or resident)):
        return hit or None
    if resident:
        # built once and kept with the resident column: every later lookup
        # reuses it, so only its size matters, not this call's lookup count
        # (lineitem.l_orderkey at SF100: 2.4 GB of int32 for 600M rows)
        if queries is None or queries < DENSE_RESIDENT_MIN_QUERIES:
            return None
        with unlogged():
            return _dense_index_build(big, None, resident=True)
    if not build:
        return None
    rng = tags.RANGE.get(big)
    if hit is False and rng is not None and rng[1] - rng[0] + 1 > _dense_limit(big.numel(), queries):
        return None           # still too sparse for this many lookups: nothing to build
    return _dense_index_build(big, queries)    # an intermediate: built (and read back) every execution


#: resident columns: lookups per call that justify building the table once,
#: and the largest table (entries) worth its HBM when the keys are sparser
#: than DENSE_INDEX_MAX_SPAN_RATIO (a hash-partitioned rank's slice of a fact
#: table keeps the whole key span)
DENSE_RESIDENT_MIN_QUERIES = 4096
DENSE_RESIDENT_MAX_ENTRIES = 1 << 30


def _dense_limit(nb: int, queries: Optional[int], resident: bool = False) -> int:
    """Largest key span worth a table: small next to both the indexed rows and
    the lookups it serves (resident columns: next to the rows, or 4 GiB)."""
    if resident:
        return max(DENSE_INDEX_MAX_SPAN_RATIO * nb, DENSE_RESIDENT_MAX_ENTRIES) + 4096
    return DENSE_INDEX_MAX_SPAN_RATIO * min(nb, queries if queries is not None else nb) + 4096


#: index entries (key span + 1) from which a resident column's index takes the
#: two-level forms. Below it the flat table stays: 2^20 int32 entries are
#: 4 MiB, one XCD's L2, so its lookups are served on chip and a smaller
#: structure saves no HBM traffic, while the rank level adds a popcount and
#: (for repeated keys) a dependent load. SF100's supplier keys (1M) stay flat;
#: customer (15M), part (20M), orders and lineitem (600M key values) do not.
RANK_INDEX_MIN_ENTRIES = 1 << 20
#: False: columns with repeated keys and holes keep the flat table
RANK_INDEX_STARTS = not _sw.debug("rank_flat_starts")

FLAT, IDENTITY, RANK, RANK_STARTS = "flat", "identity", "rank", "rank+starts"


def rank_index_form(nb: int, ndistinct: int, span: int) -> str:
    """Form of the index over ``nb`` sorted rows holding ``ndistinct``
    different keys in a span of ``span`` key values: distinct keys need no
    starts level, keys without holes no rank level (the flat table is the
    starts level under an identity rank)."""
    if ndistinct == nb:
        return IDENTITY if nb == span else RANK
    return FLAT if ndistinct == span or not RANK_INDEX_STARTS else RANK_STARTS


def rank_index_nbytes(form: str, nb: int, ndistinct: int, span: int) -> int:
    """Device bytes of an index of that form (what utils/memory.py charges)."""
    width = 8 if nb >= INT32_MAX else 4
    if form == FLAT:
        return (span + 1) * width
    entries = 16 * ((span + 63) // 64) if form in (RANK, RANK_STARTS) else 0
    return entries + ((ndistinct + 1) * width if form == RANK_STARTS else 0)


def dense_form(idx) -> str:
    """Which form a ``dense_index`` result has."""
    if len(idx) == 3:
        return FLAT
    _, _, starts, entries, _ = idx
    return IDENTITY if entries is None else RANK if starts is None else RANK_STARTS


def _rank_index_build(big: torch.Tensor, kmin: int, kmax: int):
    """The two-level index of a resident column (ranges.hip): presence bits
    from the run starts, an exclusive scan of their popcounts, and the run
    starts scattered to their ranks. None when the form is the flat table."""
    nb, span = big.numel(), kmax - kmin + 1
    nw = (span + 63) // 64
    N = launch("rank_index_build")
    st, key64, dev = stream(big), big.dtype == torch.int64, big.device
    entries = torch.zeros(2 * nw, dtype=torch.int64, device=dev)     # 16 bytes each: (word, rank)
    N.rank_index_bits(ptr(big), key64, nb, kmin, kmax, ptr(entries), st)
    counts = torch.empty(nw, dtype=torch.int32, device=dev)
    N.rank_index_counts(ptr(entries), nw, ptr(counts), st)
    off, nd = exclusive_scan(counts)
    form = rank_index_form(nb, nd, span)
    if form == FLAT:
        return None
    if form == IDENTITY:
        return (kmin, kmax, None, None, nd)
    N.rank_index_finish(ptr(entries), nw, ptr(off), st)
    if form == RANK:
        return (kmin, kmax, None, entries, nd)
    starts = torch.empty(nd + 1, dtype=torch.int64 if nb >= INT32_MAX else torch.int32, device=dev)
    N.rank_index_starts(ptr(big), key64, nb, kmin, kmax, ptr(entries), ptr(starts), starts.dtype == torch.int64, nd, st)
    return (kmin, kmax, starts, entries, nd)


def _flat_index_build(big: torch.Tensor, kmin: int, kmax: int):
    nb, span = big.numel(), kmax - kmin + 1
    it = torch.int64 if nb >= INT32_MAX else torch.int32
    first = torch.empty(span + 1, dtype=it, device=big.device)
    gap = torch.zeros(1, dtype=torch.int32, device=big.device)
    N = launch("dense_index_build")
    st = stream(big)
    N.dense_index_build(ptr(big), big.dtype == torch.int64, nb, kmin, kmax, ptr(first),
                        it == torch.int64, ptr(gap), st)
    if to_host_int(gap):
        # long key gaps: rebuild over a -1 fill, then search the entries left at -1
        first.fill_(-1)
        N.dense_index_build(ptr(big), big.dtype == torch.int64, nb, kmin, kmax, ptr(first),
                            it == torch.int64, ptr(gap), st)
        N.dense_index_build(ptr(big), big.dtype == torch.int64, nb, kmin, kmax, ptr(first),
                            it == torch.int64, 0, st)
    return (kmin, kmax, first)


def _dense_index_build(big: torch.Tensor, queries: Optional[int], resident: bool = False):
    nb = big.numel()
    idx = False
    if nb:
        rng = tags.RANGE.get(big)
        if rng is None:
            rng = tuple(to_host_ints(torch.stack([big[0].to(torch.int64), big[-1].to(torch.int64)])))
            tags.RANGE.set(big, rng)
        kmin, kmax = rng
        span = kmax - kmin + 1
        if span <= _dense_limit(nb, queries, resident):
            idx = None
            # (resident columns only: an intermediate's index is rebuilt every
            # execution, where the scan's readback would cost more than it saves;
            # ranks are 32-bit)
            if resident and span + 1 > RANK_INDEX_MIN_ENTRIES and span < 2**32:
                idx = _rank_index_build(big, kmin, kmax)
            if idx is None:
                idx = _flat_index_build(big, kmin, kmax)
    tags.DENSE.set(big, idx)
    return idx or None


def sorted_ranges(big: torch.Tensor, q: torch.Tensor, qvalid: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """For each probe key q[i]: (lo, cnt) with big[lo : lo+cnt] == q[i] (big non-decreasing).
    GPU: one fused search kernel (csrc/kernels/ranges.hip)."""
    big = _keys_ok(big)
    q = q.to(big.dtype).contiguous()
    nq = q.numel()
    if not is_gpu(big):
        lo = torch.searchsorted(big, q)
        cnt = torch.searchsorted(big, q, right=True) - lo
        if qvalid is not None:
            cnt = torch.where(qvalid, cnt, torch.zeros_like(cnt))
        return lo, cnt
    lo = torch.empty(nq, dtype=torch.int64, device=big.device)
    cnt = torch.empty(nq, dtype=torch.int64, device=big.device)
    idx = dense_index(big, build=nq >= DENSE_INDEX_MIN_QUERIES, queries=nq) if DENSE_INDEX else None
    if idx and len(idx) > 3:
        kmin, kmax, starts, entries, nd = idx
        launch("rank_ranges").rank_ranges(ptr(entries), ptr(starts), starts is not None and starts.dtype == torch.int64,
                                          nd, kmin, kmax, ptr(q), q.dtype == torch.int64,
                                          ptr(qvalid.contiguous() if qvalid is not None else None), nq, ptr(lo),
                                          ptr(cnt), stream(big))
        return lo, cnt
    if idx:
        kmin, kmax, first = idx
        launch("dense_ranges").dense_ranges(ptr(first), first.dtype == torch.int64, kmin, kmax, ptr(q),
                                            q.dtype == torch.int64,
                                            ptr(qvalid.contiguous() if qvalid is not None else None), nq, ptr(lo),
                                            ptr(cnt), stream(big))
        return lo, cnt
    fence = search_fence(big) if SEARCH_FENCE else None
    launch("sorted_ranges").sorted_ranges(ptr(big), big.dtype == torch.int64, big.numel(), ptr(q),
                                          ptr(qvalid.contiguous() if qvalid is not None else None), nq, ptr(lo),
                                          ptr(cnt), ptr(fence), 0 if fence is None else fence.numel(), stream(big))
    return lo, cnt


def unique_lookup(big: torch.Tensor, q: torch.Tensor, qvalid: Optional[torch.Tensor] = None
                  ) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """``sorted_ranges`` into DISTINCT sorted keys (``key_unique(big)``):
    (hit bool mask, int32 row in ``big``; 0 on a miss) per probe key. None
    when ``big`` has 2^31 rows or more (the caller takes ``sorted_ranges``).
    GPU: one kernel writing 5 bytes per probe row (csrc/kernels/ranges.hip
    unique_lookup) through the dense index when the column has one."""
    big = _keys_ok(big)
    nb = big.numel()
    if nb >= 2**31 - 1:
        return None
    q = q.to(big.dtype).contiguous()
    nq = q.numel()
    if not is_gpu(big):
        lo = torch.searchsorted(big, q)
        hit = lo < nb
        if nb:
            hit &= big[lo.clamp(max=nb - 1)] == q
        if qvalid is not None:
            hit &= qvalid
        return hit, torch.where(hit, lo, torch.zeros_like(lo)).to(torch.int32)
    hit = torch.empty(nq, dtype=torch.bool, device=big.device)
    pos = torch.empty(nq, dtype=torch.int32, device=big.device)
    qv = ptr(qvalid.contiguous()) if qvalid is not None else 0
    idx = dense_index(big, build=nq >= DENSE_INDEX_MIN_QUERIES, queries=nq) if DENSE_INDEX else None
    if idx and len(idx) > 3:
        kmin, kmax, starts, entries, nd = idx
        launch("rank_unique").rank_unique(ptr(entries), ptr(starts), starts is not None and starts.dtype == torch.int64,
                                          nd, kmin, kmax, ptr(q), q.dtype == torch.int64, qv, nq, ptr(hit), ptr(pos),
                                          stream(big))
        return hit, pos
    N = launch("unique_lookup")
    if idx:
        kmin, kmax, first = idx
        N.unique_lookup(0, big.dtype == torch.int64, nb, ptr(first), first.dtype == torch.int64, kmin, kmax, ptr(q),
                        qv, nq, ptr(hit), ptr(pos), 0, 0, stream(big))
    else:
        fence = search_fence(big) if SEARCH_FENCE else None
        N.unique_lookup(ptr(big), big.dtype == torch.int64, nb, 0, False, 0, 0, ptr(q), qv, nq, ptr(hit), ptr(pos),
                        ptr(fence), 0 if fence is None else fence.numel(), stream(big))
    return hit, pos


SEARCH_FENCE = True
SEARCH_FENCE_MIN_ROWS = 1 << 22


def search_fence(big: torch.Tensor) -> Optional[torch.Tensor]:
    """Every 256th key of a large sorted RESIDENT key column (1/256 of its
    bytes, kept with it like the other derived structures): binary searches
    first narrow to one 256-row window through it (L2/MALL-resident), then
    touch only that window of the column (csrc/kernels/ranges.hip)."""
    if big.numel() < SEARCH_FENCE_MIN_ROWS or not tags.RESIDENT.get(big, False):
        return None
    hit = tags.FENCE.get(big)
    if hit is None:
        check_not_capturing("search fence of a resident column")
        hit = big[::native().SEARCH_FENCE].contiguous()
        if not tags.FENCE.set(big, hit):
            return None
    return hit


def perm_index(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Secondary index of an unsorted resident key column: (keys in sorted
    order, int32 row permutation), built once per column tensor (the stable
    radix sort of ops/sort.py) and kept with it like the other derived
    structures (charged to the column in the HBM cache budget) —
    a join with a much smaller side then reads only the matching ranges
    instead of probing every row of the column."""
    hit = tags.PERM.get(keys)
    if hit is not None:
        return hit
    from .sort import perm_sort_int
    with unlogged():
        out = perm_sort_int(keys)
    if tags.SORTED.set(out[0], True) and tags.INDEX_KEYS.set(out[0], True):
        tags.PERM.set(keys, out)
    return out


def expand_ranges(lo: torch.Tensor, cnt: torch.Tensor, big_n: int, scanned=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """All pairs (s, lo[s] + k), k < cnt[s], grouped by s (int32 when they fit).
    ``scanned``: the caller's ``exclusive_scan(cnt)`` result, reused."""
    ns = lo.numel()
    dev = lo.device
    off, total = scanned if scanned is not None else exclusive_scan(cnt)
    it = torch.int32 if max(total, big_n, ns) < INT32_MAX else torch.int64
    if not is_gpu(lo):
        sidx = torch.repeat_interleave(torch.arange(ns, dtype=it), cnt, output_size=total)
        bidx = (lo.index_select(0, sidx.long()) - off.index_select(0, sidx.long())
                + torch.arange(total, dtype=torch.int64)).to(it)
        return sidx, bidx
    sidx = torch.empty(total, dtype=it, device=dev)
    bidx = torch.empty(total, dtype=it, device=dev)
    if total:
        launch("expand_ranges").expand_ranges(ptr(off), ptr(lo.contiguous()), ns, total, ptr(sidx), ptr(bidx),
                                              it == torch.int64, stream(lo))
    return sidx, bidx


def sorted_match_pairs(big1: torch.Tensor, big2: torch.Tensor, small1: torch.Tensor, small2: torch.Tensor,
                       identity_ok: bool = False) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """(small row, big row) pairs with big1 == small1 and big2 == small2, big1
    non-decreasing (ranges on the first key, then the second key checked inside
    each range on the device). Grouped by small row. ``identity_ok``: when
    every small row has exactly one match (Q9's lineitem into partsupp's
    (partkey, suppkey) key) the small side comes back as None and the count
    pass's first matches are the big rows: no scan, no write pass."""
    lo, cnt = sorted_ranges(big1, small1)
    ns = small1.numel()
    big2 = _keys_ok(big2)
    small2 = small2.to(big2.dtype).contiguous()
    if not is_gpu(big1):
        s, b = expand_ranges(lo, cnt, big1.numel())
        keep = big2.index_select(0, b.long()) == small2.index_select(0, s.long())
        return s[keep], b[keep]
    N = launch("sorted_match")
    st = stream(big1)
    counts = torch.empty(max(ns, 1), dtype=torch.int32, device=big1.device)
    k64 = big2.dtype == torch.int64
    first = torch.empty(ns, dtype=torch.int32, device=big1.device) \
        if identity_ok and ns and max(big1.numel(), ns) < INT32_MAX else None
    N.sorted_match(ptr(big2), ptr(small2), k64, ptr(lo), ptr(cnt), ns, ptr(counts), 0, 0, 0, False, 0, ptr(first), st)
    if first is not None:
        c = counts[:ns]
        total, odd = to_host_ints(torch.stack([c.sum(), (c != 1).sum()]))
        if odd == 0:
            return None, first
        off, _ = exclusive_scan(c, host_total=False)
    else:
        off, total = exclusive_scan(counts[:ns])
    it = torch.int32 if max(total, big1.numel(), ns) < INT32_MAX else torch.int64
    sidx = torch.empty(total, dtype=it, device=big1.device)
    bidx = torch.empty(total, dtype=it, device=big1.device)
    if total:
        N.sorted_match(ptr(big2), ptr(small2), k64, ptr(lo), ptr(cnt), ns, 0, ptr(off), ptr(sidx), ptr(bidx),
                       it == torch.int64, total, 0, st)
    return sidx, bidx


def masked_expand(lo: torch.Tensor, cnt: torch.Tensor, mask: torch.Tensor, big_n: int
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``expand_ranges`` keeping only the big rows set in ``mask`` (bool[big_n]):
    the pairs of a sorted join whose big side is a filtered table probed in
    place -- its own sorted key column under the filter mask, not a compacted
    copy (exec/joins.py inner_pairs). Grouped by small row."""
    ns = lo.numel()
    if not is_gpu(lo):
        s, b = expand_ranges(lo, cnt, big_n)
        keep = mask.index_select(0, b.long())
        return s[keep], b[keep]
    N = launch("sorted_masked")
    st = stream(lo)
    mk = mask.contiguous().view(torch.uint8)
    counts = torch.empty(max(ns, 1), dtype=torch.int32, device=lo.device)
    N.sorted_masked(ptr(mk), ptr(lo), ptr(cnt), ns, ptr(counts), 0, 0, 0, False, 0, st)
    off, total = exclusive_scan(counts[:ns])
    it = torch.int32 if max(total, big_n, ns) < INT32_MAX else torch.int64
    sidx = torch.empty(total, dtype=it, device=lo.device)
    bidx = torch.empty(total, dtype=it, device=lo.device)
    if total:
        N.sorted_masked(ptr(mk), ptr(lo), ptr(cnt), ns, 0, ptr(off), ptr(sidx), ptr(bidx), it == torch.int64, total,
                        st)
    return sidx, bidx


EXISTS_OPS = {"=": 0, "<>": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "any": 6}


def sorted_exists(big2: Optional[torch.Tensor], small2: Optional[torch.Tensor], lo: torch.Tensor, cnt: torch.Tensor,
                  op: str, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool[ns]: some row k of small row i's range (lo, cnt) has big2[k] OP
    small2[i] (op "any": any row; big2 / small2 unused). ``mask``: only the
    big rows set in it count (a filtered big side searched in place)."""
    ns = lo.numel()
    if op == "any":
        big2 = small2 = None
        dt = torch.int32
    else:
        dt = torch.int64 if torch.int64 in (big2.dtype, small2.dtype) else torch.int32
        big2, small2 = big2.to(dt).contiguous(), small2.to(dt).contiguous()
    if not is_gpu(lo):
        nb = mask.numel() if mask is not None else big2.numel()
        s, b = expand_ranges(lo, cnt, nb)
        if op == "any":
            ok = torch.ones(s.numel(), dtype=torch.bool)
        else:
            bv, sv = big2.index_select(0, b.long()), small2.index_select(0, s.long())
            ok = {"=": bv == sv, "<>": bv != sv, "<": bv < sv, "<=": bv <= sv, ">": bv > sv, ">=": bv >= sv}[op]
        if mask is not None:
            ok = ok & mask.index_select(0, b.long())
        hit = torch.zeros(ns, dtype=torch.bool)
        hit.index_fill_(0, s.long()[ok], True)
        return hit
    hit = torch.empty(ns, dtype=torch.bool, device=lo.device)
    mk = mask.contiguous().view(torch.uint8) if mask is not None else None
    launch("sorted_exists").sorted_exists(ptr(big2), ptr(small2), dt == torch.int64, ptr(lo), ptr(cnt), ns,
                                          EXISTS_OPS[op], ptr(mk), ptr(hit), stream(lo))
    return hit


def group_ids_ex(keys: torch.Tensor) -> Tuple[torch.Tensor, int, torch.Tensor, bool]:
    """``group_ids`` plus whether the ids are non-decreasing. Clustered keys
    (lineitem by l_orderkey, any output that follows a sorted probe side) get
    run ids from a boundary compaction instead of a hash table."""
    keys = _keys_ok(keys)
    n = keys.numel()
    if n >= SORTED_CHECK_ROWS and is_gpu(keys):
        if is_sorted(keys):
            bound = torch.empty(n, dtype=torch.bool, device=keys.device)
            launch("run_bounds").run_bounds(ptr(keys), keys.dtype == torch.int64, n, ptr(bound), stream(keys))
            starts = mask_to_indices(bound)
            g = starts.numel()
            gid = torch.empty(n, dtype=torch.int32, device=keys.device)
            launch("fill_runs").fill_runs(ptr(starts), starts.dtype == torch.int64, g, n, ptr(gid), stream(keys))
            tags.BOUND.set(gid, (0, max(g - 1, 0)))
            return gid, g, starts.to(torch.int32), True
    gid, g, rep = group_ids(keys)
    return gid, g, rep, False


def _group_table(keys: torch.Tensor, n: int) -> Tuple[int, bool, int]:
    """(kmin, direct-mapped?, cap) of the group-by table over ``keys``. A
    hashed table's per-slot arrays hold ``cap + 1`` entries: the last one is
    the reserved slot of the key equal to EMPTY_KEY (``_group_slots``)."""
    bnd = key_bound(keys)
    if bnd is not None and (bnd[1] - bnd[0] + 1 <= 2 * n + 65536 or n < BOUND_TRUST_ROWS):
        kmin, kmax = bnd         # a readback-free bound decides: no range readback
    elif tags.HASHED.get(keys, False) and n > 1:
        kmin, kmax = 0, 2**62    # 64-bit hashes: the hash table, no range readback
    else:
        kmin, kmax = key_range(keys)
    span = kmax - kmin + 1
    direct = span <= 2 * n + 65536 and span < 2**31 - 1
    return kmin, direct, span if direct else _next_pow2(2 * n)


def _group_slots(direct: bool, cap: int) -> int:
    return cap if direct else cap + 1


def _group_build(keys: torch.Tensor, n: int):
    """The group-by table over ``keys`` after its build pass: (kmin, direct,
    cap, nslots, tkeys, trow), trow[slot] = the smallest row of the slot's key
    (INT32_MAX: an empty slot)."""
    kmin, direct, cap = _group_table(keys, n)
    dev = keys.device
    nslots = _group_slots(direct, cap)
    trow = torch.full((nslots,), INT32_MAX, dtype=torch.int32, device=dev)
    tkeys = (torch.empty(1, dtype=torch.int64, device=dev) if direct
             else torch.full((nslots,), EMPTY_KEY, dtype=torch.int64, device=dev))
    launch("groupby").groupby_build(ptr(keys), keys.dtype == torch.int64, n, ptr(tkeys), ptr(trow), cap, kmin,
                                    direct, stream(keys))
    return kmin, direct, cap, nslots, tkeys, trow


def group_ids(keys: torch.Tensor) -> Tuple[torch.Tensor, int, torch.Tensor]:
    """Dense group ids for int keys (no NULLs: callers map NULL to a reserved key).

    Returns (gid int32 [n], number of groups, representative row per group int32)."""
    keys = _keys_ok(keys)
    n = keys.numel()
    dev = keys.device
    if n == 0:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return z, 0, z
    if not is_gpu(keys):
        uniq, inv = torch.unique(keys, sorted=True, return_inverse=True)
        g = uniq.numel()
        rep = torch.full((g,), n, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(n), reduce="amin")
        return inv.to(torch.int32), g, rep.to(torch.int32)
    kmin, direct, cap, nslots, tkeys, trow = _group_build(keys, n)
    N = native()
    s = stream(keys)
    occ = torch.empty(nslots, dtype=torch.bool, device=dev)
    gid_of_slot = torch.empty(nslots, dtype=torch.int32, device=dev)
    N.groupby_occupied(ptr(trow), nslots, ptr(occ), ptr(gid_of_slot), s)
    slots = mask_to_indices(occ)
    g = slots.numel()
    rep = torch.empty(g, dtype=torch.int32, device=dev)
    N.groupby_assign(ptr(slots), slots.dtype == torch.int64, g, nslots, ptr(trow), ptr(gid_of_slot), ptr(rep), s)
    gid = torch.empty(n, dtype=torch.int32, device=dev)
    N.groupby_lookup(ptr(keys), keys.dtype == torch.int64, n, ptr(tkeys), ptr(gid_of_slot), cap, kmin, direct, ptr(gid), s)
    if not direct and g > 1:
        # hashed slots depend on the order in which threads inserted colliding
        # keys, so slot-order ids differ between runs; renumber the groups by
        # their first row (the direct path is already in key order). Stable ids
        # keep every later readback that depends on them (packed-key ranges,
        # group order) identical across executions, which replayed readbacks
        # and query graphs rely on.
        from .gather import gather_tensor
        first = rep.clamp(max=n - 1).long()        # in bounds even under a mismatched replay
        mark = torch.zeros(n, dtype=torch.bool, device=dev)
        mark.index_fill_(0, first, True)
        order = mask_to_indices(mark, total=g)     # g marks: no count readback
        newpos = torch.zeros(n, dtype=torch.int32, device=dev)
        newpos.index_copy_(0, order.long(), torch.arange(order.numel(), dtype=torch.int32, device=dev))
        remap = newpos.index_select(0, first)
        gid = gather_tensor(remap, gid)
        rep = order.to(torch.int32)
    tags.BOUND.set(gid, (0, max(g - 1, 0)))   # readback-free bound for packing / regrouping
    return gid, g, rep


def first_rows_mask(keys: torch.Tensor) -> torch.Tensor:
    """bool[n]: True on the first row of every distinct key (the rows
    COUNT/SUM(DISTINCT) keep). GPU: the group-by table's build pass (which
    keeps each group's smallest row) and one pass over its slots -- no group
    ids, no group count readback, no renumbering."""
    keys = _keys_ok(keys)
    n = keys.numel()
    dev = keys.device
    if n == 0 or not is_gpu(keys):
        mark = torch.zeros(n, dtype=torch.bool, device=dev)
        if n:
            _, _, rep = group_ids(keys)
            mark[rep.long()] = True
        return mark
    _, _, _, nslots, _, trow = _group_build(keys, n)
    mark = torch.zeros(n, dtype=torch.bool, device=dev)
    launch("mark_slot_rows").mark_slot_rows(ptr(trow), nslots, n, ptr(mark), stream(keys))
    return mark


HLL_BITS = 12
HLL_M = 1 << HLL_BITS


def hll_sketch(keys: torch.Tensor, valid: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """HyperLogLog registers (uint8 [4096]) of the key column (GPU only; None on CPU).
    Sketches of several ranks merge by element-wise max."""
    src = keys
    if valid is None:
        hit = tags.HLL.get(src)
        if hit is not None:   # resident table columns are sketched once (like is_sorted)
            return hit
    if valid is None and tags.RESIDENT.get(src, False):
        check_not_capturing("sketch of a resident column")   # kept on the column: a one-time build
    keys = _keys_ok(keys)
    n = keys.numel()
    if not is_gpu(keys):
        return None
    regs = torch.zeros(HLL_M, dtype=torch.uint8, device=keys.device)
    if n == 0:
        return regs
    N = launch("hll_sketch")
    ws = torch.empty(N.hll_blocks(n) * HLL_M, dtype=torch.uint8, device=keys.device)
    N.hll_sketch(ptr(keys), keys.dtype == torch.int64, ptr(valid), n, ptr(ws), ptr(regs), stream(keys))
    if valid is None:
        tags.HLL.set(src, regs)
    return regs


def hll_terms(regs: torch.Tensor) -> torch.Tensor:
    """Per sketch (rows of ``regs``) the float64 pair (sum 2^-r, zero
    registers) the estimate is computed from, on the device."""
    r = regs.to(torch.float64)
    return torch.stack([torch.pow(2.0, -r).sum(-1), (regs == 0).sum(-1).to(torch.float64)], -1)


def hll_estimate(regs: torch.Tensor) -> float:
    """Cardinality estimate from HLL registers (bias-corrected; linear counting
    for small cardinalities). Relative error ~1.04/sqrt(4096) = 1.6%."""
    z, zeros = to_host_f64s(hll_terms(regs))
    return hll_from_terms(z, int(zeros))


def hll_from_terms(z: float, zeros: int) -> float:
    m = float(HLL_M)
    alpha = 0.7213 / (1.0 + 1.079 / m)
    e = alpha * m * m / z
    if e <= 2.5 * m and zeros > 0:
        import math
        e = m * math.log(m / zeros)
    return e


def ndv(keys: torch.Tensor, valid: Optional[torch.Tensor] = None) -> int:
    """Distinct count: HLL estimate on GPU, exact on CPU."""
    if keys.numel() == 0:
        return 0
    if is_gpu(keys):
        return max(1, int(round(hll_estimate(hll_sketch(keys, valid)))))
    k = keys if valid is None else keys[valid]
    return int(torch.unique(k).numel())


def pack_keys(cols: Sequence[torch.Tensor]) -> torch.Tensor:
    """Combine several integer key columns into ONE int64 key per row that is
    equal iff all inputs are equal. Bit-packs when the value ranges fit in 63
    bits, otherwise re-encodes pairwise through ``group_ids``."""
    assert cols
    if len(cols) == 1:
        c = cols[0]
        return c if c.dtype in (torch.int32, torch.int64) else c.to(torch.int64)
    ranges = _bounded_ranges(cols)
    bits = [max(1, int(hi - lo).bit_length()) for lo, hi in ranges]
    if sum(bits) <= 62:
        return _pack_bits(cols, ranges, bits)
    # pairwise dense re-encoding keeps every intermediate code < n
    acc = cols[0].to(torch.int64)
    for c in cols[1:]:
        g1, n1, _ = group_ids(acc)
        g2, n2, _ = group_ids(c.to(torch.int64) if c.dtype != torch.int64 else c)
        acc = g1.to(torch.int64) * max(n2, 1) + g2.to(torch.int64)
    return acc


def pack_keys_pair(left: Sequence[torch.Tensor], right: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pack multi-column join keys of both sides with ONE shared encoding."""
    if len(left) == 1:
        return left[0], right[0]
    nl = left[0].numel()
    if is_gpu(left[0]) and len(left) <= MAX_PACK_BITS:
        # one shared bit layout from both sides' ranges: each side packed in
        # place, no concatenated copies
        both = _bounded_ranges(list(left) + list(right))      # at most one readback for both sides
        rl, rr = both[:len(left)], both[len(left):]
        if right[0].numel() == 0:
            ranges = rl
        elif nl == 0:
            ranges = rr
        else:
            ranges = [(min(a[0], b[0]), max(a[1], b[1])) for a, b in zip(rl, rr)]
        bits = [max(1, int(hi - lo).bit_length()) for lo, hi in ranges]
        if sum(bits) <= 62:
            return _pack_bits(list(left), ranges, bits), _pack_bits(list(right), ranges, bits)
    both = [torch.cat([a.to(torch.int64), b.to(torch.int64)]) for a, b in zip(left, right)]
    packed = pack_keys(both)
    return packed[:nl], packed[nl:]


#: columns one pack_bits launch combines (csrc/kernels/kernels.h kMaxPackBits)
MAX_PACK_BITS = 8


def key_ranges(cols: Sequence[torch.Tensor]) -> List[Tuple[int, int]]:
    """(min, max) of each integer key column ((0, 0) for an empty one; an
    all-NULL-free column assumed), with ONE readback for all of them on the
    GPU (resident columns answer from their remembered stats)."""
    out: List[Optional[Tuple[int, int]]] = [None] * len(cols)
    todo = []
    for i, c in enumerate(cols):
        if c.numel() == 0:
            out[i] = (0, 0)
            continue
        hit = tags.STATS.get(c)
        if hit is not None and hit[0] is not None:
            out[i] = hit[0]
        elif is_gpu(c) and c.dtype in (torch.int32, torch.int64) and c.dim() == 1:
            todo.append(i)
        else:
            r = key_range(c)
            out[i] = r if r is not None else (0, 0)
    if todo:
        N = launch("column_stats")
        bufs = []
        for i in todo:
            c = cols[i].contiguous()
            buf = torch.empty(N.STATS_SLOTS, dtype=torch.int64, device=c.device)
            N.column_stats(ptr(c), c.dtype == torch.int64, 0, c.numel(), ptr(buf), stream(c))
            bufs.append(buf[:2])
        vals = to_host_ints(torch.cat(bufs))
        for j, i in enumerate(todo):
            lo, hi = vals[2 * j], vals[2 * j + 1]
            out[i] = (lo, hi) if lo <= hi else (0, 0)
    return out  # type: ignore[return-value]


def _bounded_ranges(cols: Sequence[torch.Tensor]) -> List[Tuple[int, int]]:
    """Per column an interval holding all its values: the readback-free
    bound where one is known (``key_bound``), else the exact range (read
    back together for all such columns). Packing needs no more than that."""
    out: List[Optional[Tuple[int, int]]] = [None] * len(cols)
    todo = []
    for i, c in enumerate(cols):
        b = key_bound(c) if is_gpu(c) and c.numel() else None
        if b is not None:
            out[i] = b
        else:
            todo.append(i)
    if todo:
        for i, r in zip(todo, key_ranges([cols[i] for i in todo])):
            out[i] = r
    return out  # type: ignore[return-value]


def _pack_bits(cols: Sequence[torch.Tensor], ranges, bits) -> torch.Tensor:
    n = cols[0].numel()
    if not is_gpu(cols[0]) or len(cols) > MAX_PACK_BITS or any(c.dtype not in (torch.int32, torch.int64)
                                                                for c in cols):
        out = None
        for c, (lo, _), b in zip(cols, ranges, bits):
            v = c.to(torch.int64) - lo
            out = v if out is None else (out << b) | v
        return out
    cs = [c.contiguous() for c in cols]
    out = torch.empty(n, dtype=torch.int64, device=cs[0].device)
    shifts = [0] + list(bits[1:])      # acc = (acc << bits[c]) | (v - lo) for every column after the first
    launch("pack_bits").pack_bits([ptr(c) for c in cs], [c.dtype == torch.int64 for c in cs],
                                  [int(lo) for lo, _ in ranges], shifts, n, ptr(out), stream(out))
    return out
