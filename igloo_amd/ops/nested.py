"""LIST / STRUCT / MAP column operations (csrc/kernels/nested.hip + the gather
and range-expansion kernels).

Parity: DataFusion's nested functions (reference Cargo.lock:1125
datafusion-functions-nested: make_array / ``[..]`` literals, array_length,
cardinality, array_element / ``l[i]``, unnest, array_agg, struct /
named_struct / get_field), reached through ``SessionContext::sql``
(reference crates/engine/src/lib.rs:54-57).

Layout (types.py): a LIST row is an (start, length) int64 pair into
``col.nested.child``; a STRUCT row is an int64 row id into each of
``col.nested.children``; a MAP row is the LIST's (start, length) pair over
two equally long children, ``col.nested.children["key"]`` and ``["value"]``
(entry t of row r is child row start + t in both), so map_keys / map_values
are LIST views sharing ``data`` and cardinality is ``data[:, 1]``. Row
movement (filters, joins, sorts) therefore gathers 16 / 8 bytes per row and
never touches the children; functions turn into index arithmetic plus one
child gather.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import pyarrow as pa
import torch

from .. import types as T
from ..columnar import Column, Nested
from ..utils.errors import ExecutionError, NotSupported
from ._lib import KERNEL_CALLS
from ._lib import check_not_capturing, is_gpu, launch, ptr, stream, to_host_int


def _cat_children(children: List[Column]) -> Column:
    from ..exec.joins import concat_columns
    return concat_columns(children) if len(children) > 1 else children[0]


def concat(cols: Sequence[Column], valid: Optional[torch.Tensor]) -> Column:
    """Rows of ``cols`` end to end (UNION ALL, INSERT): children concatenated,
    each part's starts / row ids shifted by the child rows before it."""
    c0 = cols[0]
    dt = c0.dtype
    datas, base = [], 0
    if dt.kind == "list":
        kids = [c.nested.child for c in cols]
        for c, ch in zip(cols, kids):
            d = c.data.clone()
            d[:, 0] += base
            datas.append(d)
            base += len(ch)
        return Column(dt, torch.cat(datas), valid, dictionary=Nested(child=_cat_children(kids)))
    kids: Dict[str, List[Column]] = {n: [] for n, _ in dt.fields}
    if dt.kind == "map":
        for c in cols:
            d = c.data.clone()
            d[:, 0] += base
            datas.append(d)
            for n in kids:
                kids[n].append(c.nested.children[n])
            base += len(c.nested)
        return Column(dt, torch.cat(datas), valid,
                      dictionary=Nested(children={n: _cat_children(v) for n, v in kids.items()}))
    for c in cols:
        datas.append(c.data + base)
        for n, _ in dt.fields:
            kids[n].append(c.nested.children[n])
        base += len(c.nested)
    return Column(dt, torch.cat(datas), valid,
                  dictionary=Nested(children={n: _cat_children(v) for n, v in kids.items()}))


def scalar_to_column(value, dtype: T.DataType, n: int, device) -> Column:
    return Column.full(value, dtype, n, device)


def make_list(cols: Sequence[Column], n: int, dtype: T.DataType, device) -> Column:
    """make_array(c0, .., ck-1): row r = [c0[r], .., ck-1[r]]. The child is
    the k columns concatenated, read back interleaved (one gather)."""
    from .gather import take
    k = len(cols)
    device = torch.device(device)
    if k == 0:
        child = Column.full(None, dtype.child if dtype.child.kind != "null" else T.INT64, 0, device)
        se = torch.zeros((n, 2), dtype=torch.int64, device=device)
        return Column(dtype, se, None, dictionary=Nested(child=child))
    flat = _cat_children(list(cols))
    idx = torch.empty(n * k, dtype=torch.int64, device=device)
    se = torch.empty((n, 2), dtype=torch.int64, device=device)
    if is_gpu(idx):
        s = stream(idx)
        launch("interleave_idx").interleave_idx(n, k, ptr(idx), s)
        launch("list_slots").list_slots(n, k, ptr(se), s)
    else:
        r = torch.arange(n, dtype=torch.int64)
        idx = (torch.arange(k, dtype=torch.int64).view(1, k) * n + r.view(n, 1)).reshape(-1)
        se = torch.stack([r * k, torch.full_like(r, k)], 1)
    child = take(flat, idx) if n * k else flat
    return Column(dtype, se, None, dictionary=Nested(child=child))


def lengths(col: Column) -> torch.Tensor:
    return col.data[:, 1].contiguous() if len(col) else torch.zeros(0, dtype=torch.int64, device=col.device)


def element(col: Column, pos, pos_valid: Optional[torch.Tensor] = None) -> Column:
    """l[i] / array_element(l, i): 1-based, negative from the end, NULL when
    out of range. ``pos``: an int constant or an int64 tensor per row."""
    from .gather import take
    n = len(col)
    child = col.nested.child
    dev = col.device
    out = torch.empty(n, dtype=torch.int64, device=dev)
    ptensor = pos.to(torch.int64).contiguous() if isinstance(pos, torch.Tensor) else None
    if is_gpu(out):
        launch("list_element_idx").list_element_idx(ptr(col.data.contiguous()), ptr(col.valid), ptr(ptensor),
                                                    ptr(pos_valid), 0 if ptensor is not None else int(pos), n,
                                                    len(child), ptr(out), stream(out))
    else:
        st, ln = col.data[:, 0], col.data[:, 1]
        i = ptensor if ptensor is not None else torch.full((n,), int(pos), dtype=torch.int64)
        k = torch.where(i > 0, i - 1, ln + i)
        ok = (i != 0) & (k >= 0) & (k < ln)
        if col.valid is not None:
            ok &= col.valid
        if pos_valid is not None:
            ok &= pos_valid
        out = torch.where(ok, st + k, torch.full_like(st, -1))
    return take(child, out, neg=True)


def unnest_rows(col: Column) -> Tuple[torch.Tensor, Column]:
    """One output row per list element: (parent row per output row, the
    elements). NULL and empty lists produce no rows (DataFusion's unnest)."""
    from .gather import take
    from .hashing import expand_ranges
    n = len(col)
    lo = col.data[:, 0].contiguous() if n else torch.zeros(0, dtype=torch.int64, device=col.device)
    cnt = lengths(col)
    if col.valid is not None:
        cnt = torch.where(col.valid, cnt, torch.zeros_like(cnt))
    parent, cidx = expand_ranges(lo, cnt, len(col.nested.child))
    return parent, take(col.nested.child, cidx)


def unnest_values(col: Column, device) -> Column:
    return unnest_rows(col)[1]


def from_groups(child: Column, starts: torch.Tensor, counts: torch.Tensor, dtype: T.DataType,
                valid: Optional[torch.Tensor]) -> Column:
    """A list per group over a child already ordered by group (array_agg)."""
    se = torch.stack([starts.to(torch.int64), counts.to(torch.int64)], 1).contiguous()
    return Column(dtype, se, valid, dictionary=Nested(child=child))


def make_struct(names: Sequence[str], cols: Sequence[Column], n: int, dtype: T.DataType, device) -> Column:
    rid = torch.arange(n, dtype=torch.int64, device=torch.device(device))
    return Column(dtype, rid, None, dictionary=Nested(children=dict(zip(names, cols))))


def field(col: Column, name: str) -> Column:
    """get_field(s, 'name') / s['name']: NULL where the struct row is NULL."""
    from .gather import take
    ch = col.nested.children.get(name)
    if ch is None:
        raise ExecutionError(f"struct has no field '{name}'")
    idx = col.data
    if col.valid is not None:
        idx = torch.where(col.valid, idx, torch.full_like(idx, -1))
        return take(ch, idx, neg=True)
    return take(ch, idx)


def to_string(col: Column, sep: str, null_str: Optional[str] = None) -> Column:
    """array_to_string(l, sep [, null_str]) via the host (Arrow)."""
    vals = col.to_arrow().to_pylist()
    out = []
    for v in vals:
        if v is None:
            out.append(None)
            continue
        parts = [("" if x is None else str(x)) if null_str is not None or x is not None else None for x in v]
        if null_str is None:
            parts = [p for p, x in zip(parts, v) if x is not None]
        else:
            parts = [null_str if x is None else p for p, x in zip(parts, v)]
        out.append(sep.join(parts))
    return Column.from_arrow(pa.array(out, pa.large_string()), device=col.device)


def has(col: Column, value) -> Column:
    """array_has(l, x): some element equals x (NULL row -> NULL)."""
    from .hashing import expand_ranges
    n = len(col)
    dev = col.device
    child = col.nested.child
    if value is None:
        return Column(T.BOOL, torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool,
                                                                                            device=dev))
    if child.dtype.is_string:
        from . import strings as S
        eq = S.in_list(child, [str(value)])
    else:
        eq = child.data == torch.as_tensor(value, dtype=child.data.dtype, device=dev)
    if child.valid is not None:
        eq = eq & child.valid
    cnt = lengths(col)
    if col.valid is not None:
        cnt = torch.where(col.valid, cnt, torch.zeros_like(cnt))
    p, c = expand_ranges(col.data[:, 0].contiguous() if n else cnt, cnt, len(child))
    hit = torch.zeros(n, dtype=torch.int64, device=dev)
    if p.numel():
        hit.index_add_(0, p.long(), eq.index_select(0, c.long()).to(torch.int64))
    return Column(T.BOOL, hit > 0, col.valid)


# ====================================================================== list functions
# DataFusion's array_* family on the (start, length) layout: slot functions
# rewrite the pairs and share the child; rebuild functions emit an int64 map
# of source rows (count -> scan -> write) and gather it once; search, set and
# sort functions work on an int64 key per child element. GPU tensors run the
# nested.hip kernels, CPU tensors the torch / generic forms below.

#: elements per list side the LDS (quadratic) kernels take; rows beyond it
#: send the call down the generic path. An LDS-budget choice (nested.hip),
#: lowered by tests to reach the generic path with small data.
LIST_FAST_MAX = 512

_I64_MAX = (1 << 63) - 1


def _i64(x, n: int, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(torch.int64).contiguous()
    return torch.full((n,), int(x), dtype=torch.int64, device=dev)


def _and(*vs) -> Optional[torch.Tensor]:
    out = None
    for v in vs:
        if v is not None:
            out = v if out is None else out & v
    return out


def _vlen(col: Column) -> torch.Tensor:
    """Lengths with NULL rows read as empty."""
    ln = lengths(col).clamp(min=0)
    return ln if col.valid is None else torch.where(col.valid, ln, torch.zeros_like(ln))


def _starts(col: Column) -> torch.Tensor:
    return col.data[:, 0].contiguous() if len(col) else torch.zeros(0, dtype=torch.int64, device=col.device)


def _list_col(dtype: T.DataType, se: torch.Tensor, valid, child: Column) -> Column:
    return Column(dtype, se, valid, dictionary=Nested(child=child))


def _offsets(lens: torch.Tensor, extra: Optional[torch.Tensor] = None):
    """Arrow offsets of ``lens``, the total on the host and, in the same
    readback, the largest of ``extra`` (the longest list a kernel met)."""
    from .select import offsets_from_lengths
    from ._lib import to_host_ints
    if lens.numel() == 0:
        return torch.zeros(1, dtype=torch.int64, device=lens.device), 0, 0
    if extra is None or not is_gpu(lens):
        off, total = offsets_from_lengths(lens)
        mx = int(extra.max().item()) if extra is not None and extra.numel() else 0
        return off, total, mx
    off, tot = offsets_from_lengths(lens, host_total=False)
    big = extra.max().reshape(1) if extra.numel() else torch.zeros(1, dtype=torch.int64, device=lens.device)
    total, mx = to_host_ints(torch.cat([tot.reshape(1), big]))
    return off, total, mx


def _se_from(off: torch.Tensor) -> torch.Tensor:
    return torch.stack([off[:-1], off[1:] - off[:-1]], 1).contiguous()


def _elements(col: Column) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Element level of a list column: (row, child row, position in the row)
    per element in row order, and the per-row lengths."""
    from .hashing import expand_ranges
    ln = _vlen(col)
    p, c = expand_ranges(_starts(col), ln, len(col.nested.child))
    p, c = p.long(), c.long()
    first = torch.cumsum(ln, 0) - ln
    t = torch.arange(p.numel(), dtype=torch.int64, device=col.device) - first.index_select(0, p)
    return p, c, t, ln


def _seg_sum(p: torch.Tensor, v: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.int64, device=p.device)
    if p.numel():
        out.index_add_(0, p, v.to(torch.int64))
    return out


def _check_flat(col: Column, what: str) -> None:
    if col.nested.child.dtype.kind in ("list", "struct"):
        raise NotSupported(f"{what} on a list whose elements are nested ({col.dtype})")


# ---------------------------------------------------------------- slot functions
def slice_(col: Column, frm, to, frm_valid=None, to_valid=None) -> Column:
    """array_slice(l, from, to): 1-based inclusive bounds, negative from the
    end, clamped; the result shares ``col``'s child. pop_front is (2, max),
    pop_back (1, -2)."""
    n = len(col)
    dev = col.device
    ft = frm.to(torch.int64).contiguous() if isinstance(frm, torch.Tensor) else None
    tt = to.to(torch.int64).contiguous() if isinstance(to, torch.Tensor) else None
    se = col.data.contiguous()
    if is_gpu(se):
        out = torch.empty((n, 2), dtype=torch.int64, device=dev)
        ok = torch.empty(n, dtype=torch.bool, device=dev)
        launch("list_slice_se").list_slice_se(ptr(se), ptr(col.valid), ptr(ft), ptr(frm_valid), ptr(tt), ptr(to_valid),
                                              0 if ft is not None else int(frm), 0 if tt is not None else int(to), n,
                                              ptr(out), ptr(ok), stream(se))
    else:
        st, ln = se[:, 0], se[:, 1].clamp(min=0)
        a, b = _i64(frm if ft is None else ft, n, dev), _i64(to if tt is None else tt, n, dev)
        a = torch.where(a > 0, a - 1, torch.where(a == 0, a, ln + a)).clamp(min=0)
        b = torch.minimum(torch.where(b > 0, b - 1, torch.where(b == 0, b - 1, ln + b)), ln - 1)
        ok = _and(col.valid, frm_valid, to_valid)
        m = (b - a + 1).clamp(min=0)
        if ok is not None:
            m = torch.where(ok, m, torch.zeros_like(m))
        out = torch.stack([torch.where(m > 0, st + a, torch.zeros_like(st)), m], 1)
    valid = ok if _and(col.valid, frm_valid, to_valid) is not None else None
    return _list_col(col.dtype, out, valid, col.nested.child)


def pop_front(col: Column) -> Column:
    return slice_(col, 2, _I64_MAX)


def pop_back(col: Column) -> Column:
    return slice_(col, 1, -2)


def is_empty(col: Column) -> Column:
    return Column(T.BOOL, lengths(col) == 0, col.valid)


# ------------------------------------------------------------- rebuild functions
def _from_parts(parts, src: Column, dtype: T.DataType, valid, n: int) -> Column:
    """Row r = its parts end to end; a part is (start, length, stride) tensors
    into ``src`` (stride 1 a list, 0 a repeated row, -1 a reversed list; a
    negative start pads with NULL). One gather builds the child."""
    from .gather import take
    dev = src.device
    k = len(parts)
    P = torch.stack([torch.stack([s, l.clamp(min=0), torch.full_like(s, st)], 1) for s, l, st in parts]).contiguous() \
        if n else torch.zeros((k, 0, 3), dtype=torch.int64, device=dev)
    if is_gpu(P):
        lens = torch.empty(n, dtype=torch.int64, device=dev)
        launch("list_parts_count").list_parts_count(ptr(P), k, n, ptr(lens), stream(P))
        off, total, _ = _offsets(lens)
        idx = torch.empty(total, dtype=torch.int64, device=dev)
        se = torch.empty((n, 2), dtype=torch.int64, device=dev)
        launch("list_parts_write").list_parts_write(ptr(P), k, n, ptr(off), len(src), total, ptr(idx), ptr(se),
                                                    stream(P))
    else:
        from .hashing import expand_ranges
        lens = P[:, :, 1].sum(0)
        off, total, _ = _offsets(lens)
        idx = torch.empty(total, dtype=torch.int64)
        before = torch.zeros(n, dtype=torch.int64)
        for j in range(k):
            s, l = P[j, :, 0].contiguous(), P[j, :, 1].contiguous()
            p, t = expand_ranges(torch.zeros_like(l), l, max(int(l.max().item()) if n else 0, 1))
            p, t = p.long(), t.long()
            v = s[p] + t * P[j, :, 2][p]
            v = torch.where((s[p] >= 0) & (v >= 0) & (v < len(src)), v, torch.full_like(v, -1))
            idx[off[:-1][p] + before[p] + t] = v
            before = before + l
        se = _se_from(off)
    return _list_col(dtype, se, valid, take(src, idx, neg=True))


def _rowids(n: int, dev) -> torch.Tensor:
    return torch.arange(n, dtype=torch.int64, device=dev)


def concat_lists(cols: Sequence[Column], dtype: T.DataType) -> Column:
    """array_concat(l1, .., lk) / ``||``: NULL lists read as empty."""
    n = len(cols[0])
    parts, base = [], 0
    for c in cols:
        parts.append((_starts(c) + base, _vlen(c), 1))
        base += len(c.nested.child)
    return _from_parts(parts, _cat_children([c.nested.child for c in cols]), dtype, None, n)


def append(col: Column, elem: Column, dtype: T.DataType, front: bool = False) -> Column:
    """array_append / array_prepend: the element column rides behind the child
    in the gather source."""
    n = len(col)
    base = len(col.nested.child)
    one = torch.ones(n, dtype=torch.int64, device=col.device)
    parts = [(_starts(col), _vlen(col), 1), (_rowids(n, col.device) + base, one, 0)]
    return _from_parts(parts[::-1] if front else parts, _cat_children([col.nested.child, elem]), dtype, None, n)


def reverse(col: Column) -> Column:
    ln = _vlen(col)
    return _from_parts([(_starts(col) + ln - 1, ln, -1)], col.nested.child, col.dtype, col.valid, len(col))


def repeat(elem: Column, count: torch.Tensor, count_valid, dtype: T.DataType) -> Column:
    """array_repeat(x, n): n <= 0 gives []."""
    n = len(elem)
    cnt = count.to(torch.int64).clamp(min=0)
    if count_valid is not None:
        cnt = torch.where(count_valid, cnt, torch.zeros_like(cnt))
    return _from_parts([(_rowids(n, elem.device), cnt, 0)], elem, dtype, count_valid, n)


def resize(col: Column, size: torch.Tensor, size_valid, fill: Optional[Column]) -> Column:
    """array_resize(l, n [, fill]): truncate, or pad with fill (NULL)."""
    n = len(col)
    valid = _and(col.valid, size_valid)
    sz = size.to(torch.int64).clamp(min=0)
    if valid is not None:
        sz = torch.where(valid, sz, torch.zeros_like(sz))
    ln = _vlen(col)
    keep = torch.minimum(ln, sz)
    base = len(col.nested.child)
    pad_row = _rowids(n, col.device) + base if fill is not None else torch.full_like(sz, -1)
    src = _cat_children([col.nested.child, fill]) if fill is not None else col.nested.child
    return _from_parts([(_starts(col), keep, 1), (pad_row, sz - keep, 0)], src, col.dtype, valid, n)


def flatten(col: Column) -> Column:
    """flatten(LIST<LIST<T>>): one level; NULL inner lists are skipped."""
    from .gather import take
    inner = col.nested.child
    if inner.dtype.kind != "list":
        raise ExecutionError(f"flatten() needs a list of lists, got {col.dtype}")
    n = len(col)
    dev = col.device
    leaf = inner.nested.child
    se = col.data.contiguous()
    if is_gpu(se):
        ise = inner.data.contiguous()
        lens = torch.empty(n, dtype=torch.int64, device=dev)
        s = stream(se)
        launch("list_flatten_count").list_flatten_count(ptr(se), ptr(col.valid), ptr(ise), ptr(inner.valid), n,
                                                        len(inner), ptr(lens), s)
        off, total, _ = _offsets(lens)
        idx = torch.empty(total, dtype=torch.int64, device=dev)
        out = torch.empty((n, 2), dtype=torch.int64, device=dev)
        launch("list_flatten_write").list_flatten_write(ptr(se), ptr(col.valid), ptr(ise), ptr(inner.valid), n,
                                                        len(inner), ptr(off), len(leaf), total, ptr(idx), ptr(out), s)
    else:
        p, c, _, _ = _elements(col)                       # outer row, inner list row
        sub = _list_col(inner.dtype, inner.data.index_select(0, c),
                        None if inner.valid is None else inner.valid.index_select(0, c), leaf)
        q, idx, _, iln = _elements(sub)
        lens = _seg_sum(p, iln, n)
        off, total, _ = _offsets(lens)
        out = _se_from(off)
    return _list_col(inner.dtype, out, col.valid, take(leaf, idx, neg=True))


# --------------------------------------------------------------------- key helpers
def _eq_keys(src: Column) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """int64 equality key per row of ``src`` and its validity: ints, dates and
    decimals as values, floats through the numeric join key, strings as
    dictionary codes (callers concatenate every column that must compare
    equal before encoding, so one dictionary covers them)."""
    from ..exec.joins import _num_key
    if src.dtype.kind in ("list", "struct"):
        raise NotSupported(f"equality on nested list elements ({src.dtype})")
    if src.dtype.is_string:
        from . import strings as S
        d = src if src.is_dict else S.dict_encode(src)
        return d.data.to(torch.int64).contiguous(), d.valid
    if src.dtype.kind == "null":
        return torch.zeros(len(src), dtype=torch.int64, device=src.device), \
            torch.zeros(len(src), dtype=torch.bool, device=src.device)
    return _num_key(src).to(torch.int64).contiguous(), src.valid


def _order_keys(src: Column) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """int64 key per row whose signed order is the value order: ints, dates,
    timestamps, bools and 64-bit decimals directly, float64 through the
    monotone bit mapping, strings through their sort rank."""
    if src.dtype.kind in ("list", "struct"):
        raise NotSupported(f"ordering of nested list elements ({src.dtype})")
    if src.dtype.is_string:
        from . import strings as S
        return S.sort_ranks(src).to(torch.int64).contiguous(), src.valid
    x = src.data
    if x.dtype in (torch.float32, torch.float64):
        x = x.to(torch.float64)
        b = torch.where(x == 0, torch.zeros_like(x), x).view(torch.int64)
        return (b ^ ((b >> 63) & _I64_MAX)).contiguous(), src.valid
    if src.is_wide:
        raise NotSupported("ordering of 128-bit decimal list elements")
    return x.to(torch.int64).contiguous(), src.valid


def _match(col: Column, keys, kv, nk, nv):
    """Element level of ``col`` with the IS NOT DISTINCT FROM match against
    the row's needle, and each match's rank among its row's matches."""
    p, c, t, ln = _elements(col)
    ev = kv.index_select(0, c) if kv is not None else torch.ones_like(c, dtype=torch.bool)
    eq = ev & (keys.index_select(0, c) == nk.index_select(0, p))
    m = eq if nv is None else torch.where(nv.index_select(0, p), eq, ~ev)
    cnt = _seg_sum(p, m, len(col))
    mi = m.to(torch.int64)
    rank = torch.cumsum(mi, 0) - mi - (torch.cumsum(cnt, 0) - cnt).index_select(0, p)
    return p, c, t, ln, m, cnt, rank


def _search_args(col: Column, others: Sequence[Column], what: str):
    """Keys of the list's child and of the per-row argument columns under one
    encoding: (source column = child ++ others, child keys, child validity,
    [(keys, validity) per other])."""
    _check_flat(col, what)
    child = col.nested.child
    src = _cat_children([child] + list(others))
    k, kv = _eq_keys(src)
    nc, n = len(child), len(col)
    outs = []
    for j in range(len(others)):
        lo = nc + j * n
        outs.append((k[lo:lo + n].contiguous(), None if kv is None else kv[lo:lo + n].contiguous()))
    return src, k[:nc].contiguous(), (None if kv is None else kv[:nc].contiguous()), outs


def _match_count(col, keys, kv, nk, nv, mode, frm=None, limit=_I64_MAX):
    n = len(col)
    out = torch.empty(n, dtype=torch.int64, device=col.device)
    lt = limit if isinstance(limit, torch.Tensor) else None
    launch("list_match_count").list_match_count(ptr(col.data.contiguous()), ptr(col.valid), ptr(keys), ptr(kv),
                                                keys.numel(), ptr(nk), ptr(nv), ptr(frm), ptr(lt),
                                                0 if lt is not None else int(limit), mode, n, ptr(out), stream(out))
    return out


def _match_write(col, keys, kv, nk, nv, mode, off, total, limit=_I64_MAX, repl_base=0):
    out = torch.empty(total, dtype=torch.int64, device=col.device)
    lt = limit if isinstance(limit, torch.Tensor) else None
    launch("list_match_write").list_match_write(ptr(col.data.contiguous()), ptr(col.valid), ptr(keys), ptr(kv),
                                                keys.numel(), ptr(nk), ptr(nv), ptr(lt),
                                                0 if lt is not None else int(limit), mode, len(col), ptr(off),
                                                repl_base, total, ptr(out), stream(out))
    return out


def position(col: Column, needle: Column, frm: Optional[torch.Tensor] = None, frm_valid=None) -> Column:
    """array_position(l, x [, from]): 1-based, NULL when nothing matches."""
    n = len(col)
    _, keys, kv, [(nk, nv)] = _search_args(col, [needle], "array_position()")
    f = None if frm is None else frm.to(torch.int64).contiguous()
    if is_gpu(keys):
        pos = _match_count(col, keys, kv, nk, nv, 0, frm=f)
    else:
        p, c, t, ln, m, _, _ = _match(col, keys, kv, nk, nv)
        if f is not None:
            m = m & (t >= (f - 1).index_select(0, p))
        big = torch.full((n,), _I64_MAX, dtype=torch.int64)
        pos = big.scatter_reduce(0, p, torch.where(m, t + 1, torch.full_like(t, _I64_MAX)), reduce="amin")
        pos = torch.where(pos == _I64_MAX, torch.zeros_like(pos), pos)
    return Column(T.INT64, pos, _and(col.valid, frm_valid, pos > 0))


def has_value(col: Column, needle: Column) -> Column:
    """array_has(l, x) / x = ANY(l) with a per-row needle."""
    _, keys, kv, [(nk, nv)] = _search_args(col, [needle], "array_has()")
    if is_gpu(keys):
        cnt = _match_count(col, keys, kv, nk, nv, 1)
    else:
        cnt = _match(col, keys, kv, nk, nv)[5]
    return Column(T.BOOL, cnt > 0, col.valid)


def positions(col: Column, needle: Column) -> Column:
    """array_positions(l, x): the 1-based positions of every match."""
    _, keys, kv, [(nk, nv)] = _search_args(col, [needle], "array_positions()")
    if is_gpu(keys):
        off, total, _ = _offsets(_match_count(col, keys, kv, nk, nv, 1))
        vals = _match_write(col, keys, kv, nk, nv, 0, off, total)
    else:
        p, c, t, ln, m, cnt, _ = _match(col, keys, kv, nk, nv)
        off, total, _ = _offsets(cnt)
        vals = (t + 1)[m]
    return _list_col(T.LIST(T.INT64), _se_from(off), col.valid, Column(T.INT64, vals, None))


def remove(col: Column, needle: Column, limit=_I64_MAX, limit_valid=None) -> Column:
    """array_remove (limit 1) / array_remove_n / array_remove_all."""
    from .gather import take
    _, keys, kv, [(nk, nv)] = _search_args(col, [needle], "array_remove()")
    lim = limit.to(torch.int64).contiguous() if isinstance(limit, torch.Tensor) else limit
    if is_gpu(keys):
        off, total, _ = _offsets(_match_count(col, keys, kv, nk, nv, 2, limit=lim))
        idx = _match_write(col, keys, kv, nk, nv, 1, off, total, limit=lim)
    else:
        p, c, t, ln, m, cnt, rank = _match(col, keys, kv, nk, nv)
        L = _i64(lim, len(col), col.device).clamp(min=0)
        keep = ~(m & (rank < L.index_select(0, p)))
        off, total, _ = _offsets(_seg_sum(p, keep, len(col)))
        idx = c[keep]
    return _list_col(col.dtype, _se_from(off), _and(col.valid, limit_valid), take(col.nested.child, idx, neg=True))


def replace(col: Column, frm: Column, to: Column, limit=_I64_MAX, limit_valid=None) -> Column:
    """array_replace (limit 1) / array_replace_n / array_replace_all."""
    from .gather import take
    n = len(col)
    src, keys, kv, [(nk, nv), _] = _search_args(col, [frm, to], "array_replace()")
    base = len(col.nested.child) + n
    lim = limit.to(torch.int64).contiguous() if isinstance(limit, torch.Tensor) else limit
    if is_gpu(keys):
        off, total, _ = _offsets(_vlen(col))
        idx = _match_write(col, keys, kv, nk, nv, 2, off, total, limit=lim, repl_base=base)
    else:
        p, c, t, ln, m, cnt, rank = _match(col, keys, kv, nk, nv)
        L = _i64(lim, n, col.device).clamp(min=0)
        off, total, _ = _offsets(ln)
        idx = torch.where(m & (rank < L.index_select(0, p)), base + p, c)
    return _list_col(col.dtype, _se_from(off), _and(col.valid, limit_valid), take(src, idx, neg=True))


def extreme(col: Column, is_max: bool) -> Column:
    """array_max / array_min: NULL elements skipped; NULL when none is left."""
    from .gather import take
    _check_flat(col, "array_max() / array_min()")
    child = col.nested.child
    n = len(col)
    keys, kv = _order_keys(child)
    if is_gpu(keys):
        idx = torch.empty(n, dtype=torch.int64, device=col.device)
        launch("list_minmax_idx").list_minmax_idx(ptr(col.data.contiguous()), ptr(col.valid), ptr(keys), ptr(kv),
                                                  keys.numel(), int(is_max), n, ptr(idx), stream(idx))
    else:
        p, c, t, ln = _elements(col)
        ok = kv.index_select(0, c) if kv is not None else torch.ones_like(c, dtype=torch.bool)
        k = keys.index_select(0, c)
        k = -1 - k if is_max else k                     # ~k: the largest key becomes the smallest
        best = torch.full((n,), _I64_MAX, dtype=torch.int64).scatter_reduce(
            0, p, torch.where(ok, k, torch.full_like(k, _I64_MAX)), reduce="amin")
        hit = ok & (k == best.index_select(0, p))
        idx = torch.full((n,), _I64_MAX, dtype=torch.int64).scatter_reduce(
            0, p, torch.where(hit, c, torch.full_like(c, _I64_MAX)), reduce="amin")
        idx = torch.where(idx == _I64_MAX, torch.full_like(idx, -1), idx)
    return take(child, idx, neg=True)


# -------------------------------------------------------------- set functions, sort
_SET_OPS = {"distinct": 0, "union": 1, "intersect": 2, "except": 3, "has_all": 4, "has_any": 5}


def _set_generic(op: str, a: Column, b: Optional[Column], src: Column, k, kv, base: int):
    """Device-agnostic set functions from the relational operators: both
    sides' elements as (row, key, is NULL) packed into one key; first
    occurrences by ``first_rows_mask`` (A's elements ahead of B's), membership
    in the other side through the shared group ids. Returns (offsets, child
    row map) or, for has_all / has_any, the per-row boolean."""
    from .hashing import first_rows_mask, group_ids, pack_keys
    from .select import mask_to_indices
    n = len(a)
    dev = a.device
    pa_, ca, _, _ = _elements(a)
    if b is not None:
        pb, cb, _, _ = _elements(b)
        cb = cb + base
    else:
        pb = cb = torch.zeros(0, dtype=torch.int64, device=dev)
    p, c = torch.cat([pa_, pb]), torch.cat([ca, cb])
    na = pa_.numel()
    ev = kv.index_select(0, c) if kv is not None else torch.ones_like(c, dtype=torch.bool)
    key = torch.where(ev, k.index_select(0, c), torch.zeros_like(c))
    if p.numel():
        gid, ng, _ = group_ids(pack_keys([p, group_ids(key)[0].to(torch.int64), (~ev).to(torch.int64)]))
        gid = gid.long()
        first = first_rows_mask(gid)
    else:
        gid, ng, first = p, 0, torch.zeros(0, dtype=torch.bool, device=dev)
    is_a = torch.arange(p.numel(), device=dev) < na
    in_a = torch.zeros(ng, dtype=torch.bool, device=dev)
    in_b = torch.zeros(ng, dtype=torch.bool, device=dev)
    in_a[gid[:na]] = True
    in_b[gid[na:]] = True
    if op in ("has_all", "has_any"):
        found = in_a.index_select(0, gid[na:])
        if op == "has_all":
            return _seg_sum(pb, ~found, n) == 0
        return _seg_sum(pb, found, n) > 0
    if op in ("distinct", "union"):
        keep = first
    elif op == "intersect":
        keep = first & is_a & in_b.index_select(0, gid)
    else:
        keep = first & is_a & ~in_b.index_select(0, gid)
    # kept elements back into row order: A's ahead of B's inside every row
    cnt_a, cnt_b = _seg_sum(pa_, keep[:na], n), _seg_sum(pb, keep[na:], n)
    off, total, _ = _offsets(cnt_a + cnt_b)
    ki = keep.to(torch.int64)
    ex = torch.cumsum(ki, 0) - ki                       # rank among all kept, A's first
    row0_a = torch.cumsum(cnt_a, 0) - cnt_a
    row0_b = torch.cumsum(cnt_b, 0) - cnt_b + cnt_a.sum()
    dest = off[:-1].index_select(0, p) + torch.where(
        is_a, ex - row0_a.index_select(0, p), cnt_a.index_select(0, p) + ex - row0_b.index_select(0, p))
    sel = mask_to_indices(keep, total).long()
    idx = torch.empty(total, dtype=torch.int64, device=dev)
    idx.index_copy_(0, dest.index_select(0, sel), c.index_select(0, sel))
    return off, idx


def _set_op(op: str, a: Column, b: Optional[Column]):
    from .gather import take
    what = f"array_{op}()"
    _check_flat(a, what)
    n = len(a)
    dev = a.device
    kids = [a.nested.child]
    if b is not None:
        _check_flat(b, what)
        kids.append(b.nested.child)
    src = _cat_children(kids)
    k, kv = _eq_keys(src)
    base = len(kids[0])
    valid = _and(a.valid, b.valid if b is not None else None)
    boolean = op in ("has_all", "has_any")
    done = None
    if is_gpu(k):
        ka, kva = k[:base].contiguous(), None if kv is None else kv[:base].contiguous()
        kb, kvb = k[base:].contiguous(), None if kv is None else kv[base:].contiguous()
        sea = a.data.contiguous()
        seb = b.data.contiguous() if b is not None else None
        bvalid = b.valid if b is not None else None
        cnt = torch.empty(n, dtype=torch.int64, device=dev)
        longest = _vlen(a) if b is None else torch.maximum(_vlen(a), _vlen(b))
        args = (ptr(sea), ptr(a.valid), ptr(ka), ptr(kva), ka.numel(), ptr(seb), ptr(bvalid), ptr(kb), ptr(kvb),
                kb.numel(), _SET_OPS[op], n)
        launch("list_set_count").list_set_count(*args, ptr(cnt), stream(cnt))
        off, total, mx = _offsets(torch.zeros_like(cnt) if boolean else cnt, longest)
        if mx <= min(LIST_FAST_MAX, launch_bound()):
            if boolean:
                return Column(T.BOOL, cnt > 0, valid)
            idx = torch.empty(total, dtype=torch.int64, device=dev)
            launch("list_set_write").list_set_write(*args, ptr(off), base, total, ptr(idx), stream(idx))
            done = (off, idx)
    if done is None:
        KERNEL_CALLS["list_set_generic"] += 1
        done = _set_generic(op, a, b, src, k, kv, base)
        if boolean:
            return Column(T.BOOL, done, valid)
    off, idx = done
    return _list_col(a.dtype, _se_from(off), valid, take(src, idx, neg=True))


def launch_bound() -> int:
    """The LDS kernels' compiled bound (nested.hip kListFastMax)."""
    from ._lib import native
    return int(native().LIST_FAST_MAX)


def distinct(col: Column) -> Column:
    return _set_op("distinct", col, None)


def union(a: Column, b: Column) -> Column:
    return _set_op("union", a, b)


def intersect(a: Column, b: Column) -> Column:
    return _set_op("intersect", a, b)


def except_(a: Column, b: Column) -> Column:
    return _set_op("except", a, b)


def has_all(a: Column, b: Column) -> Column:
    return _set_op("has_all", a, b)


def has_any(a: Column, b: Column) -> Column:
    return _set_op("has_any", a, b)


def sort(col: Column, desc: bool = False, nulls_first: bool = True) -> Column:
    """array_sort(l [, 'ASC'|'DESC' [, 'NULLS FIRST'|'NULLS LAST']])."""
    from .gather import take
    from .sort import argsort
    _check_flat(col, "array_sort()")
    child = col.nested.child
    n = len(col)
    dev = col.device
    keys, kv = _order_keys(child)
    ln = _vlen(col)
    off, total, mx = _offsets(ln, ln)
    idx = None
    if is_gpu(keys) and mx <= min(LIST_FAST_MAX, launch_bound()):
        idx = torch.empty(total, dtype=torch.int64, device=dev)
        launch("list_sort_idx").list_sort_idx(ptr(col.data.contiguous()), ptr(col.valid), ptr(keys), ptr(kv),
                                              keys.numel(), int(desc), int(nulls_first), n, ptr(off), total, ptr(idx),
                                              stream(idx))
    if idx is None:
        # generic: one stable sort of the elements by (row, key)
        KERNEL_CALLS["list_sort_generic"] += 1
        from .hashing import expand_ranges
        p, c = expand_ranges(_starts(col), ln, len(child), scanned=(off[:-1].contiguous(), total))
        p, c = p.long(), c.long()
        ev = kv.index_select(0, c) if kv is not None else None
        perm = argsort([(p, False, False, None), (keys.index_select(0, c), desc, nulls_first, ev)], total, dev)
        idx = c.index_select(0, perm.long())
    return _list_col(col.dtype, _se_from(off), col.valid, take(child, idx, neg=True))


# ======================================================================= map functions
# DataFusion's map family (datafusion-functions-nested) on the MAP layout. The
# reference carries no fixtures for these, so the semantics are fixed here:
#   * every function gives NULL for a NULL map row;
#   * map_keys / map_values / map_entries are views over the children (entry
#     order kept), cardinality is the row's length;
#   * m[k] / element_at(m, k) is the value of the FIRST entry (in entry order)
#     whose key equals k, NULL when none does; map_extract(m, k) is that value
#     as a one-element list, [NULL] when none does (DataFusion's behaviour,
#     not its documented "empty list");
#   * a NULL needle never matches (keys cannot be NULL): m[k] is NULL and
#     map_extract gives [NULL];
#   * make_map / MAP {..} / map(keys, values) validate when the statement
#     runs: a NULL key ("map key cannot be null"), two equal keys in one row
#     ("map key must be unique") and map() lists of different lengths are
#     ExecutionErrors; map() of a NULL list is NULL;
#   * imported Arrow maps are taken as they are (duplicate keys included).

#: key types a lookup or a construction accepts (the binder answers NotSupported for the rest)
def map_key_ok(t: T.DataType) -> bool:
    return t.is_integer or t.kind in ("bool", "date32", "timestamp", "utf8") or \
        (t.is_decimal and t.precision <= 18)


def _map_col(dtype: T.DataType, se: torch.Tensor, valid, keys: Column, values: Column) -> Column:
    return Column(dtype, se, valid, dictionary=Nested(children={"key": keys, "value": values}))


def map_keys(col: Column) -> Column:
    """map_keys(m): List(key), a view sharing the map's (start, length) rows."""
    return _list_col(T.LIST(col.dtype.key), col.data, col.valid, col.nested.children["key"])


def map_values(col: Column) -> Column:
    """map_values(m): List(value), a view like map_keys."""
    return _list_col(T.LIST(col.dtype.value), col.data, col.valid, col.nested.children["value"])


def map_entries(col: Column) -> Column:
    """map_entries(m): List(Struct(key, value)); the struct child is row ids
    over the map's own children."""
    kids = col.nested.children
    st = T.STRUCT(list(col.dtype.fields))
    child = Column(st, _rowids(len(col.nested), col.device), None, dictionary=Nested(children=dict(kids)))
    return _list_col(T.LIST(st), col.data, col.valid, child)


def _needle_bytes(value: str, device) -> Tuple[torch.Tensor, int, int]:
    """Device buffer of a constant string needle for map_lookup_idx_str: four
    copies, copy m at byte m * stride + m, so a key at any byte alignment has
    a copy it compares with dword by dword."""
    from . import strings as S
    b = value.encode("utf-8")
    stride = (len(b) + 3) // 4 * 4 + 4

    def build():
        buf = bytearray(4 * stride + 4)
        for m in range(4):
            buf[m * stride + m: m * stride + m + len(b)] = b
        return torch.frombuffer(buf, dtype=torch.uint8).clone().to(device)
    return S._consts(("map_needle", b, str(device)), build), len(b), stride


def _dict_code(col: Column, value: str) -> int:
    """Code of ``value`` in a dictionary column's dictionary (-1: absent),
    found once per dictionary and needle."""
    cache = col.dictionary.derived()
    key = ("code_of", value)
    if key not in cache:
        check_not_capturing("dictionary code lookup")
        vals = col.dict_values()
        cache[key] = vals.index(value) if value in vals else -1
    return cache[key]


def _lookup_by_position(col: Column, needle: Column) -> torch.Tensor:
    """Child row of the first match through the list equality keys
    (array_position): per-row needles against a dictionary-coded key child,
    and the CPU form of per-row string needles."""
    pos = position(map_keys(col), needle)
    ok = pos.valid if pos.valid is not None else torch.ones_like(pos.data, dtype=torch.bool)
    return torch.where(ok, _starts(col) + pos.data - 1, torch.full_like(pos.data, -1))


def map_lookup_idx(col: Column, needle, needle_is_const: bool) -> torch.Tensor:
    """Per row the child row of the first entry whose key equals the needle,
    -1 for none (no match, NULL map row, NULL needle). ``needle``: a constant
    in the engine's representation of the key type (None never matches) or a
    Column of the key type with one needle per row. Keys are read in place:
    fixed-width keys at their own width, plain strings by length and bytes, a
    dictionary-coded key child through its codes once the constant's code is
    known; only per-row needles over a dictionary-coded key child go through
    the list equality keys."""
    from . import strings as S
    n = len(col)
    dev = col.device
    kc = col.nested.children["key"]
    if needle_is_const and needle is None or n == 0:
        return torch.full((n,), -1, dtype=torch.int64, device=dev)
    nv = None if needle_is_const else needle.valid
    if kc.dtype.is_string:
        if needle_is_const and kc.is_dict:
            code = _dict_code(kc, str(needle))
            if code < 0:
                return torch.full((n,), -1, dtype=torch.int64, device=dev)
            keys, nconst, nt = kc.data, code, None
        elif kc.is_dict:
            return _lookup_by_position(col, needle)
        else:
            keys = None
    else:
        if kc.is_wide:
            raise NotSupported("map lookup over 128-bit decimal keys")
        keys = kc.data
        nconst = 0 if not needle_is_const else int(needle)
        nt = None if needle_is_const else needle.data.to(torch.int64).contiguous()
    se = col.data.contiguous()
    if is_gpu(se):
        out = torch.empty(n, dtype=torch.int64, device=dev)
        if keys is not None:
            keys = keys.contiguous()
            launch("map_lookup_idx").map_lookup_idx(ptr(se), ptr(col.valid), n, len(kc), keys.element_size(),
                                                    ptr(keys), ptr(kc.valid), ptr(nt), ptr(nv), nconst, ptr(out),
                                                    stream(out))
            return out
        koff, kb = kc.offsets.contiguous(), kc.data.contiguous()
        if needle_is_const:
            buf, ln, stride = _needle_bytes(str(needle), dev)
            noff, nb = None, buf
        else:
            nd = S.decode(needle) if needle.is_dict else needle
            noff, nb, ln, stride = nd.offsets.contiguous(), nd.data.contiguous(), 0, 0
        launch("map_lookup_idx").map_lookup_idx_str(ptr(se), ptr(col.valid), n, len(kc), ptr(koff), ptr(kb),
                                                    kb.numel(), ptr(kc.valid), ptr(noff), ptr(nb), nb.numel(),
                                                    ptr(nv), ln, stride, ptr(out), stream(out))
        return out
    # CPU: the first matching element per row
    if keys is None and not needle_is_const:
        return _lookup_by_position(col, needle)
    p, c, _, _ = _elements(map_keys(col))
    if keys is None:
        eq = S.in_list(kc, [str(needle)]).to(torch.bool).index_select(0, c)
    elif nt is None:
        eq = keys.index_select(0, c).to(torch.int64) == nconst
    else:
        eq = keys.index_select(0, c).to(torch.int64) == nt.index_select(0, p)
        if nv is not None:
            eq = eq & nv.index_select(0, p)
    if kc.valid is not None:
        eq = eq & kc.valid.index_select(0, c)
    idx = torch.full((n,), _I64_MAX, dtype=torch.int64).scatter_reduce(
        0, p, torch.where(eq, c, torch.full_like(c, _I64_MAX)), reduce="amin")
    return torch.where(idx == _I64_MAX, torch.full_like(idx, -1), idx)


def map_element(col: Column, needle, needle_is_const: bool) -> Column:
    """m[k] / element_at(m, k): the value, NULL when the key is absent."""
    from .gather import take
    return take(col.nested.children["value"], map_lookup_idx(col, needle, needle_is_const), neg=True)


def map_extract(col: Column, needle, needle_is_const: bool) -> Column:
    """map_extract(m, k): [value] of the first matching entry, [NULL] when
    none matches, NULL for a NULL map."""
    from .gather import take
    n = len(col)
    child = take(col.nested.children["value"], map_lookup_idx(col, needle, needle_is_const), neg=True)
    if is_gpu(col.data) and n:
        se = torch.empty((n, 2), dtype=torch.int64, device=col.device)
        launch("list_slots").list_slots(n, 1, ptr(se), stream(se))
    else:
        r = _rowids(n, col.device)
        se = torch.stack([r, torch.ones_like(r)], 1)
    return _list_col(T.LIST(col.dtype.value), se, col.valid, child)


def _check_map_keys(keys: Column, mismatch: Optional[torch.Tensor] = None) -> None:
    """Construction errors of a map whose keys are the rows of the list
    column ``keys`` (its child holds exactly the entries): a NULL key, two
    equal keys in one row (the distinct keys of a row, counted by the set
    kernels over the list equality keys, against its length) and, for map(),
    rows whose two lists differ in length. One readback for all of them."""
    from ._lib import to_host_ints
    n = len(keys)
    if n == 0:
        return
    dev = keys.device
    kc = keys.nested.child
    ln = _vlen(keys)
    flag = lambda t: t.any().reshape(1).to(torch.int64)   # noqa: E731
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    f_len = flag(mismatch) if mismatch is not None else zero
    f_null = flag(~kc.valid) if kc.valid is not None and len(kc) else zero
    k, kv = _eq_keys(kc)
    cnt = None
    if is_gpu(k):
        cnt = torch.empty(n, dtype=torch.int64, device=dev)
        launch("list_set_count").list_set_count(ptr(keys.data.contiguous()), ptr(keys.valid), ptr(k), ptr(kv),
                                                k.numel(), 0, 0, 0, 0, 0, _SET_OPS["distinct"], n, ptr(cnt),
                                                stream(cnt))
        bad_len, bad_null, bad_dup, longest = to_host_ints(torch.cat([f_len, f_null, flag(cnt != ln),
                                                                      ln.max().reshape(1)]))
        if longest > min(LIST_FAST_MAX, launch_bound()):
            cnt = None
    if cnt is None:
        if is_gpu(k):
            KERNEL_CALLS["list_set_generic"] += 1
        off, _ = _set_generic("distinct", keys, None, kc, k, kv, len(kc))
        bad_len, bad_null, bad_dup = to_host_ints(torch.cat([f_len, f_null, flag((off[1:] - off[:-1]) != ln)]))
    if bad_len:
        raise ExecutionError("map(): the key list and the value list of a row differ in length")
    if bad_null:
        raise ExecutionError("map key cannot be null")
    if bad_dup:
        raise ExecutionError("map key must be unique")


def make_map(key_cols: Sequence[Column], value_cols: Sequence[Column], n: int, dtype: T.DataType, device) -> Column:
    """make_map(k1, v1, ..) / MAP {k1: v1, ..}: one map of len(key_cols)
    entries per row, keys and values interleaved like make_array."""
    keys = make_list(key_cols, n, T.LIST(dtype.key), device)
    vals = make_list(value_cols, n, T.LIST(dtype.value), device)
    if key_cols:
        _check_map_keys(keys)
    return _map_col(dtype, keys.data, None, keys.nested.child, vals.nested.child)


def map_from_lists(keys: Column, vals: Column, dtype: T.DataType) -> Column:
    """map(keys_list, values_list): the two lists zipped per row, NULL when
    either is NULL. Both lists are compacted into one entry order (the
    list_parts kernels), whatever their children looked like."""
    n = len(keys)
    valid = _and(keys.valid, vals.valid)
    lk, lv = lengths(keys).clamp(min=0), lengths(vals).clamp(min=0)
    mismatch = lk != lv
    ln = torch.minimum(lk, lv)
    if valid is not None:
        mismatch = mismatch & valid
        ln = torch.where(valid, ln, torch.zeros_like(ln))
    k2 = _from_parts([(_starts(keys), ln, 1)], keys.nested.child, T.LIST(dtype.key), valid, n)
    v2 = _from_parts([(_starts(vals), ln, 1)], vals.nested.child, T.LIST(dtype.value), valid, n)
    _check_map_keys(k2, mismatch)
    return _map_col(dtype, k2.data, valid, k2.nested.child, v2.nested.child)
