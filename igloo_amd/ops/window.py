"""Window-function primitives (csrc/kernels/window.hip).

Rows arrive sorted by (partition, order) keys; ``ids`` are the sorted
partition (or peer-group) ids, so a segment is a run of equal ids. GPU
tensors run the hand-written gfx950 kernels; CPU tensors take the torch
reference path below (same results: the numerics oracle of the GPU tests).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import is_gpu, launch, ptr, stream, to_host_int, to_host_ints

# value sources (kernels.h WinVal)
V_I64, V_I32, V_F64, V_ONE, V_HEADIDX, V_HEAD2 = range(6)
# scan operators
SUM_I, SUM_F, MIN_I, MAX_I, MIN_F, MAX_F = range(6)
# ranking / index functions (kernels.h WinFn)
ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST, NTILE = range(6)
LAG, FIRST, LAST, NTH = 10, 11, 12, 13
FRAME_KIND = {"unbounded_preceding": 0, "preceding": 1, "current": 2, "following": 3, "unbounded_following": 4}
UNIT = {"rows": 0, "range": 1, "groups": 2}

_I64MIN, _I64MAX = -2**63, 2**63 - 1


def _identity(op: int):
    # (MIN_F / MAX_F scan ordered int64 images on the host path and take their identities there)
    return {SUM_I: 0, SUM_F: 0.0, MIN_I: _I64MAX, MAX_I: _I64MIN, MIN_F: float("inf"), MAX_F: float("-inf")}[op]


def seg_scan(ids: Optional[torch.Tensor], vals: Optional[torch.Tensor], vkind: int, op: int, n: int,
             valid: Optional[torch.Tensor] = None, ids2: Optional[torch.Tensor] = None, reverse: bool = False,
             err: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """Segmented inclusive scan in row order (``reverse``: from the end).
    Segments are runs of equal ``ids`` (None: one segment). Values: a column
    (``vals`` int64 / int32 / f64), 1 per row (V_ONE), the row index at heads
    of ``ids2`` (V_HEADIDX) or a 0/1 head flag of ``ids2`` (V_HEAD2). NULL
    rows (``valid`` False) contribute the operator's identity (0 for counts).
    f64 min / max follow the total order -inf < ... < +inf < NaN (the order of
    the GROUP BY aggregates), so the identity of MIN_F is a NaN.
    Returns int64, or float64 for the f64 operators. int64 sums wrap; ``err``
    (int32 [1]) is set if and only if some row's running sum (in scan order,
    inside its segment) lies outside int64, on both devices."""
    ref = next((t for t in (ids, vals, ids2, valid) if t is not None), None)
    dev = ref.device if ref is not None else torch.device(device or "cpu")
    f64 = op in (SUM_F, MIN_F, MAX_F)
    if n == 0:
        return torch.zeros(0, dtype=torch.float64 if f64 else torch.int64, device=dev)
    if not dev.type == "cuda":
        out = _seg_scan_cpu(ids, vals, vkind, op, n, valid, ids2, reverse)
        if err is not None and op == SUM_I and vkind == V_I64:
            # exact overflow test: the scans of the two 32-bit halves cannot
            # overflow (n < 2^31), and their carry-joined top word says whether
            # the running sum fits
            v = vals.to(torch.int64)
            s0 = _seg_scan_cpu(ids, v & 0xFFFFFFFF, V_I64, SUM_I, n, valid, ids2, reverse)
            s1 = _seg_scan_cpu(ids, v >> 32, V_I64, SUM_I, n, valid, ids2, reverse)
            top = s1 + (s0 >> 32)
            if bool(((top < -2**31) | (top >= 2**31)).any()):
                err.fill_(1)
        return out
    N = launch("win_seg_scan")
    tiles = N.win_scan_tiles(n)
    tflag = torch.empty(max(tiles, 1), dtype=torch.int32, device=dev)
    tval = torch.empty(max(tiles, 1), dtype=torch.int64, device=dev)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    if vals is not None and vkind == V_F64:
        vals = vals.to(torch.float64).contiguous().view(torch.int64)
    elif vals is not None:
        vals = vals.contiguous()
    N.win_seg_scan(ptr(ids), ids is not None and ids.dtype == torch.int64, ptr(ids2),
                   ids2 is not None and ids2.dtype == torch.int64, ptr(vals), vkind,
                   ptr(valid.contiguous() if valid is not None else None), n, op, reverse, ptr(tflag), ptr(tval),
                   ptr(out), ptr(err), stream(out))
    return out.view(torch.float64) if f64 else out


def _heads(ids: Optional[torch.Tensor], order: torch.Tensor, n: int) -> torch.Tensor:
    h = torch.zeros(n, dtype=torch.bool)
    h[0] = True
    if ids is not None and n > 1:
        x = ids.to(torch.int64)[order]
        h[1:] = x[1:] != x[:-1]
    return h


def _seg_scan_cpu(ids, vals, vkind, op, n, valid, ids2, reverse) -> torch.Tensor:
    order = torch.arange(n - 1, -1, -1) if reverse else torch.arange(n)
    f64 = op in (SUM_F, MIN_F, MAX_F)
    ident = _identity(op)
    h = _heads(ids, order, n)
    if vkind in (V_I64, V_I32):
        v = vals.to(torch.int64)[order]
    elif vkind == V_F64:
        v = vals.to(torch.float64)[order]
    elif vkind == V_ONE:
        v = torch.ones(n, dtype=torch.int64)
    elif vkind == V_HEADIDX:
        v = torch.where(_heads(ids2, order, n), order, torch.full((n,), ident, dtype=torch.int64))
    else:
        v = _heads(ids2, order, n).to(torch.int64)
    ordered = op in (MIN_F, MAX_F)
    if ordered:
        # total order of the kernels (NaN above +inf): scan the int64 images
        v = _f64_ord(v.to(torch.float64).contiguous().view(torch.int64))
        ident = _I64MAX if op == MIN_F else int(_f64_ord(torch.tensor(float("-inf")).double().view(torch.int64)))
    if valid is not None:
        z = 0 if vkind in (V_ONE, V_HEAD2) else ident
        v = torch.where(valid[order], v, torch.full_like(v, z))
    if f64 and not ordered:
        v = v.to(torch.float64)
    # Hillis-Steele segmented scan: (f1,v1)+(f2,v2) = (f1|f2, f2 ? v2 : v1 op v2)
    f = h.clone()
    d = 1
    while d < n:
        a, b = v[:-d], v[d:]
        if op in (SUM_I, SUM_F):
            comb = a + b
        elif op in (MIN_I, MIN_F):
            comb = torch.minimum(a, b)
        else:
            comb = torch.maximum(a, b)
        nv = v.clone()
        nv[d:] = torch.where(f[d:], b, comb)
        nf = f.clone()
        nf[d:] = f[d:] | f[:-d]
        v, f = nv, nf
        d *= 2
    out = torch.empty_like(v)
    out[order] = v
    return _f64_ord(out).view(torch.float64) if ordered else out


def _f64_ord(bits: torch.Tensor) -> torch.Tensor:
    """Order-preserving int64 image of f64 bit patterns (window.hip f64_ord;
    its own inverse): -inf < ... < -0.0 < +0.0 < ... < +inf < NaN."""
    return torch.where(bits >= 0, bits, bits ^ _I64MAX)


def _sat_add(a: torch.Tensor, o: int) -> torch.Tensor:
    """a + o on int64, saturating instead of wrapping (window.hip sat_add)."""
    s = a + o
    if o >= 0:
        return torch.where(s < a, torch.full_like(a, _I64MAX), s)
    return torch.where(s > a, torch.full_like(a, _I64MIN), s)


def bounds(n: int, ss, se, ps, pe, unit: str, skind: str, soff, ekind: str, eoff, key=None, key_valid=None,
           desc: bool = False, gnum=None, gpos=None, ngroups: int = 0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row frame [lo, hi] (inclusive row indices; hi < lo = empty).
    ss/se: partition start/end per row (None: the whole input), ps/pe: peer
    group start/end, key: sorted ORDER BY key (int64 or f64) for RANGE
    offsets, gnum/gpos: global peer-group number per row / first row per
    group for GROUPS offsets."""
    ref = next((t for t in (ss, ps, key, gnum) if t is not None), None)
    dev = ref.device if ref is not None else torch.device(device or "cpu")
    key_f64 = key is not None and key.dtype.is_floating_point

    def _i(o):
        return 0 if o is None else int(o)

    def _f(o):
        return 0.0 if o is None else float(o)
    if dev.type == "cuda":
        lo = torch.empty(n, dtype=torch.int64, device=dev)
        hi = torch.empty(n, dtype=torch.int64, device=dev)
        if key is not None:
            key = key.to(torch.float64 if key_f64 else torch.int64).contiguous()
        launch("win_bounds").win_bounds(n, ptr(ss), ptr(se), ptr(ps), ptr(pe), UNIT[unit], FRAME_KIND[skind],
                                        _i(soff) if not key_f64 else 0, _f(soff), FRAME_KIND[ekind],
                                        _i(eoff) if not key_f64 else 0, _f(eoff), ptr(key), key_f64,
                                        ptr(key_valid), desc, ptr(gnum), ptr(gpos), ngroups, ptr(lo), ptr(hi),
                                        stream(lo))
        return lo, hi
    r = torch.arange(n, dtype=torch.int64)
    s0 = ss if ss is not None else torch.zeros(n, dtype=torch.int64)
    e0 = se if se is not None else torch.full((n,), n - 1, dtype=torch.int64)
    lo, hi = s0.clone(), e0.clone()
    sk, ek = FRAME_KIND[skind], FRAME_KIND[ekind]
    if sk == 2:
        lo = r.clone() if unit == "rows" else ps.clone()
    if ek == 2:
        hi = r.clone() if unit == "rows" else pe.clone()
    if unit == "rows":
        if sk == 1:
            lo = _sat_add(r, -_i(soff))
        elif sk == 3:
            lo = _sat_add(r, _i(soff))
        if ek == 1:
            hi = _sat_add(r, -_i(eoff))
        elif ek == 3:
            hi = _sat_add(r, _i(eoff))
    elif unit == "range" and (sk in (1, 3) or ek in (1, 3)):
        lo, hi = _range_cpu(n, s0, e0, ps, pe, sk, soff, ek, eoff, key, key_valid, desc, lo, hi)
    elif unit == "groups":
        g, g0, g1 = gnum, gnum[s0], gnum[e0]
        gend = torch.where(torch.arange(ngroups) + 1 < ngroups,
                           torch.cat([gpos[1:], gpos.new_tensor([n])]) - 1, torch.full((ngroups,), n - 1))
        if sk == 1:
            gg = g - _i(soff)
            lo = torch.where(gg < g0, s0, gpos[gg.clamp(min=0)])
        elif sk == 3:
            gg = _sat_add(g, _i(soff))
            lo = torch.where(gg > g1, e0 + 1, gpos[gg.clamp(max=ngroups - 1)])
        if ek == 1:
            gg = g - _i(eoff)
            hi = torch.where(gg < g0, s0 - 1, gend[gg.clamp(min=0)])
        elif ek == 3:
            gg = _sat_add(g, _i(eoff))
            hi = torch.where(gg > g1, e0, gend[gg.clamp(max=ngroups - 1)])
    return torch.maximum(lo, s0), torch.minimum(hi, e0)


def _search(key, lo, hi, t, desc, upper):
    """Vectorised binary search of every row's target inside [lo, hi]
    (the kernel's lower_idx / upper_idx)."""
    a, b = lo.clone(), hi + 1
    n = key.numel()
    for _ in range(64):
        act = a < b
        if not bool(act.any()):
            break
        m = a + ((b - a) >> 1)
        km = key[m.clamp(0, max(n - 1, 0))]
        if upper:
            go_right = (km >= t) if desc else (km <= t)
        else:
            go_right = (km > t) if desc else (km < t)
        a = torch.where(act & go_right, m + 1, a)
        b = torch.where(act & ~go_right, m, b)
    return a - 1 if upper else a


def _range_cpu(n, s0, e0, ps, pe, sk, soff, ek, eoff, key, key_valid, desc, lo, hi):
    f64 = key.dtype.is_floating_point
    k = key.to(torch.float64 if f64 else torch.int64)
    nb, ne = s0.clone(), e0.clone()
    if key_valid is not None:
        kv = key_valid
        nb = torch.where(~kv[s0], pe[s0] + 1, nb)
        ne = torch.where(~kv[e0], ps[e0] - 1, ne)

    def shift(forward, off):
        up = forward != desc
        if f64:
            return k + float(off) if up else k - float(off)
        return _sat_add(k, int(off) if up else -int(off))
    if sk == 1:
        lo = _search(k, nb, ne, shift(False, soff), desc, False)
    elif sk == 3:
        lo = _search(k, nb, ne, shift(True, soff), desc, False)
    if ek == 1:
        hi = _search(k, nb, ne, shift(False, eoff), desc, True)
    elif ek == 3:
        hi = _search(k, nb, ne, shift(True, eoff), desc, True)
    if key_valid is not None:
        nul = ~key_valid
        if sk != 0:
            lo = torch.where(nul, ps, lo)
        if ek != 4:
            hi = torch.where(nul, pe, hi)
    return lo, hi


def frame_sum(psum: Optional[torch.Tensor], pcnt: Optional[torch.Tensor], lo, hi, n: int):
    """Framed sum and count from inclusive global prefixes (sum: int64
    wrapping or f64). The int64 difference is taken mod 2^64, so prefixes
    that have wrapped still give the exact frame sum whenever that sum fits;
    nothing here reports a frame sum that does not (exec/window.py sums
    32-bit halves where that can happen)."""
    if n == 0 or not lo.is_cuda:
        empty = hi < lo
        li = (lo - 1).clamp(min=0)

        def diff(p):
            if p is None:
                return None
            z = torch.zeros((), dtype=p.dtype)
            before = torch.where(lo > 0, p[li] if n else p[:0], z)
            return torch.where(empty, z, p[hi.clamp(min=0)] - before) if n else p[:0]
        return diff(psum), diff(pcnt)
    f64 = psum is not None and psum.dtype == torch.float64
    so = torch.empty(n, dtype=torch.int64, device=lo.device) if psum is not None else None
    co = torch.empty(n, dtype=torch.int64, device=lo.device) if pcnt is not None else None
    launch("win_frame_sum").win_frame_sum(ptr(psum.view(torch.int64) if f64 else psum), f64, ptr(pcnt), ptr(lo),
                                          ptr(hi), n, ptr(so), ptr(co), stream(lo))
    return (so.view(torch.float64) if f64 else so), co


#: frames at most this wide loop over their rows; wider ones use a sparse table
LOOP_MAX_WIDTH = 32


def frame_minmax(vals: torch.Tensor, valid: Optional[torch.Tensor], lo, hi, n: int, is_max: bool):
    """min / max over each row's frame [lo, hi] -> (values, valid). Narrow
    frames: a loop over the frame; wider ones: a sparse table of
    ceil(log2(width)) levels (one pass each) and two reads per row, so a
    ``ROWS BETWEEN 100000 PRECEDING`` frame costs O(n log w), not O(n w).
    Floats follow the total order of ``seg_scan`` (NaN above +inf) on every
    path. NULL rows are skipped; a frame without a value is invalid."""
    f64 = vals.dtype.is_floating_point
    if n == 0:
        return torch.zeros(0, dtype=torch.float64 if f64 else torch.int64, device=lo.device), \
            torch.zeros(0, dtype=torch.bool, device=lo.device)
    widest = to_host_int((hi - lo).max()) + 1
    v = vals.to(torch.float64 if f64 else torch.int64).contiguous()
    if lo.is_cuda and widest <= LOOP_MAX_WIDTH:
        out = torch.empty(n, dtype=torch.int64, device=lo.device)
        ov = torch.empty(n, dtype=torch.bool, device=lo.device)
        launch("win_frame_minmax").win_frame_minmax(ptr(v.view(torch.int64) if f64 else v), f64, is_max,
                                                    ptr(valid), ptr(lo), ptr(hi), n, ptr(out), ptr(ov), stream(out))
        return (out.view(torch.float64) if f64 else out), ov
    levels = max(1, widest.bit_length())
    pcnt = None
    if valid is not None:
        pcnt = torch.cumsum(valid.to(torch.int64), 0)
    if lo.is_cuda:
        table = torch.empty((levels, n), dtype=torch.int64, device=lo.device)
        out = torch.empty(n, dtype=torch.int64, device=lo.device)
        ov = torch.empty(n, dtype=torch.bool, device=lo.device)
        st = stream(out)
        N = launch("win_sparse")
        N.win_sparse_build(ptr(v.view(torch.int64) if f64 else v), f64, ptr(valid), n, is_max, levels, ptr(table), st)
        N.win_sparse_query(ptr(table), levels, n, ptr(lo.contiguous()), ptr(hi.contiguous()), ptr(pcnt), is_max,
                           f64, ptr(out), ptr(ov), st)
        del table
        return (out.view(torch.float64) if f64 else out), ov
    # host: the same sparse table with torch ops
    # (floats as their ordered int64 images, like the kernels: NaN is the greatest value)
    ident = _I64MIN if is_max else _I64MAX
    cur = _f64_ord(v.view(torch.int64)) if f64 else v.clone()
    if valid is not None:
        cur = torch.where(valid, cur, torch.full_like(cur, ident))
    tabs = [cur]
    for k in range(1, levels):
        half = 1 << (k - 1)
        prev = tabs[-1]
        nxt = prev.clone()
        if half < n:
            nxt[:n - half] = torch.maximum(prev[:n - half], prev[half:]) if is_max else \
                torch.minimum(prev[:n - half], prev[half:])
        tabs.append(nxt)
    table = torch.stack(tabs)
    ok = hi >= lo
    w = (hi - lo + 1).clamp(min=1)
    k = torch.floor(torch.log2(w.to(torch.float64))).to(torch.int64).clamp(max=levels - 1)
    lo_c = lo.clamp(0, n - 1)
    hi2 = (hi - (1 << k) + 1).clamp(0, n - 1)
    a = table[k, lo_c]
    b = table[k, hi2]
    out = torch.maximum(a, b) if is_max else torch.minimum(a, b)
    if pcnt is not None:
        cnt = pcnt[hi.clamp(0, n - 1)] - torch.where(lo > 0, pcnt[(lo - 1).clamp(min=0)], torch.zeros_like(lo))
        ok = ok & (cnt > 0)
    out = torch.where(ok, out, torch.zeros_like(out))
    if f64:
        out = torch.where(ok, _f64_ord(out), out).view(torch.float64)
    return out, ok


#: positions one workgroup sorts inside LDS when the merge-sort tree is built
#: (window_select.h kSelectTile): sizes around it cross from one tile to several
SELECT_TILE = 2048


def frame_kth(vals: torch.Tensor, valid: Optional[torch.Tensor], lo, hi, k0, k1, n: int):
    """Order statistics of each row's frame: the positions (rows of the
    window-sorted order) holding ranks ``k0`` and ``k1`` (None: one rank; then
    the second result is None) among the valid values of frame [lo, hi], in
    (value, position) order. -1 where the rank is outside [0, count), the frame
    is empty or it does not lie inside [0, n). ``vals``: int64, or float64,
    which compares as its ``_f64_ord`` image (NaN above +inf, -0.0 below +0.0).

    GPU: frames of at most LOOP_MAX_WIDTH rows take a counting loop
    (``win_frame_kth``); wider ones a merge-sort tree over value ranks
    (``win_select``: one argsort, ceil(log2 m) levels of m int32 for m valid
    rows, freed on return, and a descent of about log2(m)^2 loads per row).
    CPU: a numpy sort of every frame's valid (value, position) pairs, O(n w)
    pairs for frames of w rows: the oracle of the GPU paths, sharing no code
    with them."""
    from ..utils.errors import NotSupported
    if n >= 2**31:
        raise NotSupported("order statistics over window frames of 2^31 or more rows")
    dev = lo.device
    if n == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return z, (z.clone() if k1 is not None else None)
    v = vals.contiguous()
    v = _f64_ord(v.to(torch.float64).view(torch.int64)) if v.dtype.is_floating_point else v.to(torch.int64)
    if not lo.is_cuda:
        return _frame_kth_cpu(v, valid, lo, hi, k0, k1, n)
    lo, hi, k0 = lo.contiguous(), hi.contiguous(), k0.contiguous()
    k1 = k1.contiguous() if k1 is not None else None
    valid = valid.contiguous() if valid is not None else None
    pos0 = torch.empty(n, dtype=torch.int64, device=dev)
    pos1 = torch.empty(n, dtype=torch.int64, device=dev) if k1 is not None else None
    width = (hi - lo).max() + 1
    if valid is None:
        widest, m = to_host_int(width), n
    else:
        widest, m = to_host_ints(torch.stack([width, valid.sum()]))
    if widest <= LOOP_MAX_WIDTH:
        launch("win_frame_kth").win_frame_kth(ptr(v), ptr(valid), n, ptr(lo), ptr(hi), ptr(k0), ptr(k1), ptr(pos0),
                                              ptr(pos1), stream(pos0))
        return pos0, pos1
    from . import sort as SO
    if m <= 1:
        # no tree to build: nothing is valid, or one row is
        if m == 0:
            pos0.fill_(-1)
            return pos0, (pos1.fill_(-1) if pos1 is not None else None)
        p = valid.to(torch.int64).argmax()
        inside = (lo >= 0) & (hi < n) & (lo <= p) & (p <= hi)
        neg = torch.full_like(lo, -1)
        return torch.where(inside & (k0 == 0), p, neg), \
            (torch.where(inside & (k1 == 0), p, neg) if k1 is not None else None)
    perm = SO.argsort([(v, False, False, valid)], n, dev)
    ranks = perm[:m].to(torch.int32).contiguous()       # level 0: the valid positions by ascending value
    N = launch("win_select")
    assert N.win_select_tile() == SELECT_TILE
    levels = (m - 1).bit_length()
    tree = torch.empty((levels, m), dtype=torch.int32, device=dev)
    st = stream(pos0)
    N.win_select_build(ptr(ranks), m, levels, ptr(tree), st)
    N.win_select_query(ptr(ranks), ptr(tree), levels, m, n, ptr(lo), ptr(hi), ptr(k0), ptr(k1), ptr(pos0), ptr(pos1),
                       st)
    del tree
    return pos0, pos1


def _frame_kth_cpu(v, valid, lo, hi, k0, k1, n):
    import numpy as np
    x = v.numpy()
    ok = valid.numpy().astype(bool) if valid is not None else None
    lo_, hi_ = lo.numpy(), hi.numpy()
    ks = [k0.numpy()] + ([k1.numpy()] if k1 is not None else [])
    out = [np.full(n, -1, dtype=np.int64) for _ in ks]
    for r in range(n):
        a, b = int(lo_[r]), int(hi_[r])
        if a < 0 or b >= n or b < a:
            continue
        idx = np.arange(a, b + 1)
        if ok is not None:
            idx = idx[ok[a:b + 1]]
        order = idx[np.argsort(x[idx], kind="stable")]      # (value, position): positions ascend inside a tie
        for k, o in zip(ks, out):
            if 0 <= k[r] < order.size:
                o[r] = order[k[r]]
    return torch.from_numpy(out[0]), (torch.from_numpy(out[1]) if k1 is not None else None)


def rank(fn: int, arg: int, n: int, ss, se, ps, pe, dense, device) -> torch.Tensor:
    """Ranking functions (int64; percent_rank / cume_dist f64)."""
    f64 = fn in (PERCENT_RANK, CUME_DIST)
    if n and torch.device(device).type == "cuda":
        out = torch.empty(n, dtype=torch.int64, device=device)
        launch("win_rank").win_rank(fn, arg, n, ptr(ss), ptr(se), ptr(ps), ptr(pe), ptr(dense), ptr(out),
                                    stream(out))
        return out.view(torch.float64) if f64 else out
    r = torch.arange(n, dtype=torch.int64)
    s0 = ss if ss is not None else torch.zeros(n, dtype=torch.int64)
    e0 = se if se is not None else torch.full((n,), n - 1, dtype=torch.int64)
    size = e0 - s0 + 1
    p0 = ps if ps is not None else s0
    if fn == ROW_NUMBER:
        return r - s0 + 1
    if fn == RANK:
        return p0 - s0 + 1
    if fn == DENSE_RANK:
        return dense
    if fn == PERCENT_RANK:
        return torch.where(size > 1, (p0 - s0).double() / (size - 1).clamp(min=1).double(),
                           torch.zeros(n, dtype=torch.float64))
    if fn == CUME_DIST:
        p1 = pe if pe is not None else e0
        return (p1 - s0 + 1).double() / size.double()
    j = r - s0
    q = torch.div(size, arg, rounding_mode="floor")
    rem = size - q * arg
    big = rem * (q + 1)
    qs = q.clamp(min=1)
    return torch.where(q == 0, j + 1, torch.where(j < big, torch.div(j, q + 1, rounding_mode="floor") + 1,
                                                  torch.div(j - big, qs, rounding_mode="floor") + rem + 1))


def index(fn: int, arg: int, n: int, ss, se, lo, hi, device) -> torch.Tensor:
    """Source row of lag/lead (LAG with +-k), first/last/nth_value; -1 = none."""
    if n and torch.device(device).type == "cuda":
        out = torch.empty(n, dtype=torch.int64, device=device)
        launch("win_index").win_index(fn, arg, n, ptr(ss), ptr(se), ptr(lo), ptr(hi), ptr(out), stream(out))
        return out
    r = torch.arange(n, dtype=torch.int64)
    neg = torch.full((n,), -1, dtype=torch.int64)
    if fn == LAG:
        s0 = ss if ss is not None else torch.zeros(n, dtype=torch.int64)
        e0 = se if se is not None else torch.full((n,), n - 1, dtype=torch.int64)
        j = r - arg
        return torch.where((j >= s0) & (j <= e0), j, neg)
    ok = lo <= hi
    if fn == FIRST:
        return torch.where(ok, lo, neg)
    if fn == LAST:
        return torch.where(ok, hi, neg)
    j = lo + arg - 1
    return torch.where(ok & (j <= hi), j, neg)
