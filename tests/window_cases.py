"""Case lists and checkers shared by tests/test_window_ref.py (torch CPU path)
and tests/test_window_kernels_gpu.py (gfx950 kernels): every checker runs
``igloo_amd.ops.window`` on ``device`` and compares with tests/window_ref.py.
A plain helper module; the inputs are seeded, the references are cached per
process so both files share them.
"""
import functools
import zlib

import numpy as np
import torch

import window_ref as R
from igloo_amd.ops import window as W
from igloo_amd.ops._lib import KERNEL_CALLS

TILE = 2048            # rows per scan tile: 256 threads x 8 rows; a wave covers 512
SCAN_SIZES = [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 3 * 2048 + 5]
LAYOUTS = ["one", "each", "borders", "long_then_short", "geometric"]
# (value kind, operator, name); the head-index scans run in the direction exec/window.py uses
SCAN_OPS = [
    (R.V_I64, R.SUM_I, "i64_sum"), (R.V_I64, R.MIN_I, "i64_min"), (R.V_I64, R.MAX_I, "i64_max"),
    (R.V_I32, R.SUM_I, "i32_sum"), (R.V_I32, R.MIN_I, "i32_min"), (R.V_I32, R.MAX_I, "i32_max"),
    (R.V_F64, R.SUM_F, "f64_sum"), (R.V_F64, R.MIN_F, "f64_min"), (R.V_F64, R.MAX_F, "f64_max"),
    (R.V_ONE, R.SUM_I, "count"), (R.V_HEADIDX, R.MAX_I, "headidx_fwd"), (R.V_HEADIDX, R.MIN_I, "headidx_rev"),
    (R.V_HEAD2, R.SUM_I, "head2"),
]
# scanned in both directions at every size; the others alternate above one wave
BOTH_WAYS = {"i64_sum", "i64_min", "f64_max"}


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


def dev_t(a, device, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device)


class ran:
    """On a GPU: assert that the named native launch happened inside the block."""

    def __init__(self, device, name):
        self.on = torch.device(device).type == "cuda"
        self.name = name

    def __enter__(self):
        self.before = KERNEL_CALLS[self.name]

    def __exit__(self, et, ev, tb):
        if self.on and et is None:
            assert KERNEL_CALLS[self.name] > self.before, f"kernel {self.name} did not run"
        return False


# ------------------------------------------------------------------- seg_scan
def layout_ids(layout: str, n: int, rng) -> np.ndarray:
    """Sorted segment ids (int64, increasing, with gaps) of one layout."""
    heads = np.zeros(n, dtype=bool)
    if layout == "each":
        heads[:] = True
    elif layout == "borders":
        # heads exactly at every wave (512) and tile (2048) border, and one row before and after each
        for k in range(512, n + 512, 512):
            for j in (k - 1, k, k + 1):
                if 0 < j < n:
                    heads[j] = True
    elif layout == "long_then_short":
        # one segment over tiles 0..2 (two of them head-less after the first row), then runs of 3
        first = min(n, 2 * TILE + 100)
        heads[first::3] = True
    elif layout == "geometric":
        pos = 0
        while pos < n:
            heads[pos] = True
            pos += int(rng.geometric(0.02 if rng.random() < 0.5 else 0.3))
    heads[0] = True
    return np.cumsum(heads).astype(np.int64) * 3 + 11


def nested_ids2(ids: np.ndarray, rng) -> np.ndarray:
    """Peer-group ids nested in the segments of ``ids``: every segment head
    is a peer head, and so are about a third of the other rows."""
    n = len(ids)
    h = rng.random(n) < 0.3
    h[0] = True
    h[1:] |= ids[1:] != ids[:-1]
    return np.cumsum(h).astype(np.int64)


def scan_values(vkind, op, n, rng):
    if vkind == R.V_I64 and op == R.SUM_I:
        return rng.integers(-1000, 1000, n, dtype=np.int64)
    if vkind == R.V_I64:
        # the full range, with both identities among the values
        v = rng.integers(R.I64MIN, R.I64MAX, n, dtype=np.int64, endpoint=True)
        v[rng.random(n) < 0.05] = R.I64MIN
        v[rng.random(n) < 0.05] = R.I64MAX
        return v
    if vkind == R.V_I32:
        v = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64, endpoint=True).astype(np.int32)
        v[rng.random(n) < 0.05] = -2**31
        v[rng.random(n) < 0.05] = 2**31 - 1
        return v
    if vkind == R.V_F64 and op == R.SUM_F:
        return rng.normal(size=n) * 10.0 ** rng.integers(-3, 6, n)
    if vkind == R.V_F64:
        v = rng.normal(size=n)
        for x in (float("inf"), float("-inf"), float("nan"), 0.0, -0.0):
            v[rng.random(n) < 0.03] = x
        return v
    return None


def scan_configs(n: int, layout: str):
    """[(name, vkind, op, ids kind, reverse, valid kind, ids2 kind)] run at one size and layout."""
    out = []
    i = _seed(n, layout) % 6
    for vkind, op, name in SCAN_OPS:
        if name == "headidx_fwd":
            ways = [False]
        elif name == "headidx_rev":
            ways = [True]
        elif n <= 513 or name in BOTH_WAYS:
            ways = [False, True]
        else:
            ways = [bool(i % 2)]
        for rev in ways:
            i += 1
            ids_kind = "none" if layout == "one" and i % 2 else ("i32" if i % 3 == 0 else "i64")
            valid_kind = ("none", "random", "none", "all_null", "random", "none")[i % 6]
            ids2_kind = None
            if vkind in (R.V_HEADIDX, R.V_HEAD2):
                # exec/window.py passes ids2 with and without ids
                ids2_kind = "i32" if i % 4 == 0 else "i64"
                if i % 3 == 1:
                    ids_kind = "none"
                valid_kind = "none" if i % 2 else valid_kind
            out.append((name, vkind, op, ids_kind, rev, valid_kind, ids2_kind))
    return out


@functools.lru_cache(maxsize=None)
def scan_case(n: int, layout: str):
    """Inputs and reference results of every config at one size and layout."""
    cases = []
    for cfg in scan_configs(n, layout):
        name, vkind, op, ids_kind, rev, valid_kind, ids2_kind = cfg
        rng = np.random.default_rng(_seed(n, layout, cfg))
        seg = layout_ids(layout, n, rng)
        ids = None if ids_kind == "none" else seg
        ids2 = nested_ids2(seg, rng) if ids2_kind else None
        vals = scan_values(vkind, op, n, rng)
        valid = {"none": None, "random": rng.random(n) >= 0.3, "all_null": np.zeros(n, dtype=bool)}[valid_kind]
        want, info = R.seg_scan_ref(ids, vals, vkind, op, n, valid, ids2, rev)
        cases.append((cfg, ids, ids2, vals, valid, want, info))
    return cases


def check_scan(n: int, layout: str, device) -> None:
    for cfg, ids, ids2, vals, valid, want, info in scan_case(n, layout):
        name, vkind, op, ids_kind, rev, valid_kind, ids2_kind = cfg
        idt = {"i32": torch.int32, "i64": torch.int64, "none": None}
        err = torch.zeros(1, dtype=torch.int32, device=device)
        with ran(device, "win_seg_scan"):
            got = W.seg_scan(dev_t(ids, device, idt[ids_kind]), dev_t(vals, device), vkind, op, n,
                             valid=dev_t(valid, device), ids2=dev_t(ids2, device, idt.get(ids2_kind)), reverse=rev,
                             err=err, device=device)
        got = got.cpu().tolist()
        err = int(err.cpu()[0])
        tag = f"n={n} layout={layout} {cfg}"
        assert len(got) == n, tag
        if op == R.SUM_F:
            # any order of adding m terms stays within (m - 1) u sum|x| of the exact sum
            for r in range(n):
                bound = (info["terms"][r] - 1) * R.U * info["abs"][r]
                assert abs(got[r] - want[r]) <= bound, f"{tag} row {r}: {got[r]!r} vs {want[r]!r}, bound {bound!r}"
        elif op in (R.MIN_F, R.MAX_F):
            bad = [r for r in range(n) if not R.same_f64(got[r], want[r])]
            assert not bad, f"{tag} rows {bad[:5]}: {[got[r] for r in bad[:5]]} vs {[want[r] for r in bad[:5]]}"
        else:
            bad = [r for r in range(n) if got[r] != want[r]]
            assert not bad, f"{tag} rows {bad[:5]}: {[got[r] for r in bad[:5]]} vs {[want[r] for r in bad[:5]]}"
        if op == R.SUM_I:
            assert err == int(info["overflow"]) == 0, tag


def overflow_cases():
    """(name, ids, vals, reverse): int64 sums around the overflow line."""
    big, top = 2**60, 2**63 - 1
    out = []
    # a thread's eight rows sum to 2^63 although every running sum fits
    v = np.zeros(40, dtype=np.int64)
    v[7] = -top
    v[8:16] = big
    out.append(("thread_partial", None, v, False))
    # the same across a wave border (rows 504..519) and a tile border, inside one of several segments
    n = 3 * TILE + 5
    v = np.ones(n, dtype=np.int64)
    v[500] = -top
    v[508:516] = big
    out.append(("wave_partial", None, v.copy(), False))
    ids = np.repeat(np.arange(n // 1500 + 1), 1500)[:n].astype(np.int64)
    v = np.ones(n, dtype=np.int64)
    v[TILE - 3] = -top
    v[TILE + 1:TILE + 9] = big
    out.append(("tile_partial", ids.copy(), v.copy(), False))
    v = v[::-1].copy()
    out.append(("tile_partial_reverse", ids.copy(), v, True))
    # mixed signs: large partial sums cancel inside every prefix
    v = np.tile(np.array([top, -top, top - 5, -(top - 5)], dtype=np.int64), n // 4 + 1)[:n]
    out.append(("alternating", None, v.copy(), False))
    # real overflows: inside one thread of a late tile, and only through the tile carry
    v = np.ones(n, dtype=np.int64)
    v[2 * TILE + 900] = 2**62
    v[2 * TILE + 901] = 2**62
    out.append(("real_late_tile", None, v.copy(), False))
    v = np.ones(n, dtype=np.int64)
    v[100] = 2**62
    v[2 * TILE + 8] = 2**62
    out.append(("real_through_carry", None, v.copy(), False))
    out.append(("real_through_carry_reverse", None, v.copy(), True))
    v = -np.ones(n, dtype=np.int64)
    v[10] = -2**62
    v[TILE + 77] = -2**62
    v[n - 1] = -2**61
    out.append(("real_negative", None, v.copy(), False))
    # the same pair of values in different segments does not overflow
    v = np.ones(n, dtype=np.int64)
    v[100] = 2**62
    v[1600] = 2**62
    out.append(("split_by_head", ids.copy(), v.copy(), False))
    # exactly INT64_MAX is reached, not passed; one more passes it
    v = np.zeros(n, dtype=np.int64)
    v[5] = top - 3
    v[n - 2] = 3
    out.append(("touches_max", None, v.copy(), False))
    v[n - 1] = 1
    out.append(("passes_max_by_one", None, v.copy(), False))
    rng = np.random.default_rng(77)
    for i in range(4):
        seg = layout_ids("geometric", n, rng)
        v = rng.integers(-2**61, 2**61, n, dtype=np.int64)
        v[rng.random(n) < 0.9] //= 2**(20 + 10 * i)
        out.append((f"random_{i}", seg, v, bool(i % 2)))
    return out


@functools.lru_cache(maxsize=None)
def overflow_refs():
    return [(name, ids, v, rev, *R.seg_scan_ref(ids, v, R.V_I64, R.SUM_I, len(v), None, None, rev))
            for name, ids, v, rev in overflow_cases()]


def check_overflow(device) -> None:
    seen = set()
    for name, ids, v, rev, want, info in overflow_refs():
        err = torch.zeros(1, dtype=torch.int32, device=device)
        got = W.seg_scan(dev_t(ids, device), dev_t(v, device), R.V_I64, R.SUM_I, len(v), reverse=rev, err=err,
                         device=device).cpu().tolist()
        assert int(err.cpu()[0]) == int(info["overflow"]), \
            f"{name}: err {int(err.cpu()[0])}, some running sum left int64: {info['overflow']}"
        assert got == want, name       # sums wrap: equal mod 2^64 either way
        seen.add(info["overflow"])
    assert seen == {False, True}


# --------------------------------------------------------------------- bounds
BN = 700
PART_SIZES = [1, 2, 300, 97, 1, 299]     # sums to 700: three blocks of 256 rows
PSIZE = 300
OFFSETS = [0, 1, 3, PSIZE, PSIZE + 1, 2**63 - 1]
ORDER = ["unbounded_preceding", "preceding", "current", "following", "unbounded_following"]
# every legal (start, end): the start is no unbounded following, the end no
# unbounded preceding, and the start does not come after the end
PAIRS = [(s, e) for s in ORDER[:4] for e in ORDER[1:] if ORDER.index(s) <= ORDER.index(e)]
# offset pairs of frames with two offsets
TWO = [(o, o) for o in OFFSETS] + [(0, 2**63 - 1), (2**63 - 1, 0), (1, 3), (3, 1), (PSIZE, 1), (1, PSIZE + 1),
                                   (PSIZE + 1, 3), (3, PSIZE)]


def frames(offsets, two):
    out = []
    for s, e in PAIRS:
        so, eo = s in ("preceding", "following"), e in ("preceding", "following")
        if so and eo:
            out += [(s, a, e, b) for a, b in two]
        elif so:
            out += [(s, a, e, None) for a in offsets]
        elif eo:
            out += [(s, None, e, b) for b in offsets]
        else:
            out.append((s, None, e, None))
    return out


def bounds_data(kind: str, desc: bool, nulls: str):
    """Sorted ORDER BY keys of the six partitions. kind: i64 | f64; nulls:
    none | first | last. Partition 3 (97 rows) has only NULL keys when there
    are NULLs. Keys repeat (peer groups); the 300-row partition reaches within
    10 of both int64 ends (f64: both infinities)."""
    rng = np.random.default_rng(_seed(kind, desc, nulls))
    part = np.repeat(np.arange(len(PART_SIZES)), PART_SIZES).astype(np.int64) * 5 + 2
    key = np.zeros(BN, dtype=np.int64 if kind == "i64" else np.float64)
    kv = np.ones(BN, dtype=bool)
    pos = 0
    for p, size in enumerate(PART_SIZES):
        if kind == "i64":
            k = rng.integers(-40, 40, size, dtype=np.int64)
            if size >= 200:
                k[:8] = [R.I64MIN, R.I64MIN + 3, R.I64MIN + 9, R.I64MIN + 9, R.I64MAX - 10, R.I64MAX - 5, R.I64MAX - 5,
                         R.I64MAX]
        else:
            k = np.round(rng.normal(size=size) * 8) / 2
            if size >= 200:
                k[:5] = [float("-inf"), float("-inf"), float("inf"), 1e300, -1e300]
        k = np.sort(k)
        if desc:
            k = k[::-1]
        v = np.ones(size, dtype=bool)
        if nulls != "none":
            cnt = size if p == 3 else (size // 7 if size > 2 else (1 if p == 0 else 0))
            if nulls == "first":
                v[:cnt] = False
            elif cnt:
                v[size - cnt:] = False
            k = k.copy()
            k[~v] = 0
        key[pos:pos + size], kv[pos:pos + size] = k, v
        pos += size
    # peers: equal partition and key; NULL keys are peers of each other
    h = np.ones(BN, dtype=bool)
    h[1:] = (part[1:] != part[:-1]) | (kv[1:] != kv[:-1]) | ((key[1:] != key[:-1]) & kv[1:] & kv[:-1])
    peer = np.cumsum(h).astype(np.int64)
    return part, peer, key, (kv if nulls != "none" else None)


def spans(ids: np.ndarray):
    """Per row: first and last row of its run of equal ids (plain numpy)."""
    n = len(ids)
    h = np.ones(n, dtype=bool)
    h[1:] = ids[1:] != ids[:-1]
    starts = np.flatnonzero(h)
    ends = np.concatenate([starts[1:], [n]]) - 1
    run = np.cumsum(h) - 1
    return starts[run].astype(np.int64), ends[run].astype(np.int64), run.astype(np.int64), starts.astype(np.int64)


@functools.lru_cache(maxsize=None)
def bounds_case(unit: str, kind: str, desc: bool, nulls: str):
    part, peer, key, kv = bounds_data(kind, desc, nulls)
    if unit == "range":
        offs = list(OFFSETS) + [100, 2**62]
        two = TWO + [(100, 100), (2**62, 2**62), (100, 2**62), (2**62, 100), (0, 100)]
        if kind == "f64":
            offs += [0.5]
            two += [(0.5, 0.5), (0.5, 3)]
    else:
        offs, two = OFFSETS, TWO
    out = []
    for s, so, e, eo in frames(offs, two):
        want = R.bounds_ref(BN, part, peer, unit, s, so, e, eo, key if unit == "range" else None,
                            kv if unit == "range" else None, desc)
        out.append(((s, so, e, eo), want))
    return (part, peer, key, kv), out


def check_bounds(unit: str, kind: str, desc: bool, nulls: str, device) -> None:
    (part, peer, key, kv), cases = bounds_case(unit, kind, desc, nulls)
    ss, se, _, _ = spans(part)
    ps, pe, gnum, gpos = spans(peer)
    d = functools.partial(dev_t, device=device)
    t_ss, t_se, t_ps, t_pe, t_gnum, t_gpos = d(ss), d(se), d(ps), d(pe), d(gnum), d(gpos)
    t_key, t_kv = (d(key), d(kv)) if unit == "range" else (None, None)
    for (s, so, e, eo), (wlo, whi) in cases:
        with ran(device, "win_bounds"):
            lo, hi = W.bounds(BN, t_ss, t_se, t_ps, t_pe, unit, s, so, e, eo, key=t_key, key_valid=t_kv, desc=desc,
                              gnum=t_gnum if unit == "groups" else None, gpos=t_gpos if unit == "groups" else None,
                              ngroups=len(gpos) if unit == "groups" else 0, device=device)
        lo, hi = lo.cpu().tolist(), hi.cpu().tolist()
        tag = f"{unit} {kind} desc={desc} nulls={nulls} {s} {so} .. {e} {eo}"
        for r in range(BN):
            if whi[r] < wlo[r]:
                assert hi[r] < lo[r], f"{tag} row {r}: [{lo[r]}, {hi[r]}], the frame is empty"
            else:
                assert (lo[r], hi[r]) == (wlo[r], whi[r]), f"{tag} row {r}: [{lo[r]}, {hi[r]}] vs [{wlo[r]}, {whi[r]}]"


# ------------------------------------------------------------------ frame_sum
def check_frame_sum(device) -> None:
    n = 700
    rng = np.random.default_rng(31)
    lo = rng.integers(0, n, n)
    hi = np.minimum(lo + rng.integers(0, 2, n) * rng.integers(0, n, n) + rng.integers(0, 40, n), n - 1)
    lo[:40:3] = 0
    hi = np.maximum(hi, lo)
    hi[::9] = lo[::9] - 1                       # empty frames, among them [0, -1]
    hi[0], lo[1], hi[1] = n - 1, 0, n - 1       # the whole input
    assert (hi < lo).any() and (lo == 0).any() and ((hi == -1) & (lo == 0)).any()
    valid = rng.random(n) >= 0.3
    t_lo, t_hi = dev_t(lo, device), dev_t(hi, device)
    # integers: a global prefix that has wrapped many times still gives exact frame sums mod 2^64
    vi = rng.integers(R.I64MIN // 2, R.I64MAX // 2, n, dtype=np.int64)
    for vv in (None, valid):
        masked = vi if vv is None else np.where(vv, vi, 0)
        with np.errstate(over="ignore"):
            psum = np.cumsum(masked)            # int64: wraps
        exact = 0
        wrapped = False
        for x in masked.tolist():
            exact += x
            wrapped |= not (R.I64MIN <= exact <= R.I64MAX)
        assert wrapped
        pcnt = np.cumsum(np.ones(n, dtype=np.int64) if vv is None else vv.astype(np.int64))
        wsum, wcnt, _ = R.frame_sum_ref(vi.tolist(), None if vv is None else vv.tolist(), lo.tolist(), hi.tolist())
        with ran(device, "win_frame_sum"):
            s, c = W.frame_sum(dev_t(psum, device), dev_t(pcnt, device), t_lo, t_hi, n)
        assert s.cpu().tolist() == wsum
        assert c.cpu().tolist() == wcnt
    # f64: both prefixes are within h u sum|x| of exact, their difference rounds once more
    vf = rng.normal(size=n) * 10.0 ** rng.integers(-3, 6, n)
    psum = np.cumsum(np.where(valid, vf, 0.0))
    wsum, wcnt, sabs = R.frame_sum_ref(vf.tolist(), valid.tolist(), lo.tolist(), hi.tolist())
    s, c = W.frame_sum(dev_t(psum, device), None, t_lo, t_hi, n)
    assert c is None
    got = s.cpu().tolist()
    for r in range(n):
        bound = 2 * (int(hi[r]) + 1) * R.U * sabs[r]
        assert abs(got[r] - wsum[r]) <= bound, (r, got[r], wsum[r], bound)
    s, c = W.frame_sum(None, dev_t(np.cumsum(valid.astype(np.int64)), device), t_lo, t_hi, n)
    assert s is None and c.cpu().tolist() == wcnt


# --------------------------------------------------------------- frame_minmax
MN = 3000
WIDTHS = [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, MN]
MM_PARTS = [1, 2, 1400, 597, 1000]


def minmax_values(kind: str, rng):
    if kind == "i64":
        v = rng.integers(R.I64MIN, R.I64MAX, MN, dtype=np.int64, endpoint=True)
        v[rng.random(MN) < 0.02] = R.I64MIN
        v[rng.random(MN) < 0.02] = R.I64MAX
        return v
    v = rng.normal(size=MN)
    # (NaN is float('nan') only: NaNs with the sign bit set are out of scope)
    for x in (float("inf"), float("-inf"), float("nan"), 0.0, -0.0):
        v[rng.random(MN) < 0.01] = x
    return v


def minmax_frames(width, rng):
    """[lo, hi] per row. int: constant-width ROWS frames clipped at the
    partition ends (one partition for the full width). 'mixed32' / 'mixed33':
    widths from 0 (empty) up to exactly 32 / 33."""
    r = np.arange(MN)
    if isinstance(width, int):
        sizes = [MN] if width == MN else MM_PARTS
        ids = np.repeat(np.arange(len(sizes)), sizes)
        ss, se, _, _ = spans(ids)
        a = width // 2
        lo, hi = np.maximum(ss, r - a), np.minimum(se, r + (width - 1 - a))
        assert int((hi - lo).max()) + 1 == width
        return lo, hi
    top = 32 if width == "mixed32" else 33
    w = rng.integers(0, top + 1, MN)
    lo = np.minimum(r, MN - top)
    hi = lo + w - 1
    assert int((hi - lo).max()) + 1 == top and (hi < lo).any()
    return lo, hi


@functools.lru_cache(maxsize=None)
def minmax_case(width):
    rng = np.random.default_rng(_seed("minmax", width))
    lo, hi = minmax_frames(width, rng)
    valid = rng.random(MN) >= 0.3
    valid[1500:1500 + 1100] = False            # frames without a value, at every width but the widest
    out = []
    for kind in ("i64", "f64"):
        vals = minmax_values(kind, rng)
        for is_max in (False, True):
            for vv in (None, valid):
                out.append((kind, is_max, vals, vv, R.frame_minmax_ref(vals, vv, lo.tolist(), hi.tolist(), is_max)))
    return lo, hi, out


def check_minmax(width, device) -> None:
    lo, hi, cases = minmax_case(width)
    widest = int((hi - lo).max()) + 1
    kernel = "win_frame_minmax" if widest <= 32 else "win_sparse"
    t_lo, t_hi = dev_t(lo, device), dev_t(hi, device)
    for kind, is_max, vals, vv, (want, wok) in cases:
        with ran(device, kernel):
            got, ok = W.frame_minmax(dev_t(vals, device), dev_t(vv, device), t_lo, t_hi, MN, is_max)
        got, ok = got.cpu().tolist(), ok.cpu().tolist()
        tag = f"width={width} {kind} max={is_max} nulls={vv is not None}"
        assert ok == wok, tag
        if vv is not None and width != MN:
            assert not all(wok), tag
        # (== on floats: the sign of a zero result is not pinned)
        bad = [r for r in range(MN) if wok[r] and not (R.same_f64(got[r], want[r]) if kind == "f64"
                                                       else got[r] == want[r])]
        assert not bad, f"{tag} rows {bad[:5]}: {[got[r] for r in bad[:5]]} vs {[want[r] for r in bad[:5]]}"


# ----------------------------------------------------------------- rank, index
RN = 2100
RANK_PARTS = [1, 2, 513, 700, 3, 881]
RANK_PSIZE = 700


@functools.lru_cache(maxsize=None)
def rank_data():
    rng = np.random.default_rng(5)
    part = np.repeat(np.arange(len(RANK_PARTS)), RANK_PARTS).astype(np.int64)
    h = rng.random(RN) < 0.4
    h[0] = True
    h[1:] |= part[1:] != part[:-1]
    peer = np.cumsum(h).astype(np.int64)
    return part, peer


def check_rank(fn: int, arg: int, device) -> None:
    part, peer = rank_data()
    ss, se, _, _ = spans(part)
    ps, pe, _, _ = spans(peer)
    dense = np.asarray(R.rank_ref(R.DENSE_RANK, 0, part, peer, RN), dtype=np.int64)
    want = R.rank_ref(fn, arg, part, peer, RN)
    with ran(device, "win_rank"):
        got = W.rank(fn, arg, RN, dev_t(ss, device), dev_t(se, device), dev_t(ps, device), dev_t(pe, device),
                     dev_t(dense, device), device)
    # percent_rank / cume_dist: one correctly rounded division of exact integers on both sides
    assert got.cpu().tolist() == want, (fn, arg)


def check_index(device) -> None:
    part, _ = rank_data()
    ss, se, _, _ = spans(part)
    t_ss, t_se = dev_t(ss, device), dev_t(se, device)
    for arg in (0, 1, -1, 3, -3, RANK_PSIZE, -RANK_PSIZE):
        want = R.index_ref(R.LAG, arg, RN, ss.tolist(), se.tolist(), None, None)
        with ran(device, "win_index"):
            got = W.index(R.LAG, arg, RN, t_ss, t_se, None, None, device)
        assert got.cpu().tolist() == want, ("lag", arg)
    for arg in (0, 1, -1, 3, -3):
        want = R.index_ref(R.LAG, arg, RN, None, None, None, None)
        assert W.index(R.LAG, arg, RN, None, None, None, None, device).cpu().tolist() == want, ("lag, one partition", arg)
    width = 9
    r = np.arange(RN)
    lo, hi = np.maximum(ss, r - 4), np.minimum(se, r + 4)
    hi[::11] = lo[::11] - 1                     # empty frames
    t_lo, t_hi = dev_t(lo, device), dev_t(hi, device)
    for fn, args in ((R.FIRST, [0]), (R.LAST, [0]), (R.NTH, [1, 2, width, width + 1])):
        for arg in args:
            want = R.index_ref(fn, arg, RN, None, None, lo.tolist(), hi.tolist())
            for with_seg in (False, True):
                got = W.index(fn, arg, RN, t_ss if with_seg else None, t_se if with_seg else None, t_lo, t_hi, device)
                assert got.cpu().tolist() == want, (fn, arg, with_seg)
    assert (hi - lo + 1).max() == width


# ------------------------------------------------------------------ SQL level
SQL_N = 5000


@functools.lru_cache(maxsize=None)
def nan_table():
    rng = np.random.default_rng(9)
    f = rng.normal(size=SQL_N)
    for x in (float("nan"), float("inf"), float("-inf")):
        f[rng.random(SQL_N) < 0.02] = x
    null = rng.random(SQL_N) < 0.1
    g = rng.integers(0, 4, SQL_N)
    g[:3] = [0, 1, 2]
    g[g == 3] = np.where(np.arange(SQL_N)[g == 3] < 40, 3, 0)     # a small partition too
    vals = [None if null[i] else float(f[i]) for i in range(SQL_N)]
    # group 3: only NaN and NULL; a stretch of NULLs wider than any sliding frame
    for i in range(SQL_N):
        if g[i] == 3:
            vals[i] = None if i % 2 else float("nan")
    for i in range(2000, 2300):
        vals[i] = None
    return list(range(SQL_N)), g.tolist(), vals


NAN_FRAMES = [
    ("running", "partition by g order by id", lambda j, m: (0, j)),
    ("loop", "partition by g order by id rows between 3 preceding and current row", lambda j, m: (j - 3, j)),
    ("sparse", "partition by g order by id rows between 100 preceding and 2 following", lambda j, m: (j - 100, j + 2)),
    ("reverse", "partition by g order by id rows between current row and unbounded following",
     lambda j, m: (j, m - 1)),
]


def _pick(xs, is_max):
    xs = [x for x in xs if x is not None]
    if not xs:
        return None
    return max(xs, key=R.fkey) if is_max else min(xs, key=R.fkey)


def _same_opt(a, b):
    return (a is None and b is None) or (a is not None and b is not None and R.same_f64(a, b))


def check_sql_nan(device) -> None:
    import pyarrow as pa
    import igloo_amd as ig
    ids, g, vals = nan_table()
    e = ig.QueryEngine(device=device)
    e.register_table("t", pa.table({"id": pa.array(ids, pa.int64()), "g": pa.array(g, pa.int64()),
                                    "f": pa.array(vals, pa.float64())}))
    cols = ", ".join(f"min(f) over ({spec}) mn_{name}, max(f) over ({spec}) mx_{name}" for name, spec, _ in NAN_FRAMES)
    with ran(device, "win_seg_scan"), ran(device, "win_frame_minmax"), ran(device, "win_sparse"):
        got = e.sql(f"select id, {cols}, max(f) over (partition by g) mx_all from t order by id").table.to_pylist()
    groups = {}
    for i in ids:
        groups.setdefault(g[i], []).append(i)
    for name, _, frame in NAN_FRAMES:
        for rows in groups.values():
            m = len(rows)
            for j, i in enumerate(rows):
                a, b = frame(j, m)
                xs = [vals[rows[k]] for k in range(max(a, 0), min(b, m - 1) + 1)]
                for is_max, col in ((False, f"mn_{name}"), (True, f"mx_{name}")):
                    want = _pick(xs, is_max)
                    assert _same_opt(got[i][col], want), (name, col, i, got[i][col], want)
    by_group = {r["g"]: r["m"] for r in e.sql("select g, max(f) m from t group by g").table.to_pylist()}
    for gid, rows in groups.items():
        want = _pick([vals[i] for i in rows], True)
        assert _same_opt(by_group[gid], want), ("group by", gid, by_group[gid], want)
        for i in rows:
            assert _same_opt(got[i]["mx_all"], by_group[gid]), ("over (partition by g)", i)


def check_sql_overflow(device) -> None:
    """A window SUM over BIGINT raises iff some output row's exact sum is outside int64."""
    import pyarrow as pa
    import igloo_amd as ig
    from igloo_amd.utils.errors import ExecutionError
    e = ig.QueryEngine(device=device)

    def table(name, xs):
        e.register_table(name, pa.table({"id": pa.array(range(len(xs)), pa.int64()), "x": pa.array(xs, pa.int64())}))
    # A: the global prefix of a sliding frame wraps, every frame sum fits
    xs = [3 * 2**60] * 8
    table("a", xs)
    r = e.sql("select id, sum(x) over (order by id rows between 1 preceding and current row) s from a "
              "order by id").table.to_pylist()
    assert [row["s"] for row in r] == [sum(xs[max(i - 1, 0):i + 1]) for i in range(8)]
    assert r[1]["s"] == 6 * 2**60
    # ... over three tiles, with NULLs and partitions, against exact Python sums
    rng = np.random.default_rng(3)
    big = rng.integers(-2**61, 2**61, SQL_N, dtype=np.int64).tolist()
    big = [None if i % 13 == 5 else v for i, v in enumerate(big)]
    g = (np.arange(SQL_N) // 1700).tolist()
    e.register_table("w", pa.table({"id": pa.array(range(SQL_N), pa.int64()), "g": pa.array(g, pa.int64()),
                                    "x": pa.array(big, pa.int64())}))
    r = e.sql("select id, sum(x) over (partition by g order by id rows between 2 preceding and 1 following) s "
              "from w order by id").table.to_pylist()
    for i in range(SQL_N):
        xs = [big[k] for k in range(max(i - 2, 0), min(i + 1, SQL_N - 1) + 1) if g[k] == g[i] and big[k] is not None]
        assert r[i]["s"] == (sum(xs) if xs else None), i
    # a sliding frame whose exact sum is outside int64 raises
    table("a2", [3 * 2**60] * 8)
    try:
        e.sql("select sum(x) over (order by id rows between 3 preceding and current row) s from a2").table
        raise AssertionError("a frame sum of 12 * 2**60 did not raise")
    except ExecutionError as ex:
        assert "overflow" in str(ex)
    # B: mixed signs: a thread's partial sum wraps, every running sum fits
    xs = [0] * 7 + [-(2**63 - 1)] + [2**60] * 8 + [1] * 24
    table("b", xs)
    r = e.sql("select id, sum(x) over (order by id) s from b order by id").table.to_pylist()
    assert [row["s"] for row in r] == [sum(xs[:i + 1]) for i in range(len(xs))]
    # a running sum that no output row reads may leave int64: the whole partition, and a peer group's end
    xs = [2**62, 2**62, 2**62, -2**63]
    table("d", xs)
    r = e.sql("select sum(x) over () s, sum(x) over (order by id / 4) p from d").table.to_pylist()
    assert [(row["s"], row["p"]) for row in r] == [(2**62, 2**62)] * 4
    # C: a real overflow raises
    table("c", [2**62] * 3)
    try:
        e.sql("select sum(x) over () s from c").table
        raise AssertionError("sum of three 2**62 did not raise")
    except ExecutionError as ex:
        assert "overflow" in str(ex)
