"""Case generators and checkers shared by tests/test_groupby_ref.py (torch CPU
paths) and tests/test_hash_tables_gpu.py / tests/test_agg_edges_gpu.py (gfx950
kernels): every checker runs ``igloo_amd.ops.hashing`` / ``ops.agg`` on
``device`` and compares with tests/groupby_ref.py (check_having_general: the
run-folding HAVING kernel, GPU only). A plain helper module; the
inputs are seeded, the references are cached per process so the files share
them. The hash function of the tables is deliberately not reproduced here:
the sentinel cases rely on numbers (twelve key sets) instead.
"""
import functools
import zlib

import numpy as np
import torch

import groupby_ref as R
from igloo_amd.ops import agg as A
from igloo_amd.ops import hashing as H
from igloo_amd.ops._lib import KERNEL_CALLS, native

I64_MIN, I64_MAX, I32_MIN, I32_MAX = R.I64_MIN, R.I64_MAX, R.I32_MIN, R.I32_MAX
PROBE_TILE = 8192       # rows per probe_hits / probe_write tile


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def is_gpu(device) -> bool:
    return torch.device(device).type == "cuda"


def dev_t(a, device):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device)


def _wide_keys(r, n, avoid=()):
    """n distinct int64 keys over the whole range (none of ``avoid``)."""
    out, seen = [], set(avoid)
    while len(out) < n:
        for k in r.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True).tolist():
            if k not in seen and len(out) < n:
                seen.add(k)
                out.append(k)
    return out


# ------------------------------------------------------------------ key sets
SENTINEL_SETS = 12
SENTINEL_ROWS = 4096    # a power of two: the hashed tables get 2 * 4096 slots


@functools.lru_cache(maxsize=None)
def sentinel_keys(seed: int, with_min: bool = True):
    """4096 int64 keys spread over the whole range: INT64_MAX, -1, 0 and, with
    ``with_min``, INT64_MIN on four rows (two early, one in the middle, the
    last row); every other key distinct. 4093 (4096 without INT64_MIN) distinct
    keys in the 8192 slots a hashed table of 4096 rows gets: load factor 0.5
    (to three digits; duplicates and an exact 0.5 exclude each other, the slot
    count following the row count)."""
    r = _rng("sentinel", seed)
    n = SENTINEL_ROWS
    special = [I64_MAX, -1, 0]
    keys = _wide_keys(r, n - len(special), avoid=special + [I64_MIN]) + special
    keys = [keys[i] for i in r.permutation(n).tolist()]
    if with_min:
        for pos in (1, 3, n // 2 + 3, n - 1):       # overwrite plain keys only
            while keys[pos] in special:
                pos -= 1
            keys[pos] = I64_MIN
    k = np.array(keys, dtype=np.int64)
    assert (k == I64_MIN).sum() == (4 if with_min else 0) and len(set(keys)) == n - (3 if with_min else 0)
    return k


def _mask(r, n, p, keep=None):
    m = r.random(n) < p
    if keep is not None:
        m |= keep
    return m


def _probe_of(r, build, m, extra):
    """m probe keys: about half drawn from the build keys, the rest fresh
    random keys of the build's dtype range, with ``extra`` spliced in at
    random rows."""
    dt = build.dtype
    lo, hi = (I64_MIN, I64_MAX) if dt == np.int64 else (I32_MIN, I32_MAX)
    p = r.integers(lo, hi, m, dtype=dt, endpoint=True)
    if len(build):
        take = r.random(m) < 0.5
        p[take] = build[r.integers(0, len(build), int(take.sum()))]
    pos = r.choice(m, size=min(len(extra), m), replace=False)
    p[pos] = np.array(extra[:len(pos)], dtype=dt)
    return p


class JoinCase:
    def __init__(self, name, build, bvalid, probes, mode):
        self.name, self.build, self.bvalid, self.probes, self.mode = name, build, bvalid, probes, mode

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def join_cases():
    """name -> JoinCase. ``probes``: [(probe keys, validity or None)];
    ``mode``: 'hashed', 'direct' or 'empty' (no non-NULL build key)."""
    cs = []
    for s in range(SENTINEL_SETS):
        r = _rng("join-sentinel", s)
        kb = sentinel_keys(s, True)
        # (odd sets: a build validity mask that keeps the special keys)
        bv = _mask(r, len(kb), 0.95, np.isin(kb, [I64_MIN, I64_MAX, -1, 0])) if s % 2 else None
        pa = _probe_of(r, kb, 5000, [I64_MIN] * 5 + [I64_MAX, -1, 0, I64_MIN + 1, I64_MAX - 1])
        cs.append(JoinCase(f"sentinel{s:02d}_with_min", kb, bv, [(pa, None if s % 3 else _mask(r, 5000, 0.9))], "hashed"))
        kn = sentinel_keys(s, False)
        # (4 * 4096 + 37 rows: the Bloom filter of the hashed table is consulted)
        pb = _probe_of(r, kn, 4 * SENTINEL_ROWS + 37, [I64_MIN] * 5 + [I64_MAX, -1, 0, I64_MIN + 1])
        cs.append(JoinCase(f"sentinel{s:02d}_without_min", kn, None, [(pb, None)], "hashed"))
    r = _rng("join-int32")
    k32 = np.concatenate([r.integers(I32_MIN, I32_MAX, 2990, dtype=np.int32, endpoint=True),
                          np.array([I32_MIN, I32_MAX, I32_MIN, I32_MAX, -1, 0, 0, 1, -2, I32_MIN], dtype=np.int32)])
    k32 = k32[r.permutation(len(k32))]
    p32 = _probe_of(r, k32, 7001, [I32_MIN, I32_MAX, -1, 0, I32_MIN + 1, I32_MAX - 1])
    cs.append(JoinCase("int32_hashed", k32, _mask(r, len(k32), 0.9), [(p32, None), (p32[:900], _mask(r, 900, 0.8))],
                       "hashed"))
    # mixed widths: an int32 build probed with int64 keys that agree in the low 32 bits only
    wide = k32.astype(np.int64)
    off = np.array([1, -1, 2, 3, -7], dtype=np.int64)[r.integers(0, 5, len(wide))] << 32
    mixed = np.concatenate([wide[:500], wide + off])
    cs.append(JoinCase("int32_hashed_int64_probe", k32, None, [(mixed, None)], "hashed"))
    d32 = r.integers(-300, 300, 2000).astype(np.int32)
    wd = d32.astype(np.int64)
    cs.append(JoinCase("int32_direct_int64_probe", d32, None,
                       [(np.concatenate([wd[:300], wd + (1 << 32), wd - (1 << 32), wd + (5 << 32)]), None)], "direct"))
    far = [I64_MIN, I64_MAX, 0, -1, 1, 2**62, -2**62, I64_MIN + 1, I64_MAX - 1]
    for name, lo, hi, near in (("direct_low_end", I64_MIN, I64_MIN + 1000, [I64_MIN + 1001, I64_MIN + 5000]),
                               ("direct_high_end", I64_MAX - 1000, I64_MAX, [I64_MAX - 1001, I64_MAX - 5000]),
                               ("direct_across_zero", -500, 500, [-501, 501, -2**40, 2**40])):
        r = _rng(name)
        kb = np.concatenate([r.integers(lo, hi, 1498, dtype=np.int64, endpoint=True), np.array([lo, hi], dtype=np.int64)])
        kb = kb[r.permutation(len(kb))]
        inside = r.integers(lo, hi, 400, dtype=np.int64, endpoint=True)
        small = np.concatenate([inside, np.array(far + near, dtype=np.int64)])
        # (4 * build rows + 13: the exact membership bitmap answers the probe)
        big = np.concatenate([small, r.integers(lo, hi, 4 * len(kb) + 13 - len(small), dtype=np.int64, endpoint=True)])
        big = big[r.permutation(len(big))]
        cs.append(JoinCase(name, kb, _mask(r, len(kb), 0.9, (kb == lo) | (kb == hi)),
                           [(small, None), (big, _mask(r, len(big), 0.9))], "direct"))
        u = np.arange(lo, lo + 900, dtype=np.int64)[r.permutation(900)]     # unique keys: head layout, no CSR runs
        cs.append(JoinCase(name + "_unique", u, None, [(small, None), (big, None)], "direct"))
    for name, direct in (("skew_hashed", False), ("skew_direct", True)):
        r = _rng(name)
        n = 20000
        rest = np.array(_wide_keys(r, n // 10, avoid=[77]), dtype=np.int64) if not direct else \
            (100 + r.permutation(50000)[: n // 10]).astype(np.int64)
        kb = np.concatenate([np.full(n - n // 10, 77, dtype=np.int64), rest])
        kb = kb[r.permutation(n)]
        # (the hot key on three probe rows only: each matches 18,000 build rows)
        pk = _probe_of(r, rest, 3000, [77, 77, 78, 76, 77])
        cs.append(JoinCase(name, kb, _mask(r, n, 0.97), [(pk, None)], "direct" if direct else "hashed"))
    r = _rng("join-degenerate")
    some = r.integers(-50, 50, 300).astype(np.int64)
    e64 = np.zeros(0, dtype=np.int64)
    cs.append(JoinCase("build_empty", e64, None, [(some, None), (e64, None)], "empty"))
    cs.append(JoinCase("build_all_null", some, np.zeros(len(some), dtype=bool), [(some, None)], "empty"))
    cs.append(JoinCase("build_single_row", np.array([I64_MAX], dtype=np.int64), None,
                       [(np.array([I64_MAX, I64_MIN, 0, I64_MAX], dtype=np.int64), None)], "direct"))
    wide = np.array(_wide_keys(r, 1000), dtype=np.int64)
    cs.append(JoinCase("probe_edges_hashed", wide, None,
                       [(e64, None), (wide[:50], np.zeros(50, dtype=bool)),
                        (_probe_of(r, wide, PROBE_TILE + 5, []), None),
                        (_probe_of(r, wide, 3 * PROBE_TILE - 1, []), _mask(r, 3 * PROBE_TILE - 1, 0.7))], "hashed"))
    dense = r.permutation(4000)[:1500].astype(np.int64)
    cs.append(JoinCase("probe_edges_direct", dense, None,
                       [(e64, None), (dense[:50], np.zeros(50, dtype=bool)),
                        (r.integers(-100, 4100, PROBE_TILE + 5).astype(np.int64), None),
                        (r.integers(-100, 4100, 3 * PROBE_TILE - 1).astype(np.int64),
                         _mask(r, 3 * PROBE_TILE - 1, 0.7))], "direct"))
    return {c.name: c for c in cs}


@functools.lru_cache(maxsize=None)
def _join_expect(name, pi):
    c = join_cases()[name]
    pk, pv = c.probes[pi]
    return R.join_ref(c.build.tolist(), None if c.bvalid is None else c.bvalid.tolist(), pk.tolist(),
                      None if pv is None else pv.tolist())


def check_csr(t, build, bvalid):
    """Every CSR run of a duplicate-key table holds exactly one key's rows."""
    cs = t.cstart.cpu().numpy().astype(np.int64)
    rows = t.crows.cpu().numpy().astype(np.int64)
    live = np.flatnonzero(np.ones(len(build), dtype=bool) if bvalid is None else bvalid)
    assert cs[0] == 0 and cs[-1] == len(live) and (np.diff(cs) >= 0).all()
    rows = rows[:len(live)]
    assert np.array_equal(np.sort(rows), live), "the runs do not hold every non-NULL build row once"
    lens = np.diff(cs)
    run = np.repeat(np.arange(len(lens)), lens)
    keys = build[rows]
    assert np.array_equal(keys, keys[cs[run]]), "a run mixes the rows of two keys"
    assert len(np.unique(keys)) == int((lens > 0).sum()), "a key's rows are split over two runs"


def check_join(name, device):
    c = join_cases()[name]
    gpu = is_gpu(device)
    nb = len(c.build)
    kb, bv = dev_t(c.build, device), dev_t(c.bvalid, device)
    t = H.JoinTable(kb, bv)
    assert t.empty == (c.mode == "empty")
    if not t.empty:
        assert t.direct == (c.mode == "direct"), f"{name}: the {'direct' if t.direct else 'hashed'} table ran"
    dup_ref = len(set(c.build[c.bvalid if c.bvalid is not None else slice(None)].tolist())) < \
        (nb if c.bvalid is None else int(c.bvalid.sum()))
    assert t.unique == (not dup_ref)
    if gpu and not t.empty:
        assert (t.cstart is not None) == dup_ref
        if dup_ref:
            check_csr(t, c.build, c.bvalid)
    for pi, (pk_np, pv_np) in enumerate(c.probes):
        counts, pairs, matched = _join_expect(name, pi)
        m = len(pk_np)
        pk, pv = dev_t(pk_np, device), dev_t(pv_np, device)
        where = f"{name} probe {pi}"
        # every pair, the counts, and the build-side marks
        bm = torch.zeros(nb, dtype=torch.bool, device=device)
        pidx, bidx, cnt = t.probe_pairs(pk, pv, build_matched=bm)
        assert cnt.cpu().tolist() == counts, where
        got = list(zip(pidx.cpu().tolist(), bidx.cpu().tolist()))
        assert len(got) == len(pairs) and set(got) == pairs, where
        assert pidx.cpu().tolist() == sorted(pidx.cpu().tolist()), where + ": pairs not grouped by probe row"
        assert set(np.flatnonzero(bm.cpu().numpy()).tolist()) == matched, where
        # one match per row (or -1), and its build-side marks
        bm1 = torch.zeros(nb, dtype=torch.bool, device=device)
        first = t.probe_first(pk, pv, build_matched=bm1).cpu().tolist()
        assert len(first) == m
        for j, f in enumerate(first):
            assert (f == -1) if counts[j] == 0 else ((j, f) in pairs), (where, j, f)
        if not dup_ref:
            assert set(np.flatnonzero(bm1.cpu().numpy()).tolist()) == matched, where
        assert t.probe_first(pk, pv).cpu().tolist() == first or dup_ref, where
        # hit rows / miss rows in row order
        hits = [j for j in range(m) if counts[j]]
        miss = [j for j in range(m) if not counts[j]]
        res = t.probe_select(pk, pv)
        if res is None:
            assert dup_ref, where      # only a duplicate build may leave the pairs to the multi-match probe
        else:
            sel, b = res
            assert sel.cpu().tolist() == hits, where
            assert all(p in pairs for p in zip(sel.cpu().tolist(), b.cpu().tolist())), where
        sel, b = t.probe_select(pk, pv, want_build=False)
        assert sel.cpu().tolist() == hits and b is None, where
        sel, b = t.probe_select(pk, pv, negate=True)
        assert sel.cpu().tolist() == miss and b is None, where


class GroupCase:
    def __init__(self, name, keys, mode):
        self.name, self.keys, self.mode = name, keys, mode


@functools.lru_cache(maxsize=None)
def group_cases():
    """name -> GroupCase; ``mode``: 'hashed' or 'direct' (the group table)."""
    j = join_cases()
    cs = [GroupCase(f"sentinel{s:02d}", sentinel_keys(s, True), "hashed") for s in range(SENTINEL_SETS)]
    cs.append(GroupCase("sentinel_without_min", sentinel_keys(0, False), "hashed"))
    cs.append(GroupCase("int32_hashed", j["int32_hashed"].build, "hashed"))
    for name in ("direct_low_end", "direct_high_end", "direct_across_zero", "skew_hashed", "skew_direct"):
        cs.append(GroupCase(name, j[name].build, j[name].mode))
    cs.append(GroupCase("single_row", np.array([I64_MIN], dtype=np.int64), "direct"))
    cs.append(GroupCase("int32_direct", j["int32_direct_int64_probe"].build, "direct"))
    return {c.name: c for c in cs}


@functools.lru_cache(maxsize=None)
def _group_expect(name):
    return R.group_ref(group_cases()[name].keys.tolist())


def check_partition(keys_np, gid, ng, rep, groups, first, where):
    """gid / ng / rep against group_ref: the same partition of the rows (up to
    the numbering of the groups) and each group's first row as ``rep``."""
    n = len(keys_np)
    gid, rep = gid.cpu().numpy().astype(np.int64), rep.cpu().numpy().astype(np.int64)
    assert ng == len(groups) and len(rep) == ng and len(gid) == n, where
    if n == 0:
        return
    assert gid.min() >= 0 and gid.max() < ng, where
    assert sorted(rep.tolist()) == sorted(first), where + ": rep is not the set of first rows"
    # rep[gid[i]] is the first row of row i's own group: equal partitions
    want = np.empty(n, dtype=np.int64)
    for g in groups:
        want[g] = g[0]
    assert np.array_equal(rep[gid], want), where


def check_group(name, device):
    c = group_cases()[name]
    groups, first = _group_expect(name)
    keys = dev_t(c.keys, device)
    n = len(c.keys)
    if is_gpu(device):
        assert H._group_table(keys, n)[1] == (c.mode == "direct"), f"{name}: the other group table ran"
    gid, ng, rep = H.group_ids(keys)
    check_partition(c.keys, gid, ng, rep, groups, first, name)
    gid2, ng2, rep2 = H.group_ids(dev_t(c.keys, device))
    assert ng2 == ng and torch.equal(gid2, gid) and torch.equal(rep2, rep), name + ": a second run differs"
    gx, ngx, repx, srt = H.group_ids_ex(dev_t(c.keys, device))
    assert not srt          # below SORTED_CHECK_ROWS: the table path
    check_partition(c.keys, gx, ngx, repx, groups, first, name + " (group_ids_ex)")
    mark = H.first_rows_mask(dev_t(c.keys, device))
    assert np.flatnonzero(mark.cpu().numpy()).tolist() == sorted(first), name


# ---------------------------------------------------------- sorted run path
SORTED_ROWS = 20011


@functools.lru_cache(maxsize=None)
def sorted_keys(dtype_name):
    """Non-decreasing keys from the type's least to its greatest value: runs
    of one row, mixed short runs and runs longer than a workgroup's rows."""
    dt = np.dtype(dtype_name)
    lo, hi = (I64_MIN, I64_MAX) if dt == np.int64 else (I32_MIN, I32_MAX)
    r = _rng("sorted", dtype_name)
    lens = [1] * 300 + [5000, 1, 1, 2100] + r.integers(1, 9, 2000).tolist() + [1] * 50 + [700, 3]
    out, total = [], 0
    for ln in lens:
        ln = min(ln, SORTED_ROWS - total)
        if ln <= 0:
            break
        out.append(ln)
        total += ln
    out[-1] += SORTED_ROWS - total
    step = (hi - lo) // (len(out) - 1)
    vals = [lo + i * step for i in range(len(out) - 1)] + [hi]
    return np.repeat(np.array(vals, dtype=dt), out)


def check_sorted_runs(dtype_name, device, monkeypatch):
    monkeypatch.setattr(H, "SORTED_CHECK_ROWS", 16384)
    k = sorted_keys(dtype_name)
    assert k[0] == np.iinfo(k.dtype).min and k[-1] == np.iinfo(k.dtype).max and len(k) == SORTED_ROWS
    groups, first = R.group_ref(k.tolist())
    before = KERNEL_CALLS["run_bounds"]
    gid, ng, rep, srt = H.group_ids_ex(dev_t(k, device))
    check_partition(k, gid, ng, rep, groups, first, dtype_name)
    if is_gpu(device):
        assert srt and KERNEL_CALLS["run_bounds"] > before, "the sorted run path did not run"
        assert gid.cpu().tolist() == sorted(gid.cpu().tolist()) and rep.cpu().tolist() == first
    rev = np.ascontiguousarray(k[::-1])
    groups, first = R.group_ref(rev.tolist())
    gid, ng, rep, srt = H.group_ids_ex(dev_t(rev, device))
    assert not srt, "reversed keys reported as sorted"
    check_partition(rev, gid, ng, rep, groups, first, dtype_name + " reversed")


# ---------------------------------------------------------------- aggregates
AGG_ROWS = 20011        # several workgroups, no multiple of the 512-row wave tile
PART_ROWS, PART_GROUPS, PART_MIN_ROWS = 40009, 9001, 32768
NAN_POS = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
NAN_NEG = np.array([0xfff8000000000000], dtype=np.uint64).view(np.float64)[0]
DBL_MAX, DENORM = np.finfo(np.float64).max, 5e-324
#: (operator, value column) of every launch: 16 aggregates = two launches of eight
AGG_SPECS = [("sum_int", "i64"), ("min_int", "i64"), ("max_int", "i64"), ("and_int", "i64"), ("or_int", "i64"),
             ("xor_int", "i64"), ("count", None), ("sum_f64", "fsum"),
             ("sum_int", "i32"), ("min_int", "i32"), ("max_int", "i32"), ("and_int", "i32"), ("or_int", "i32"),
             ("xor_int", "i32"), ("min_f64", "fmm"), ("max_f64", "fmm")]
#: launches of a single aggregate: every operator once, the int32 source for the bit operations
SINGLE_SPECS = [0, 1, 2, 6, 7, 8, 11, 12, 13, 14, 15]
REGIMES = ["single_nogid", "single_one_group", "lds_3", "lds_max", "sorted", "global", "global_just_above",
           "partitioned"]


def agg_groups(regime: str, nagg: int) -> int:
    lim = native().agg_lds_max_groups(nagg)
    return {"single_nogid": 1, "single_one_group": 1, "lds_3": 3, "lds_max": lim, "sorted": 2 * lim + 17,
            "global": 2 * lim + 17, "global_just_above": lim + 1, "partitioned": PART_GROUPS}[regime]


def expected_regime(has_gid: bool, ngroups: int, nagg: int, sorted_gids: bool, n: int) -> str:
    """The regime ``grouped_aggregate`` takes, from its thresholds and arguments."""
    lim = native().agg_lds_max_groups(nagg)
    if has_gid and not sorted_gids and A._partitioned_ok(n, ngroups, nagg):
        return "partitioned"
    if not has_gid or ngroups <= 1:
        return "single"
    if ngroups <= lim:
        return "lds"
    return "sorted" if sorted_gids else "global"


_I64_POOL = [I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1, 2**62, -2**62, 0x5555555555555555, -0x5555555555555556]
_I32_POOL = [I32_MIN, I32_MAX, -1, 0, 1, I32_MIN + 1, I32_MAX - 1, -2, -0x55555556, 0x55555555, -65536]
_FMM_POOL = [np.inf, -np.inf, 0.0, -0.0, DENORM, -DENORM, 2.0 * DENORM, DBL_MAX, -DBL_MAX, NAN_POS, NAN_NEG, 1.5, -2.25]
_FSUM_POOL = [0.0, -0.0, DENORM, -DENORM, 3.0 * DENORM, 1e300, -1e300, 1e-300, 0.1, -0.3]
#: per-group rows of the sets with eight groups or more: (i64, i32, f64 for MIN/MAX, f64 for SUM)
_ROLES = [
    # sums crossing 2^63 and 2^64 upwards; a group that is all NaN, of both signs
    ([I64_MAX] * 5, [I32_MAX] * 5, [NAN_POS, NAN_NEG, NAN_NEG, NAN_POS, NAN_NEG], [DBL_MAX, 1.0, -0.0, DENORM, -1.0]),
    # ... and downwards; one sign-bit NaN among finite values
    ([I64_MIN] * 5, [I32_MIN] * 5, [3.5, NAN_NEG, -7.25, 0.0, 2.0], [-DBL_MAX, DENORM, -DENORM, 0.0, 1.0]),
    # a sum that crosses both ways and cancels to 7; +inf and -inf in one SUM group
    ([I64_MAX] * 3 + [-I64_MAX] * 3 + [7], [-1, -2, -4, -8, 0x7fff0000, -0x10000, 3],
     [np.inf, -np.inf, 1.0, -1.0, 0.0, 2.0, 3.0], [np.inf, -np.inf, 1.0, 2.0, 3.0, 4.0, 5.0]),
    # MIN equal to the MIN state's identity, MAX equal to the MAX state's
    ([I64_MAX] * 3, [I32_MAX] * 3, [np.inf, np.inf, np.inf], [np.inf, 1.0, -2.0]),
    ([I64_MIN] * 3, [I32_MIN] * 3, [-np.inf, -np.inf, -np.inf], [-np.inf, 1.0, -2.0]),
    # one clear-sign NaN among finite values; signed zeros and denormals only
    ([1, -1, 0], [-1, -1, -1], [NAN_POS, -1.0, 1.0], [NAN_NEG, 1.0, 2.0]),
    ([-1, -1, -1], [I32_MIN, -1, 1], [-0.0, 0.0, -DENORM], [-0.0, -0.0, -0.0]),
    ([I64_MIN, I64_MAX, 1], [I32_MIN, I32_MAX, 1], [DBL_MAX, -DBL_MAX, DENORM], [DENORM, DENORM, -3.0 * DENORM]),
]


class AggCase:
    pass


@functools.lru_cache(maxsize=None)
def agg_case(regime: str, nagg: int, masked: bool):
    """Inputs of one regime at one launch width. Sets with eight groups or
    more: groups 0..7 hold the rows of _ROLES alone, group G-1 has no row,
    group G-2 only NULL rows (with a mask), the others draw from the pools;
    rows with the ids -1 and G+5 belong to no group. Smaller sets: group 0
    takes every value (G=3: group 1 is all NULL under a mask, group 2 empty)."""
    r = _rng("agg", regime, nagg, masked)
    c = AggCase()
    c.regime, c.nagg, c.masked = regime, nagg, masked
    G = c.ngroups = agg_groups(regime, nagg)
    n = c.n = PART_ROWS if regime == "partitioned" else AGG_ROWS
    c.sorted = regime == "sorted"

    def draw(pool, dt, rand):
        v = rand.astype(dt)
        sp = r.random(n) < 0.4
        v[sp] = np.array(pool, dtype=dt)[r.integers(0, len(pool), int(sp.sum()))]
        return v
    i64 = draw(_I64_POOL, np.int64, r.integers(-2**40, 2**40, n))
    i32 = draw(_I32_POOL, np.int32, r.integers(-10**6, 10**6, n))
    fsum = draw(_FSUM_POOL, np.float64, r.standard_normal(n) * 1e3)
    valid = _mask(r, n, 0.8) if masked else None
    if G >= 8:
        fmm = draw(_FMM_POOL[:9], np.float64, r.standard_normal(n) * 1e3)     # NaN only where the roles put it
        gid = r.integers(8, G - 1, n).astype(np.int32)                        # G-1 stays empty
        row = 0
        for g, (a, b, x, y) in enumerate(_ROLES):
            k = len(a)
            gid[row:row + k] = g
            i64[row:row + k], i32[row:row + k], fmm[row:row + k], fsum[row:row + k] = a, b, x, y
            if valid is not None:
                valid[row:row + k] = True
            row += k
        gid[row:row + 4] = G - 2
        if valid is not None:
            valid[gid == G - 2] = False
        row += 4
        skip = row + r.choice(n - row, 40, replace=False)
        gid[skip[:20]], gid[skip[20:]] = -1, G + 5
        perm = r.permutation(n)
        gid, i64, i32, fmm, fsum = gid[perm], i64[perm], i32[perm], fmm[perm], fsum[perm]
        valid = valid[perm] if valid is not None else None
    else:
        fmm = draw(_FMM_POOL, np.float64, r.standard_normal(n) * 1e3)
        gid = np.zeros(n, dtype=np.int32)
        if G == 3:
            one = r.random(n) < 0.2
            gid[one] = 1
            if valid is not None:
                valid[one] = False
        skip = r.choice(n, 40, replace=False)
        gid[skip[:20]], gid[skip[20:]] = -1, G + 5
        if regime == "single_nogid":
            gid = None
    if c.sorted:
        order = np.argsort(gid, kind="stable")
        gid, i64, i32, fmm, fsum = gid[order], i64[order], i32[order], fmm[order], fsum[order]
        valid = valid[order] if valid is not None else None
    c.gid, c.valid = gid, valid
    c.cols = {"i64": i64, "i32": i32, "fmm": fmm, "fsum": fsum}
    return c


@functools.lru_cache(maxsize=None)
def _agg_expect(regime, nagg, masked, si):
    c = agg_case(regime, nagg, masked)
    op, col = AGG_SPECS[si]
    return R.agg_ref(None if c.gid is None else c.gid.tolist(), c.ngroups, op,
                     None if col is None else c.cols[col].tolist(),
                     None if c.valid is None else c.valid.tolist(), n=c.n)


def compare_agg(op, got, want, where):
    """One aggregate's result tensor against agg_ref's states, group by group."""
    if op == "sum_f64":
        ref, absum, terms = want
        got = got.cpu().tolist()
        assert len(got) == len(ref), where
        for g, (x, e, a, t) in enumerate(zip(got, ref, absum, terms)):
            if e != e or abs(e) == float("inf"):
                assert R.same_f64(x, e), (where, g, x, e)
            else:
                assert abs(x - e) <= R.sum_bound(a, t), (where, g, x, e, R.sum_bound(a, t))
    elif op in ("min_f64", "max_f64"):
        got = got.cpu().tolist()
        assert len(got) == len(want), where
        for g, (x, e) in enumerate(zip(got, want)):
            assert R.same_f64(x, e), (where, g, x, e)
    else:
        got = A.wide_to_python(got)
        assert got == want, (where, [(g, x, e) for g, (x, e) in enumerate(zip(got, want)) if x != e][:5])


def check_agg(regime, nagg, masked, device, monkeypatch):
    """Every operator through one regime: launches of eight aggregates
    (``nagg`` 8) or of a single one (``nagg`` 1)."""
    c = agg_case(regime, nagg, masked)
    gpu = is_gpu(device)
    if regime == "partitioned":
        monkeypatch.setattr(A, "AGG_PART_MIN_ROWS", PART_MIN_ROWS)
    gid = dev_t(c.gid, device)
    valid = dev_t(c.valid, device)
    cols = {k: dev_t(v, device) for k, v in c.cols.items()}
    if gpu:
        assert expected_regime(gid is not None, c.ngroups, nagg, c.sorted, c.n) == regime.split("_")[0], \
            f"{regime}: the thresholds now send this case elsewhere"
    todo = [list(range(len(AGG_SPECS)))] if nagg == 8 else [[si] for si in SINGLE_SPECS]
    for chunk in todo:
        specs = [(AGG_SPECS[si][0], None if AGG_SPECS[si][1] is None else cols[AGG_SPECS[si][1]], valid) for si in chunk]
        before = KERNEL_CALLS["agg_partitioned"], KERNEL_CALLS["agg_update"]
        outs = A.grouped_aggregate(gid, c.ngroups, specs, c.n, device, sorted_gids=c.sorted)
        if gpu:
            ran = KERNEL_CALLS["agg_partitioned"] - before[0], KERNEL_CALLS["agg_update"] - before[1]
            launches = -(-len(chunk) // 8)
            assert ran == ((launches, 0) if regime == "partitioned" else (0, launches)), (regime, ran)
        for si, out in zip(chunk, outs):
            op = AGG_SPECS[si][0]
            compare_agg(op, out, _agg_expect(regime, nagg, masked, si),
                        f"{regime} nagg={nagg} masked={masked} {op}({AGG_SPECS[si][1]})")


# ------------------------------------------------- run-folding HAVING kernel
HAVING_MAX_RUN = 256    # kHavingMaxRun of csrc/kernels/agg.hip: longer runs send the caller to the general path


@functools.lru_cache(maxsize=None)
def _having_runs(masked):
    """(run start rows, run index per row) of the sorted regime's group ids
    taken as keys: -1 and G+5 are ordinary keys here."""
    k = agg_case("sorted", 8, masked).gid
    first = np.r_[True, k[1:] != k[:-1]]
    return np.flatnonzero(first), np.cumsum(first) - 1


@functools.lru_cache(maxsize=None)
def _having_expect(masked, si):
    c = agg_case("sorted", 8, masked)
    starts, run = _having_runs(masked)
    op, col = AGG_SPECS[si]
    return R.agg_ref(run.tolist(), len(starts), op, None if col is None else c.cols[col].tolist(),
                     None if c.valid is None else c.valid.tolist(), n=c.n)


def check_having_general(masked, device, monkeypatch):
    """Every operator through the run-folding sorted_having_kernel
    (IGLOO_DEBUG=having_general), three aggregates plus the COUNT(*) that
    HAVING compares (>= 1: every run passes) per launch, against agg_ref over
    the run index as group id."""
    monkeypatch.setenv("IGLOO_DEBUG", "having_general")     # (C++ reads it per call)
    c = agg_case("sorted", 8, masked)
    assert c.n == AGG_ROWS and (np.diff(c.gid) >= 0).all()
    starts, _run = _having_runs(masked)
    lens = np.diff(np.r_[starts, c.n])
    # the kernel's limits, from the data: else it reports overflow and returns None
    assert lens.max() < HAVING_MAX_RUN and len(starts) <= c.n // 64 + 4096
    keys = dev_t(c.gid, device)
    valid = dev_t(c.valid, device)
    cols = {k: dev_t(v, device) for k, v in c.cols.items()}
    for i in range(0, len(AGG_SPECS), 3):
        chunk = list(range(i, min(i + 3, len(AGG_SPECS))))
        specs = [(AGG_SPECS[si][0], None if AGG_SPECS[si][1] is None else cols[AGG_SPECS[si][1]], valid) for si in chunk]
        specs.append(("count", None, None))
        before = KERNEL_CALLS["sorted_having"]
        got = A.sorted_having(keys, specs, len(specs) - 1, ">=", 1)
        assert got is not None, "a run past the kernel's limits"
        assert KERNEL_CALLS["sorted_having"] > before
        rep, outs = got
        assert np.array_equal(rep.cpu().numpy(), starts) and np.array_equal(outs[-1].cpu().numpy(), lens)
        for si, out in zip(chunk, outs):
            op = AGG_SPECS[si][0]
            compare_agg(op, out, _having_expect(masked, si), f"having_general masked={masked} {op}({AGG_SPECS[si][1]})")
