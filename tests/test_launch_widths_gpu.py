"""Both values of every width / mode flag that the kernel launchers turn into
template arguments (csrc/kernels/launch.h): int64 row ids, 64-bit index
outputs and permutations, int32 and int64 keys, at the smallest sizes where a
launcher that casts a buffer at the wrong width gives a wrong answer. The wide
variants otherwise run only from 2^31 rows. References: the CPU paths of the
same operators, torch / numpy, or the narrow variant on the same input."""
import numpy as np
import pytest
import torch

from igloo_amd import types as T
from igloo_amd.columnar import Column
from igloo_amd.ops import agg as A
from igloo_amd.ops import hashing as H
from igloo_amd.ops import misc as M
from igloo_amd.ops import pack as PK
from igloo_amd.ops import sort as SO
from igloo_amd.ops._lib import native, ptr, stream
from igloo_amd.ops.gather import take_many
from igloo_amd.ops.select import exclusive_scan, mask_to_indices

pytestmark = pytest.mark.gpu

SIZES = [1, 257, 5000]
INTS = [torch.int32, torch.int64]
NB, NP = 1000, 8195      # build rows; probe rows: one 8192-row hit tile and a ragged tail


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ join tables
def _join_keys(key_dt, dense, dups, seed):
    """Build keys (about 5% NULL) and probe keys (half of them build keys)."""
    r = np.random.default_rng(seed)
    if dense:
        lo, hi = 100, 100 + NB
        bk = r.choice(np.arange(lo, hi), NB, replace=dups)
        plo, phi = lo - 50, hi + 50
    else:
        lo, hi = (-2**31, 2**31 - 1) if key_dt == torch.int32 else (-10**15, 10**15)
        u = np.unique(np.concatenate([[lo, hi - 1], r.integers(lo, hi, 2 * NB)]))
        bk = np.concatenate([[lo, hi - 1], r.permutation(u[1:-1])[:NB - 2]])     # the span's two ends are keys
        if dups:
            bk[2::3] = bk[3::3]
        bk = r.permutation(bk)
        plo, phi = lo, hi
    bvalid = r.random(NB) >= 0.05
    pk = np.where(r.random(NP) < 0.5, bk[r.integers(0, NB, NP)], r.integers(plo, phi, NP))
    return torch.from_numpy(bk).to(key_dt), torch.from_numpy(bvalid), torch.from_numpy(pk).to(key_dt)


def _probe_write_native(t, pk, out_dt):
    """probe_hits + probe_write as JoinTable.probe_select runs them, with the
    probe-index output of the given width."""
    N = native()
    m, dev, st = pk.numel(), pk.device, stream(pk)
    tiles = N.probe_hit_tiles(m)
    words = torch.empty(tiles * 128, dtype=torch.int64, device=dev)
    tcount = torch.empty(tiles, dtype=torch.int64, device=dev)
    col = N.KeyColumn(ptr(pk), pk.dtype == torch.int64, 0, m)
    N.probe_hits(t._ref, col, t._use_filter(m), False, ptr(words), ptr(tcount), st)
    toff, total = exclusive_scan(tcount)
    pidx = torch.full((total,), -7, dtype=out_dt, device=dev)
    bidx = torch.full((total,), -7, dtype=t.rid, device=dev)
    N.probe_write(t._ref, col, ptr(words), ptr(toff), ptr(pidx), out_dt == torch.int64, ptr(bidx), total, st)
    _sync()
    return pidx, bidx


@pytest.mark.parametrize("rid64", [False, True])
@pytest.mark.parametrize("dups", [False, True])
@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("key_dt", INTS)
def test_join_table_key_and_row_id_widths(gpu_device, monkeypatch, key_dt, dense, dups, rid64):
    """join_build, join_csr_count / join_csr_scatter, join_probe (counts,
    first match, build marks), join_expand, probe_hits and probe_write over
    key width x direct / hashed x unique / duplicate keys x row-id width,
    against the CPU JoinTable. Wide row ids come from the constructor seeing a
    row limit of 0; the probes run with the real one."""
    bk, bvalid, pk = _join_keys(key_dt, dense, dups, seed=17)
    cpu = H.JoinTable(bk, bvalid)
    with monkeypatch.context() as mp:
        if rid64:
            mp.setattr(H, "INT32_MAX", 0)
        gpu = H.JoinTable(bk.to(gpu_device), bvalid.to(gpu_device))
    rid = torch.int64 if rid64 else torch.int32
    assert gpu.thead.dtype == rid and gpu.rid64 == rid64
    assert gpu.direct == dense and cpu.unique == gpu.unique == (not dups)
    assert (gpu.cstart is not None) == dups
    if dups:
        assert gpu.cstart.dtype == rid and gpu.crows.dtype == rid
        assert int(gpu.cstart[-1]) == int(bvalid.sum())
    pkd = pk.to(gpu_device)
    # all pairs, counts and build-side marks
    mc = torch.zeros(NB, dtype=torch.bool)
    mg = torch.zeros(NB, dtype=torch.bool, device=gpu_device)
    rp, rb, rc = cpu.probe_pairs(pk, build_matched=mc)
    gp, gb, gc = gpu.probe_pairs(pkd, build_matched=mg)
    assert gb.dtype == rid
    assert torch.equal(rc, gc.cpu())
    assert sorted(zip(rp.tolist(), rb.tolist())) == sorted(zip(gp.cpu().tolist(), gb.cpu().tolist()))
    assert torch.equal(mc, mg.cpu())
    # first match
    fm = gpu.probe_first(pkd).cpu()
    assert fm.dtype == rid
    assert torch.equal(fm >= 0, rc > 0)
    ok = fm >= 0
    assert torch.equal(bk[fm[ok].long()], pk[ok]) and bool(bvalid[fm[ok].long()].all())
    # hit selection: scalar kernel, then the planned one (the bitmap kernel on a direct table)
    N = native()
    for mode, kern in ((0, "hits"), (2, "bits" if dense else "hits")):
        N.set_probe_bits(mode)
        try:
            for negate in (False, True):
                want_build = not negate and not dups
                p, b = gpu.probe_select(pkd, None, negate=negate, want_build=want_build)
                assert N.last_probe_kernel() == kern
                want = mask_to_indices(rc == 0 if negate else rc > 0)
                assert torch.equal(p.cpu().long(), want.long())
                if want_build:
                    assert b.dtype == rid
                    assert torch.equal(bk[b.cpu().long()], pk[want.long()])
                else:
                    assert b is None
        finally:
            N.set_probe_bits(2)
    # probe_write with 32- and 64-bit probe-index outputs
    p32, b32 = _probe_write_native(gpu, pkd, torch.int32)
    p64, b64 = _probe_write_native(gpu, pkd, torch.int64)
    hits = mask_to_indices(rc > 0).long()
    assert torch.equal(p32.cpu().long(), hits) and torch.equal(p64.cpu(), hits)
    assert torch.equal(b32, b64) and torch.equal(bk[b64.cpu().long()], pk[hits])


@pytest.mark.parametrize("use_filter", [True, False])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("key_dt", INTS)
def test_probe_first_direct_ragged_tails(gpu_device, monkeypatch, key_dt, masked, use_filter):
    """JoinTable.probe_first on a direct unique table (the 4-rows-per-lane
    first-match kernel, which batches its loads through probe_heads) against
    the CPU JoinTable: row counts around the 4-row batch and the 256-lane
    workgroup, with and without a validity mask, with the exact bitmap
    consulted (ratio 0: at every row count; the last count also under the real
    ratio) and not consulted (a ratio no probe reaches)."""
    r = np.random.default_rng(23)
    lo = 10**12 if key_dt == torch.int64 else -300
    bk = torch.from_numpy(r.choice(np.arange(lo, lo + 1100), NB, replace=False)).to(key_dt)
    cpu = H.JoinTable(bk)
    gpu = H.JoinTable(bk.to(gpu_device))
    assert gpu.direct and gpu.unique and gpu.cstart is None and gpu.bmask >> 63
    real = H.BLOOM_MIN_RATIO * NB + 1       # a probe the unpatched rule filters
    for m in (1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 2 + 1, real):
        pk = torch.from_numpy(r.integers(lo - 50, lo + 1150, m)).to(key_dt)
        pv = torch.from_numpy(r.random(m) < 0.7) if masked else None
        want = cpu.probe_first(pk, pv)
        with monkeypatch.context() as mp:
            if not use_filter:
                mp.setattr(H, "BLOOM_MIN_RATIO", 2**40)
            elif m != real:
                mp.setattr(H, "BLOOM_MIN_RATIO", 0)
            assert gpu._use_filter(m) == use_filter
            got = gpu.probe_first(pk.to(gpu_device), None if pv is None else pv.to(gpu_device))
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), m


# ------------------------------------------------------------------ sorted ranges
def _range_case(dtype, jump, seed=5):
    g = torch.Generator().manual_seed(seed)
    keys = torch.sort(torch.randint(0, 600, (NB,), generator=g)).values * 2 + 7
    keys[NB // 2:] += jump                       # a key hole past kGapFill: the dense index's long-gap path
    q = torch.randint(-5, 1220 + jump, (3000,), generator=g)
    qvalid = torch.rand(3000, generator=g) > 0.1
    return keys.to(dtype), q.to(dtype), qvalid


def _ranges_ref(big, q, qvalid):
    lo = torch.searchsorted(big, q)
    cnt = torch.searchsorted(big, q, right=True) - lo
    return lo, torch.where(qvalid, cnt, torch.zeros_like(cnt))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("dtype", INTS)
def test_range_launchers_output_widths(gpu_device, monkeypatch, dtype, wide):
    """sorted_ranges + expand_ranges, sorted_match, sorted_masked and
    sorted_exists with 32- and 64-bit pair outputs (out64), against
    torch.searchsorted and the operators' CPU paths."""
    monkeypatch.setattr(H, "DENSE_INDEX", False)
    if wide:
        monkeypatch.setattr(H, "INT32_MAX", 0)
    it = torch.int64 if wide else torch.int32
    big, q, qvalid = _range_case(dtype, 0)
    lo_ref, cnt_ref = _ranges_ref(big, q, qvalid)
    lo, cnt = H.sorted_ranges(big.to(gpu_device), q.to(gpu_device), qvalid.to(gpu_device))
    assert torch.equal(cnt.cpu(), cnt_ref)
    assert torch.equal(lo.cpu()[cnt_ref > 0], lo_ref[cnt_ref > 0])
    s, b = H.expand_ranges(lo, cnt, NB)
    assert s.dtype == it and b.dtype == it
    s_ref = torch.repeat_interleave(torch.arange(q.numel()), cnt_ref)
    within = torch.arange(s_ref.numel()) - (torch.cumsum(cnt_ref, 0) - cnt_ref)[s_ref]
    assert torch.equal(s.cpu().long(), s_ref) and torch.equal(b.cpu().long(), lo_ref[s_ref] + within)
    g = torch.Generator().manual_seed(2)
    big2 = torch.randint(0, 3, (NB,), generator=g).to(dtype)
    small2 = torch.randint(0, 3, (q.numel(),), generator=g).to(dtype)
    sm, bm = H.sorted_match_pairs(big.to(gpu_device), big2.to(gpu_device), q.to(gpu_device), small2.to(gpu_device))
    sm_ref, bm_ref = H.sorted_match_pairs(big, big2, q, small2)
    assert sm.dtype == it and bm.dtype == it and sm_ref.numel() > 0
    assert torch.equal(sm.cpu().long(), sm_ref.long()) and torch.equal(bm.cpu().long(), bm_ref.long())
    mask = torch.rand(NB, generator=g) > 0.4
    se, be = H.masked_expand(lo, cnt, mask.to(gpu_device), NB)
    se_ref, be_ref = H.masked_expand(lo_ref, cnt_ref, mask, NB)
    assert se.dtype == it and be.dtype == it
    assert torch.equal(se.cpu().long(), se_ref.long()) and torch.equal(be.cpu().long(), be_ref.long())
    for op in ("<>", "<"):
        hit = H.sorted_exists(big2.to(gpu_device), small2.to(gpu_device), lo, cnt, op)
        assert torch.equal(hit.cpu(), H.sorted_exists(big2, small2, lo_ref, cnt_ref, op))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("jump", [0, 200])
@pytest.mark.parametrize("dtype", INTS)
def test_dense_index_entry_widths(gpu_device, monkeypatch, dtype, jump, wide):
    """dense_index_build (fill, long-gap fix-up), dense_ranges and
    unique_lookup (through the index and by search) with int32 and int64 table
    entries (first64) under int32 and int64 keys, against torch.searchsorted."""
    monkeypatch.setattr(H, "DENSE_INDEX_MIN_QUERIES", 0)
    if wide:
        monkeypatch.setattr(H, "INT32_MAX", 0)
    it = torch.int64 if wide else torch.int32
    big, q, qvalid = _range_case(dtype, jump)
    lo_ref, cnt_ref = _ranges_ref(big, q, qvalid)
    bd = big.to(gpu_device)
    lo, cnt = H.sorted_ranges(bd, q.to(gpu_device), qvalid.to(gpu_device))
    idx = H.dense_index(bd, build=False)
    assert idx is not None and idx[2].dtype == it
    assert torch.equal(cnt.cpu(), cnt_ref)
    assert torch.equal(lo.cpu()[cnt_ref > 0], lo_ref[cnt_ref > 0])
    # distinct keys: one position per probe key
    uq = torch.unique(big)
    pos_ref = torch.searchsorted(uq, q)
    hit_ref = (pos_ref < uq.numel()) & (uq[pos_ref.clamp(max=uq.numel() - 1)] == q) & qvalid
    for dense in (True, False):
        monkeypatch.setattr(H, "DENSE_INDEX", dense)
        ud = uq.to(gpu_device)
        hit, pos = H.unique_lookup(ud, q.to(gpu_device), qvalid.to(gpu_device))
        if dense:
            assert H.dense_index(ud, build=False)[2].dtype == it
        assert torch.equal(hit.cpu(), hit_ref)
        assert torch.equal(pos.cpu().long(), torch.where(hit_ref, pos_ref, torch.zeros_like(pos_ref)))


# ------------------------------------------------------------------ group ids, histograms, HAVING
@pytest.mark.parametrize("span", [40, 20000, 10**9])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", INTS)
def test_group_ids_key_widths(gpu_device, dtype, n, span):
    """groupby_build (LDS direct table / direct / hashed), groupby_lookup and
    key_histogram under int32 and int64 keys, against the CPU paths."""
    k = torch.from_numpy(np.random.default_rng(n).integers(-span, span, n)).to(dtype)
    gid, ng, rep = H.group_ids(k.to(gpu_device))
    uniq, inv = torch.unique(k, return_inverse=True)
    assert ng == uniq.numel()
    assert torch.equal(k[rep.cpu().long()][gid.cpu().long()], k)
    first = torch.full((ng,), n, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(n), reduce="amin")
    assert torch.equal(torch.sort(rep.cpu().long()).values, torch.sort(first).values)
    if span == 40:
        valid = torch.from_numpy(np.random.default_rng(1).random(n) > 0.3)
        got = A.key_histogram(k.to(gpu_device), -30, 55, valid.to(gpu_device))
        assert torch.equal(got.cpu(), A.key_histogram(k, -30, 55, valid))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_fill_runs_and_groupby_assign_index_widths(gpu_device, n, wide):
    """fill_runs (starts64) and groupby_assign (slots64) read their int32 or
    int64 index input at its own width."""
    N = native()
    it = torch.int64 if wide else torch.int32
    r = np.random.default_rng(n)
    bound = r.random(n) < 0.2
    bound[0] = True
    starts = torch.from_numpy(np.flatnonzero(bound)).to(it).to(gpu_device)
    gid = torch.full((n,), -1, dtype=torch.int32, device=gpu_device)
    N.fill_runs(ptr(starts), wide, starts.numel(), n, ptr(gid), stream(gid))
    assert np.array_equal(gid.cpu().numpy(), np.cumsum(bound) - 1)
    # occupied slots of a direct group table -> group id per slot, first row per group
    cap = 2 * n + 3
    occ = r.random(cap) < 0.4
    occ[cap - 1] = True
    slots = np.flatnonzero(occ)
    trow = np.full(cap, 2**31 - 1, dtype=np.int32)
    trow[slots] = r.integers(0, n, slots.size)
    td = torch.from_numpy(trow).to(gpu_device)
    sd = torch.from_numpy(slots).to(it).to(gpu_device)
    gid_of_slot = torch.full((cap,), -1, dtype=torch.int32, device=gpu_device)
    rep = torch.full((slots.size,), -1, dtype=torch.int32, device=gpu_device)
    N.groupby_assign(ptr(sd), wide, slots.size, cap, ptr(td), ptr(gid_of_slot), ptr(rep), stream(td))
    assert np.array_equal(rep.cpu().numpy(), trow[slots])
    assert np.array_equal(gid_of_slot.cpu().numpy()[slots], np.arange(slots.size))


@pytest.mark.parametrize("k64", [False, True])
def test_sorted_having_general_kernel_key_widths(gpu_device, monkeypatch, k64):
    """sorted_having_kernel (the run-folding kernel behind the having_general
    switch) under int32 and int64 keys, short runs, against numpy."""
    monkeypatch.setenv("IGLOO_DEBUG", "having_general")     # (C++ reads it per call)
    r = np.random.default_rng(4)
    runs = r.integers(1, 9, 1200)
    k = np.repeat(np.arange(runs.size, dtype=np.int64) * 3 - 500, runs)
    q = r.integers(-20, 60, k.size).astype(np.int32)
    keys = torch.from_numpy(k if k64 else k.astype(np.int32)).to(gpu_device)
    specs = [("count", None, None), ("sum_int", torch.from_numpy(q).to(gpu_device), None)]
    got = A.sorted_having(keys, specs, 1, ">", 100)
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    sums = np.add.reduceat(q.astype(np.int64), starts)
    sel = sums > 100
    assert got is not None and sel.any()
    rep, outs = got
    assert np.array_equal(rep.cpu().numpy(), starts[sel])
    assert np.array_equal(outs[0].cpu().numpy(), np.diff(np.r_[starts, k.size])[sel])
    assert np.array_equal(outs[1].cpu().numpy(), sums[sel])


# ------------------------------------------------------------------ gather, select, pack, partition
@pytest.mark.parametrize("n", SIZES)
def test_gather_index_widths(gpu_device, n):
    """gather_multi, str_gather_lengths / str_gather_copy and str_eq_rows with
    int32 and int64 row indices (idx64): equal outputs, and equal to the CPU path."""
    import pyarrow as pa
    r = np.random.default_rng(n)
    rows = 700
    cols = [Column(T.INT64, torch.from_numpy(r.integers(-10**12, 10**12, rows))),
            Column.from_arrow(pa.array(["s" * (i % 13) + str(i) for i in range(rows)], pa.large_string()),
                              dict_encode=False),
            Column(T.DATE32, torch.from_numpy(r.integers(0, 20000, rows).astype(np.int32)),
                   torch.from_numpy(r.random(rows) < 0.9))]
    idx = torch.from_numpy(r.integers(-1, rows, n))
    ref = take_many(cols, idx.to(torch.int32), neg=True)
    dcols = [c.to(gpu_device) for c in cols]
    for it in INTS:
        got = take_many(dcols, idx.to(it).to(gpu_device), neg=True)
        for a, b in zip(ref, got):
            assert a.to_arrow().equals(b.to_arrow())
    # string equality of row pairs (a count of waves that saw a mismatch): rows i and i + 350 hold
    # equal strings; then one differing pair in the last position, which a narrow read of wide
    # indices never reaches
    N = native()
    s = Column.from_arrow(pa.array([f"v{i % 350}" for i in range(rows)], pa.large_string()),
                          dict_encode=False).to(gpu_device)
    ai = torch.from_numpy(r.integers(0, rows, n))
    for last, want in ((350, False), (351, True)):
        bi = (ai + 350) % rows
        bi[-1] = (ai[-1] + last) % rows
        for it in INTS:
            a, b = ai.to(it).to(gpu_device), bi.to(it).to(gpu_device)
            mism = torch.zeros(1, dtype=torch.int32, device=gpu_device)
            N.str_eq_rows(ptr(s.offsets), ptr(s.data), ptr(a), ptr(s.offsets), ptr(s.data), ptr(b),
                          it == torch.int64, n, ptr(mism), stream(mism))
            assert (int(mism.item()) > 0) == want


@pytest.mark.parametrize("n", SIZES)
def test_select_write_index_widths(gpu_device, n):
    """select_write with an int64 index output (idx64) equals the int32 one."""
    N = native()
    mask = torch.from_numpy(np.random.default_rng(n).random(n) < 0.6)
    mask[0] = True
    md = mask.to(gpu_device)
    want = torch.nonzero(mask).flatten()
    assert torch.equal(mask_to_indices(md).cpu().long(), want)
    tiles = N.select_num_tiles(n)
    ws = torch.empty(tiles + 1, dtype=torch.int64, device=gpu_device)
    N.select_count(ptr(md), n, ptr(ws), ptr(ws) + 8 * tiles, stream(md))
    out = torch.full((want.numel(),), -7, dtype=torch.int64, device=gpu_device)
    N.select_write(ptr(md), n, ptr(ws), ptr(out), True, want.numel(), stream(md))
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", INTS)
def test_partition_key_and_perm_widths(gpu_device, dtype, n):
    """partition_ids and partition_run under int32 / int64 keys, the
    permutation written as int32 and as int64 (perm64), against the CPU path."""
    N = native()
    nparts = 5
    keys = torch.from_numpy(np.random.default_rng(n).integers(-10**6, 10**6, n)).to(dtype)
    kd = keys.to(gpu_device)
    assert torch.equal(M.partition_ids(kd, nparts).cpu(), M.partition_ids(keys, nparts))
    perm_ref, counts_ref = M.hash_partition(keys, nparts)
    perm, counts = M.hash_partition(kd, nparts)
    assert counts == counts_ref and torch.equal(perm.cpu().long(), perm_ref.long())
    blocks = N.partition_run_blocks(n)
    ws = torch.empty(nparts * blocks + 1, dtype=torch.int64, device=gpu_device)
    wide = torch.full((n,), -7, dtype=torch.int64, device=gpu_device)
    N.partition_run(ptr(kd), dtype == torch.int64, n, nparts, ptr(ws), ptr(ws) + 8 * nparts * blocks, ptr(wide), True,
                    stream(kd))
    assert torch.equal(wide.cpu(), perm_ref.long())


@pytest.mark.parametrize("n", SIZES)
def test_pack_rows_and_sort_key_pack_perm_widths(gpu_device, n):
    """pack_rows and sort_key_pack read an int32 or int64 row permutation
    (perm64); sort_key_pack writes 32- or 64-bit keys (out32)."""
    r = np.random.default_rng(n)
    rows = 900
    a = torch.from_numpy(r.integers(-10**12, 10**12, rows)).to(gpu_device)
    b = torch.from_numpy(r.integers(0, 1000, rows).astype(np.int32)).to(gpu_device)
    perm = torch.from_numpy(r.integers(0, rows, n))
    ref, (_, fields) = PK.pack_rows([a.cpu(), b.cpu()], perm, n)
    used = sum(w for _, w, _ in fields)          # (the row's padding bytes are not written)
    for it in INTS:
        got, _ = PK.pack_rows([a, b], perm.to(it).to(gpu_device), n)
        assert torch.equal(got.cpu()[:, :used], ref[:, :used])
    for col, out_dt in ((b, torch.int32), (a, torch.int64)):       # 10 key bits / 41 key bits
        lo, hi = int(col.min()), int(col.max())
        group = SO._fields_from([(col, False, False, None)], [lo, hi])
        for it in INTS:
            keys, bits = SO._pack(group, n, perm.to(it).to(gpu_device), gpu_device)
            assert keys.dtype == out_dt and bits == (hi - lo).bit_length()
            assert torch.equal(keys.cpu().long(), col.cpu().long()[perm] - lo)


# ------------------------------------------------------------------ sort, util
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("vdt", INTS)
@pytest.mark.parametrize("kdt", INTS)
def test_sort_pairs_key_and_value_widths(gpu_device, kdt, vdt, n):
    """radix_sort_pairs (one-workgroup and tiled) over key width x value width
    (val64), radix_digit_hist and radix_le_mask over key width: a stable sort
    against torch.sort, histogram against bincount."""
    N = native()
    bits = 20
    k = torch.from_numpy(np.random.default_rng(n).integers(0, 1 << bits, n)).to(kdt)
    v = torch.arange(n).to(vdt)
    sk, sv = SO.sort_pairs(k.to(gpu_device), v.to(gpu_device), bits)
    order = torch.sort(k.long(), stable=True).indices
    assert sk.dtype == kdt and sv.dtype == vdt
    assert torch.equal(sk.cpu(), k[order]) and torch.equal(sv.cpu().long(), order)
    kd = k.to(gpu_device)
    hist = torch.full((256,), -1, dtype=torch.int64, device=gpu_device)
    N.radix_digit_hist(ptr(kd), kdt == torch.int64, n, 8, 0, 64, ptr(hist), stream(kd))
    assert torch.equal(hist.cpu(), torch.bincount((k.long() >> 8) & 255, minlength=256))
    mask = torch.zeros(n, dtype=torch.bool, device=gpu_device)
    N.radix_le_mask(ptr(kd), kdt == torch.int64, n, 1 << (bits - 1), ptr(mask), stream(kd))
    assert torch.equal(mask.cpu(), k.long() <= (1 << (bits - 1)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("wide", [False, True])
def test_differs_from_rep_index_widths(gpu_device, wide, n):
    """differs_from_rep over every element size, the representative rows as
    int32 and int64 (rep64): the flag is set exactly when a row differs."""
    N = native()
    r = np.random.default_rng(n)
    lab = r.integers(0, 7, n)
    first = {}
    rep = np.array([first.setdefault(int(v), i) for i, v in enumerate(lab)])     # first row with the same label
    repd = torch.from_numpy(rep).to(torch.int64 if wide else torch.int32).to(gpu_device)
    later = np.flatnonzero(rep != np.arange(n))
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
        same = torch.from_numpy(lab * 3).to(dt)
        cases = [(same, 0)]
        if later.size:
            diff = same.clone()
            diff[int(later[-1])] += 1
            cases.append((diff, 1))
        for vals, want in cases:
            vd = vals.to(gpu_device)
            flag = torch.full((1,), -1, dtype=torch.int32, device=gpu_device)
            N.differs_from_rep(ptr(vd), vd.element_size(), ptr(repd), wide, n, ptr(flag), stream(vd))
            assert int(flag.item()) == want, (dt, want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", INTS)
def test_key_marks_and_sketch_key_widths(gpu_device, dtype, n):
    """mark_keys / probe_marks and hll_sketch under int32 and int64 keys:
    marks against numpy, and the same registers for both key widths."""
    N = native()
    r = np.random.default_rng(n)
    dom, base = 300, -40
    keys = torch.from_numpy(r.integers(base - 20, base + dom + 20, n)).to(dtype)
    valid = torch.from_numpy(r.random(n) > 0.2)
    kd, vd = keys.to(gpu_device), valid.to(gpu_device)
    marks = torch.zeros(dom, dtype=torch.bool, device=gpu_device)
    N.mark_keys(ptr(kd), dtype == torch.int64, ptr(vd), n, base, dom, ptr(marks), stream(kd))
    inside = valid & (keys >= base) & (keys < base + dom)
    want = torch.zeros(dom, dtype=torch.bool)
    want[(keys[inside] - base).long()] = True
    assert torch.equal(marks.cpu(), want)
    probe = torch.from_numpy(r.integers(base - 20, base + dom + 20, n)).to(dtype)
    pd = probe.to(gpu_device)
    for negate in (False, True):
        out = torch.zeros(n, dtype=torch.bool, device=gpu_device)
        N.probe_marks(ptr(pd), dtype == torch.int64, ptr(vd), n, base, dom, ptr(marks), negate, ptr(out), stream(pd))
        pin = (probe >= base) & (probe < base + dom)
        hit = torch.zeros(n, dtype=torch.bool)
        hit[pin] = want[(probe[pin] - base).long()]
        assert torch.equal(out.cpu(), (hit & valid) != negate)
    regs = H.hll_sketch(kd, vd)
    assert int((regs > 0).sum()) > 0
    assert torch.equal(regs, H.hll_sketch(kd.to(torch.int64 if dtype == torch.int32 else torch.int32), vd))
