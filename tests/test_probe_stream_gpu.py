"""The folded-bitmap join probes (csrc/kernels/hashtable.hip probe_fold_kernel
for short probe sides, probe_stream_kernel for long ones, the per-table fold
pre-pass and the rule that keeps a dense fold away from the streaming loop) against
the scalar probe and numpy, at the row counts around the fold kernels' lower
bound; and join_table_init against torch.full / torch.zeros."""
import zlib

import numpy as np
import pytest
import torch

from igloo_amd.ops import hashing as H

pytestmark = pytest.mark.gpu


def _native():
    from igloo_amd.ops._lib import native
    return native()


def _m0() -> int:
    return int(_native().kFoldMinRows)


#: rows past the fold kernels' minimum: whole tiles, one row / one vector /
#: one wave step / one tile more, and the sizes next to them
TAILS = [0, 1, 3, 255, 257, 8191, 8193]

#: (span, build keys, key dtype, kmin): the fold is exact at 524,288 keys
#: (16,384 bitmap words), inexact from 524,289 on; 1 << 25 is the widest
#: exact bitmap (4 MiB). kmin is never 0: negative for int32 keys (the 32-bit
#: range test), beyond int32 for int64 keys.
CASES = {
    "exact-i32": (524_288, 20_000, torch.int32, -70_001),
    "exact-i64": (524_288, 20_000, torch.int64, 10**12 + 7),
    "inexact-i32": (524_289, 20_000, torch.int32, -70_001),
    "inexact-i64": (524_289, 20_000, torch.int64, 10**12 + 7),
    "wide-i32": (1 << 25, 100_000, torch.int32, 12_345),
    "wide-i64": (1 << 25, 100_000, torch.int64, -(10**12) - 5),
    # int32 probe keys against a table whose span runs past 2^31: the fold
    # kernels keep 64-bit key arithmetic there
    "inexact-i32-past-int32": (524_289, 20_000, torch.int32, 2**31 - 300_000),
}

_DATA = {}


def _case(name, dev):
    """Build table, probe keys, validity and numpy's verdict per probe row at
    the largest row count, computed once per case: every test takes prefixes."""
    if name in _DATA:
        return _DATA[name]
    span, nb, dt, kmin = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    off = rng.choice(np.arange(1, span - 1), nb - 2, replace=False)
    build = kmin + np.concatenate([[0, span - 1], off]).astype(np.int64)     # the span's two ends are keys
    rng.shuffle(build)
    mmax = _m0() + max(TAILS)
    lo, hi = kmin - 1000, kmin + span + 1000                                  # below kmin and past the span
    if dt == torch.int32:
        lo, hi = max(lo, -2**31), min(hi, 2**31)
    probe = rng.integers(lo, hi, mmax)
    there = build[(build >= lo) & (build < hi)]                               # (build keys the probe dtype holds)
    pick = rng.random(mmax) < 0.5                                             # half the rows: keys that are there
    probe[pick] = there[rng.integers(0, there.size, int(pick.sum()))]
    probe[-9:] = there[:9]                                                    # hits in every tail
    probe[:4] = [lo, kmin, min(kmin + span, hi) - 1, hi - 1]
    valid = rng.random(mmax) < 0.5
    build_dt = torch.int64 if build.max() >= 2**31 or build.min() < -2**31 else dt
    table = H.JoinTable(torch.from_numpy(build).to(build_dt).to(dev), None, defer_unique=False)
    assert table.direct and table.cap == span and table.kmin == kmin
    _DATA[name] = (table, torch.from_numpy(probe).to(dt).to(dev), torch.from_numpy(valid).to(dev),
                   np.isin(probe, build), valid)
    return _DATA[name]


#: knobs that send every fold probe to the tile loop / to the streaming loop
#: (the built-in rule splits them at a row count and a fold fill; -1: built-in)
FOLD = ("fold", 1 << 62, -1.0)
STREAM = ("stream", 0, 1.0)


def _check(table, probe, valid, hit, negate, kernels):
    """probe_select under each of ``kernels`` (expected kernel, asserted
    through the getter; streaming loop's minimum rows; its maximum fold fill)
    equals the scalar probe and numpy's row list."""
    N = _native()
    m = probe.numel()
    want = torch.from_numpy(np.nonzero(~hit if negate else hit)[0]).to(probe.device)
    N.set_probe_bits(0)
    try:
        p0, b0 = table.probe_select(probe, valid, negate=negate, want_build=not negate)
        assert N.last_probe_kernel() == "hits"
    finally:
        N.set_probe_bits(2)
    assert torch.equal(p0.long(), want)
    for kern, min_rows, max_fill in kernels:
        N.set_probe_stream_min_rows(min_rows)
        N.set_probe_stream_max_fill(max_fill)
        try:
            p, b = table.probe_select(probe, valid, negate=negate, want_build=not negate)
            assert N.last_probe_kernel() == kern, (N.last_probe_kernel(), kern, m)
        finally:
            N.set_probe_stream_min_rows(-1)
            N.set_probe_stream_max_fill(-1)
        assert p.dtype == p0.dtype and torch.equal(p, p0)
        assert (b is None and b0 is None) or torch.equal(b, b0)


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("name", list(CASES))
def test_fold_probes_match_scalar_and_numpy(gpu_device, name, tail):
    table, probe, valid, hit, valid_np = _case(name, gpu_device)
    m = _m0() + tail
    bits, bmask = table._bloom(m)
    assert bits and bmask >> 63
    for masked in (False, True):
        for negate in (False, True):
            h = hit[:m] & valid_np[:m] if masked else hit[:m]
            _check(table, probe[:m], valid[:m] if masked else None, h, negate, (FOLD, STREAM))


def test_default_rule_takes_a_fold_kernel(gpu_device):
    """With no knob set, a probe of the minimum row count runs one of the two
    fold kernels, one row fewer the plain bitmap probe."""
    N = _native()
    table, probe, valid, hit, valid_np = _case("inexact-i32", gpu_device)
    m = _m0()
    table.probe_select(probe[:m], valid[:m])
    assert N.last_probe_kernel() in ("fold", "stream")
    table.probe_select(probe[:m - 1], valid[:m - 1])
    assert N.last_probe_kernel() == "bits"


def test_dense_inexact_fold_stays_off_the_streaming_loop(gpu_device):
    """1.1M keys over a 20M span fold to ~88% set bits. The rule first planned
    for this shape (hand it to probe_bits_kernel) did not pay: at 600M rows
    the tile loop took 1.49 ms, probe_bits_kernel 1.79 ms, the streaming loop
    1.81 ms. What the fill estimate decides instead is which fold kernel runs:
    with the row minimum out of the way a sparse fold streams, this one takes
    the tile loop; either way the rows equal the scalar probe's and numpy's."""
    N = _native()
    rng = np.random.default_rng(9)
    span, nb, m = 20_000_000, 1_100_000, 4_500_001
    build = rng.choice(np.arange(1, span + 1), nb, replace=False).astype(np.int32)
    probe = rng.integers(-5, span + 7, m).astype(np.int32)
    valid = rng.random(m) < 0.5
    table = H.JoinTable(torch.from_numpy(build).to(gpu_device), None, defer_unique=False)
    bits, bmask = table._bloom(m)
    assert table.direct and bits and bmask >> 63
    assert m >= _m0() and N.probe_fold_needed(m, table.cap)
    hit = np.isin(probe, build) & valid
    _check(table, torch.from_numpy(probe).to(gpu_device), torch.from_numpy(valid).to(gpu_device), hit, False,
           (("fold", 0, -1.0), STREAM, ("fold", -1, -1.0)))
    assert table._fold is not None
    sparse, sprobe, svalid, shit, svalid_np = _case("wide-i32", gpu_device)     # ~17% of its folded bits set
    _check(sparse, sprobe, svalid, shit & svalid_np, False, (("fold", 0, -1.0), ("stream", 0, 0.2)))


@pytest.mark.parametrize("rid64", [False, True])
@pytest.mark.parametrize("cap", [1, 3, 4, 5, 1023, 2**20 + 1])
def test_join_table_init_matches_torch_fills(gpu_device, cap, rid64):
    """One launch leaves thead = -1, tkeys = the empty key, bits = 0 and
    dups = 0, and writes nothing past any of them (sentinels behind each
    array), for whole 16-byte chunks and for every tail length."""
    N = _native()
    dev = gpu_device
    rid = torch.int64 if rid64 else torch.int32
    pad = 8
    for hashed in (False, True):
        for nbw in (0, 1, 2, 3, 6, 1021, (cap + 31) // 32):
            thead = torch.full((cap + pad,), 7, dtype=rid, device=dev)
            tkeys = torch.full((cap + pad,), 7, dtype=torch.int64, device=dev) if hashed else None
            bits = torch.full((nbw + pad,), 7, dtype=torch.int32, device=dev) if nbw else None
            dups = torch.full((1 + pad,), 7, dtype=torch.int64, device=dev)
            N.join_table_init(thead.data_ptr(), rid64, cap, 0 if tkeys is None else tkeys.data_ptr(),
                              0 if bits is None else bits.data_ptr(), nbw, dups.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
            seven = lambda t: torch.full((pad,), 7, dtype=t.dtype, device=dev)
            assert torch.equal(thead[:cap], torch.full((cap,), -1, dtype=rid, device=dev))
            assert torch.equal(thead[cap:], seven(thead))
            if hashed:
                assert torch.equal(tkeys[:cap], torch.full((cap,), H.EMPTY_KEY, dtype=torch.int64, device=dev))
                assert torch.equal(tkeys[cap:], seven(tkeys))
            if nbw:
                assert torch.equal(bits[:nbw], torch.zeros(nbw, dtype=torch.int32, device=dev))
                assert torch.equal(bits[nbw:], seven(bits))
            assert torch.equal(dups[:1], torch.zeros(1, dtype=torch.int64, device=dev))
            assert torch.equal(dups[1:], seven(dups))
