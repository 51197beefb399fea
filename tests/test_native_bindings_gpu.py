"""The adaptor-bound launchers that nothing else in the suite reaches.

str_prefix_key and probe_hash16 have no caller in igloo_amd (probe_hash16 is
the MFMA-vs-VALU experiment of scripts/mfma_hash_ab.py) and end_capture runs
only after a failed graph capture, so each is called directly here and
compared, exactly, with a host computation over the same tensors. Shapes: one
block of the launcher (kBlock = 256 rows) plus one row.
"""
import numpy as np
import pytest
import torch

from igloo_amd.ops._lib import native, ptr, stream

pytestmark = pytest.mark.gpu

N_ROWS = 256 + 1
M64 = (1 << 64) - 1


def test_str_prefix_key_matches_host(gpu_device):
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 13, N_ROWS)           # shorter than, equal to and longer than skip + 8
    off_h = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    chars_h = torch.from_numpy(rng.integers(0, 256, int(off_h[-1]), dtype=np.uint8))
    off, chars = off_h.to(gpu_device), chars_h.to(gpu_device)
    raw, o = chars_h.numpy().tobytes(), off_h.tolist()
    for skip in (0, 3):
        out = torch.empty(N_ROWS, dtype=torch.int64, device=gpu_device)
        native().str_prefix_key(ptr(off), ptr(chars), N_ROWS, skip, ptr(out), stream(out))
        want = []
        for i in range(N_ROWS):
            k = int.from_bytes(raw[o[i] + skip:o[i + 1]][:8].ljust(8, b"\0"), "big") ^ (1 << 63)
            want.append(k - (1 << 64) if k >> 63 else k)
        assert out.cpu().tolist() == want


def _mix64(k):
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & M64
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & M64
    return k ^ (k >> 33)


def _fmix32(h):
    h = h ^ (h >> 16)
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ (h >> 16)


def _fmix32_xor(values):
    x = 0
    for v in values:
        x ^= _fmix32(v)
    return x


@pytest.mark.parametrize("mfma", [False, True])
def test_probe_hash16_matches_host(gpu_device, mfma):
    rng = np.random.default_rng(5)
    keys_h = [torch.from_numpy(rng.integers(-2**31, 2**31, N_ROWS, dtype=np.int64).astype(np.int32)) for _ in range(4)]
    proj_h = torch.from_numpy(rng.integers(-127, 128, (16, 16), dtype=np.int64).astype(np.int8))
    keys = [k.to(gpu_device) for k in keys_h]
    proj = proj_h.to(gpu_device)
    out = torch.empty(N_ROWS, dtype=torch.int32, device=gpu_device)
    native().probe_hash16(mfma, *[ptr(k) for k in keys], N_ROWS, ptr(proj), ptr(out), stream(out))
    got = (out.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    if mfma:
        # 16 key bytes (signed) projected on 16 int8 directions; every projection mixed, XOR over the directions
        x = np.stack([k.numpy() for k in keys_h], axis=1).view(np.int8).astype(np.int64)
        d = (x @ proj_h.numpy().astype(np.int64)) & 0xFFFFFFFF
        v = (d + 0x9E3779B9 * np.arange(16, dtype=np.int64)) & 0xFFFFFFFF
        want = [_fmix32_xor(row) for row in v.tolist()]
    else:
        u = [[int(v) & 0xFFFFFFFF for v in k.tolist()] for k in keys_h]
        want = []
        for r in range(N_ROWS):
            a, b = u[0][r] | u[1][r] << 32, u[2][r] | u[3][r] << 32
            want.append((_mix64(a) ^ ((_mix64(b) * 0x9E3779B97F4A7C15 & M64) >> 7)) & 0xFFFFFFFF)
    assert got == want


def test_end_capture_outside_a_capture_is_a_no_op(gpu_device):
    t = torch.arange(N_ROWS, dtype=torch.int32, device=gpu_device)
    assert native().end_capture(stream(t)) is None
    assert not torch.cuda.is_current_stream_capturing()
    # the stream still takes launches
    from igloo_amd.ops import misc
    assert torch.equal(misc.date_part(t, "day").cpu(), misc.date_part(t.cpu(), "day"))
