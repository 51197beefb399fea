"""BINARY functions (csrc/kernels/binary.hip): encode / decode in hex and
base64, CAST between Utf8 and Binary (UTF-8 validation), byte lengths.

Parity: DataFusion's encoding functions (``encode`` / ``decode``). Hex is
lowercase; base64 is the standard alphabet without padding, which is what
DataFusion's encoding module writes to our knowledge -- the reference has no
fixture for it, so parity unpinned. ``decode`` accepts both letter cases of
hex and the unpadded or correctly padded form of base64, and raises
``ExecutionError`` naming the first bad row; a NULL row never raises.

On the GPU every function is native kernels only (no host step): flat hex
streams, a cooperative base64 writer, and a tiled UTF-8 validator. One
readback per call carries the smallest bad row (as ``str_parse`` does). The
CPU engine's twins use binascii / base64 / ``bytes.decode``.
"""
from __future__ import annotations

import base64
import binascii
from typing import Optional

import pyarrow as pa
import torch

from .. import types as T
from ..columnar import Column
from ..utils.errors import ExecutionError, PlanError
from ._lib import device_ints, is_gpu, launch, ptr, stream, to_host_int, to_host_ints
from .select import offsets_from_lengths

FORMATS = ("hex", "base64")
_B64 = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")


def check_format(fmt, what: str) -> str:
    f = fmt.lower() if isinstance(fmt, str) else None
    if f not in FORMATS:
        raise PlanError(f"{what}(): the format must be one of 'hex', 'base64', got {fmt!r}")
    return f


# ------------------------------------------------------------------ host twins
def py_encode(v: bytes, fmt: str) -> str:
    if fmt == "hex":
        return binascii.hexlify(v).decode("ascii")
    return base64.b64encode(v).rstrip(b"=").decode("ascii")


def py_decode(v: bytes, fmt: str) -> bytes:
    """The decode contract on one value; ValueError on a malformed one."""
    if fmt == "hex":
        if len(v) % 2:
            raise ValueError("odd number of hex digits")
        try:
            return binascii.unhexlify(v)
        except binascii.Error as e:
            raise ValueError(str(e)) from None
    pad = 2 if v.endswith(b"==") else 1 if v.endswith(b"=") else 0
    body = v[:len(v) - pad]
    if pad and len(v) % 4:
        raise ValueError("padding does not complete a group of four")
    if len(body) % 4 == 1:
        raise ValueError("length 1 (mod 4)")
    if any(c not in _B64 for c in body):
        raise ValueError("byte outside the base64 alphabet")
    out = base64.b64decode(body + b"=" * (-len(body) % 4))
    if base64.b64encode(out).rstrip(b"=") != body:
        raise ValueError("non-zero trailing bits")
    return out


def _as_bytes(v) -> bytes:
    return v if isinstance(v, bytes) else v.encode("utf-8")


def _host_column(vals, dtype, device) -> Column:
    return Column.from_arrow(pa.array(vals, dtype.to_arrow()), device=device, dtype=dtype, dict_encode=False)


def _plain(col: Column) -> Column:
    from . import strings as S
    return S.decode(col) if col.is_dict else col


def _valid_ptr(col: Column):
    return None if col.valid is None else col.valid.contiguous()


# ---------------------------------------------------------------------- encode
def encode(col: Column, fmt: str) -> Column:
    """encode(x, 'hex' | 'base64') -> Utf8; a dictionary column keeps its codes
    over the encoded dictionary (the map is injective: no re-encoding)."""
    fmt = check_format(fmt, "encode")
    if col.is_dict:
        return Column(T.UTF8, col.data, col.valid, dictionary=encode(_plain(col.dictionary), fmt))
    n = len(col)
    if not is_gpu(col.data):
        vals = [None if v is None else py_encode(_as_bytes(v), fmt) for v in col.to_pylist()]
        return _host_column(vals, T.UTF8, col.device)
    data, off = col.data.contiguous(), col.offsets.contiguous()
    s = stream(data)
    if fmt == "hex":
        # every byte of the buffer, whatever the rows: the offsets simply double
        out = torch.empty(2 * data.numel(), dtype=torch.uint8, device=data.device)
        launch("bin_hex_encode").bin_hex_encode(ptr(data), data.numel(), ptr(out), s)
        return Column(T.UTF8, out, col.valid, offsets=off * 2)
    valid = _valid_ptr(col)
    lens = torch.empty(max(n, 1), dtype=torch.int64, device=data.device)[:n]
    launch("bin_b64_enc_lengths").bin_b64_enc_lengths(ptr(off), ptr(valid), n, ptr(lens), s)
    ooff, total = offsets_from_lengths(lens)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=data.device)[:total]
    if total:
        launch("bin_b64_encode").bin_b64_write(True, ptr(off), ptr(data), ptr(ooff), n, out.numel(), ptr(out), s)
    return Column(T.UTF8, out, col.valid, offsets=ooff)


# ---------------------------------------------------------------------- decode
def _bad_row(what: str, fmt: str, row: int):
    return ExecutionError(f"{what}: invalid {fmt} input at row {row}")


def decode(col: Column, fmt: str) -> Column:
    """decode(x, 'hex' | 'base64') -> Binary; raises ExecutionError naming the
    first malformed row (NULL rows never raise)."""
    fmt = check_format(fmt, "decode")
    if col.is_dict:
        # once per dictionary entry; an entry that does not decode may be unused or
        # only under NULL rows, so the per-row path decides (and names the row)
        from .gather import take
        try:
            d = decode(_plain(col.dictionary), fmt)
        except ExecutionError:
            return decode(_plain(col), fmt)
        idx = col.data if col.valid is None else torch.where(col.valid, col.data, torch.full_like(col.data, -1))
        out = take(d, idx, neg=col.valid is not None)
        out.valid = col.valid
        return out
    n = len(col)
    if not is_gpu(col.data):
        vals = []
        for r, v in enumerate(col.to_pylist()):
            try:
                vals.append(None if v is None else py_decode(_as_bytes(v), fmt))
            except ValueError:
                raise _bad_row("decode()", fmt, r) from None
        return _host_column(vals, T.BINARY, col.device)
    data, off = col.data.contiguous(), col.offsets.contiguous()
    dev = data.device
    s = stream(data)
    valid = _valid_ptr(col)
    if n == 0:
        return Column(T.BINARY, torch.zeros(0, dtype=torch.uint8, device=dev), col.valid, offsets=off)
    if fmt == "hex":
        err = device_ints([n, 0], dev)
        launch("bin_hex_validate").bin_hex_validate(ptr(off), ptr(data), ptr(valid), n, data.numel(), ptr(err), s)
        bad, null_bytes, nbytes = to_host_ints(torch.cat([err, off[-1:] - off[:1]]))
        if bad < n:
            raise _bad_row("decode()", fmt, bad)
        if null_bytes:
            # NULL rows holding bytes (maybe an odd number): empty them, so the dense rows are all even
            from .gather import take
            rows = torch.arange(n, dtype=torch.int64, device=dev)
            dense = take(col, torch.where(col.valid, rows, torch.full_like(rows, -1)), neg=True)
            data, off = dense.data.contiguous(), dense.offsets.contiguous()
            nbytes = to_host_int(off[-1:] - off[:1])
        out = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)[:nbytes // 2]
        launch("bin_hex_decode").bin_hex_decode(ptr(off), n, ptr(data), out.numel(), ptr(out), s)
        return Column(T.BINARY, out, col.valid, offsets=(off - off[:1]) >> 1)
    err = device_ints([n], dev)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    launch("bin_b64_dec_lengths").bin_b64_dec_lengths(ptr(off), ptr(data), ptr(valid), n, data.numel(), ptr(lens),
                                                      ptr(err), s)
    bad = to_host_int(err)
    if bad < n:
        raise _bad_row("decode()", fmt, bad)
    ooff, total = offsets_from_lengths(lens)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    if total:
        launch("bin_b64_decode").bin_b64_write(False, ptr(off), ptr(data), ptr(ooff), n, out.numel(), ptr(out), s)
    return Column(T.BINARY, out, col.valid, offsets=ooff)


# ----------------------------------------------------------------------- casts
def to_binary(col: Column) -> Column:
    """CAST(utf8 AS BYTEA): the same buffers under the other type (a dictionary column is decoded first)."""
    p = _plain(col)
    return Column(T.BINARY, p.data, p.valid, offsets=p.offsets)


def utf8_validate(col: Column) -> Optional[int]:
    """First row of a plain column that is not valid UTF-8 on its own, or None."""
    n = len(col)
    if not is_gpu(col.data):
        for r, v in enumerate(col.to_pylist()):
            if v is not None:
                try:
                    _as_bytes(v).decode("utf-8")
                except UnicodeDecodeError:
                    return r
        return None
    data, off = col.data.contiguous(), col.offsets.contiguous()
    if n == 0 or data.numel() == 0:
        return None
    N = launch("utf8_validate")
    flags = torch.empty(N.utf8_num_tiles(data.numel()), dtype=torch.uint8, device=data.device)
    err = device_ints([n], data.device)
    N.utf8_validate(ptr(off), ptr(data), ptr(_valid_ptr(col)), n, data.numel(), ptr(flags), ptr(err), stream(data))
    bad = to_host_int(err)
    return bad if bad < n else None


def to_utf8(col: Column) -> Column:
    """CAST(binary AS VARCHAR): every row must be valid UTF-8 on its own."""
    p = _plain(col)
    bad = utf8_validate(p)
    if bad is not None:
        raise ExecutionError(f"CAST(Binary AS Utf8): invalid UTF-8 at row {bad}")
    return Column(T.UTF8, p.data, p.valid, offsets=p.offsets)


def byte_length(col: Column) -> torch.Tensor:
    """Bytes per row of a plain or dictionary varlen column, int32 (NULL rows: their stored length)."""
    if col.is_dict:
        from .gather import gather_tensor
        d = _plain(col.dictionary)
        lut = (d.offsets[1:] - d.offsets[:-1]).to(torch.int32)
        return gather_tensor(lut, col.data) if lut.numel() else torch.zeros(len(col), dtype=torch.int32, device=col.device)
    return (col.offsets[1:] - col.offsets[:-1]).to(torch.int32)
