"""TRY_CAST conversions (csrc/kernels/trycast.hip): NULL where CAST raises or wraps.

``try_parse`` reads text (integers at the target's own width, decimals with
their precision, doubles, reals, dates, booleans, timestamps) and
``cast_checked`` narrows numbers (integer / float / decimal / 128-bit decimal
to an integer or a decimal). Both write a validity byte per row in the one
launch that converts: no error flag, no readback, so a query that uses them
is captured into a graph like any other. A dictionary column is parsed once
per dictionary entry and the values and validity are gathered by code.

CPU tensors take the Python twins below, which follow the same grammar and
the same integer arithmetic; they are the CPU engine's implementation and
share no code with the kernels.
"""
from __future__ import annotations

import datetime
import math
import re
from typing import Optional

import numpy as np
import torch

from ..columnar import Column
from ._lib import is_gpu, launch, ptr, stream

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
_INT_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64}

#: try_parse kinds (trycast.hip)
_P_I64, _P_I32, _P_DEC, _P_DATE, _P_F64, _P_BOOL, _P_I16, _P_I8, _P_F32, _P_TS = range(10)
#: cast_checked kinds (castcheck.h CastKind)
_K = {"int8": 0, "int16": 1, "int32": 2, "int64": 3, "float32": 4, "float64": 5, "decimal": 6}
_K_WIDE = 7


def _parse_kind(t):
    """(kernel kind, scale, precision, storage dtype) of a try_parse target, or None."""
    if t.is_decimal:
        return _P_DEC, t.scale, t.precision, torch.int64
    if t.is_integer:
        return {"int64": _P_I64, "int32": _P_I32, "int16": _P_I16, "int8": _P_I8}[t.kind], 0, 0, t.torch_dtype
    if t.kind == "float64":
        return _P_F64, 0, 0, torch.float64
    if t.kind == "float32":
        return _P_F32, 0, 0, torch.float32
    if t.kind == "date32":
        return _P_DATE, 0, 0, torch.int32
    if t.kind == "bool":
        return _P_BOOL, 0, 0, torch.uint8
    if t.kind == "timestamp" and not t.is_zoned:
        return _P_TS, 0, 0, torch.int64
    return None


def can_parse(t) -> bool:
    return _parse_kind(t) is not None


def can_fail(src, t) -> bool:
    """A numeric conversion ``cast_checked`` covers: the pairs of the TRY_CAST
    table that can give NULL. Everything else converts exactly as CAST does."""
    if not (t.is_integer or t.is_decimal):
        return False
    if src.is_float or src.is_decimal:
        return True
    if not src.is_integer:
        return False
    if t.is_integer:
        return _INT_BITS[src.kind] > _INT_BITS[t.kind]
    return True         # integer -> decimal: the product or the precision bound can fail


# ------------------------------------------------------------------ try_parse
def try_parse(col: Column, t) -> Column:
    """TRY_CAST(varchar AS t): the parsed values, NULL where the text is not a value of t."""
    kind, scale, precision, dt = _parse_kind(t)
    if col.is_dict:
        d = col.dictionary
        from .strings import decode
        per_entry = try_parse(decode(d) if d.is_dict else d, t)
        if len(per_entry) == 0:
            return Column.full(None, t, len(col), col.device)
        from .gather import take
        if col.valid is None:
            return take(per_entry, col.data)
        # codes under NULL rows are unspecified: never dereference them (a negative index gathers NULL)
        out = take(per_entry, torch.where(col.valid, col.data, torch.full_like(col.data, -1)), neg=True)
        return Column(t, torch.where(out.valid, out.data, torch.zeros_like(out.data)), out.valid)
    n = len(col)
    if not is_gpu(col.data):
        return _try_parse_host(col, t)
    out = torch.empty(n, dtype=dt, device=col.device)
    ok = torch.empty(n, dtype=torch.uint8, device=col.device)
    valid = col.valid.view(torch.uint8) if col.valid is not None else None
    launch("try_parse").try_parse(ptr(col.offsets), ptr(col.data), n, ptr(valid), kind, scale, precision, ptr(out),
                                  ptr(ok), stream(out))
    if dt == torch.uint8:
        out = out.view(torch.bool)
    return Column(t, out, ok.view(torch.bool))


_RX_INT = re.compile(rb"[+-]?[0-9]+")
_RX_DEC = re.compile(rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)")
_RX_F64 = re.compile(rb"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?"
                     rb"|[nN][aA][nN])")
_RX_DATE = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})")
_RX_TS = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})"
                    rb"(?:[Tt ]([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:\.([0-9]{1,9}))?)?)?"
                    rb"(?:[Zz]|([+-])([0-9]{2})(?::?([0-9]{2}))?)?")
_TRUE, _FALSE = (b"true", b"t", b"1"), (b"false", b"f", b"0")
_EPOCH_ORD = datetime.date(1970, 1, 1).toordinal()


def _days(y: bytes, m: bytes, d: bytes) -> Optional[int]:
    try:
        return datetime.date(int(y), int(m), int(d)).toordinal() - _EPOCH_ORD      # year 0000: ValueError
    except ValueError:
        return None


def parse_timestamp_py(s: bytes) -> Optional[int]:
    """The timestamp grammar of textparse.h ``parse_timestamp``: microseconds, or None."""
    m = _RX_TS.fullmatch(s)
    if m is None:
        return None
    days = _days(m.group(1), m.group(2), m.group(3))
    if days is None:
        return None
    hh, mi, ss = (int(g) if g is not None else 0 for g in m.group(4, 5, 6))
    if hh > 23 or mi > 59 or ss > 59:
        return None
    frac = int((m.group(7) or b"0").ljust(9, b"0")[:6])
    shift = 0
    if m.group(8) is not None:
        oh, om = int(m.group(9)), int(m.group(10) or 0)
        if oh > 23 or om > 59:
            return None
        shift = (oh * 3600 + om * 60) * (-1 if m.group(8) == b"-" else 1)
    return (days * 86400 + hh * 3600 + mi * 60 + ss - shift) * 1_000_000 + frac


def parse_text_py(s: bytes, t):
    """One text as a value of t in the engine's representation, or None (the rules of try_parse)."""
    if t.is_integer:
        if not _RX_INT.fullmatch(s):
            return None
        if len(s.lstrip(b"+-").lstrip(b"0")) > 19:            # (and int() refuses very long digit strings)
            return None
        v = int(s)
        b = _INT_BITS[t.kind]
        return v if -(1 << (b - 1)) <= v < (1 << (b - 1)) else None
    if t.is_decimal:
        if not _RX_DEC.fullmatch(s):
            return None
        whole, _, frac = s.lstrip(b"+-").partition(b".")
        whole = whole.lstrip(b"0")
        if frac[t.scale:].strip(b"0") or len(whole) > 19:     # not exact at this scale / beyond int64 already
            return None
        v = int((whole + frac[:t.scale].ljust(t.scale, b"0")) or b"0")
        v = -v if s[:1] == b"-" else v
        if not INT64_MIN <= v <= INT64_MAX or (t.precision <= 18 and abs(v) >= 10**t.precision):
            return None
        return v
    if t.is_float:
        if not _RX_F64.fullmatch(s):
            return None
        v = float(s)
        if t.kind == "float32":
            with np.errstate(over="ignore"):
                return float(np.float32(v))             # the correctly rounded double, rounded once more
        return v
    if t.kind == "date32":
        m = _RX_DATE.fullmatch(s)
        return _days(*m.groups()) if m else None
    if t.kind == "bool":
        low = bytes(c + 32 if 65 <= c <= 90 else c for c in s)
        return True if low in _TRUE else False if low in _FALSE else None
    return parse_timestamp_py(s)


def _column_from_values(vals, t, device) -> Column:
    """Engine-representation values (None: NULL) -> a fixed-width column with its validity."""
    ok = torch.tensor([v is not None for v in vals], dtype=torch.bool)
    fill = False if t.kind == "bool" else 0.0 if t.is_float else 0
    dt = torch.int64 if t.is_decimal else t.torch_dtype
    data = torch.tensor([fill if v is None else v for v in vals], dtype=dt)
    return Column(t, data.to(device), ok.to(device))


def _try_parse_host(col: Column, t) -> Column:
    off = col.offsets.tolist()
    raw = col.data.numpy().tobytes()
    valid = col.valid.tolist() if col.valid is not None else None
    vals = [parse_text_py(raw[off[i]:off[i + 1]], t) if valid is None or valid[i] else None for i in range(len(col))]
    return _column_from_values(vals, t, col.device)


# --------------------------------------------------------------- cast_checked
def cast_checked(col: Column, t) -> Column:
    """TRY_CAST between numbers where the value may not fit (``can_fail``): NULL for those rows."""
    src = col.dtype
    n = len(col)
    x = col.data
    if not is_gpu(x):
        return _cast_checked_host(col, t)
    if col.is_wide:
        sk, ss = _K_WIDE, (src.scale if src.is_decimal else 0)
        x = x.contiguous()
    else:
        sk, ss = _K[src.kind], (src.scale if src.is_decimal else 0)
        if x.stride(0) != 1 and n > 1:
            x = x.contiguous()
    dk = _K[t.kind]
    out = torch.empty(n, dtype=torch.int64 if t.is_decimal else t.torch_dtype, device=x.device)
    ok = torch.empty(n, dtype=torch.uint8, device=x.device)
    valid = col.valid.view(torch.uint8) if col.valid is not None else None
    launch("cast_checked").cast_checked(ptr(x), sk, ss, n, ptr(valid), dk, t.scale if t.is_decimal else 0,
                                        t.precision if t.is_decimal else 0, ptr(out), ptr(ok), stream(out))
    return Column(t, out, ok.view(torch.bool))


def _round_half_away(u: int, f: int) -> int:
    return (u + f // 2) // f


def convert_py(v, src, t):
    """One number of type src (engine representation; a wide value is its Python int) as a value of
    t (an integer or a decimal), or None where it does not fit: the rules of castcheck.h."""
    if t.is_integer:
        b = _INT_BITS[t.kind]
        if src.is_float:
            if math.isnan(v) or math.isinf(v):
                return None
            r = math.trunc(v)
        elif src.is_decimal:
            r = abs(v) // 10**src.scale * (-1 if v < 0 else 1)
        else:
            r = int(v)
        return r if -(1 << (b - 1)) <= r < (1 << (b - 1)) else None
    if src.is_float:
        if math.isnan(v) or math.isinf(v):
            return None
        with np.errstate(over="ignore"):
            # the product in the source's precision, as CAST forms it
            p = np.float32(v) * np.float32(float(10**t.scale)) if src.kind == "float32" else v * float(10**t.scale)
        if not math.isfinite(p):
            return None
        r = int(np.rint(p))
    else:
        up = t.scale - (src.scale if src.is_decimal else 0)
        v = int(v)
        r = v * 10**up if up >= 0 else _round_half_away(abs(v), 10**(-up)) * (-1 if v < 0 else 1)
    if not INT64_MIN <= r <= INT64_MAX or (t.precision <= 18 and abs(r) >= 10**t.precision):
        return None
    return r


def _cast_checked_host(col: Column, t) -> Column:
    src = col.dtype
    x = col.data
    valid = col.valid
    if t.is_integer and not col.is_wide and not src.is_decimal:
        b = _INT_BITS[t.kind]
        a = x.numpy()
        if src.is_float:
            with np.errstate(invalid="ignore"):
                tr = np.trunc(a.astype(np.float64))
                ok = (tr >= -(2.0 ** (b - 1))) & (tr < 2.0 ** (b - 1))      # NaN fails both
                vals = np.where(ok, tr, 0.0).astype(np.int64)
        else:
            a = a.astype(np.int64)
            ok = (a >= -(1 << (b - 1))) & (a <= (1 << (b - 1)) - 1)
            vals = np.where(ok, a, 0)
        if valid is not None:
            ok = ok & valid.numpy()
            vals = np.where(ok, vals, 0)
        return Column(t, torch.from_numpy(vals).to(t.torch_dtype), torch.from_numpy(ok))
    if col.is_wide:
        rows = [(hi << 64) | (lo & 0xFFFFFFFFFFFFFFFF) for lo, hi in x.tolist()]
    else:
        rows = x.tolist()
    vm = valid.tolist() if valid is not None else None
    vals = [convert_py(v, src, t) if vm is None or vm[i] else None for i, v in enumerate(rows)]
    return _column_from_values(vals, t, col.device)
