"""Zone-aware timestamp functions (csrc/kernels/tz.hip): UTC <-> local wall
time, date_trunc and date_part in a zone's local time.

Values are int64 microseconds. A zone is the flat table ``utils/tzdb.py``
compiles from its TZif file; the device copy is cached per (zone, device), so
its pointer is stable across the replays of a captured query graph. On the GPU
every function is one launch of a hand-written kernel; the CPU twins search
the same compiled table with numpy (never ``zoneinfo``) and reuse the naive
``trunc_ts`` / ``ts_part`` on the local values.

Wall times inside a DST gap or fold take the offset in force before the
transition (PEP 495 ``fold=0``): 01:30 on the autumn night is its first
occurrence, 02:30 on the spring night lands one hour later.
"""
from __future__ import annotations

import threading
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..utils import tzdb
from ..utils.errors import NotSupported
from ._lib import check_not_capturing, is_gpu, launch, ptr, stream

TRUNC_UNITS = {"second": 0, "minute": 1, "hour": 2, "day": 3, "week": 4, "month": 5, "quarter": 6, "year": 7}
PART_FIELDS = {"year": 0, "month": 1, "day": 2, "quarter": 3, "dow": 4, "doy": 5, "hour": 6, "minute": 7,
               "second": 8, "millisecond": 9, "microsecond": 10, "week": 11}

_US = 1_000_000
_lock = threading.Lock()
_device_tables: Dict[tuple, Optional[torch.Tensor]] = {}


def device_table(zone: str, device) -> Tuple[tzdb.ZoneTable, Optional[torch.Tensor]]:
    """The compiled zone and its device buffer (None for a fixed offset), built once per (zone, device)."""
    zt = tzdb.zone_table(zone)
    if zt.fixed:
        return zt, None
    key = (zone, tzdb.tz_dir(), str(device))
    tab = _device_tables.get(key)
    if tab is None:
        check_not_capturing(f"time zone table {zone}")
        tab = torch.from_numpy(zt.padded()).to(device)
        with _lock:
            _device_tables[key] = tab
    return zt, tab


def _zone_args(zone: str, data: torch.Tensor):
    zt, tab = device_table(zone, data.device)
    return ptr(tab), zt.log2p, int(zt.offs[0]) if zt.fixed else 0, zt.utc_lo, zt.wall_lo


def _i64(data: torch.Tensor) -> torch.Tensor:
    return data.to(torch.int64).contiguous()


def _np(data: torch.Tensor) -> np.ndarray:
    return data.to(torch.int64).contiguous().numpy()


def to_local(data: torch.Tensor, zone: str, want_offsets: bool = False):
    """UTC us -> wall-clock us in ``zone``; with ``want_offsets`` also each row's offset (int32 seconds)."""
    if not is_gpu(data):
        a = _np(data)
        off = tzdb.zone_table(zone).offsets_utc(a)
        out = torch.from_numpy(a + off * _US)
        return (out, torch.from_numpy(off.astype(np.int32))) if want_offsets else out
    v = _i64(data)
    n = v.numel()
    out = torch.empty(n, dtype=torch.int64, device=v.device)
    offs = torch.empty(n, dtype=torch.int32, device=v.device) if want_offsets else None
    launch("tz_to_local").tz_to_local(ptr(v), n, *_zone_args(zone, v), ptr(out), ptr(offs), stream(v))
    return (out, offs) if want_offsets else out


def to_utc(data: torch.Tensor, zone: str) -> torch.Tensor:
    """Wall-clock us in ``zone`` -> UTC us (gap / fold: the offset before the transition)."""
    if not is_gpu(data):
        a = _np(data)
        return torch.from_numpy(a - tzdb.zone_table(zone).offsets_wall(a) * _US)
    v = _i64(data)
    n = v.numel()
    out = torch.empty(n, dtype=torch.int64, device=v.device)
    launch("tz_to_utc").tz_to_utc(ptr(v), n, *_zone_args(zone, v), ptr(out), stream(v))
    return out


def trunc(data: torch.Tensor, zone: str, unit: str) -> torch.Tensor:
    """date_trunc in local time: UTC us -> UTC us of the local period's start."""
    if unit not in TRUNC_UNITS:
        raise NotSupported(f"date_trunc('{unit}') on a timestamp with time zone")
    if not is_gpu(data):
        from ..exec.expr_eval import trunc_ts
        zt = tzdb.zone_table(zone)
        a = _np(data)
        t = trunc_ts(torch.from_numpy(a + zt.offsets_utc(a) * _US), unit).numpy()
        return torch.from_numpy(t - zt.offsets_wall(t) * _US)
    v = _i64(data)
    n = v.numel()
    out = torch.empty(n, dtype=torch.int64, device=v.device)
    launch("tz_trunc").tz_trunc(ptr(v), n, *_zone_args(zone, v), TRUNC_UNITS[unit], ptr(out), stream(v))
    return out


def part(data: torch.Tensor, zone: str, field: str) -> torch.Tensor:
    """date_part in local time (int32)."""
    if field not in PART_FIELDS:
        raise NotSupported(f"date_part('{field}') on a timestamp with time zone")
    if not is_gpu(data):
        from ..exec.expr_eval import ts_part
        return ts_part(to_local(data, zone), field).to(torch.int32)
    v = _i64(data)
    n = v.numel()
    out = torch.empty(n, dtype=torch.int32, device=v.device)
    launch("tz_part").tz_part(ptr(v), n, *_zone_args(zone, v), PART_FIELDS[field], ptr(out), stream(v))
    return out


# ------------------------------------------------------------------ host scalars
def _one(us: int) -> torch.Tensor:
    return torch.tensor([int(us)], dtype=torch.int64)


def to_local_py(us: int, zone: str) -> int:
    return int(to_local(_one(us), zone)[0])


def offset_py(us: int, zone: str) -> int:
    return int(tzdb.zone_table(zone).offsets_utc(np.array([int(us)], dtype=np.int64))[0])


def to_utc_py(us: int, zone: str) -> int:
    return int(to_utc(_one(us), zone)[0])


def trunc_py(us: int, zone: str, unit: str) -> int:
    return int(trunc(_one(us), zone, unit)[0])


def part_py(us: int, zone: str, field: str) -> int:
    return int(part(_one(us), zone, field)[0])


def format_offset(off: int, colon: bool = True) -> str:
    """+HH:MM / +HHMM, rounded to the nearest minute as chrono's %:z / %z (strfmt.hip does the same)."""
    sign = "-" if off < 0 else "+"
    mins = (abs(int(off)) + 30) // 60
    return f"{sign}{mins // 60:02d}{':' if colon else ''}{mins % 60:02d}"
