"""Time-zone database: an own TZif reader (RFC 8536, version 2+) and the flat
per-zone table the tz kernels and their CPU twins search.

``zoneinfo.ZoneInfo`` exposes no transition table, so it cannot feed a kernel;
it stays what the tests compare against. A zone is looked up in

1. ``tz_dir`` (``set_tz_dir`` / the ``IGLOO_TZDIR`` environment switch),
2. ``zoneinfo.TZPATH``,
3. the installed ``tzdata`` package.

``'UTC'`` / ``'Z'`` and fixed offsets (``'+05:30'``, ``'-08'``) need no files.

The compiled table (``ZoneTable``) holds the explicit transitions of the
64-bit data block followed, when the POSIX TZ footer carries a DST rule, by
that rule expanded over one 400-year Gregorian cycle (146097 days, a whole
number of weeks, so the rule repeats exactly): later instants fold back by
whole cycles. ``offs[i]`` is the UTC offset in force after ``i`` transitions
(``offs[0]``: before the first, the first standard-time type of the file, as
``zoneinfo`` does). ``wall[i] = trans[i] + max(offs[i], offs[i + 1])`` is the
key of the inverse direction: a wall time that occurs twice (fold) or never
(gap) takes the offset in force before the transition (PEP 495 ``fold=0``).
Leap-second records are skipped.
"""
from __future__ import annotations

import os
import re
import struct
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from .errors import PlanError

CYCLE_S = 146097 * 86400          # 400 Gregorian years
_NO_FOLD = 1 << 62                # utc_lo / wall_lo of a zone without a repeating rule
_KEY_PAD = np.iinfo(np.int64).max

_tz_dir: Optional[str] = None
_lock = threading.Lock()
_tables: Dict[tuple, "ZoneTable"] = {}


def set_tz_dir(path: Optional[str]) -> None:
    """The ``tz_dir`` option: a directory of TZif files searched first."""
    global _tz_dir
    with _lock:
        _tz_dir = path
        _tables.clear()


def tz_dir() -> Optional[str]:
    return _tz_dir or os.environ.get("IGLOO_TZDIR") or None


@dataclass
class ZoneTable:
    name: str
    trans: np.ndarray          # int64 [n] UTC seconds, strictly increasing
    offs: np.ndarray           # int32 [n + 1]
    wall: np.ndarray           # int64 [n] non-decreasing
    utc_lo: int = _NO_FOLD     # instants >= utc_lo + CYCLE_S fold back into [utc_lo, utc_lo + CYCLE_S)
    wall_lo: int = _NO_FOLD

    @property
    def fixed(self) -> bool:
        return self.trans.size == 0

    @property
    def log2p(self) -> int:
        """Padded size exponent of the device table (-1: fixed offset, no table)."""
        if self.fixed:
            return -1
        return max(1, int(self.trans.size).bit_length())     # 2**k > n: at least one padding key

    def padded(self) -> np.ndarray:
        """[trans P][wall P] int64 + [offs P] int32 in one int64 buffer (csrc/kernels/tz.hip)."""
        p = 1 << self.log2p
        n = self.trans.size
        keys = np.full(2 * p, _KEY_PAD, dtype=np.int64)
        keys[:n] = self.trans
        keys[p:p + n] = self.wall
        offs = np.full(p, self.offs[-1], dtype=np.int32)
        offs[:n + 1] = self.offs
        return np.concatenate([keys, offs.view(np.int64)])

    # ------------------------------------------------------------ host lookups
    def _fold(self, s: np.ndarray, lo: int) -> np.ndarray:
        if lo == _NO_FOLD:
            return s
        return np.where(s >= lo + CYCLE_S, lo + (s - lo) % CYCLE_S, s)

    def offsets_utc(self, us: np.ndarray) -> np.ndarray:
        """UTC offset in seconds (int64) of each instant (int64 microseconds)."""
        s = self._fold(np.floor_divide(us, 1_000_000), self.utc_lo)
        return self.offs[np.searchsorted(self.trans, s, side="right")].astype(np.int64)

    def offsets_wall(self, us: np.ndarray) -> np.ndarray:
        s = self._fold(np.floor_divide(us, 1_000_000), self.wall_lo)
        return self.offs[np.searchsorted(self.wall, s, side="right")].astype(np.int64)


# --------------------------------------------------------------------- fixed offsets
_FIXED = re.compile(r"^([+-])(\d{1,2})(?::?(\d{2}))?(?::?(\d{2}))?$")


def fixed_offset_seconds(name: str) -> Optional[int]:
    """'+05:30' / '-08' / '-08:00' / 'UTC' / 'Z' -> seconds east of UTC; None for a named zone."""
    n = name.strip()
    if n.upper() in ("UTC", "Z"):
        return 0
    m = _FIXED.match(n)
    if not m:
        return None
    h, mi, se = int(m.group(2)), int(m.group(3) or 0), int(m.group(4) or 0)
    if h > 23 or mi > 59 or se > 59:
        raise PlanError(f"time zone offset {name!r} out of range")
    v = h * 3600 + mi * 60 + se
    return -v if m.group(1) == "-" else v


def _fixed_table(name: str, off: int) -> ZoneTable:
    return ZoneTable(name, np.zeros(0, np.int64), np.array([off], np.int32), np.zeros(0, np.int64))


# --------------------------------------------------------------------------- lookup
def _search_dirs() -> List[str]:
    dirs: List[str] = []
    d = tz_dir()
    if d:
        dirs.append(d)
    import zoneinfo
    dirs.extend(zoneinfo.TZPATH)
    try:
        import tzdata
        dirs.append(os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo"))
    except ImportError:
        pass
    return dirs


def find_zone_file(name: str) -> str:
    parts = name.split("/")
    if not name or name.startswith("/") or any(p in ("", ".", "..") for p in parts) \
            or not re.match(r"^[A-Za-z0-9_+\-/]+$", name):
        raise PlanError(f"invalid time zone name {name!r}")
    dirs = _search_dirs()
    for d in dirs:
        p = os.path.join(d, *parts)
        if os.path.isfile(p):
            return p
    raise PlanError(f"unknown time zone {name!r} (looked in {', '.join(dirs) or 'no directory'}; "
                    f"set tz_dir / IGLOO_TZDIR to a zoneinfo directory)")


def zone_table(name: str) -> ZoneTable:
    """The compiled table of a zone name (cached)."""
    key = (name, tz_dir())
    t = _tables.get(key)
    if t is not None:
        return t
    off = fixed_offset_seconds(name)
    if off is not None:
        t = _fixed_table(name, off)
    else:
        path = find_zone_file(name)
        with open(path, "rb") as f:
            raw = f.read()
        t = compile_tzif(raw, name, path)
    with _lock:
        _tables[key] = t
    return t


def check_zone(name: str) -> str:
    """Validate a zone name at plan time (PlanError if it cannot be resolved); returns it."""
    zone_table(name)
    return name


# ---------------------------------------------------------------------------- TZif
_HDR = struct.Struct(">4sc15x6l")


def _header(raw: bytes, pos: int, path: str):
    if len(raw) < pos + _HDR.size:
        raise PlanError(f"time zone file {path}: truncated header")
    magic, ver, isutcnt, isstdcnt, leapcnt, timecnt, typecnt, charcnt = _HDR.unpack_from(raw, pos)
    if magic != b"TZif":
        raise PlanError(f"time zone file {path}: bad magic {magic!r} (not a TZif file)")
    if min(isutcnt, isstdcnt, leapcnt, timecnt, typecnt, charcnt) < 0:
        raise PlanError(f"time zone file {path}: negative count in header")
    return ver, isutcnt, isstdcnt, leapcnt, timecnt, typecnt, charcnt


def parse_tzif(raw: bytes, path: str = "<bytes>") -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, int]], str]:
    """-> (transition instants, type index per transition, [(utoff, isdst)] per type, footer)."""
    ver, isutcnt, isstdcnt, leapcnt, timecnt, typecnt, charcnt = _header(raw, 0, path)
    if ver in (b"\x00", b"1"):
        raise PlanError(f"time zone file {path}: version 1 TZif (no 64-bit block); version 2 or later is needed")
    v1 = timecnt * 4 + timecnt + typecnt * 6 + charcnt + leapcnt * 8 + isstdcnt + isutcnt
    pos = _HDR.size + v1
    ver, isutcnt, isstdcnt, leapcnt, timecnt, typecnt, charcnt = _header(raw, pos, path)
    pos += _HDR.size
    body = timecnt * 8 + timecnt + typecnt * 6 + charcnt + leapcnt * 12 + isstdcnt + isutcnt
    if len(raw) < pos + body:
        raise PlanError(f"time zone file {path}: truncated 64-bit data block")
    if typecnt == 0:
        raise PlanError(f"time zone file {path}: no local time type")
    trans = np.frombuffer(raw, dtype=">i8", count=timecnt, offset=pos).astype(np.int64)
    pos += timecnt * 8
    idx = np.frombuffer(raw, dtype=np.uint8, count=timecnt, offset=pos).astype(np.int64)
    pos += timecnt
    types = []
    for i in range(typecnt):
        utoff, isdst, _ = struct.unpack_from(">lBB", raw, pos + 6 * i)
        types.append((utoff, isdst))
    pos += typecnt * 6 + charcnt + leapcnt * 12 + isstdcnt + isutcnt
    if timecnt and int(idx.max()) >= typecnt:
        raise PlanError(f"time zone file {path}: transition type out of range")
    if timecnt > 1 and not bool(np.all(trans[1:] > trans[:-1])):
        raise PlanError(f"time zone file {path}: transition times are not increasing")
    # footer: NL TZ-string NL
    if len(raw) <= pos or raw[pos:pos + 1] != b"\n":
        raise PlanError(f"time zone file {path}: truncated footer")
    end = raw.find(b"\n", pos + 1)
    if end < 0:
        raise PlanError(f"time zone file {path}: truncated footer")
    try:
        footer = raw[pos + 1:end].decode("ascii")
    except UnicodeDecodeError:
        raise PlanError(f"time zone file {path}: footer is not ASCII") from None
    return trans, idx, types, footer


# ------------------------------------------------------------------ POSIX TZ string
def _days_from_civil(y: int, m: int, d: int) -> int:
    y -= m <= 2
    era = (y if y >= 0 else y - 399) // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def _is_leap(y: int) -> bool:
    return (y % 4 == 0 and y % 100 != 0) or y % 400 == 0


_NAME = r"(?:<[A-Za-z0-9+\-]+>|[A-Za-z]{3,})"
_OFF = r"[+-]?\d{1,3}(?::\d{1,2}(?::\d{1,2})?)?"
_TZSTR = re.compile(rf"^({_NAME})({_OFF})(?:({_NAME})({_OFF})?(?:,([^,]+),([^,]+))?)?$")


def _hms(s: str) -> int:
    sign = -1 if s.startswith("-") else 1
    p = [int(x) for x in s.lstrip("+-").split(":")]
    p += [0] * (3 - len(p))
    return sign * (p[0] * 3600 + p[1] * 60 + p[2])


@dataclass
class _Rule:
    kind: str          # 'M' | 'J' | 'N'
    a: int
    b: int = 0
    c: int = 0
    time: int = 7200

    def day_seconds(self, year: int) -> int:
        """Local seconds since the epoch of the rule's switch in ``year`` (the caller subtracts the offset)."""
        if self.kind == "M":
            m, w, d = self.a, self.b, self.c
            first = _days_from_civil(year, m, 1)
            dow = (first + 4) % 7                      # 0 = Sunday
            day = first + (d - dow) % 7 + (w - 1) * 7
            nxt = _days_from_civil(year + (m == 12), m % 12 + 1, 1)
            if day >= nxt:
                day -= 7
        elif self.kind == "J":                         # 1..365, February 29 never counted
            day = _days_from_civil(year, 1, 1) + self.a - 1 + (1 if _is_leap(year) and self.a >= 60 else 0)
        else:                                          # 0..365, leap days counted
            day = _days_from_civil(year, 1, 1) + self.a
        return day * 86400 + self.time


def _parse_rule(s: str, path: str) -> _Rule:
    date, _, tm = s.partition("/")
    t = _hms(tm) if tm else 7200
    m = re.match(r"^M(\d{1,2})\.(\d)\.(\d)$", date)
    if m:
        mo, w, d = (int(x) for x in m.groups())
        if not (1 <= mo <= 12 and 1 <= w <= 5 and 0 <= d <= 6):
            raise PlanError(f"time zone file {path}: bad rule {s!r} in footer")
        return _Rule("M", mo, w, d, t)
    m = re.match(r"^J(\d{1,3})$", date)
    if m and 1 <= int(m.group(1)) <= 365:
        return _Rule("J", int(m.group(1)), time=t)
    m = re.match(r"^(\d{1,3})$", date)
    if m and int(m.group(1)) <= 365:
        return _Rule("N", int(m.group(1)), time=t)
    raise PlanError(f"time zone file {path}: bad rule {s!r} in footer")


def parse_posix_tz(s: str, path: str = "<footer>"):
    """-> (std offset, dst offset or None, start rule, end rule); offsets in seconds east of UTC."""
    m = _TZSTR.match(s)
    if not m:
        raise PlanError(f"time zone file {path}: cannot read the footer {s!r}")
    std = -_hms(m.group(2))
    if m.group(3) is None:
        return std, None, None, None
    dst = -_hms(m.group(4)) if m.group(4) else std + 3600
    if m.group(5) is None:
        raise PlanError(f"time zone file {path}: footer {s!r} names daylight time without a rule")
    return std, dst, _parse_rule(m.group(5), path), _parse_rule(m.group(6), path)


# -------------------------------------------------------------------------- compile
def compile_tzif(raw: bytes, name: str = "<bytes>", path: str = "<bytes>") -> ZoneTable:
    trans, idx, types, footer = parse_tzif(raw, path)
    before = next((u for u, isdst in types if not isdst), types[0][0])
    tr = [int(t) for t in trans]
    offs = [before] + [types[int(i)][0] for i in idx]
    utc_lo = _NO_FOLD
    if footer:
        std, dst, start, end = parse_posix_tz(footer, path)
        if dst is None:
            if not tr:
                offs = [std]
        else:
            last = tr[-1] if tr else -(1 << 40)
            y_last = 1970 if not tr else 1970 + int(last // 31556952)
            y0 = max(y_last + 1, 1971)
            utc_lo = _days_from_civil(y0, 1, 1) * 86400
            hi = utc_lo + CYCLE_S + 4 * 86400
            ext = []
            for y in range(y_last - 1, y0 + 402):
                ext.append((start.day_seconds(y) - std, dst))
                ext.append((end.day_seconds(y) - dst, std))
            ext.sort(key=lambda e: e[0])
            for t, o in ext:
                if t <= last or t > hi:
                    continue
                if tr and t == tr[-1]:            # two switches at one instant: the later one wins
                    offs[-1] = o
                    continue
                if o == offs[-1]:                 # already in this state (the last explicit transition)
                    continue
                tr.append(t)
                offs.append(o)
            if not tr:
                offs = [std]
    t64 = np.array(tr, dtype=np.int64)
    o32 = np.array(offs, dtype=np.int32)
    if t64.size > 1 and not bool(np.all(t64[1:] > t64[:-1])):
        raise PlanError(f"time zone file {path}: transition table is not monotone")
    o64 = o32.astype(np.int64)
    wall = t64 + np.maximum(o64[:-1], o64[1:]) if t64.size else np.zeros(0, np.int64)
    if wall.size:
        wall = np.maximum.accumulate(wall)
    if t64.size == 0:
        return _fixed_table(name, int(o32[0]))
    zt = ZoneTable(name, t64, o32, wall, utc_lo, utc_lo + 2 * 86400 if utc_lo != _NO_FOLD else _NO_FOLD)
    if zt.log2p > 11:       # the device table's limit (csrc/kernels/tz.hip: 2048 padded entries in LDS)
        raise PlanError(f"time zone file {path}: more than 2047 transitions after expanding the footer rule")
    return zt
