"""to_timestamp(s, fmt, ...) / to_date(s, fmt, ...): text parsed by a list of
chrono-style formats (csrc/kernels/strptime.hip), the inverse of ``to_char``.

``compile_formats`` turns the formats into one flat op program (opcode bytes
plus literal bytes, the composites %F %T %R %D expanded, each format closed
by an END op); the formats are tried in order and the first that consumes
the whole text and passes the range checks gives the value. The grammar is
the table in the README ("Parsing dates and timestamps by format").

On the GPU one kernel interprets the program, one lane per row; one readback
per call carries the smallest row no format matched and the call raises
``ExecutionError`` naming it (NULL rows never raise). A dictionary column is
parsed once per entry and gathered by code; if an entry fails, the decoded
column decides, so an unused entry or one only under NULL rows does not
raise and the error names a row.

``py_strptime`` is the Python twin: the CPU engine's implementation and the
plan-time fold. It interprets the same program with its own code (``datetime``
for the calendar) and shares nothing with the kernel.
"""
from __future__ import annotations

import datetime
from typing import List, Optional, Sequence

import torch

from .. import types as T
from ..columnar import Column
from ..utils.errors import ExecutionError, PlanError
from ._lib import device_ints, is_gpu, launch, ptr, stream, to_host_int, to_host_ints

MAX_FORMATS, MAX_FORMAT_BYTES, MAX_PROGRAM = 8, 128, 256

# opcodes (csrc/kernels/strptime.h StrptimeOp)
(OP_END, OP_LIT, OP_YEAR, OP_CENT, OP_YY, OP_MON, OP_DAY, OP_DAY_SP, OP_HOUR, OP_HOUR_SP, OP_H12, OP_H12_SP, OP_MIN,
 OP_SEC, OP_DOY, OP_MONNAME, OP_WDAY, OP_AMPM, OP_NANOS, OP_FRAC_OPT, OP_FRAC3, OP_FRAC6, OP_FRAC9, OP_OFFSET,
 OP_OFFSET_Z, OP_EPOCH) = range(26)

#: what the instant is floored to (StrptimeUnit): int64 microseconds, or int32 day numbers
UNIT_MICROS, UNIT_MILLIS, UNIT_SECONDS, UNIT_DAY = range(4)
#: Func("strptime") option -> (SQL function as written, unit). The engine's timestamp is
#: microseconds, so to_timestamp_nanos keeps microseconds.
UNITS = {"timestamp": ("to_timestamp", UNIT_MICROS), "seconds": ("to_timestamp_seconds", UNIT_SECONDS),
         "millis": ("to_timestamp_millis", UNIT_MILLIS), "micros": ("to_timestamp_micros", UNIT_MICROS),
         "nanos": ("to_timestamp_nanos", UNIT_MICROS), "date": ("to_date", UNIT_DAY)}

# specifier byte -> (op, the field it sets)
_SPEC = {
    "Y": (OP_YEAR, "year"), "C": (OP_CENT, "century"), "y": (OP_YY, "year of century"), "m": (OP_MON, "month"),
    "d": (OP_DAY, "day"), "e": (OP_DAY_SP, "day"), "H": (OP_HOUR, "hour"), "k": (OP_HOUR_SP, "hour"),
    "I": (OP_H12, "hour12"), "l": (OP_H12_SP, "hour12"), "M": (OP_MIN, "minute"), "S": (OP_SEC, "second"),
    "j": (OP_DOY, "day of year"), "b": (OP_MONNAME, "month"), "h": (OP_MONNAME, "month"), "B": (OP_MONNAME, "month"),
    "a": (OP_WDAY, None), "A": (OP_WDAY, None), "p": (OP_AMPM, "am/pm"), "P": (OP_AMPM, "am/pm"),
    "f": (OP_NANOS, "fraction"), "z": (OP_OFFSET, "offset"), "s": (OP_EPOCH, "epoch"),
}
_COMPOSITE = {"F": "%Y-%m-%d", "T": "%H:%M:%S", "R": "%H:%M", "D": "%m/%d/%y"}
_MONTHS = ("january", "february", "march", "april", "may", "june", "july", "august", "september", "october",
           "november", "december")
_DAYS = ("sunday", "monday", "tuesday", "wednesday", "thursday", "friday", "saturday")
_MIN_EPOCH_S, _MAX_EPOCH_S = -62135596800, 253402300799       # 0001-01-01T00:00:00 .. 9999-12-31T23:59:59
_EPOCH_ORD = datetime.date(1970, 1, 1).toordinal()


# ------------------------------------------------------------------ compiler
def _compile_one(fmt: str) -> bytes:
    raw = fmt.encode("utf-8")
    if len(raw) > MAX_FORMAT_BYTES:
        raise PlanError(f"format {fmt!r} is longer than {MAX_FORMAT_BYTES} bytes")
    ops: List[tuple] = []       # (op,) or (OP_LIT, bytes)
    seen: set = set()

    def field(name: Optional[str], spec: str) -> None:
        if name is None:
            return
        if name in seen:
            raise PlanError(f"format {fmt!r}: %{spec} sets the {name} a second time")
        seen.add(name)

    def lit(b: bytes) -> None:
        if ops and ops[-1][0] == OP_LIT:
            ops[-1] = (OP_LIT, ops[-1][1] + b)
        else:
            ops.append((OP_LIT, b))

    def emit(b: bytes) -> None:
        i = 0
        while i < len(b):
            if b[i] != 0x25:
                lit(b[i:i + 1])
                i += 1
                continue
            if i + 1 >= len(b):
                raise PlanError(f"format {fmt!r} ends with a lone '%'")
            s = chr(b[i + 1])
            i += 2
            if s == "%":
                lit(b"%")
            elif s == ".":
                if b[i:i + 1] == b"f":
                    op, i = OP_FRAC_OPT, i + 1
                elif b[i:i + 2] in (b"3f", b"6f", b"9f"):
                    op, i = {b"3": OP_FRAC3, b"6": OP_FRAC6, b"9": OP_FRAC9}[b[i:i + 1]], i + 2
                else:
                    raise PlanError(f"format {fmt!r}: unknown specifier '%.{b[i:i + 1].decode('utf-8', 'replace')}'")
                field("fraction", ".f")
                ops.append((op,))
            elif s in ":#":
                if b[i:i + 1] != b"z":
                    raise PlanError(f"format {fmt!r}: unknown specifier '%{s}{b[i:i + 1].decode('utf-8', 'replace')}'")
                i += 1
                field("offset", s + "z")
                ops.append((OP_OFFSET if s == ":" else OP_OFFSET_Z,))
            elif s in _COMPOSITE:
                emit(_COMPOSITE[s].encode("ascii"))
            elif s in _SPEC:
                op, name = _SPEC[s]
                field(name, s)
                ops.append((op,))
            else:
                raise PlanError(f"format {fmt!r}: unknown specifier '%{s}'" if s.isascii() and s.isprintable()
                                else f"format {fmt!r}: unknown specifier after '%'")

    emit(raw)
    has = seen.__contains__
    if has("year") and (has("century") or has("year of century")):
        raise PlanError(f"format {fmt!r} sets the year twice (%Y with %C or %y)")
    if has("hour") and has("hour12"):
        raise PlanError(f"format {fmt!r} sets the hour twice (%H with %I)")
    if has("century") and not has("year of century"):
        raise PlanError(f"format {fmt!r}: %C needs %y")
    if has("hour12") and not has("am/pm"):
        raise PlanError(f"format {fmt!r}: %I needs %p")
    if has("am/pm") and not has("hour12"):
        raise PlanError(f"format {fmt!r}: %p needs %I or %l")
    if has("day of year") and (has("month") or has("day")):
        raise PlanError(f"format {fmt!r}: %j excludes the month and the day of the month")
    if has("epoch"):
        if len(seen) > 1 or any(o[0] == OP_WDAY for o in ops):
            raise PlanError(f"format {fmt!r}: %s excludes every other date and time field")
    else:
        year = has("year") or has("year of century")
        if not (year and (has("day of year") or (has("month") and has("day")))):
            raise PlanError(f"format {fmt!r} does not fix a date (it needs a year with month and day, a year with %j, or %s)")
    out = bytearray()
    for o in ops:
        if o[0] == OP_LIT:
            for k in range(0, len(o[1]), 255):
                chunk = o[1][k:k + 255]
                out += bytes((OP_LIT, len(chunk))) + chunk
        else:
            out.append(o[0])
    out.append(OP_END)
    return bytes(out)


def compile_formats(formats: Sequence[str]) -> bytes:
    """The formats as one op program; ``PlanError`` for a format outside the grammar, more than
    8 formats, a format over 128 bytes or a program over 256 bytes."""
    formats = list(formats)
    if not formats:
        raise PlanError("at least one format is needed")
    if len(formats) > MAX_FORMATS:
        raise PlanError(f"at most {MAX_FORMATS} formats, got {len(formats)}")
    program = b"".join(_compile_one(f) for f in formats)
    if len(program) > MAX_PROGRAM:
        raise PlanError(f"the formats compile to {len(program)} bytes, more than the {MAX_PROGRAM} the kernel takes")
    return program


# ---------------------------------------------------------------------- twin
class _NoMatch(Exception):
    pass


def _digits(s: bytes, i: int, most: int) -> int:
    """End of the run of at most ``most`` ASCII digits at s[i:]; _NoMatch when there is none."""
    j = i
    while j < len(s) and j - i < most and 0x30 <= s[j] <= 0x39:
        j += 1
    if j == i:
        raise _NoMatch
    return j


def _name(s: bytes, i: int, names) -> tuple:
    low = bytes(c + 32 if 65 <= c <= 90 else c for c in s[i:i + 9])
    for cut in (None, 3):
        for k, nm in enumerate(names):
            want = nm[:cut].encode("ascii")
            if low.startswith(want):
                return k, i + len(want)
    raise _NoMatch


def _one(s: bytes, ops: list, unit: int) -> int:
    f: dict = {}
    i = 0
    for op, arg in ops:
        if op == OP_LIT:
            if s[i:i + len(arg)] != arg:
                raise _NoMatch
            i += len(arg)
        elif op == OP_YEAR:
            j = _digits(s, i, 4)
            f["year"], i = int(s[i:j]), j
        elif op in (OP_CENT, OP_YY, OP_MON, OP_DAY, OP_DAY_SP, OP_HOUR, OP_HOUR_SP, OP_H12, OP_H12_SP, OP_MIN, OP_SEC):
            if op in (OP_DAY_SP, OP_HOUR_SP, OP_H12_SP) and s[i:i + 1] == b" ":
                i += 1
            j = _digits(s, i, 2)
            v, i = int(s[i:j]), j
            key, lo, hi = {OP_CENT: ("cent", 0, 99), OP_YY: ("yy", 0, 99), OP_MON: ("mon", 1, 12),
                           OP_DAY: ("day", 1, 31), OP_DAY_SP: ("day", 1, 31), OP_HOUR: ("hour", 0, 23),
                           OP_HOUR_SP: ("hour", 0, 23), OP_H12: ("h12", 1, 12), OP_H12_SP: ("h12", 1, 12),
                           OP_MIN: ("min", 0, 59), OP_SEC: ("sec", 0, 59)}[op]
            if not lo <= v <= hi:
                raise _NoMatch
            f[key] = v
        elif op == OP_DOY:
            j = _digits(s, i, 3)
            f["doy"], i = int(s[i:j]), j
        elif op == OP_MONNAME:
            k, i = _name(s, i, _MONTHS)
            f["mon"] = k + 1
        elif op == OP_WDAY:
            f["wday"], i = _name(s, i, _DAYS)
        elif op == OP_AMPM:
            w = s[i:i + 2].upper()
            if w not in (b"AM", b"PM"):
                raise _NoMatch
            f["pm"], i = w == b"PM", i + 2
        elif op == OP_NANOS:
            j = _digits(s, i, 9)
            f["ns"], i = int(s[i:j]), j
        elif op in (OP_FRAC_OPT, OP_FRAC3, OP_FRAC6, OP_FRAC9):
            want = {OP_FRAC_OPT: 9, OP_FRAC3: 3, OP_FRAC6: 6, OP_FRAC9: 9}[op]
            if op == OP_FRAC_OPT and not (s[i:i + 1] == b"." and s[i + 1:i + 2].isdigit() and s[i + 1] < 0x80):
                continue
            if s[i:i + 1] != b".":
                raise _NoMatch
            j = _digits(s, i + 1, want)
            if op != OP_FRAC_OPT and j - (i + 1) != want:
                raise _NoMatch
            f["ns"], i = int(s[i + 1:j].ljust(9, b"0")), j
        elif op in (OP_OFFSET, OP_OFFSET_Z):
            if op == OP_OFFSET_Z and s[i:i + 1] in (b"Z", b"z"):
                f["off"], i = 0, i + 1
                continue
            sign = s[i:i + 1]
            if sign not in (b"+", b"-") or _digits(s, i + 1, 2) != i + 3:
                raise _NoMatch
            oh, i = int(s[i + 1:i + 3]), i + 3
            k = i + 1 if s[i:i + 1] == b":" else i
            om = None
            try:
                if _digits(s, k, 2) == k + 2:
                    om, i = int(s[k:k + 2]), k + 2
            except _NoMatch:
                pass
            if om is None:
                if op == OP_OFFSET:
                    raise _NoMatch
                om = 0
            if oh > 23 or om > 59:
                raise _NoMatch
            f["off"] = (oh * 3600 + om * 60) * (-1 if sign == b"-" else 1)
        elif op == OP_EPOCH:
            neg = s[i:i + 1] == b"-"
            j = _digits(s, i + neg, 18)
            v, i = int(s[i + neg:j]) * (-1 if neg else 1), j
            if not _MIN_EPOCH_S <= v <= _MAX_EPOCH_S:
                raise _NoMatch
            f["epoch"] = v
        else:
            raise ValueError(f"strptime program: unknown op {op}")
    if i != len(s):
        raise _NoMatch
    if "epoch" in f:
        secs = f["epoch"]
    else:
        year = f.get("year")
        if year is None:
            yy = f["yy"]
            year = f["cent"] * 100 + yy if "cent" in f else (2000 + yy if yy <= 68 else 1900 + yy)
        if not 1 <= year <= 9999:
            raise _NoMatch
        try:
            if "doy" in f:
                date = datetime.date(year, 1, 1) + datetime.timedelta(days=f["doy"] - 1)
                if f["doy"] < 1 or date.year != year:
                    raise _NoMatch
            else:
                date = datetime.date(year, f["mon"], f["day"])
        except (ValueError, OverflowError):
            raise _NoMatch from None
        if "wday" in f and (date.weekday() + 1) % 7 != f["wday"]:
            raise _NoMatch
        hour = f.get("hour", 0)
        if "h12" in f:
            hour = f["h12"] % 12 + (12 if f["pm"] else 0)
        secs = (date.toordinal() - _EPOCH_ORD) * 86400 + hour * 3600 + f.get("min", 0) * 60 + f.get("sec", 0) \
            - f.get("off", 0)
    us = f.get("ns", 0) // 1000
    if unit == UNIT_DAY:
        return secs // 86400
    if unit == UNIT_SECONDS:
        return secs * 1_000_000
    if unit == UNIT_MILLIS:
        return secs * 1_000_000 + us // 1000 * 1000
    return secs * 1_000_000 + us


def _split(program: bytes) -> list:
    """The program as one op list [(op, literal bytes | None)] per format."""
    out, cur, pc = [], [], 0
    while pc < len(program):
        op = program[pc]
        pc += 1
        if op == OP_END:
            out.append(cur)
            cur = []
        elif op == OP_LIT:
            n = program[pc]
            cur.append((op, program[pc + 1:pc + 1 + n]))
            pc += 1 + n
        else:
            cur.append((op, None))
    if cur:
        raise ValueError("strptime program: the last format has no END")
    return out


def py_strptime(text: bytes, program: bytes, unit: int) -> Optional[int]:
    """One text by the program: microseconds floored to ``unit`` (day numbers for UNIT_DAY),
    or None when no format matches."""
    for ops in _split(program):
        try:
            return _one(text, ops, unit)
        except _NoMatch:
            continue
    return None


# ------------------------------------------------------------------ operator
def _no_match(unit: str, row: int, text: bytes, formats) -> ExecutionError:
    shown = text[:40].decode("utf-8", "replace") + ("..." if len(text) > 40 else "")
    fm = ", ".join(repr(f) for f in formats)
    return ExecutionError(f"{UNITS[unit][0]}(): row {row}: {shown!r} matches none of the formats ({fm})")


def fold(text: Optional[str], formats, unit: str) -> Optional[int]:
    """The plan-time value of an all-literal call (through the twin)."""
    if text is None:
        return None
    raw = text.encode("utf-8")
    v = py_strptime(raw, compile_formats(formats), UNITS[unit][1])
    if v is None:
        raise _no_match(unit, 0, raw, formats)
    return v


def strptime(col: Column, formats, unit: str = "timestamp", to_date: bool = False) -> Column:
    """to_timestamp*(col, formats...) (``unit``: a key of UNITS) or to_date(col, formats...)."""
    if to_date:
        unit = "date"
    code = UNITS[unit][1]
    t = T.DATE32 if code == UNIT_DAY else T.TIMESTAMP
    program = compile_formats(formats)
    if col.is_dict:
        from .gather import take
        from .strings import decode
        d = col.dictionary
        try:
            per_entry = strptime(decode(d) if d.is_dict else d, formats, unit)
        except ExecutionError:
            # the entry may be unused or only under NULL rows: the rows decide (and name the row)
            return strptime(decode(col), formats, unit)
        if len(per_entry) == 0:
            return Column.full(None, t, len(col), col.device)
        idx = col.data if col.valid is None else torch.where(col.valid, col.data, torch.full_like(col.data, -1))
        out = take(per_entry, idx, neg=col.valid is not None)
        if col.valid is None:
            return Column(t, out.data, None)
        return Column(t, torch.where(col.valid, out.data, torch.zeros_like(out.data)), col.valid)   # 0 under NULL, as the kernel
    n = len(col)
    dt = torch.int32 if code == UNIT_DAY else torch.int64
    if not is_gpu(col.data):
        off = col.offsets.tolist()
        raw = col.data.numpy().tobytes()
        ok = col.valid.tolist() if col.valid is not None else None
        vals = [0] * n
        for r in range(n):
            if ok is None or ok[r]:
                v = py_strptime(raw[off[r]:off[r + 1]], program, code)
                if v is None:
                    raise _no_match(unit, r, raw[off[r]:off[r + 1]], formats)
                vals[r] = v
        return Column(t, torch.tensor(vals, dtype=dt), col.valid)
    data, off = col.data.contiguous(), col.offsets.contiguous()
    out = torch.empty(n, dtype=dt, device=data.device)
    if n == 0:
        return Column(t, out, col.valid)
    valid = col.valid.contiguous().view(torch.uint8) if col.valid is not None else None
    err = device_ints([n], data.device)
    prog = torch.frombuffer(bytearray(program), dtype=torch.uint8)      # host memory: copied into the kernel arguments
    launch("strptime").strptime(ptr(prog), len(program), code, ptr(off), ptr(data), data.numel(), ptr(valid), n,
                                ptr(out), ptr(err), stream(out))
    bad = to_host_int(err)
    if bad < n:
        lo, hi = to_host_ints(off[bad:bad + 2])
        lo, hi = max(lo, 0), min(hi, data.numel())
        raise _no_match(unit, bad, bytes(data[lo:max(lo, min(hi, lo + 41))].tolist()), formats)
    return Column(t, out, col.valid)
