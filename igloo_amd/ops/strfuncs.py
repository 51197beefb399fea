"""Scalar string functions (csrc/kernels/strfunc.hip): btrim / ltrim / rtrim,
replace, lpad / rpad, reverse, repeat, left / right, initcap, translate,
split_part, substr_index, strpos, ascii, octet_length; the functions of two
string operands per row (csrc/kernels/strpair.hip, ``apply_pair``):
levenshtein, contains, find_in_set and strpos / starts_with / ends_with with a
per-row second operand, either operand a column or a constant; regexp_like / regexp_count /
regexp_replace / regexp_match (csrc/kernels/regex.hip: a DFA of the pattern
walked per row; regexp_count, regexp_replace with a literal replacement and
regexp_match without capture groups find leftmost-first match spans there.
Patterns outside the DFA subset or able to match the empty string, other
flags, group references and capture groups use the host regex engine,
reported as a host step).

Plain device columns run the two-pass kernels; dictionary columns apply the
function to their dictionary only (ops/strings.py ``_dict_transform``); CPU
columns use the Python definitions below, which are also the numerics oracle
of the GPU tests. Parity: DataFusion's string functions (reference
Cargo.lock:1062 datafusion-functions 48.0.0) behind SessionContext::sql
(reference crates/engine/src/lib.rs:54-57).
"""
from __future__ import annotations

import re
from typing import Callable, Optional

import pyarrow as pa
import pyarrow.compute as pc
import torch

from .. import types as T
from ..columnar import Column
from ._lib import is_gpu, launch, native, ptr, stream
from .select import offsets_from_lengths

CODES = {"trim": 0, "replace": 1, "lpad": 2, "rpad": 3, "reverse": 4, "repeat": 5, "left": 6, "right": 7,
         "initcap": 8, "translate": 9, "split_part": 10, "substr_index": 11}
INT_CODES = {"strpos": 20, "ascii": 21, "octet_length": 22}
#: two-operand functions of strpair.hip str_pair_int (levenshtein has kernels of its own)
PAIR_CODES = {"strpos": 0, "contains": 1, "starts_with": 2, "ends_with": 3, "find_in_set": 4}
PAIR_FUNCS = ("levenshtein",) + tuple(PAIR_CODES)
PAIR_BOOL = ("contains", "starts_with", "ends_with")
#: worker lanes of the long-row edit-distance kernel (each owns a slab of the scratch)
LEV_LONG_LANES = 1024
#: bound of that scratch in bytes: fewer lanes work when the rows are long, so
#: it holds max(this, 4 * (longest shorter side + 1)) bytes whatever the data
LEV_LONG_SCRATCH = 256 << 20


# ------------------------------------------------------------ Python semantics
def py_fn(name: str, opts: tuple) -> Callable[[str], object]:
    if name == "trim":
        mode, chars = opts
        if mode == 3:
            return lambda s: s.strip(chars)
        return (lambda s: s.lstrip(chars)) if mode == 1 else (lambda s: s.rstrip(chars))
    if name == "replace":
        a, b = opts
        return (lambda s: s) if a == "" else (lambda s: s.replace(a, b))
    if name in ("lpad", "rpad"):
        n, fill = opts
        n = max(int(n), 0)

        def pad(s):
            if len(s) >= n:
                return s[:n]
            if not fill:
                return s
            k = n - len(s)
            f = (fill * (k // len(fill) + 1))[:k]
            return f + s if name == "lpad" else s + f
        return pad
    if name == "reverse":
        return lambda s: s[::-1]
    if name == "repeat":
        n = max(int(opts[0]), 0)
        return lambda s: s * n
    if name == "left":
        n = int(opts[0])
        return lambda s: s[:n] if n >= 0 else s[:max(len(s) + n, 0)]
    if name == "right":
        n = int(opts[0])
        return lambda s: (s[max(len(s) - n, 0):] if n >= 0 else s[min(-n, len(s)):])
    if name == "initcap":
        def initcap(s):
            out, start = [], True
            for ch in s:
                if ch.isascii():
                    out.append(ch.upper() if start else ch.lower())
                else:
                    out.append(ch)
                start = not (ch.isalnum() or not ch.isascii())
            return "".join(out)
        return initcap
    if name == "translate":
        a, b = opts

        def tr(s):
            out = []
            for ch in s:
                k = a.find(ch)
                if k < 0:
                    out.append(ch)
                elif k < len(b):
                    out.append(b[k])
            return "".join(out)
        return tr
    if name == "split_part":
        d, n = opts
        n = int(n)

        def sp(s):
            parts = s.split(d) if d else [s]
            idx = n - 1 if n > 0 else len(parts) + n
            return parts[idx] if 0 <= idx < len(parts) and n != 0 else ""
        return sp
    if name == "substr_index":
        d, n = opts
        n = int(n)

        def si(s):
            if not s or not d or n == 0:
                return ""
            return d.join(s.split(d)[:n]) if n > 0 else d.join(s.rsplit(d)[n:])
        return si
    if name == "strpos":
        sub = opts[0]
        return lambda s: s.find(sub) + 1
    if name == "ascii":
        return lambda s: ord(s[0]) if s else 0
    if name == "octet_length":
        return lambda s: len(s.encode("utf-8"))
    raise KeyError(name)


def _dev_bytes(s: str, device) -> torch.Tensor:
    from .strings import _consts
    b = s.encode("utf-8")
    key = ("strfn_arg", s, str(device))
    return _consts(key, lambda: torch.tensor(list(b) or [0], dtype=torch.uint8).to(device))


def apply(col: Column, name: str, opts: tuple) -> Column:
    """string -> string function ``name`` with constant options."""
    from .strings import _dict_transform, decode
    fn = py_fn(name, opts)
    if col.is_dict:
        return _dict_transform(col, fn, lambda d: apply(d, name, opts))
    if not is_gpu(col.data):
        vals = [None if v is None else fn(v) for v in col.to_arrow().to_pylist()]
        c = Column.from_arrow(pa.array(vals, pa.large_string()), device=col.device, dict_encode=False)
        c.valid = col.valid
        return c
    n = len(col)
    code = CODES[name]
    n1, a, b = 0, "", ""
    if name == "trim":
        n1, a = opts
    elif name == "replace":
        a, b = opts
    elif name in ("lpad", "rpad"):
        n1, a = int(opts[0]), opts[1]
    elif name in ("repeat", "left", "right"):
        n1 = int(opts[0])
    elif name == "translate":
        a, b = opts
    elif name in ("split_part", "substr_index"):
        a, n1 = opts[0], int(opts[1])
    ta, tb = _dev_bytes(a, col.device), _dev_bytes(b, col.device)
    la, lb = len(a.encode("utf-8")), len(b.encode("utf-8"))
    N = launch("str_fn")
    s = stream(col.data)
    lens = torch.empty(n, dtype=torch.int64, device=col.device)
    N.str_fn_lengths(code, n1, ptr(ta), la, ptr(tb), lb, ptr(col.offsets), ptr(col.data), n, ptr(lens), s)
    off, total = offsets_from_lengths(lens)
    chars = torch.empty(max(total, 1), dtype=torch.uint8, device=col.device)[:total]
    if total:
        N.str_fn_copy(code, n1, ptr(ta), la, ptr(tb), lb, ptr(col.offsets), ptr(col.data), n, ptr(off),
                      ptr(chars), int(chars.numel()), s)
    return Column(T.UTF8, chars, col.valid, offsets=off)


def apply_int(col: Column, name: str, opts: tuple) -> torch.Tensor:
    """string -> int32 function (NULL rows: 0; the caller keeps the validity)."""
    from .strings import _dict_lut_dev, _lut_apply
    fn = py_fn(name, opts)
    if col.is_dict:
        key = ("strfn_int", name) + tuple(opts)
        if is_gpu(col.data):
            return _dict_lut_dev(col, key, lambda d: apply_int(d, name, opts)).to(torch.int32)
        return _lut_apply(col, lambda: [0 if v is None else fn(v) for v in col.dict_values()], key).to(torch.int32)
    if not is_gpu(col.data):
        vals = [0 if v is None else fn(v) for v in col.to_arrow().to_pylist()]
        return torch.tensor(vals, dtype=torch.int32, device=col.device)
    n = len(col)
    pat = opts[0] if name == "strpos" else ""
    tp = _dev_bytes(pat, col.device)
    out = torch.empty(n, dtype=torch.int32, device=col.device)
    launch("str_fn_int").str_fn_int(INT_CODES[name], ptr(tp), len(pat.encode("utf-8")), ptr(col.offsets),
                                    ptr(col.data), n, ptr(out), stream(out))
    return out


# ------------------------------------------------- two string operands per row
def _py_levenshtein(a: str, b: str) -> int:
    if len(a) > len(b):
        a, b = b, a
    row = list(range(len(a) + 1))
    for i, cb in enumerate(b, 1):
        diag, row[0] = row[0], i
        for j, ca in enumerate(a, 1):
            diag, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, diag + (ca != cb))
    return row[len(a)]


def py_fn2(name: str) -> Callable[[str, str], object]:
    """Python definition of a two-operand function (the CPU engine and the
    binder's constant folding)."""
    if name == "levenshtein":
        return _py_levenshtein
    if name == "strpos":
        return lambda a, b: a.find(b) + 1
    if name == "contains":
        return lambda a, b: b in a
    if name == "starts_with":
        return lambda a, b: a.startswith(b)
    if name == "ends_with":
        return lambda a, b: a.endswith(b)
    if name == "find_in_set":
        def fis(a, lst):
            parts = lst.split(",")
            return parts.index(a) + 1 if a in parts else 0
        return fis
    raise KeyError(name)


def apply_pair(a, b, name: str, n: Optional[int] = None):
    """Two-operand function ``name`` over ``n`` rows: (result tensor, combined
    validity or None). int32 for levenshtein / strpos / find_in_set, bool for
    contains / starts_with / ends_with; NULL rows hold an unspecified value.
    An operand is a string column or a Python ``str`` (a constant); a one-row
    column is broadcast when ``n`` says so. A dictionary column against a
    constant runs over its dictionary and maps the result through the codes;
    two columns are decoded and walked row by row (strpair.hip)."""
    from .strings import _dict_lut_dev, const_column, decode
    dev = (a if isinstance(a, Column) else b).device
    const_a, const_b = isinstance(a, str), isinstance(b, str)
    ca = const_column(a, dev) if const_a else a
    cb = const_column(b, dev) if const_b else b
    if n is None:
        n = len(cb) if const_a else len(ca) if const_b else max(len(ca), len(cb))
    ba, bb = len(ca) == 1 and n != 1, len(cb) == 1 and n != 1
    va = None if ca.valid is None else (ca.valid.expand(n) if ba else ca.valid)
    vb = None if cb.valid is None else (cb.valid.expand(n) if bb else cb.valid)
    valid = va if vb is None else (vb if va is None else va & vb)
    valid = valid.contiguous() if valid is not None else None
    as_bool = name in PAIR_BOOL
    if not is_gpu(ca.data) or not is_gpu(cb.data):
        fn = py_fn2(name)
        xs, ys = ca.to_arrow().to_pylist(), cb.to_arrow().to_pylist()
        xs, ys = (xs * n if ba else xs), (ys * n if bb else ys)
        vals = [0 if x is None or y is None else fn(x, y) for x, y in zip(xs, ys)]
        return torch.tensor(vals, dtype=torch.bool if as_bool else torch.int32, device=dev), valid
    if const_b and ca.is_dict and not const_a:
        out = _dict_lut_dev(ca, ("strpair", name, 0, b), lambda d: _lut_build(d, cb, False, name))
    elif const_a and cb.is_dict and not const_b:
        out = _dict_lut_dev(cb, ("strpair", name, 1, a), lambda d: _lut_build(ca, d, True, name))
    else:
        out = _pair_dev(decode(ca), decode(cb), ba, bb, n, name)
    return (out != 0 if as_bool else out), valid


def _lut_build(a: Column, b: Column, const_first: bool, name: str) -> torch.Tensor:
    """Per-entry result over a dictionary (the other side a one-row
    constant). Outside a graph capture the table is kept on the dictionary
    (strings.py _dict_lut_dev), so its readback (levenshtein's long-row
    counter) is a one-time build and stays out of the speculation log."""
    from ._lib import capturing, unlogged
    n = len(a) if not const_first else len(b)
    ba, bb = const_first and n != 1, (not const_first) and n != 1
    if capturing() or name != "levenshtein":
        return _pair_dev(a, b, ba, bb, n, name)
    with unlogged():
        return _pair_dev(a, b, ba, bb, n, name)


def _pair_dev(a: Column, b: Column, ba: bool, bb: bool, n: int, name: str) -> torch.Tensor:
    """int32 result of ``name`` over plain device string columns (0 / 1 for
    the boolean functions); ``ba`` / ``bb``: that side is one row for all."""
    from ._lib import to_host_ints
    dev = a.device
    out = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return out
    s = stream(out)
    sides = (ptr(a.offsets), ptr(a.data), ba, ptr(b.offsets), ptr(b.data), bb, n)
    if name != "levenshtein":
        launch("str_pair").str_pair_int(PAIR_CODES[name], *sides, ptr(out), s)
        return out
    # rows whose DP row fits LDS are answered at once; the kernel counts the
    # others (written as -1) and the longest shorter side among them
    left = torch.zeros(2, dtype=torch.int64, device=dev)
    launch("str_lev").str_levenshtein(*sides, ptr(out), ptr(left), s)
    rows, longest = to_host_ints(left)
    if rows:
        # one slab of (longest + 1) int32 cells per worker lane, LEV_LONG_SCRATCH
        # bytes at the most in all (a single slab longer than that: one lane)
        cells = longest + 1
        lanes = max(1, min(LEV_LONG_LANES, -(-rows // 64) * 64, LEV_LONG_SCRATCH // (4 * cells)))
        scratch = torch.empty(lanes * cells, dtype=torch.int32, device=dev)
        launch("str_lev").str_levenshtein_long(*sides, ptr(out), ptr(scratch), lanes, cells, s)
    return out


# --------------------------------------------------------------------- regexps
def _re_flags(flags: str) -> str:
    return "".join(f for f in flags if f in "imsx")


def regexp(col: Column, name: str, pattern: str, repl: Optional[str] = None, flags: str = "", start: int = 1):
    """regexp_like (bool tensor), regexp_count (int64 tensor; counting from
    the ``start``-th character), regexp_replace (Column). Device columns walk
    a DFA of the pattern (csrc/kernels/regex.hip) where the pattern, the
    flags and the replacement allow it; everything else is evaluated by the
    host regex engine over the column's values (dictionary columns: over the
    dictionary only) and reported as a host step."""
    from .strings import note_host_step
    from ..utils.errors import PlanError
    try:
        re.compile(pattern)
    except re.error as e:
        raise PlanError(f"invalid regular expression {pattern!r}: {e}") from None
    if name == "regexp_like" and set(flags) <= {"i", "c"} and col.data.is_cuda:
        m = _regexp_like_gpu(col, pattern, "i" in flags and not flags.endswith("c"))
        if m is not None:
            return m
    if name == "regexp_count" and set(flags) <= {"i", "c"} and col.data.is_cuda:
        m = _regexp_count_gpu(col, pattern, "i" in flags, start)
        if m is not None:
            return m
    if name == "regexp_replace" and set(flags) <= {"g", "i", "c"} and col.data.is_cuda \
            and not set(repl or "") & {"$", "\\"}:
        # ('$' / '\' in the replacement: group references and the engines'
        # own escapes, all left to the host engine)
        m = _regexp_replace_gpu(col, pattern, repl or "", "i" in flags, "g" in flags)
        if m is not None:
            return m
    note_host_step(name)
    fl = _re_flags(flags)
    pat = f"(?{fl}){pattern}" if fl else pattern

    def subject(arr):
        return pc.utf8_slice_codeunits(arr, start - 1) if start > 1 else arr
    if col.is_dict:
        vals = col.dict_values()
        d = col.dictionary
        arr = subject(pa.array(vals, pa.large_string()))
        res = _regexp_arrow(arr, name, pat, repl, flags)
        if name == "regexp_replace":
            from .strings import _lut_apply
            uniq, remap = {}, []
            for v in res.to_pylist():
                remap.append(uniq.setdefault(v, len(uniq)))
            nd = Column.from_arrow(pa.array(list(uniq), pa.large_string()), device=col.device, dict_encode=False)
            codes = _lut_apply(col, remap, ("re_remap", pattern, repl, flags)).to(torch.int32)
            return Column(T.UTF8, codes, col.valid, dictionary=nd)
        lut = torch.tensor([0 if v is None else int(v) for v in res.to_pylist()] or [0], dtype=torch.int64,
                           device=col.device)
        out = lut.index_select(0, col.data.to(torch.int64).clamp(min=0)) if len(col) else lut[:0]
        return out.to(torch.bool) if name == "regexp_like" else out
    arr = subject(col.to_arrow())
    res = _regexp_arrow(arr, name, pat, repl, flags)
    if name == "regexp_replace":
        c = Column.from_arrow(res.cast(pa.large_string()), device=col.device, dict_encode=False)
        c.valid = col.valid
        return c
    t = torch.tensor(res.cast(pa.int64()).fill_null(0).to_numpy(zero_copy_only=False), device=col.device)
    return t.to(torch.bool) if name == "regexp_like" else t


def _regexp_like_gpu(col: Column, pattern: str, icase: bool) -> Optional[torch.Tensor]:
    """regexp_like on the device: the pattern as a byte DFA (ops/regex_dfa.py)
    walked by csrc/kernels/regex.hip, one lane per string (dictionary columns:
    per dictionary entry, then the codes gather the flags). None when the
    pattern needs the host engine."""
    from . import regex_dfa as RD
    from .gather import gather_tensor
    from .strings import decode
    try:
        d = RD.compile_dfa(pattern, icase)
    except (RD.Unsupported, RecursionError):
        return None
    if native().regex_lds_bytes(d.nstates, d.nclasses) > 64 * 1024:
        return None
    dev = col.device
    src = col.dictionary if col.is_dict else (col if col.is_plain_string else decode(col))
    n = len(src)
    table = torch.tensor([x for row in d.table for x in row], dtype=torch.int32).to(torch.int16).to(dev)
    cls = torch.tensor(d.cls, dtype=torch.uint8).to(dev)
    flg = torch.tensor(d.accept, dtype=torch.uint8).to(dev)
    out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[:n]
    launch("regex_dfa").regex_dfa_match(ptr(src.offsets), ptr(src.data), n, ptr(table), ptr(cls), ptr(flg),
                                        d.nstates, d.nclasses, d.start, d.anchored_end, False, ptr(out),
                                        stream(out))
    m = out.view(torch.bool)
    if col.is_dict:
        m = gather_tensor(m, col.data) if len(col) else m[:0]
    return m


# Match spans on the device (regex.hip regex_span_*): regexp_count,
# regexp_replace with a literal replacement and regexp_match without capture
# groups. Each helper returns None when the call needs the host engine: the
# pattern has no span automaton (ops/regex_dfa.py compile_span_dfa), or a row
# ran out of its lookup budget in the kernel.
def _span_dfa(pattern: str, icase: bool, dev):
    """(automaton, its device tables as the kernels' argument) or None."""
    from . import regex_dfa as RD
    from .strings import _consts
    try:
        d = RD.compile_span_dfa(pattern, icase)
    except (RD.Unsupported, RecursionError):
        return None
    if native().regex_lds_bytes(d.nstates, d.nclasses) > 64 * 1024:
        return None
    t = _consts(("span_dfa", pattern, icase, str(dev)), lambda: (
        torch.tensor([x for row in d.table for x in row], dtype=torch.int32).to(torch.int16).to(dev),
        torch.tensor(d.cls, dtype=torch.uint8).to(dev),
        torch.tensor(d.accept, dtype=torch.uint8).to(dev)))
    return d, (ptr(t[0]), ptr(t[1]), ptr(t[2]), d.nstates, d.nclasses, d.anchored_start, d.anchored_end)


def _plain(col: Column) -> Column:
    """The plain string column the kernels walk: a dictionary column's
    dictionary (the caller maps the result through the codes)."""
    from .strings import decode
    src = col.dictionary if col.is_dict else col
    return src if src.is_plain_string else decode(src)


def _sizes(lens: torch.Tensor, exhausted: torch.Tensor):
    """Offsets of ``lens``, their total and the kernels' count of rows that
    ran out of budget: one logged readback for both."""
    from ._lib import to_host_ints
    off, total = offsets_from_lengths(lens, host_total=False)
    total, ex = to_host_ints(torch.cat([total, exhausted]))
    return off, total, ex


def span_count(src: Column, dfa, start: int = 1) -> Optional[torch.Tensor]:
    """Matches per row of a plain device string column (int64)."""
    from ._lib import to_host_int
    n = len(src)
    out = torch.empty(n, dtype=torch.int64, device=src.device)
    ex = torch.zeros(1, dtype=torch.int64, device=src.device)
    launch("regex_span_count").regex_span_count(dfa, ptr(src.offsets), ptr(src.data), n, True, -1,
                                                int(start), ptr(out), ptr(ex), stream(out))
    return None if to_host_int(ex) else out


def span_replace(src: Column, dfa, repl: str, all: bool) -> Optional[Column]:
    """The first (``all``: every) match of each row replaced by the literal
    ``repl``: count -> scan -> write, as ``apply``."""
    n = len(src)
    dev = src.device
    rb = _dev_bytes(repl, dev)
    lr = len(repl.encode("utf-8"))
    s = stream(src.data)
    lens = torch.empty(n, dtype=torch.int64, device=dev)
    ex = torch.zeros(1, dtype=torch.int64, device=dev)
    launch("regex_span_count").regex_span_count(dfa, ptr(src.offsets), ptr(src.data), n, all, lr, 1, ptr(lens),
                                                ptr(ex), s)
    off, total, exhausted = _sizes(lens, ex)
    if exhausted:
        return None
    chars = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    if total:
        launch("regex_span_replace").regex_span_replace(dfa, ptr(src.offsets), ptr(src.data), n, all, ptr(rb), lr,
                                                        ptr(off), ptr(chars), int(chars.numel()), s)
    return Column(T.UTF8, chars, src.valid, offsets=off)


def span_first(src: Column, dfa):
    """(the first match of each row as a string column, '' where there is
    none; bool tensor: the row has a match) or None."""
    from ._lib import to_host_int
    n = len(src)
    dev = src.device
    s = stream(src.data)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    mlen = torch.empty(n, dtype=torch.int64, device=dev)
    ex = torch.zeros(1, dtype=torch.int64, device=dev)
    launch("regex_span_first").regex_span_first(dfa, ptr(src.offsets), ptr(src.data), n, ptr(pos), ptr(mlen),
                                                ptr(ex), s)
    if to_host_int(ex):
        return None
    return span_gather(src.data, pos, mlen), mlen >= 0


def span_gather(chars: torch.Tensor, pos: torch.Tensor, mlen: torch.Tensor) -> Column:
    """The byte spans [pos, pos + max(mlen, 0)) of ``chars`` (ascending, not
    overlapping: one per row of a column) as a string column. The span ends
    are laid out as the offsets [pos0, end0, pos1, end1, ..] of a column over
    the same bytes whose even rows are the spans, and those rows are taken
    with the string gather (gather.hip str_gather_*): its copy is bounded by
    the capacity of the buffer sized from the logged readback."""
    from .gather import take
    n = pos.numel()
    if n == 0:
        return Column(T.UTF8, chars[:0], None, offsets=torch.zeros(1, dtype=torch.int64, device=pos.device))
    bounds = torch.stack([pos, pos + mlen.clamp(min=0)], 1).reshape(-1)
    rows = torch.arange(0, 2 * n, 2, dtype=torch.int64, device=pos.device)
    return take(Column(T.UTF8, chars, None, offsets=bounds), rows)


def _regexp_count_gpu(col: Column, pattern: str, icase: bool, start: int) -> Optional[torch.Tensor]:
    from .gather import gather_tensor
    dfa = _span_dfa(pattern, icase, col.device)
    if dfa is None:
        return None
    cnt = span_count(_plain(col), dfa[1], start)
    if cnt is None or not col.is_dict:
        return cnt
    if cnt.numel() == 0:
        return torch.zeros(len(col), dtype=torch.int64, device=col.device)
    return gather_tensor(cnt, col.data)


def _regexp_replace_gpu(col: Column, pattern: str, repl: str, icase: bool, all: bool) -> Optional[Column]:
    from .strings import _dict_transform
    dfa = _span_dfa(pattern, icase, col.device)
    if dfa is None:
        return None
    res = span_replace(_plain(col), dfa[1], repl, all)
    if res is None:
        return None
    if col.is_dict:
        # replaced entries may coincide: re-encoded on the device
        return _dict_transform(col, None, lambda d: res)
    res.valid = col.valid
    return res


def regexp_match_gpu(col: Column, pattern: str, icase: bool, dtype) -> Optional[Column]:
    """regexp_match of a pattern without capture groups: LIST<UTF8> of the
    first match, NULL where there is none."""
    from ..columnar import Nested
    dfa = _span_dfa(pattern, icase, col.device)
    if dfa is None:
        return None
    res = span_first(_plain(col), dfa[1])
    if res is None:
        return None
    child, hit = res
    n = len(col)
    if col.is_dict:
        codes = col.data.to(torch.int64).clamp(min=0)
        hit = hit.index_select(0, codes) if hit.numel() else torch.zeros(n, dtype=torch.bool, device=col.device)
        se = torch.stack([codes, torch.ones_like(codes)], 1).contiguous()
    else:
        se = torch.empty((n, 2), dtype=torch.int64, device=col.device)
        launch("list_slots").list_slots(n, 1, ptr(se), stream(se))
    valid = hit if col.valid is None else hit & col.valid
    return Column(dtype, se, valid, dictionary=Nested(child=child))


def _has_start_anchor(pat: str) -> bool:
    """``pat`` holds ``^`` (outside a character class) or ``\\A``."""
    i, in_class = 0, False
    while i < len(pat):
        c = pat[i]
        if c == "\\":
            if not in_class and pat[i + 1:i + 2] == "A":
                return True
            i += 2
            continue
        if in_class:
            in_class = c != "]"
        elif c == "[":
            in_class = True
            i += 2 if pat[i + 1:i + 2] == "^" else 1       # [^..] negates, []..] / [^]..] start with a literal ]
            if pat[i:i + 1] == "]":
                i += 1
            continue
        elif c == "^":
            return True
        i += 1
    return False


def _regexp_arrow(arr, name, pat, repl, flags):
    if name == "regexp_like":
        return pc.match_substring_regex(arr, pat)
    if name == "regexp_count":
        if _has_start_anchor(pat):
            # count_substring_regex searches the rest of the value again after
            # each match, where '^' would match once more ('^a' in 'aaa': 3).
            # Anchored patterns are counted over the whole value instead
            # (ASCII digit / word / space classes as RE2, ASCII case folding as the kernels).
            rx = re.compile(pat, re.ASCII)
            return pa.array([None if v is None else sum(1 for _ in rx.finditer(v)) for v in arr.to_pylist()],
                            pa.int64())
        return pc.count_substring_regex(arr, pat)
    # Rust-regex replacement syntax ${1} / $1 -> RE2 \1
    r = re.sub(r"\$\{(\d+)\}|\$(\d+)", lambda m: "\\" + (m.group(1) or m.group(2)), repl or "")
    return pc.replace_substring_regex(arr, pat, r, max_replacements=None if "g" in flags else 1)
