"""String functions whose extra arguments vary per row: substr / left / right /
split_part / repeat / lpad / rpad / replace / overlay / chr / to_hex
(``apply_rows``), LIKE with a per-row pattern (``like_rows``) and greatest /
least over strings (``compare_rows``, ``extreme_rows``).

An operand is a ``Column``, or a Python ``str`` / ``int`` constant that stays a
constant; ``None`` is the NULL constant. Dictionary operands are decoded, as
in ``strfuncs.apply_pair``. The result is NULL where any operand is.

``apply_rows`` and ``like_rows`` run on the CPU engine only, through the Python
definitions below, built from the literal forms' (``strfuncs.py_fn``,
``strings._py_substr``): per-row and literal calls share one definition. On a
device column they raise ``NotSupported``: there is no kernel for them and no
fall-back. The three-way compare behind greatest / least is a device kernel
(csrc/kernels/strrow.hip ``str_row_cmp``); the chosen rows are assembled by
``strings.select_rows``. Parity with DataFusion (reference Cargo.lock:1062
datafusion-functions 48.0.0) is unpinned; these definitions are the contract.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Union

import pyarrow as pa
import torch

from .. import types as T
from ..columnar import Column
from ..utils.errors import ExecutionError
from ._lib import is_gpu, launch, ptr, stream

#: (string operands, least and most integer operands)
ARITY = {"substr": (1, 1, 2), "left": (1, 1, 1), "right": (1, 1, 1), "split_part": (2, 1, 1), "repeat": (1, 1, 1),
         "lpad": (2, 1, 1), "rpad": (2, 1, 1), "replace": (3, 0, 0), "overlay": (2, 1, 2), "chr": (0, 1, 1),
         "to_hex": (0, 1, 1)}
#: bytes of one result row
ROW_MAX = 2**31 - 1

Operand = Union[Column, str, int, None]


# ------------------------------------------------------------ Python semantics
def _too_long(name: str):
    return ValueError(f"{name}(): the result is longer than {ROW_MAX} bytes")


def py_row(name: str) -> Callable[[Sequence[str], Sequence[int]], str]:
    """One row of ``name`` over its string and integer arguments: the literal
    form's definition with that row's arguments. Raises ValueError for a row
    that has no result (an invalid code point, a result past ROW_MAX)."""
    from .strfuncs import py_fn
    from .strings import _py_substr
    if name == "substr":
        return lambda s, k: _py_substr(s[0], k[0], k[1] if len(k) > 1 else None)
    if name in ("left", "right"):
        return lambda s, k: py_fn(name, (k[0],))(s[0])
    if name == "split_part":
        return lambda s, k: py_fn(name, (s[1], k[0]))(s[0])
    if name == "repeat":
        def rep(s, k):
            if len(s[0].encode("utf-8")) * max(k[0], 0) > ROW_MAX:
                raise _too_long(name)
            return py_fn(name, (k[0],))(s[0])
        return rep
    if name in ("lpad", "rpad"):
        def pad(s, k):
            if s[1] and k[0] - len(s[0]) > ROW_MAX:       # a fill character is a byte at the least
                raise _too_long(name)
            out = py_fn(name, (k[0], s[1]))(s[0])
            if len(out.encode("utf-8")) > ROW_MAX:
                raise _too_long(name)
            return out
        return pad
    if name == "replace":
        return lambda s, k: py_fn(name, (s[1], s[2]))(s[0])
    if name == "overlay":
        def overlay(s, k):
            a, b = k[0], (k[1] if len(k) > 1 else len(s[1]))
            return _py_substr(s[0], 1, a - 1) + s[1] + _py_substr(s[0], a + b, None)
        return overlay
    if name == "chr":
        def chr_(s, k):
            n = k[0]
            if n <= 0 or n > 0x10FFFF or 0xD800 <= n <= 0xDFFF:
                raise ValueError(f"chr(): {n} is not a valid code point")
            return chr(n)
        return chr_
    if name == "to_hex":
        return lambda s, k: format(k[0] & (2**64 - 1), "x")
    raise KeyError(name)


def py_like(x: str, p: str, escape: str) -> bool:
    from .strings import like_regex
    return like_regex(p, False, escape or None).fullmatch(x) is not None


def _no_kernel(what: str):
    from ..utils.errors import NotSupported
    return NotSupported(f"{what} on a device column (the CPU engine evaluates it)")


def _on_device(operands) -> bool:
    return any(isinstance(x, Column) and is_gpu(x.data) for x in operands)


def _row_error(name: str, row: int) -> ExecutionError:
    what = "invalid code point" if name == "chr" else f"result longer than {ROW_MAX} bytes"
    return ExecutionError(f"{name}(): {what} at row {row}")


# ------------------------------------------------------------------- operands
class _Ops:
    """The operands of one call over ``n`` rows of the CPU engine: plain string
    columns and int64 tensors with their broadcast flags, and the combined validity."""

    def __init__(self, strs: Sequence[Operand], ints: Sequence[Operand], n: int):
        from .strings import const_column, decode
        cols = [x for x in list(strs) + list(ints) if isinstance(x, Column)]
        if not cols:
            raise ValueError("per-row string function without a column operand")
        self.n = n
        self.device = dev = cols[0].device
        self.all_null = any(x is None for x in list(strs) + list(ints))
        self.strs: List[Column] = []
        self.ints: List[torch.Tensor] = []
        self.bs: List[bool] = []
        self.bk: List[bool] = []
        valid = None
        for x in strs:
            c = decode(x) if isinstance(x, Column) else const_column(x or "", dev)
            b = len(c) == 1 and n != 1
            valid = self._and(valid, c.valid, b)
            self.strs.append(c)
            self.bs.append(b)
        for k in ints:
            if isinstance(k, Column):
                t = k.data.to(torch.int64).contiguous()
                b = t.numel() == 1 and n != 1
                valid = self._and(valid, k.valid, b)
            else:
                t, b = torch.tensor([int(k or 0)], dtype=torch.int64, device=dev), True
            self.ints.append(t)
            self.bk.append(b)
        self.valid = valid.contiguous() if valid is not None else None

    def _and(self, valid, v, broadcast):
        if v is None:
            return valid
        v = v.expand(self.n) if broadcast else v
        return v if valid is None else valid & v

    def py_strs(self) -> List[list]:
        return [c.to_arrow().to_pylist() * (self.n if b else 1) for c, b in zip(self.strs, self.bs)]

    def py_ints(self) -> List[list]:
        return [t.tolist() * (self.n if b else 1) for t, b in zip(self.ints, self.bk)]

    def py_valid(self) -> list:
        return [True] * self.n if self.valid is None else self.valid.tolist()


def _null_strings(n: int, dev) -> Column:
    return Column.full(None, T.UTF8, n, dev)


def _from_py(vals: list, dev) -> Column:
    return Column.from_arrow(pa.array(vals, pa.large_string()), device=dev, dict_encode=False)


# -------------------------------------------------------------- apply_rows
def apply_rows(name: str, strs: Sequence[Operand], ints: Sequence[Operand], n: int) -> Column:
    """``name`` over ``n`` rows of its string operands ``strs`` and integer
    operands ``ints`` (lpad / rpad without a fill: pass ' ')."""
    ns, lo, hi = ARITY[name]
    if len(strs) != ns or not lo <= len(ints) <= hi:
        raise ValueError(f"{name}(): {len(strs)} string and {len(ints)} integer operands")
    if _on_device(list(strs) + list(ints)):
        raise _no_kernel(f"{name}() with a per-row argument")
    o = _Ops(strs, ints, n)
    if o.all_null:
        return _null_strings(n, o.device)
    return _apply_py(name, o)


def _apply_py(name: str, o: _Ops) -> Column:
    fn = py_row(name)
    ss, ks, ok = o.py_strs(), o.py_ints(), o.py_valid()
    vals = []
    for i in range(o.n):
        if not ok[i]:
            vals.append(None)
            continue
        try:
            vals.append(fn([x[i] for x in ss], [k[i] for k in ks]))
        except ValueError:
            raise _row_error(name, i) from None
    c = _from_py(vals, o.device)
    c.valid = o.valid
    return c


# --------------------------------------------------------------- like_rows
def escape_byte(escape: Optional[str], what: str = "LIKE") -> int:
    """The escape of a per-row LIKE: one ASCII byte, 0 for none."""
    from ..utils.errors import NotSupported
    if not escape:
        return 0
    if len(escape) != 1 or ord(escape) > 127:
        raise NotSupported(f"{what} with a per-row pattern: the escape must be a single ASCII character")
    return ord(escape)


def like_rows(x: Operand, p: Operand, escape: Optional[str], negated: bool, n: int) -> Column:
    """``x [NOT] LIKE p`` over ``n`` rows, the pattern read per row; NULL where either side is."""
    escape_byte(escape)
    if _on_device([x, p]):
        raise _no_kernel("LIKE with a per-row pattern")
    o = _Ops([x, p], [], n)
    if o.all_null:
        return Column.full(None, T.BOOL, n, o.device)
    (xs, ps), ok = o.py_strs(), o.py_valid()
    vals = [ok[i] and (py_like(xs[i], ps[i], escape or "") != negated) for i in range(n)]
    return Column(T.BOOL, torch.tensor(vals, dtype=torch.bool, device=o.device), o.valid)


# ------------------------------------------------------- compare / extremes
def compare_rows(a: Column, b: Column, n: int) -> torch.Tensor:
    """Byte-wise three-way compare per row of two string columns (a one-row
    column is a constant when ``n`` says so): int32 -1 / 0 / 1, a shorter
    prefix first. NULL rows hold an unspecified value (the caller keeps the
    validity). Device columns: strrow.hip str_row_cmp over the decoded sides."""
    from .strings import decode
    a, b = decode(a), decode(b)
    ba, bb = len(a) == 1 and n != 1, len(b) == 1 and n != 1
    dev = a.device
    if not is_gpu(a.data) or not is_gpu(b.data):
        xs, ys = a.to_arrow().to_pylist(), b.to_arrow().to_pylist()
        xs, ys = (xs * n if ba else xs), (ys * n if bb else ys)
        keys = [((u or "").encode("utf-8"), (v or "").encode("utf-8")) for u, v in zip(xs, ys)]
        return torch.tensor([(u > v) - (u < v) for u, v in keys], dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        launch("str_row_cmp").str_row_cmp(ptr(a.offsets), ptr(a.data), ba, ptr(b.offsets), ptr(b.data), bb, n, ptr(out),
                                          stream(out))
    return out


def extreme_rows(args: Sequence[Column], greatest: bool, n: int) -> Column:
    """greatest / least over string columns (a one-row column is a constant):
    NULL arguments are skipped, the result is NULL only where all are. Each
    argument is compared with the ones before it, the comparison against the
    row's best so far is picked by the choice index, and one string gather
    (``strings.select_rows``) assembles the result."""
    from .strings import select_rows
    dev = args[0].device

    def ok_of(c: Column) -> torch.Tensor:
        if c.valid is None:
            return torch.ones(n, dtype=torch.bool, device=dev)
        return c.valid.expand(n) if len(c) == 1 and n != 1 else c.valid
    choice = torch.zeros(n, dtype=torch.int64, device=dev)
    valid = ok_of(args[0])
    for k in range(1, len(args)):
        cmps = torch.stack([compare_rows(args[k], args[j], n) for j in range(k)])
        c = cmps.gather(0, choice.unsqueeze(0))[0]
        ok = ok_of(args[k])
        take_k = ok & (~valid | (c > 0 if greatest else c < 0))
        choice = torch.where(take_k, torch.full_like(choice, k), choice)
        valid = valid | ok
    return select_rows(list(args), choice, n)
