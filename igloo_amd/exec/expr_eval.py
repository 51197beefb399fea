"""Vectorized evaluation of bound expressions over a device ``Batch``.

Numeric work is elementwise torch on the batch's device (fully on-GPU for
GPU batches); string predicates/transforms, date parts, gathers and
hash-based operators dispatch to the gfx950 kernels in ``igloo_amd.ops``.
NULLs follow SQL three-valued logic via validity masks.

Parity: DataFusion ``PhysicalExpr::evaluate`` as called by the reference's
FilterExec / ProjectionExec (reference crates/engine/src/operators/filter.rs:47,
projection.rs:60-64).
"""
from __future__ import annotations

import math
import os
from typing import Any, Optional, Tuple, Union

import numpy as np
import re

import pyarrow as pa
import pyarrow.compute as pc
import torch

from .. import types as T
from ..columnar import Batch, Column, batch_device
from ..ops import misc as M
from ..ops._lib import to_host_ints
from ..ops import strings as S
from ..sql.expr import (AggCall, BinOp, Case, Cast, ColRef, Expr, Func, InList, IsNull, Like, Lit, Neg, Not,
                        SubqueryExpr, col_refs)
from ..types import DataType
from ..utils.errors import ExecutionError, NotSupported

#: generated expression kernels (exec/expr_jit.py) for composite expressions
#: over GPU batches of at least this many rows
JIT_MIN_ROWS = 1
_JIT_ROOTS = {BinOp, Case, Cast, Func, Not, Neg, IsNull, InList}
_JIT_ON_CPU = False   # tests: run the generator (source collection only) on CPU batches


_NESTED = ("make_array", "struct", "array_length", "array_element", "get_field", "array_has", "array_to_string",
           "regexp_match", "unnest")
#: the array_* family (ops/nested.py): index arithmetic over (start, length) rows plus one child gather
_LIST_FAMILY = ("array_slice", "array_pop_front", "array_pop_back", "array_empty", "array_append", "array_prepend",
                "array_concat", "array_reverse", "array_repeat", "array_resize", "flatten", "array_position",
                "array_positions", "array_has_expr", "array_has_all", "array_has_any", "array_remove",
                "array_replace", "array_max", "array_min", "array_distinct", "array_union", "array_intersect",
                "array_except", "array_sort", "list_cast")
#: the MAP family (ops/nested.py): views over the key / value children, the lookup kernel, construction
_MAP_FAMILY = ("make_map", "map_from_lists", "map_keys", "map_values", "map_entries", "map_element", "map_extract")
_NESTED = _NESTED + _LIST_FAMILY + _MAP_FAMILY


class Scalar:
    __slots__ = ("value", "dtype")

    def __init__(self, value: Any, dtype: DataType):
        self.value = value
        self.dtype = dtype

    def __repr__(self):
        return f"Scalar({self.value!r}, {self.dtype})"


Value = Union[Column, Scalar]


def _and_valid(a: Optional[torch.Tensor], b: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if a is None:
        return b
    if b is None:
        return a
    return a & b


class Evaluator:
    def __init__(self, ctx=None):
        self.ctx = ctx

    # ------------------------------------------------------------------ entry
    _jit_off = 0   # > 0 while a generated kernel's uncovered subtree is evaluated here

    def eval(self, e: Expr, b: Batch) -> Value:
        if not self._jit_off and type(e) in _JIT_ROOTS and b.num_rows >= JIT_MIN_ROWS and b.columns \
                and (_JIT_ON_CPU or getattr(batch_device(b), "type", None) == "cuda"):
            from . import expr_jit
            r = expr_jit.evaluate(e, b, self)
            if isinstance(r, Column):
                return r
            if r is expr_jit.PENDING:
                # compiling in the background: this run goes node by node without
                # generating code for the subtrees as well
                self._jit_off += 1
                try:
                    return self._eval_nodes(e, b)
                finally:
                    self._jit_off -= 1
        return self._eval_nodes(e, b)

    def _eval_nodes(self, e: Expr, b: Batch) -> Value:
        m = getattr(self, "_" + type(e).__name__, None)
        if m is None:
            if isinstance(e, ColRef):
                return self._ColRef(e, b)
            raise NotSupported(f"cannot evaluate {type(e).__name__}")
        return m(e, b)

    @staticmethod
    def prefetch(exprs, b: Batch) -> None:
        """A join result's (LateBatch) columns read by ``exprs``: gathered
        together, part by part, before they are read one by one."""
        pf = getattr(b, "prefetch", None)
        if pf is not None:
            cids = set()
            for e in exprs:
                if e is not None:
                    cids |= col_refs(e)
            if len(cids) > 1:
                pf(cids)

    def column(self, e: Expr, b: Batch) -> Column:
        """Evaluate and broadcast to a full column."""
        self.prefetch((e,), b)
        v = self.eval(e, b)
        if isinstance(v, Scalar):
            return Column.full(v.value, e.dtype if v.dtype.kind == "null" else v.dtype, b.num_rows, self.device(b))
        return v

    def mask(self, e: Expr, b: Batch) -> torch.Tensor:
        """Predicate -> bool tensor (NULL counts as False)."""
        self.prefetch((e,), b)
        v = self.eval(e, b)
        dev = self.device(b)
        if isinstance(v, Scalar):
            return torch.full((b.num_rows,), bool(v.value) if v.value is not None else False, dtype=torch.bool, device=dev)
        m = v.data if v.data.dtype == torch.bool else v.data != 0
        if v.valid is not None:
            m = m & v.valid
        return m

    def device(self, b: Batch) -> torch.device:
        d = batch_device(b)
        if d is not None:
            return d
        return torch.device(self.ctx.device if self.ctx is not None else "cpu")

    # ------------------------------------------------------------ leaf nodes
    def _ColRef(self, e: ColRef, b: Batch) -> Value:
        try:
            return b.columns[e.cid]
        except KeyError:
            raise ExecutionError(f"column {e.sql()} not available in batch {list(b.columns)}") from None

    def _Passthrough(self, e, b):
        return self._ColRef(e, b)

    def _Lit(self, e: Lit, b: Batch) -> Value:
        return Scalar(e.value, e.dtype)

    def _SubqueryExpr(self, e: SubqueryExpr, b: Batch) -> Value:
        if e.kind != "scalar":
            raise ExecutionError("unexpected EXISTS/IN subquery at execution (not decorrelated)")
        if self.ctx is None:
            raise ExecutionError("scalar subquery needs an execution context")
        val = self.ctx.scalar_subquery(e)
        return Scalar(val, e.dtype)

    # ------------------------------------------------------- numeric helpers
    def _num(self, v: Value, t: DataType):
        """Value -> (tensor | python number, validity) in representation of type t."""
        if isinstance(v, Scalar):
            x = v.value
            if x is None:
                return None, None
            return _convert_scalar(x, v.dtype, t), None
        return _convert_tensor(v, t), v.valid

    # ---------------------------------------------------------------- binops
    def _BinOp(self, e: BinOp, b: Batch) -> Value:
        op = e.op
        if op in ("and", "or"):
            return self._logic(e, b)
        l = self.eval(e.left, b)
        r = self.eval(e.right, b)
        if op in ("=", "<>", "<", "<=", ">", ">=", "is_distinct_from", "is_not_distinct_from"):
            return self._compare(op, l, r, e.left.dtype, e.right.dtype, b)
        if isinstance(l, Scalar) and isinstance(r, Scalar):
            from ..sql.binder import _fold
            f = _fold(BinOp(op, Lit(l.value, l.dtype), Lit(r.value, r.dtype), e.dtype))
            if isinstance(f, Lit):
                return Scalar(f.value, f.dtype)
        t = e.dtype
        if t.kind == "date32":
            a, va = self._num(l, T.INT32 if l.dtype.kind == "date32" else T.INT64)
            c, vc = self._num(r, T.INT32 if r.dtype.kind == "date32" else T.INT64)
            out = a + c if op == "+" else a - c
            return self._mk(out, t, _and_valid(va, vc), b)
        lt = t
        if t.is_decimal and op == "*":
            a, va = self._num(l, l.dtype if l.dtype.is_decimal else T.DECIMAL(19, 0))
            c, vc = self._num(r, r.dtype if r.dtype.is_decimal else T.DECIMAL(19, 0))
            if t.precision > 18:
                a, c = _overflow_guard(a, c)
            out = a * c
            return self._mk(out, t, _and_valid(va, vc), b)
        if t.kind == "int64" and op in ("-",) and l.dtype.kind == "date32":
            a, va = self._num(l, T.INT64)
            c, vc = self._num(r, T.INT64)
            return self._mk(a - c, t, _and_valid(va, vc), b)
        a, va = self._num(l, lt)
        c, vc = self._num(r, lt)
        valid = _and_valid(va, vc)
        if a is None or c is None:
            return Scalar(None, t)
        if op == "+":
            out = a + c
        elif op == "-":
            out = a - c
        elif op == "*":
            out = a * c
        elif op == "/":
            if t.is_float:
                out = a / c
                zero = (c == 0) if isinstance(c, torch.Tensor) else None
                if zero is not None and _any(zero):
                    valid = _and_valid(valid, ~zero)
                elif not isinstance(c, torch.Tensor) and c == 0:
                    return Scalar(None, t)
            else:
                if isinstance(c, torch.Tensor):
                    zero = c == 0
                    safe = torch.where(zero, torch.ones_like(c), c)
                    out = torch.div(a, safe, rounding_mode="trunc")
                    if _any(zero):
                        valid = _and_valid(valid, ~zero)
                else:
                    if c == 0:
                        return Scalar(None, t)
                    out = torch.div(a, c, rounding_mode="trunc")
        elif op == "%":
            out = torch.fmod(a, c) if isinstance(a, torch.Tensor) else torch.fmod(torch.as_tensor(a), c)
        else:
            raise NotSupported(f"operator {op}")
        return self._mk(out, t, valid, b)

    def _mk(self, out, t: DataType, valid, b: Batch) -> Value:
        if not isinstance(out, torch.Tensor):
            return Scalar(out, t)
        if out.dim() == 0:
            out = out.expand(b.num_rows)
        return Column(t, out.to(t.torch_dtype) if t.kind != "decimal" else out.to(torch.int64), valid)

    def _logic(self, e: BinOp, b: Batch) -> Value:
        l = self.eval(e.left, b)
        r = self.eval(e.right, b)
        is_and = e.op == "and"
        # scalar short-circuits
        for x, y in ((l, r), (r, l)):
            if isinstance(x, Scalar):
                if x.value is None:
                    if isinstance(y, Scalar):
                        return Scalar(None if (y.value is None or y.value == is_and) else y.value, T.BOOL)
                    # NULL AND y -> (y false -> false else null); NULL OR y -> (y true -> true else null)
                    yv, yvalid = _bool_parts(y)
                    known = (~yv if is_and else yv)
                    if yvalid is not None:
                        known = known & yvalid
                    return Column(T.BOOL, yv if not is_and else torch.zeros_like(yv), known)
                if bool(x.value) == (not is_and):
                    return Scalar(not is_and, T.BOOL)
                return y
        lv, lval = _bool_parts(l)
        rv, rval = _bool_parts(r)
        if is_and:
            out = lv & rv
            if lval is None and rval is None:
                return Column(T.BOOL, out)
            la = lval if lval is not None else torch.ones_like(lv)
            ra = rval if rval is not None else torch.ones_like(rv)
            valid = (la & ra) | (la & ~lv) | (ra & ~rv)
            return Column(T.BOOL, out & la & ra, valid)
        out = lv | rv
        if lval is None and rval is None:
            return Column(T.BOOL, out)
        la = lval if lval is not None else torch.ones_like(lv)
        ra = rval if rval is not None else torch.ones_like(rv)
        valid = (la & ra) | (la & lv) | (ra & rv)
        return Column(T.BOOL, (lv & la) | (rv & ra), valid)

    def _compare(self, op, l: Value, r: Value, lt: DataType, rt: DataType, b: Batch) -> Value:
        if isinstance(l, Scalar) and isinstance(r, Scalar):
            if l.value is None or r.value is None:
                return Scalar(None, T.BOOL)
            import operator as o
            f = {"=": o.eq, "<>": o.ne, "<": o.lt, "<=": o.le, ">": o.gt, ">=": o.ge}[op]
            return Scalar(bool(f(l.value, r.value)), T.BOOL)
        if lt.is_varlen or rt.is_varlen:
            return self._compare_strings(op, l, r, b)
        if isinstance(l, Scalar) and l.value is None or isinstance(r, Scalar) and r.value is None:
            return Scalar(None, T.BOOL)
        t = lt if lt == rt else T.common_numeric(lt, rt)
        rep = T.INT64 if t.kind in ("date32", "timestamp", "bool") else t
        if t.kind == "bool":
            def bpart(v):
                if isinstance(v, Scalar):
                    return int(bool(v.value)), None
                return _bool_parts(v)[0].to(torch.int8), v.valid
            a, va = bpart(l)
            c, vc = bpart(r)
        else:
            a, va = self._num(l, rep)
            c, vc = self._num(r, rep)
        fn = {"=": torch.eq, "<>": torch.ne, "<": torch.lt, "<=": torch.le, ">": torch.gt, ">=": torch.ge}[op]
        if not isinstance(a, torch.Tensor):
            # flip so the tensor is on the left
            flip = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "<>": "<>"}[op]
            fn = {"=": torch.eq, "<>": torch.ne, "<": torch.lt, "<=": torch.le, ">": torch.gt, ">=": torch.ge}[flip]
            a, c = c, a
        out = fn(a, c)
        return Column(T.BOOL, out, _and_valid(va, vc))

    def _compare_strings(self, op, l: Value, r: Value, b: Batch) -> Value:
        if isinstance(r, Scalar) or isinstance(l, Scalar):
            if isinstance(l, Scalar):
                flip = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "<>": "<>"}[op]
                l, r, op = r, l, flip
            if r.value is None:
                return Scalar(None, T.BOOL)
            return Column(T.BOOL, S.compare_const(l, op, _text(r.value)), l.valid)
        # two string columns: compare through one shared dictionary
        if l.is_dict and r.is_dict and l.dictionary is r.dictionary and op in ("=", "<>"):
            out = l.data == r.data if op == "=" else l.data != r.data
            return Column(T.BOOL, out, _and_valid(l.valid, r.valid))
        n = len(l)
        both = _concat_strings(S.decode(l), S.decode(r))
        ranks = S.sort_ranks(both)
        a, c = ranks[:n], ranks[n:]
        fn = {"=": torch.eq, "<>": torch.ne, "<": torch.lt, "<=": torch.le, ">": torch.gt, ">=": torch.ge}[op]
        return Column(T.BOOL, fn(a, c), _and_valid(l.valid, r.valid))

    # ---------------------------------------------------------------- unary
    def _Not(self, e: Not, b: Batch) -> Value:
        v = self.eval(e.x, b)
        if isinstance(v, Scalar):
            return Scalar(None if v.value is None else not v.value, T.BOOL)
        d, valid = _bool_parts(v)
        return Column(T.BOOL, ~d, valid)

    def _Neg(self, e: Neg, b: Batch) -> Value:
        v = self.eval(e.x, b)
        if isinstance(v, Scalar):
            return Scalar(None if v.value is None else -v.value, v.dtype)
        return Column(v.dtype, -v.data, v.valid)

    def _IsNull(self, e: IsNull, b: Batch) -> Value:
        v = self.eval(e.x, b)
        if isinstance(v, Scalar):
            return Scalar((v.value is None) != e.negated, T.BOOL)
        dev = v.device
        if v.valid is None:
            return Scalar(e.negated, T.BOOL)
        return Column(T.BOOL, v.valid.clone() if e.negated else ~v.valid)

    # ------------------------------------------------------------- functions
    def _Cast(self, e: Cast, b: Batch) -> Value:
        v = self.eval(e.x, b)
        t = e.dtype
        if isinstance(v, Scalar):
            from ..sql.binder import _fold_cast
            return Scalar(_fold_cast(Lit(v.value, v.dtype), t).value, t)
        return self._cast_column(v, t)

    def _cast_column(self, v: Column, t: DataType) -> Column:
        src = v.dtype
        if src == t:
            return v
        if src.is_zoned and t.is_zoned:
            return Column(t, v.data, v.valid)    # AT TIME ZONE on a zoned value: the same instants retagged
        if t.is_binary and src.is_string:
            from ..ops import binary as BN
            return BN.to_binary(v)           # the same buffers relabelled
        if t.is_string and src.is_binary:
            from ..ops import binary as BN
            return BN.to_utf8(v)             # validated per row (binary.hip)
        if src.is_binary or t.is_binary:
            raise NotSupported(f"CAST({src} AS {t}): Binary casts only to and from Utf8")
        if t.is_string:
            if src.is_string:
                return v
            if src.is_decimal or src.kind in ("date32",) or src.is_numeric or src.kind == "bool":
                return S.to_string(v)       # GPU text formatting (strexpr.hip)
        if t.kind == "timestamp" and src.kind == "date32":
            return Column(t, v.data.to(torch.int64) * _US_DAY, v.valid)
        if t.kind == "date32" and src.kind == "timestamp":
            return Column(t, torch.div(v.data, _US_DAY, rounding_mode="floor").to(torch.int32), v.valid)
        if src.is_string and t.kind == "timestamp":
            return _parse_ts_host(v)
        if src.is_string:
            return S.parse(v, t)            # GPU parse (strexpr.hip); malformed -> error
        if t.kind == "bool":
            return Column(t, v.data != 0, v.valid)
        if src.kind == "null":
            return Column.full(None, t, len(v), v.device)
        return Column(t, _convert_tensor(v, t if t.kind not in ("date32",) else T.INT32).to(t.torch_dtype), v.valid)

    def _Case(self, e: Case, b: Batch) -> Value:
        n = b.num_rows
        dev = self.device(b)
        t = e.dtype
        vals = []
        for cond, val in e.whens:
            vals.append((self.mask(cond, b), self.eval(val, b)))
        els = self.eval(e.else_, b) if e.else_ is not None else Scalar(None, t)
        if t.is_varlen:
            return self._case_strings(vals, els, n, dev, t)
        rep = t
        out_v, out_valid = _full_of(els, rep, n, dev)
        for m, v in reversed(vals):
            x, xv = _full_of(v, rep, n, dev)
            out_v = torch.where(m, x, out_v)
            if out_valid is not None or xv is not None:
                ov = out_valid if out_valid is not None else torch.ones(n, dtype=torch.bool, device=dev)
                xvv = xv if xv is not None else torch.ones(n, dtype=torch.bool, device=dev)
                out_valid = torch.where(m, xvv, ov)
        return Column(t, out_v.to(t.torch_dtype) if t.kind != "null" else out_v, out_valid)

    def _case_strings(self, vals, els, n, dev, t=T.UTF8) -> Column:
        branches = [v for _, v in vals] + [els]
        if all(isinstance(v, Scalar) for v in branches):
            lits = []
            for v in branches:
                if v.value is not None and v.value not in lits:
                    lits.append(v.value)
            code = {s: i for i, s in enumerate(lits)}
            ev = els.value
            codes = torch.full((n,), code.get(ev, 0), dtype=torch.int32, device=dev)
            valid = None if ev is not None else torch.zeros(n, dtype=torch.bool, device=dev)
            for m, v in reversed(vals):
                codes = torch.where(m, torch.full_like(codes, code.get(v.value, 0)), codes)
                if valid is not None or v.value is None:
                    valid = torch.where(m, torch.full((n,), v.value is not None, dtype=torch.bool, device=dev),
                                        valid if valid is not None else torch.ones(n, dtype=torch.bool, device=dev))
            dic = Column.from_arrow(pa.array(lits or [b"" if t.is_binary else ""], t.to_arrow()), device=dev, dtype=t,
                                    dict_encode=False)
            return Column(t, codes, valid, dictionary=dic)
        # general case: the first matching WHEN picks its branch (else the
        # ELSE branch); one device string gather assembles the rows
        choice = torch.full((n,), len(vals), dtype=torch.int64, device=dev)
        for k in range(len(vals) - 1, -1, -1):
            choice = torch.where(vals[k][0], torch.full_like(choice, k), choice)
        return S.select_rows([self._str_col(v, dev, t) for v in branches], choice, n)

    @staticmethod
    def _str_col(v, dev, t=T.UTF8) -> Column:
        """A string / byte-string operand as a column (a scalar becomes a
        one-row constant; NULL a one-row NULL)."""
        if isinstance(v, Scalar):
            if v.value is None:
                c = S.const_column(b"" if t.is_binary else "", dev)
                return Column(t, c.data, torch.zeros(1, dtype=torch.bool, device=dev), offsets=c.offsets)
            return S.const_column(_text(v.value), dev)
        return v

    def _InList(self, e: InList, b: Batch) -> Value:
        x = e.x
        if isinstance(x, Func) and x.name == "substr" and x.options[0] == 1 and x.options[1] \
                and x.options[1] >= 1 and all(isinstance(y, Lit) for y in e.values):
            # substr(s, 1, L) IN (...): the prefixes compared in place (ops/strings.py in_set)
            c = self.eval(x.args[0], b)
            if isinstance(c, Column) and c.is_plain_string and c.data.is_cuda:
                m = S.in_set(c, [str(y.value) for y in e.values if y.value is not None], prefix_chars=x.options[1])
                return Column(T.BOOL, ~m if e.negated else m, c.valid)
        v = self.eval(e.x, b)
        if isinstance(v, Scalar):
            hit = any(x.value == v.value for x in e.values)
            return Scalar(hit != e.negated if v.value is not None else None, T.BOOL)
        vals = [x.value for x in e.values if x.value is not None]
        if v.dtype.is_varlen:
            m = S.in_list(v, [_text(x) for x in vals])
        else:
            t = v.dtype
            lits = torch.tensor([_convert_scalar(x, xx.dtype, t) for x, xx in zip(vals, [y for y in e.values if y.value is not None])],
                                dtype=v.data.dtype, device=v.device)
            m = torch.isin(v.data, lits)
        if e.negated:
            m = ~m
        return Column(T.BOOL, m, v.valid)

    def _Like(self, e: Like, b: Batch) -> Value:
        v = self.eval(e.x, b)
        if isinstance(v, Scalar):
            if v.value is None:
                return Scalar(None, T.BOOL)
            rx = S.like_regex(e.pattern, e.case_insensitive, e.escape)
            return Scalar((rx.fullmatch(v.value) is not None) != e.negated, T.BOOL)
        return Column(T.BOOL, S.like(v, e.pattern, e.case_insensitive, e.negated, e.escape), v.valid)

    def _try_cast(self, e: Func, b: Batch) -> Value:
        """TRY_CAST: the validity-writing kernels (ops/trycast.py) for the pairs that can fail, CAST's own
        conversion for the rest. No readback and no host step on the GPU."""
        from ..ops import trycast as TC
        v = self.eval(e.args[0], b)
        t = e.dtype
        if isinstance(v, Scalar):
            from ..sql.binder import _fold_try_cast
            return Scalar(_fold_try_cast(Lit(v.value, v.dtype), t).value, t)
        src = v.dtype
        if src.is_string and TC.can_parse(t):
            return TC.try_parse(v, t)
        if src.is_numeric and (TC.can_fail(src, t) or (v.is_wide and (t.is_integer or t.is_decimal))):
            return TC.cast_checked(v, t)
        return self._cast_column(v, t)

    def _Func(self, e: Func, b: Batch) -> Value:
        name = e.name
        if name == "try_cast":
            return self._try_cast(e, b)
        args = [self.eval(a, b) for a in e.args]
        if args and all(isinstance(a, Scalar) for a in args) and name not in ("coalesce",):
            return self._func_scalar(e, args)
        if name in _NESTED:
            return self._nested(e, args, b)
        if name in ("hex_digest", "to_char"):
            from ..ops import digest as DG
            c = args[0]
            if isinstance(c, Scalar):
                c = Column.full(c.value, e.args[0].dtype, b.num_rows, self.device(b))
            return DG.hex_digest(c, e.options[0]) if name == "hex_digest" else DG.to_char(c, e.options[0])
        if name == "strptime":
            from ..ops import strptime as SP
            return SP.strptime(args[0], *e.options)
        if name in ("bin_encode", "bin_decode", "byte_length"):
            from ..ops import binary as BN
            c = args[0]
            if name == "byte_length":
                return Column(T.INT32, BN.byte_length(c), c.valid)
            return BN.encode(c, e.options[0]) if name == "bin_encode" else BN.decode(c, e.options[0])
        if name == "upper":
            return S.upper(args[0])
        if name == "lower":
            return S.lower(args[0])
        if name == "substr":
            start, ln = e.options
            return S.substr(args[0], start, ln)
        if name == "char_length":
            c = args[0]
            return Column(T.INT32, S.char_length(c), c.valid)
        if name == "date_part":
            c = args[0]
            if e.options[0] == "week":
                return Column(T.INT32, iso_week(c.data.to(torch.int64)).to(torch.int32), c.valid)
            return Column(T.INT32, M.date_part(c.data, e.options[0]), c.valid)
        if name in _STRFN:
            from ..ops import strfuncs as SF
            c = args[0]
            return SF.apply(c, name, e.options)
        if name in _STRPAIR and len(args) == 2:
            # two string operands per row (ops/strfuncs.py apply_pair): a
            # constant operand stays a constant, NULL makes every row NULL
            from ..ops import strfuncs as SF
            if any(isinstance(a, Scalar) and a.value is None for a in args):
                return Column.full(None, e.dtype, b.num_rows, self.device(b))
            x, y = [str(a.value) if isinstance(a, Scalar) else a for a in args]
            out, valid = SF.apply_pair(x, y, name, b.num_rows)
            return Column(e.dtype, out, valid)
        if name in ("strpos", "ascii", "octet_length"):
            from ..ops import strfuncs as SF
            c = args[0]
            return Column(T.INT32, SF.apply_int(c, name, e.options), c.valid)
        if name in _STRROW:
            # arguments that vary per row (ops/strrow.py): a constant stays a constant
            from ..ops import strrow as SR
            strs, ints = _row_operands(name, [a.value if isinstance(a, Scalar) else a for a in args])
            return SR.apply_rows(name[:-4], strs, ints, b.num_rows)
        if name == "like_row":
            from ..ops import strrow as SR
            negated, esc = e.options
            x, p = [(None if a.value is None else _text(a.value)) if isinstance(a, Scalar) else a for a in args]
            return SR.like_rows(x, p, esc, negated, b.num_rows)
        if name in ("regexp_like", "regexp_count", "regexp_replace"):
            from ..ops import strfuncs as SF
            c = args[0]
            if name == "regexp_replace":
                pat, rep, flags = e.options
                return SF.regexp(c, name, pat, rep, flags)
            pat, flags, *start = e.options      # regexp_count(s, p, start[, flags]) carries its start
            return Column(e.dtype, SF.regexp(c, name, pat, None, flags, *start), c.valid)
        if name in _MATH1:
            c = args[0]
            x = _convert_tensor(c, T.FLOAT64) if name != "factorial" else c.data.to(torch.int64)
            return Column(e.dtype, _math1(name, x, e.options), c.valid)
        if name in ("logb", "atan2", "nanvl"):
            a, va = self._num(args[0], T.FLOAT64)
            c, vc = self._num(args[1], T.FLOAT64)
            a = a if isinstance(a, torch.Tensor) else torch.tensor(a, dtype=torch.float64, device=self.device(b))
            if name == "logb":
                out = torch.log(c) / torch.log(a)
            elif name == "atan2":
                out = torch.atan2(a, c)
            else:
                out = torch.where(torch.isnan(a), c if isinstance(c, torch.Tensor) else torch.full_like(a, c), a)
            return self._mk(out, T.FLOAT64, _and_valid(va, vc), b)
        if name == "random":
            return Column(T.FLOAT64, torch.rand(b.num_rows, dtype=torch.float64, device=self.device(b)))
        if name == "uuid":
            from ..ops import digest as DG
            return DG.uuid_column(b.num_rows, self.device(b))
        if name in ("greatest", "least"):
            return self._extreme(e, args, b)
        if name in ("gcd", "lcm"):
            a, va = self._num(args[0], T.INT64)
            c, vc = self._num(args[1], T.INT64)
            a = a if isinstance(a, torch.Tensor) else torch.full((b.num_rows,), a, dtype=torch.int64,
                                                                  device=self.device(b))
            g = torch.gcd(a, c if isinstance(c, torch.Tensor) else torch.full_like(a, c))
            out = g if name == "gcd" else torch.where(g == 0, torch.zeros_like(g), (a * c).abs() // g.clamp(min=1))
            return self._mk(out, T.INT64, _and_valid(va, vc), b)
        if name == "date_trunc":
            c = args[0]
            return Column(e.dtype, trunc_ts(c.data.to(torch.int64), e.options[0]), c.valid)
        if name == "ts_add":
            c = args[0]
            return Column(e.dtype, ts_add(c.data.to(torch.int64), *e.options), c.valid)
        if name == "date_bin":
            c = args[0]
            stride, origin = e.options
            d = c.data.to(torch.int64) - origin
            return Column(e.dtype, torch.div(d, stride, rounding_mode="floor") * stride + origin, c.valid)
        if name in _TZ_FUNCS:
            return self._tz_func(e, args[0])
        if name == "ts_part":
            c = args[0]
            out = ts_part(c.data.to(torch.int64), e.options[0])
            return Column(e.dtype, out.to(e.dtype.torch_dtype), c.valid)
        if name == "to_unixtime":
            c = args[0]
            return Column(T.INT64, torch.div(c.data.to(torch.int64), 1_000_000, rounding_mode="floor"), c.valid)
        if name == "ts_from_nanos":
            c = args[0]
            return Column(T.TIMESTAMP, torch.div(c.data.to(torch.int64), 1000, rounding_mode="floor"), c.valid)
        if name == "ts_from_float":
            c = args[0]
            return Column(T.TIMESTAMP, (c.data.to(torch.float64) * 1e6).round().to(torch.int64), c.valid)
        if name == "make_date":
            ys, ms, ds = [self._num(a, T.INT64) for a in args]
            vals = [x if isinstance(x, torch.Tensor) else torch.full((b.num_rows,), x, dtype=torch.int64,
                                                                    device=self.device(b)) for x, _ in (ys, ms, ds)]
            valid = _and_valid(_and_valid(ys[1], ms[1]), ds[1])
            return Column(T.DATE32, days_from_civil(*vals).to(torch.int32), valid)
        if name == "add_months":
            months, days = e.options
            c = args[0]
            return Column(T.DATE32, add_months(c.data, months, days), c.valid)
        if name == "abs":
            c = args[0]
            return Column(c.dtype, c.data.abs(), c.valid)
        if name == "round":
            c = args[0]
            d = e.options[0]
            if c.dtype.is_decimal:
                s = c.dtype.scale
                drop = s - min(s, max(d, 0))
                if drop <= 0:
                    return Column(e.dtype, c.data, c.valid)
                f = 10**drop
                q = torch.div(c.data.abs() + f // 2, f, rounding_mode="floor") * torch.sign(c.data)
                return Column(e.dtype, q, c.valid)
            if c.dtype.is_integer:
                return c
            f = 10.0**d
            x = c.data.double() * f
            # half away from zero (Rust f64::round, what DataFusion's round uses)
            return Column(T.FLOAT64, torch.sign(x) * torch.floor(x.abs() + 0.5) / f, c.valid)
        if name == "coalesce":
            return self._coalesce(e, args, b)
        if name == "concat":
            dev = self.device(b)
            l, r = [self._str_col(a, dev) if isinstance(a, Scalar) else a for a in args]
            return S.concat(l, r, b.num_rows)
        if name in ("sqrt", "ln", "log10", "exp", "floor", "ceil"):
            c = args[0]
            x = _convert_tensor(c, T.FLOAT64)
            fn = {"sqrt": torch.sqrt, "ln": torch.log, "log10": torch.log10, "exp": torch.exp, "floor": torch.floor,
                  "ceil": torch.ceil}[name]
            return Column(T.FLOAT64, fn(x), c.valid)
        if name == "power":
            a, va = self._num(args[0], T.FLOAT64)
            c, vc = self._num(args[1], T.FLOAT64)
            return self._mk(torch.pow(a, c) if isinstance(a, torch.Tensor) else torch.pow(torch.as_tensor(a), c), T.FLOAT64, _and_valid(va, vc), b)
        raise NotSupported(f"function {name}")

    def _nested(self, e: Func, args, b: Batch) -> Value:
        from ..ops import nested as NS
        name = e.name
        n = b.num_rows
        dev = self.device(b)

        def col(i):
            a = args[i]
            if isinstance(a, Scalar):
                return Column.full(a.value, e.args[i].dtype if a.dtype.kind == "null" else a.dtype, n, dev)
            return a
        if name == "make_array":
            return NS.make_list([col(i) for i in range(len(args))], n, e.dtype, dev)
        if name == "struct":
            return NS.make_struct(list(e.options), [col(i) for i in range(len(args))], n, e.dtype, dev)
        if name == "array_length":
            c = col(0)
            return Column(T.INT64, NS.lengths(c).clone(), c.valid)
        if name == "array_element":
            c = col(0)
            if len(args) > 1:
                p = col(1)
                return NS.element(c, p.data, p.valid)
            return NS.element(c, e.options[0])
        if name == "get_field":
            return NS.field(col(0), e.options[0])
        if name == "array_has":
            return NS.has(col(0), e.options[0])
        if name == "array_to_string":
            c = col(0)
            return NS.to_string(c, *e.options)
        if name == "regexp_match":
            import pyarrow.compute as pc
            c = col(0)
            pat, flags = e.options
            rx = re.compile(pat, re.I if "i" in flags else 0)
            if not rx.groups and set(flags) <= {"i", "c"} and c.data.is_cuda:
                # no capture group: the first match, found on the device
                from ..ops import strfuncs as SF
                m = SF.regexp_match_gpu(c, pat, "i" in flags, e.dtype)
                if m is not None:
                    return m
            vals = []
            for v in c.to_arrow().to_pylist():
                m = rx.search(v) if v is not None else None
                vals.append(None if m is None else (list(m.groups()) if rx.groups else [m.group(0)]))
            from ..ops._lib import HOST_STEPS
            HOST_STEPS["regexp_match"] += 1
            return Column.from_arrow(pa.array(vals, pa.list_(pa.large_string())), device=dev, dtype=e.dtype)
        if name == "unnest":
            raise ExecutionError("unnest() is only valid as a SELECT list item or in FROM")
        if name in _LIST_FAMILY:
            return self._list_family(e, [col(i) for i in range(len(args))])
        if name in _MAP_FAMILY:
            return self._map_family(e, [col(i) for i in range(len(args))], n, dev)
        raise NotSupported(f"function {name}")

    def _map_family(self, e: Func, c, n: int, dev) -> Value:
        from ..ops import nested as NS
        name = e.name
        if name == "make_map":
            return NS.make_map(c[0::2], c[1::2], n, e.dtype, dev)
        if name == "map_from_lists":
            return NS.map_from_lists(c[0], c[1], e.dtype)
        if name in ("map_element", "map_extract"):
            fn = NS.map_element if name == "map_element" else NS.map_extract
            # a constant key stays a constant (e.options), a key expression is one needle per row
            return fn(c[0], c[1], False) if len(c) > 1 else fn(c[0], e.options[0], True)
        return {"map_keys": NS.map_keys, "map_values": NS.map_values, "map_entries": NS.map_entries}[name](c[0])

    def _list_family(self, e: Func, c) -> Value:
        from ..columnar import Nested
        from ..ops import nested as NS
        name = e.name
        if name == "list_cast":
            a = c[0]
            kid = a.nested.child
            cast = Cast(ColRef(0, "child", kid.dtype), e.dtype.child)
            return Column(e.dtype, a.data, a.valid,
                          dictionary=Nested(child=self._Cast(cast, Batch({0: kid}, len(kid)))))
        if name == "array_slice":
            return NS.slice_(c[0], c[1].data, c[2].data, c[1].valid, c[2].valid)
        if name in ("array_remove", "array_replace"):
            return (NS.remove if name == "array_remove" else NS.replace)(*c[:-1], c[-1].data, c[-1].valid)
        if name == "array_position":
            return NS.position(c[0], c[1], *((c[2].data, c[2].valid) if len(c) > 2 else ()))
        if name == "array_repeat":
            return NS.repeat(c[0], c[1].data, c[1].valid, e.dtype)
        if name == "array_resize":
            return NS.resize(c[0], c[1].data, c[1].valid, c[2] if len(c) > 2 else None)
        if name == "array_concat":
            return NS.concat_lists(c, e.dtype)
        if name in ("array_append", "array_prepend"):
            return NS.append(c[0], c[1], e.dtype, front=name == "array_prepend")
        if name == "array_sort":
            return NS.sort(c[0], *e.options)
        if name in ("array_max", "array_min"):
            return NS.extreme(c[0], name == "array_max")
        fn = {"array_pop_front": NS.pop_front, "array_pop_back": NS.pop_back, "array_empty": NS.is_empty,
              "array_reverse": NS.reverse, "flatten": NS.flatten, "array_positions": NS.positions,
              "array_has_expr": NS.has_value, "array_has_all": NS.has_all, "array_has_any": NS.has_any,
              "array_distinct": NS.distinct, "array_union": NS.union, "array_intersect": NS.intersect,
              "array_except": NS.except_}[name]
        return fn(*c)

    def _tz_func(self, e: Func, c: Column) -> Column:
        """Zone-aware timestamp functions: one tz.hip kernel each on the GPU (ops/timezone.py)."""
        from ..ops import timezone as TZ
        name, zone = e.name, e.options[0]
        if name == "tz_parse":
            return _parse_tstz_host(c, e.dtype)
        if name == "tz_to_utc":
            return Column(e.dtype, TZ.to_utc(c.data, zone), c.valid)
        if name == "tz_to_local":
            return Column(e.dtype, TZ.to_local(c.data, zone), c.valid)
        if name == "tz_trunc":
            return Column(e.dtype, TZ.trunc(c.data, zone, e.options[1]), c.valid)
        if name == "tz_part":
            return Column(e.dtype, TZ.part(c.data, zone, e.options[1]), c.valid)
        if name == "tz_add":
            # months and days move the local wall clock (the clock time survives a DST change),
            # the sub-day part moves the instant
            _, months, days, us = e.options
            out = TZ.to_utc(ts_add(TZ.to_local(c.data, zone), months, days, 0), zone)
            return Column(e.dtype, out + us if us else out, c.valid)
        # tz_to_char: the local wall time formatted, %z / %:z from the row's offset
        from ..ops import digest as DG
        local, offs = TZ.to_local(c.data, zone, want_offsets=True)
        return DG.to_char(Column(T.TIMESTAMP, local, c.valid), e.options[1], offs)

    def _func_scalar(self, e: Func, args) -> Scalar:
        vals = [a.value for a in args]
        name = e.name
        if name == "make_array":
            return Scalar(list(vals), e.dtype)
        if name == "struct":
            return Scalar(dict(zip(e.options, vals)), e.dtype)
        if name in ("greatest", "least") and e.dtype.is_string:
            # NULL arguments are skipped; byte-wise order, as the kernel compares
            keys = [_text(v).encode("utf-8") for v in vals if v is not None]
            return Scalar((max(keys) if name == "greatest" else min(keys)).decode("utf-8") if keys else None, e.dtype)
        if any(v is None for v in vals) and name not in _LIST_FAMILY + _MAP_FAMILY:   # own NULL rules
            return Scalar(None, e.dtype)
        if name in _STRROW or name == "like_row":
            from ..ops import strrow as SR
            if name == "like_row":
                negated, esc = e.options
                return Scalar(SR.py_like(_text(vals[0]), _text(vals[1]), esc) != negated, T.BOOL)
            strs, ints = _row_operands(name, vals)
            try:
                return Scalar(SR.py_row(name[:-4])(strs, ints), T.UTF8)
            except ValueError as ex:
                raise ExecutionError(str(ex)) from None
        if name == "strptime":
            from ..ops import strptime as SP
            return Scalar(SP.fold(_text(vals[0]), *e.options), e.dtype)
        if name == "ts_from_nanos":
            return Scalar(int(vals[0]) // 1000, e.dtype)
        if name == "upper":
            return Scalar(vals[0].upper(), T.UTF8)
        if name == "lower":
            return Scalar(vals[0].lower(), T.UTF8)
        if name == "substr":
            return Scalar(S._py_substr(vals[0], *e.options), T.UTF8)
        if name == "char_length":
            return Scalar(len(vals[0]), T.INT32)
        if name == "date_part":
            from ..sql.binder import _date_part_py
            return Scalar(_date_part_py(vals[0], e.options[0]), T.INT32)
        if name == "abs":
            return Scalar(abs(vals[0]), e.dtype)
        if name == "concat":
            return Scalar(str(vals[0]) + str(vals[1]), T.UTF8)
        if name in _STRPAIR and len(vals) == 2:
            from ..ops import strfuncs as SF
            return Scalar(SF.py_fn2(name)(str(vals[0]), str(vals[1])), e.dtype)
        if name == "round":
            if e.dtype.is_decimal:
                s = args[0].dtype.scale
                drop = s - e.dtype.scale
                f = 10**drop
                q = (abs(vals[0]) + f // 2) // f
                return Scalar(q if vals[0] >= 0 else -q, e.dtype)
            return Scalar(round(float(vals[0]), e.options[0]), e.dtype)
        if name in ("sqrt", "ln", "log10", "exp", "floor", "ceil", "power"):
            f = {"sqrt": math.sqrt, "ln": math.log, "log10": math.log10, "exp": math.exp, "floor": math.floor,
                 "ceil": math.ceil, "power": math.pow}[name]
            return Scalar(float(f(*[float(v) for v in vals])), T.FLOAT64)
        # everything else: the column path over a one-row batch
        dev = torch.device(self.ctx.device if self.ctx is not None else "cpu")
        cols = {i: Column.full(v, a.dtype, 1, dev) for i, (v, a) in enumerate(zip(vals, args))}
        from ..sql.expr import ColRef as _CR
        e1 = Func(e.name, [_CR(i, f"a{i}", a.dtype) for i, a in enumerate(args)], e.dtype, e.options)
        r = self._Func(e1, Batch(cols, 1))
        if isinstance(r, Scalar):
            return r
        return Scalar(_host_value(r, e.dtype), e.dtype)

    def _extreme(self, e: Func, args, b: Batch) -> Value:
        """greatest / least: the largest / smallest non-NULL argument."""
        n = b.num_rows
        dev = self.device(b)
        t = e.dtype
        if t.is_string:
            from ..ops import strrow as SR
            return SR.extreme_rows([self._str_col(a, dev, t) for a in args], e.name == "greatest", n)
        out, valid = None, None
        for a in args:
            x, xv = _full_of(a, t, n, dev)
            ok = xv if xv is not None else torch.ones(n, dtype=torch.bool, device=dev)
            if out is None:
                out, valid = x, ok
                continue
            better = (x > out) if e.name == "greatest" else (x < out)
            take_x = ok & (~valid | better)
            out = torch.where(take_x, x, out)
            valid = valid | ok
        return Column(t, out, None if bool(valid.all()) and not valid.is_cuda else valid)

    def _coalesce(self, e: Func, args, b: Batch) -> Value:
        n = b.num_rows
        dev = self.device(b)
        t = e.dtype
        if t.is_varlen:
            # first non-NULL argument per row, assembled by one device gather
            choice = torch.full((n,), len(args) - 1, dtype=torch.int64, device=dev)
            for k in range(len(args) - 2, -1, -1):
                a = args[k]
                if isinstance(a, Scalar):
                    if a.value is not None:
                        choice = torch.full_like(choice, k)
                    continue
                ok = a.valid if a.valid is not None else torch.ones(n, dtype=torch.bool, device=dev)
                choice = torch.where(ok, torch.full_like(choice, k), choice)
            return S.select_rows([self._str_col(a, dev, t) for a in args], choice, n)
        out, valid = _full_of(args[-1], t, n, dev)
        for a in reversed(args[:-1]):
            x, xv = _full_of(a, t, n, dev)
            if xv is None:
                out, valid = x, None
                continue
            out = torch.where(xv, x, out)
            valid = xv | valid if valid is not None else None
        return Column(t, out, valid)


_STRFN = ("trim", "replace", "lpad", "rpad", "reverse", "repeat", "left", "right", "initcap", "translate",
          "split_part", "substr_index")
# with two arguments: the per-row forms (one-argument strpos keeps its literal in the options)
_STRPAIR = ("levenshtein", "strpos", "contains", "starts_with", "ends_with", "find_in_set")
# per-row arguments (ops/strrow.py): the name, then which arguments are strings
_STRROW = {"substr_row": (0,), "left_row": (0,), "right_row": (0,), "repeat_row": (0,), "split_part_row": (0, 1),
           "lpad_row": (0, 2), "rpad_row": (0, 2), "replace_row": (0, 1, 2), "overlay_row": (0, 1), "chr_row": (),
           "to_hex_row": ()}


def _row_operands(name: str, vals: list):
    """(string operands, integer operands) of a ``*_row`` call, in argument order; lpad / rpad
    without a fill pad with a blank."""
    at = _STRROW[name]
    strs = [(_text(v) if v is not None and not isinstance(v, Column) else v) for i, v in enumerate(vals) if i in at]
    ints = [(int(v) if v is not None and not isinstance(v, Column) else v) for i, v in enumerate(vals) if i not in at]
    if name in ("lpad_row", "rpad_row") and len(strs) == 1:
        strs.append(" ")
    return strs, ints


_MATH1 = ("sign", "trunc", "log2", "cbrt", "degrees", "radians", "sin", "cos", "tan", "asin", "acos", "atan", "sinh",
          "cosh", "tanh", "isnan", "iszero", "factorial")
_US_DAY = 86_400_000_000


def _math1(name: str, x: torch.Tensor, options) -> torch.Tensor:
    if name == "sign":
        return torch.sign(x)
    if name == "trunc":
        d = options[0] if options else 0
        f = 10.0 ** d
        return torch.trunc(x * f) / f
    if name == "log2":
        return torch.log2(x)
    if name == "cbrt":
        return torch.sign(x) * x.abs().pow(1.0 / 3.0)
    if name == "degrees":
        return torch.rad2deg(x)
    if name == "radians":
        return torch.deg2rad(x)
    if name == "isnan":
        return torch.isnan(x)
    if name == "iszero":
        return x == 0
    if name == "factorial":
        lut = torch.tensor([math.factorial(i) for i in range(21)], dtype=torch.int64, device=x.device)
        return lut.index_select(0, x.clamp(0, 20))
    return getattr(torch, name)(x)


def civil_from_days(days: torch.Tensor):
    """(year, month, day) int64 tensors from days since 1970-01-01 (Hinnant)."""
    z = days.to(torch.int64) + 719468
    era = torch.div(z, 146097, rounding_mode="floor")
    doe = z - era * 146097
    yoe = torch.div(doe - torch.div(doe, 1460, rounding_mode="floor") + torch.div(doe, 36524, rounding_mode="floor")
                    - torch.div(doe, 146096, rounding_mode="floor"), 365, rounding_mode="floor")
    doy = doe - (365 * yoe + torch.div(yoe, 4, rounding_mode="floor") - torch.div(yoe, 100, rounding_mode="floor"))
    mp = torch.div(5 * doy + 2, 153, rounding_mode="floor")
    d = doy - torch.div(153 * mp + 2, 5, rounding_mode="floor") + 1
    m = torch.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2).to(torch.int64)
    return y, m, d


def days_from_civil(y: torch.Tensor, m: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    yy = y - (m <= 2).to(torch.int64)
    era = torch.div(yy, 400, rounding_mode="floor")
    yoe = yy - era * 400
    doy = torch.div(153 * torch.where(m > 2, m - 3, m + 9) + 2, 5, rounding_mode="floor") + d - 1
    doe = yoe * 365 + torch.div(yoe, 4, rounding_mode="floor") - torch.div(yoe, 100, rounding_mode="floor") + doy
    return era * 146097 + doe - 719468


def iso_week(days: torch.Tensor) -> torch.Tensor:
    wd = torch.remainder(days + 3, 7)            # Monday = 0 (1970-01-01 was a Thursday)
    thu = days - wd + 3
    y, _, _ = civil_from_days(thu)
    jan1 = days_from_civil(y, torch.ones_like(y), torch.ones_like(y))
    return torch.div(thu - jan1, 7, rounding_mode="floor") + 1


_TZ_FUNCS = ("tz_to_utc", "tz_to_local", "tz_trunc", "tz_part", "tz_add", "tz_to_char", "tz_parse")
_TS_TEXT_OFFSET = r"[T ]\d{2}:\d{2}.*(Z|z|[+-]\d{2}(:?\d{2})?)$"      # a time of day followed by Z / +HH / +HHMM / +HH:MM


def trunc_ts(us: torch.Tensor, unit: str) -> torch.Tensor:
    """date_trunc over timestamps (microseconds since the epoch)."""
    step = {"microsecond": 1, "millisecond": 1000, "second": 1_000_000, "minute": 60_000_000,
            "hour": 3_600_000_000, "day": _US_DAY}.get(unit)
    if step is not None:
        return torch.div(us, step, rounding_mode="floor") * step
    days = torch.div(us, _US_DAY, rounding_mode="floor")
    if unit == "week":
        return (days - torch.remainder(days + 3, 7)) * _US_DAY
    y, m, _ = civil_from_days(days)
    if unit == "quarter":
        m = torch.div(m - 1, 3, rounding_mode="floor") * 3 + 1
    elif unit == "year":
        m = torch.ones_like(m)
    return days_from_civil(y, m, torch.ones_like(m)) * _US_DAY


def ts_add(us: torch.Tensor, months: int, days: int, micros: int) -> torch.Tensor:
    d = torch.div(us, _US_DAY, rounding_mode="floor")
    rem = us - d * _US_DAY
    if months:
        d = add_months(d, months).to(torch.int64)
    return (d + days) * _US_DAY + rem + micros


def ts_part(us: torch.Tensor, field: str) -> torch.Tensor:
    if field == "epoch":
        return us.to(torch.float64) / 1e6
    days = torch.div(us, _US_DAY, rounding_mode="floor")
    rem = us - days * _US_DAY
    if field == "hour":
        return torch.div(rem, 3_600_000_000, rounding_mode="floor")
    if field == "minute":
        return torch.remainder(torch.div(rem, 60_000_000, rounding_mode="floor"), 60)
    if field == "second":
        return torch.remainder(torch.div(rem, 1_000_000, rounding_mode="floor"), 60)
    if field == "millisecond":
        return torch.remainder(torch.div(rem, 1000, rounding_mode="floor"), 60_000)
    if field == "microsecond":
        return torch.remainder(rem, 60_000_000)
    if field == "week":
        return iso_week(days)
    if field in ("dow", "doy", "quarter"):
        y, m, d = civil_from_days(days)
        if field == "dow":
            return torch.remainder(days + 4, 7)
        if field == "quarter":
            return torch.div(m - 1, 3, rounding_mode="floor") + 1
        return days - days_from_civil(y, torch.ones_like(y), torch.ones_like(y)) + 1
    y, m, d = civil_from_days(days)
    return {"year": y, "month": m, "day": d}[field]


def trunc_ts_py(us: int, unit: str) -> int:
    return int(trunc_ts(torch.tensor([us], dtype=torch.int64), unit)[0])


def ts_part_py(us: int, field: str):
    v = ts_part(torch.tensor([us], dtype=torch.int64), field)[0]
    return float(v) if field == "epoch" else int(v)


def _host_value(c: Column, t: DataType):
    """Engine representation of a one-row column's value (dates in days,
    timestamps in microseconds, decimals unscaled)."""
    if c.valid is not None and not bool(c.valid.cpu()[0]):
        return None
    if t.is_varlen or t.is_nested:
        return c.to_arrow()[0].as_py()
    v = c.data.cpu()[0]
    if t.kind == "bool":
        return bool(v)
    if t.is_float:
        return float(v)
    return int(v)


def add_months(days: torch.Tensor, months: int, extra_days: int = 0) -> torch.Tensor:
    """date32 + INTERVAL 'n' MONTH (+ days) on the device: civil date from
    days (Hinnant), month arithmetic, day clamped to the target month's
    length (Jan 31 + 1 month = Feb 28/29), back to days — integer tensor ops,
    no host round trip."""
    z = days.to(torch.int64) + 719468
    era = torch.div(z, 146097, rounding_mode="floor")      # floor division: no negative-year adjustment
    doe = z - era * 146097
    yoe = torch.div(doe - torch.div(doe, 1460, rounding_mode="floor") + torch.div(doe, 36524, rounding_mode="floor")
                    - torch.div(doe, 146096, rounding_mode="floor"), 365, rounding_mode="floor")
    doy = doe - (365 * yoe + torch.div(yoe, 4, rounding_mode="floor") - torch.div(yoe, 100, rounding_mode="floor"))
    mp = torch.div(5 * doy + 2, 153, rounding_mode="floor")
    d = doy - torch.div(153 * mp + 2, 5, rounding_mode="floor") + 1
    m = torch.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2).to(torch.int64)
    k = y * 12 + (m - 1) + months
    y2 = torch.div(k, 12, rounding_mode="floor")
    m2 = k - y2 * 12 + 1
    leap = ((y2 % 4 == 0) & (y2 % 100 != 0)) | (y2 % 400 == 0)
    mdays = torch.tensor([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], dtype=torch.int64,
                         device=days.device).index_select(0, m2 - 1) + (leap & (m2 == 2)).to(torch.int64)
    d2 = torch.minimum(d, mdays)
    # days_from_civil
    yy = y2 - (m2 <= 2).to(torch.int64)
    era2 = torch.div(yy, 400, rounding_mode="floor")
    yoe2 = yy - era2 * 400
    doy2 = torch.div(153 * torch.where(m2 > 2, m2 - 3, m2 + 9) + 2, 5, rounding_mode="floor") + d2 - 1
    doe2 = yoe2 * 365 + torch.div(yoe2, 4, rounding_mode="floor") - torch.div(yoe2, 100, rounding_mode="floor") + doy2
    return (era2 * 146097 + doe2 - 719468 + extra_days).to(torch.int32)


# =============================================================== conversions
def _parse_ts_host(v: Column) -> Column:
    from ..ops.strings import note_host_step
    note_host_step("string -> timestamp")
    arr = v.to_arrow()
    try:
        ts = pc.cast(pc.strptime(arr, "%Y-%m-%dT%H:%M:%S", "us", error_is_null=True), pa.timestamp("us"))
        miss = pc.and_(pc.is_null(ts), pc.is_valid(arr))
        if pc.any(miss).as_py():
            ts = pc.cast(arr, pa.timestamp("us"))
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
        raise ExecutionError(f"cannot parse timestamp: {e}") from None
    out = Column.from_arrow(ts, device=v.device)
    return Column(T.TIMESTAMP, out.data.to(torch.int64), out.valid)


def _parse_tstz_host(v: Column, t: DataType) -> Column:
    """CAST(string AS TIMESTAMPTZ) per row: text that carries an offset is that instant, the rest is
    wall time in t's zone (tz_to_utc). Parsed on the host like the naive string -> timestamp cast."""
    from ..ops import timezone as TZ
    arr = v.to_arrow()
    has_off = pc.fill_null(pc.match_substring_regex(arr, _TS_TEXT_OFFSET), False)
    none = pa.nulls(len(arr), arr.type)
    wall = _parse_ts_host(Column.from_arrow(pc.if_else(has_off, none, arr), device=v.device, dict_encode=False))
    try:
        inst = pc.cast(pc.if_else(has_off, arr, none), pa.timestamp("us", tz="UTC"))
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError) as e:
        raise ExecutionError(f"cannot parse timestamp: {e}") from None
    inst = Column.from_arrow(inst, device=v.device)
    m = torch.from_numpy(has_off.to_numpy(zero_copy_only=False).astype(bool)).to(v.device)
    return Column(t, torch.where(m, inst.data.to(torch.int64), TZ.to_utc(wall.data, t.tz)), v.valid)


def _convert_scalar(x, src: DataType, t: DataType):
    if t.is_decimal:
        if src.is_decimal:
            d = t.scale - src.scale
            return x * 10**d if d >= 0 else int(round(x / 10**(-d)))
        if src.is_float:
            return int(round(x * 10**t.scale))
        return int(x) * 10**t.scale
    if t.is_float:
        if src.is_decimal:
            return x / 10**src.scale
        return float(x)
    if t.kind == "bool":
        return bool(x)
    if src.is_decimal and t.is_integer:
        return int(x // 10**src.scale)
    return x


def _convert_tensor(c: Column, t: DataType) -> torch.Tensor:
    src = c.dtype
    x = c.data
    if c.is_wide:
        if t.is_float:
            lo = x[:, 0].to(torch.float64)
            hi = x[:, 1].to(torch.float64)
            lo = torch.where(lo < 0, lo + 18446744073709551616.0, lo)
            v = hi * 18446744073709551616.0 + lo
            return v / 10**src.scale if src.is_decimal else v
        raise ExecutionError("128-bit decimal value used in integer arithmetic (value exceeds 64 bits)")
    if t.is_decimal:
        if src.is_decimal:
            d = t.scale - src.scale
            if d == 0:
                return x
            if d > 0:
                return x * (10**d)
            f = 10**(-d)
            return torch.div(x + torch.sign(x) * (f // 2), f, rounding_mode="trunc")
        if src.is_float:
            return torch.round(x * 10**t.scale).to(torch.int64)
        return x.to(torch.int64) * (10**t.scale)
    if t.is_float:
        if src.is_decimal:
            return x.to(torch.float64) / (10**src.scale)
        return x.to(torch.float64)
    if t.is_integer or t.kind in ("date32", "timestamp"):
        if src.is_decimal:
            return torch.div(x, 10**src.scale, rounding_mode="trunc").to(torch.int64)
        if src.is_float:
            return x.to(torch.int64)
        if src.kind == "bool":
            return x.to(torch.int64)
        return x if x.dtype == t.torch_dtype or t.kind == "int64" and x.dtype in (torch.int32, torch.int64) else x.to(t.torch_dtype)
    return x


def _overflow_guard(a, c):
    """Decimal product whose static precision exceeds 18 digits: verify at run time
    that the int64 product cannot overflow (raises otherwise)."""
    ts = [v for v in (a, c) if isinstance(v, torch.Tensor) and v.numel()]
    dev_max = iter(to_host_ints(torch.stack([v.abs().max().to(torch.int64) for v in ts])) if ts else [])  # one sync

    def mx(v):
        if isinstance(v, torch.Tensor):
            return int(next(dev_max)) if v.numel() else 0
        return abs(int(v))
    if mx(a) * mx(c) >= 2**63:
        raise ExecutionError("decimal multiplication overflows 64-bit fixed point; CAST to DOUBLE")
    return a, c


def _any(m: torch.Tensor) -> bool:
    return bool(to_host_ints(m.any().to(torch.int64))[0]) if m.is_cuda else bool(m.any())


def _bool_parts(v: Column):
    d = v.data if v.data.dtype == torch.bool else v.data != 0
    return d, v.valid


def _full_of(v: Value, t: DataType, n: int, dev):
    if isinstance(v, Scalar):
        if v.value is None:
            td = t.torch_dtype if t.kind != "null" else torch.bool
            return torch.zeros(n, dtype=td, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
        val = _convert_scalar(v.value, v.dtype, t)
        return torch.full((n,), val, dtype=t.torch_dtype if t.kind != "null" else torch.bool, device=dev), None
    x = _convert_tensor(v, t) if v.dtype != t else v.data
    return x.to(t.torch_dtype) if t.kind != "null" else x, v.valid


def _concat_strings(a: Column, b: Column) -> Column:
    na, nb = len(a), len(b)
    off = torch.cat([a.offsets, b.offsets[1:] + a.offsets[-1]])
    chars = torch.cat([a.data, b.data])
    valid = None
    if a.valid is not None or b.valid is not None:
        va = a.valid if a.valid is not None else torch.ones(na, dtype=torch.bool, device=a.device)
        vb = b.valid if b.valid is not None else torch.ones(nb, dtype=torch.bool, device=b.device)
        valid = torch.cat([va, vb])
    return Column(a.dtype, chars, valid, offsets=off)


def _text(v):
    """A varlen constant for the string kernels: bytes stay bytes (Binary), anything else its text."""
    return v if isinstance(v, bytes) else str(v)
