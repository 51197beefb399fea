"""Range slices of replicated tables (SPMD).

The multi-rank layout replicates the dimension tables on every rank (at SF100
~125M rows, a few GB of HBM against 288 GB per GPU), so a fact-dimension join
needs no exchange. A query that reads ONLY replicated tables (TPC-H Q2, Q11,
Q16: part / partsupp / supplier / nation / region) would then do identical
work on every GPU. Such a query instead splits its largest table by key range:
rank r takes the rows whose key k satisfies ``(k - kmin) // chunk == r``
(``chunk = ceil((kmax - kmin + 1) / world)``) -- contiguous rows of the table,
which is clustered on that key, so each rank's slice is a set of views of the
resident columns (no copy, no gather, sortedness and derived indexes kept).
The slice is placed ``(("range", world, kmin, chunk), key cid)``: GROUP BY the
key is rank-local, joins with the other (replicated) inputs are rank-local,
and two scans sliced with the same mapping are co-partitioned on the key.

A query mixing replicated and partitioned tables slices its largest replicated
table too when every partitioned input is REDUCED before it meets that table's
rows in a join:
under an aggregate, inside a subquery expression, or on the subquery side of
a semi / anti join (TPC-H Q22: customer anti-joined with orders -- the
anti-join marks come from a dense reduce-scatter over the customer key range,
parallel/exchange.py semi_by_key_set; Q20: partsupp against per-(part,
supplier) lineitem sums). Inner joins with a partitioned table keep the
replicated side whole (they are rank-local that way).

The same range mapping places the output of the partitioned dense aggregates
reduced with RCCL reduce-scatter (exec/aggregate.py eager COUNT, Q13): each
rank receives the counts of one contiguous key chunk.

Reference parity: the reference places one whole table per worker
(crates/coordinator/src/distributed_planner.rs:44-63, :152-157:
``sum(chars(table_name)) % N``) -- no intra-table split at all.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from ..columnar import Column
from ..sql import logical as L
from ..sql.expr import Expr, SubqueryExpr
from ..utils import tags


def range_tag(world: int, kmin: int, chunk: int) -> tuple:
    return ("range", int(world), int(kmin), int(chunk))


def range_chunk(kmin: int, kmax: int, world: int) -> int:
    return max(1, -(-(kmax - kmin + 1) // max(world, 1)))


def _exprs_of(node):
    """Expressions held by a logical node (subquery plans live inside them)."""
    if isinstance(node, L.Filter):
        yield node.pred
    elif isinstance(node, L.Project):
        for _, e in node.exprs:
            yield e
    elif isinstance(node, L.Join):
        for a, b in node.on:
            yield a
            yield b
        if node.residual is not None:
            yield node.residual
    elif isinstance(node, L.MultiJoin):
        yield from node.conds
        for s in node.semis:
            for a, b in s.on:
                yield a
                yield b
            if s.residual is not None:
                yield s.residual
    elif isinstance(node, L.Aggregate):
        for _, e in node.groups:
            yield e
        for _, a in node.aggs:
            yield a
    elif isinstance(node, L.Sort):
        for e, _, _ in node.keys:
            yield e
    elif isinstance(node, L.Scan):
        yield from node.filters


def _subplans(e: Expr):
    stack = [e]
    while stack:
        x = stack.pop()
        if isinstance(x, SubqueryExpr):
            yield x.plan
        stack.extend(k for k in x.children() if k is not None)


def all_scans(plan: L.Plan):
    """Every Scan of ``plan``, subquery plans inside expressions included."""
    stack = [plan]
    seen = set()
    while stack:
        p = stack.pop()
        if id(p) in seen:
            continue
        seen.add(id(p))
        if isinstance(p, L.Scan):
            yield p
        for e in _exprs_of(p):
            stack.extend(_subplans(e))
        stack.extend(p.inputs)
        if isinstance(p, L.Values):
            for row in p.rows:
                for e in row:
                    stack.extend(_subplans(e))


def _unsliceable(plan: L.Plan) -> set:
    """ids of the replicated sources whose rows meet UNREDUCED rows of a
    partitioned table in a join (an inner / outer join input holds the
    replicated table while another holds a partitioned scan with no aggregate
    in between): slicing them would turn a rank-local join into an exchange.
    Rows under an aggregate, on the subquery side of a semi / anti join, or
    inside a subquery expression count as reduced."""
    bad = set()

    def visit(p):
        """(partitioned rows flow out unreduced, replicated sources whose rows flow out)"""
        for e in _exprs_of(p):
            for sp in _subplans(e):
                visit(sp)
        if isinstance(p, L.Scan):
            return (False, {id(p.source)}) if getattr(p.source, "replicated", False) else (True, set())
        if isinstance(p, L.Aggregate):
            for c in p.inputs:
                visit(c)
            return False, set()
        if isinstance(p, L.Join) and p.kind in ("semi", "anti"):
            visit(p.right)
            return visit(p.left)
        if isinstance(p, (L.Join, L.MultiJoin)):
            kids = [p.left, p.right] if isinstance(p, L.Join) else list(p.children)
            if isinstance(p, L.MultiJoin):
                for sp in p.semis:
                    visit(sp.right)
            infos = [visit(c) for c in kids]
            for i, (part, _) in enumerate(infos):
                if part:
                    for k, (_, reps) in enumerate(infos):
                        if k != i:
                            bad.update(reps)
            return any(x[0] for x in infos), set().union(*[x[1] for x in infos])
        part, reps = False, set()
        for c in p.inputs:
            a, r = visit(c)
            part, reps = part or a, reps | r
        return part, reps

    visit(plan)
    return bad


def plan_slices(plan: L.Plan, comm) -> Dict[int, str]:
    """{id(source): key column name} of the replicated table a query splits
    by key range: a query over replicated tables only, or one whose
    table's rows meet partitioned rows only after those are reduced
    (``_unsliceable``; then it must hold SLICE_MIXED_MIN_ROWS). Empty outside SPMD. Decided
    from the plan and the catalog alone, so every rank decides alike."""
    if comm is None or not comm.spmd:
        return {}
    scans = list(all_scans(plan))
    if not scans:
        return {}
    mixed = any(not getattr(s.source, "replicated", False) for s in scans)
    bad = _unsliceable(plan) if mixed else set()
    best = None
    for s in scans:
        if not getattr(s.source, "replicated", False) or id(s.source) in bad:
            continue
        key = getattr(s.source, "cluster_key", None)
        if key is None:
            continue
        try:
            n = int(s.source.num_rows())
        except Exception:  # noqa: BLE001 - sources without a cheap row count are not sliced
            continue
        if best is None or n > best[0]:
            best = (n, s.source, key)
    if best is None or best[0] < (SLICE_MIXED_MIN_ROWS if mixed else SLICE_MIN_ROWS):
        return {}
    return {id(best[1]): best[2]}


#: tables smaller than this are not worth splitting (the exchange of the
#: partial results costs more than the repeated work)
SLICE_MIN_ROWS = 1 << 16
#: ... in a query that also reads partitioned tables (its joins with the
#: reduced partitioned side may need an exchange the whole table avoids)
SLICE_MIXED_MIN_ROWS = 1 << 22


def _cut(c: Column, a: int, b: int) -> Column:
    from ..cache.cdc import _slice
    from ..catalog import _mark_resident
    out = _slice(c, a, b)
    _mark_resident(out)
    return out


def _range_cut_rows(kt: torch.Tensor, n: int, kmin: int, kmax: int, chunk: int, rank: int) -> Tuple[int, int]:
    """Rows [a, b) of sorted keys ``kt`` owned by ``rank``: keys in
    [kmin + rank*chunk, kmin + (rank+1)*chunk). The cut values stay unclamped
    Python ints (kmin + world*chunk can pass the key type's range, e.g. int32
    keys near INT32_MAX); a cut past kmax means "end of the rows" and is never
    searched, so every row lands on exactly one rank."""
    from ..ops._lib import device_ints, to_host_ints
    lo, hi = kmin + rank * chunk, kmin + (rank + 1) * chunk
    search = [v for v in (lo, hi) if v <= kmax]
    found = []
    if search:
        cuts = device_ints(search, kt.device, kt.dtype) if kt.is_cuda else torch.tensor(search, dtype=kt.dtype)
        found = to_host_ints(torch.searchsorted(kt, cuts).to(torch.int64))
    a = n if lo > kmax else found[0]
    b = n if hi > kmax else found[-1]
    return a, b


def slice_columns(cols: Dict[str, Column], n: int, key: str, world: int, rank: int
                  ) -> Tuple[Dict[str, Column], int, Optional[tuple]]:
    """This rank's key-range slice of a replicated table's resident columns:
    (columns, rows, range tag or None when the key column is not sorted --
    then an even split by rows, placed by no key). Slices are views cached
    on the resident key tensor, so a query replaying over the same columns
    reuses them (and the indexes built on them)."""
    from ..ops import hashing as H
    from ..ops._lib import device_ints, to_host_ints, unlogged
    kc = cols.get(key)
    kt = kc.data if kc is not None else None
    memo = tags.SLICES.get(kt)      # (no key column: kt is None, nothing is remembered)
    if memo is None:
        memo = {}
        tags.SLICES.set(kt, memo)
    plan = memo.get(("bounds", world, rank))
    if plan is None:
        with unlogged():    # remembered on the resident key tensor: a one-time cost
            if kc is not None and kc.valid is None and kt.dim() == 1 and not kc.dtype.is_varlen \
                    and kt.dtype in (torch.int32, torch.int64) and n and H.is_sorted(kt):
                kmin, kmax = to_host_ints(kt[[0, -1]].to(torch.int64))
                chunk = range_chunk(kmin, kmax, world)
                a, b = _range_cut_rows(kt, n, kmin, kmax, chunk, rank)
                tag = range_tag(world, kmin, chunk)
            else:
                a, b = n * rank // world, n * (rank + 1) // world
                tag = None
        plan = memo[("bounds", world, rank)] = (a, b, tag)
    a, b, tag = plan
    out = {}
    for name, c in cols.items():
        hit = memo.get((name, world, rank))
        if hit is None or hit[0] is not c.data:
            with unlogged():    # string byte bounds: one readback, then cached
                hit = memo[(name, world, rank)] = (c.data, _cut(c, a, b))
        out[name] = hit[1]
    return out, b - a, tag
