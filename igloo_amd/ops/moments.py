"""Grouped second-order moments of (x, y) pairs (csrc/kernels/moments.hip).

``grouped_moments2`` returns, per group, the number of pairs, both means and
the centred sums M2x = sum((x - mean_x)^2), M2y, Cxy = sum((x - mean_x)(y -
mean_y)): the states of the regr_* family (exec/aggregate.py).

GPU: one pass over x and y accumulating sums around a per-group shift (the
group's first valid pair), then the finaliser below over one element per
group; no readback and no host synchronisation. CPU: the two-pass definition
(group mean, then sums of centred products), which shares nothing with the
kernel's shifted-sum algebra.

A pair counts when ``valid`` (None: every row) holds and its group id lies in
[0, ngroups). A group without a pair reports count 0; its other values mean
nothing (the regr_* functions are NULL or 0 there).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import idx_dtype, launch, ptr, stream
from .gather import gather_tensor

Moments = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


def grouped_moments2(gid: Optional[torch.Tensor], ngroups: int, x: torch.Tensor, y: torch.Tensor,
                     valid: Optional[torch.Tensor], n: int, device, sorted_gids: bool = False) -> Moments:
    """(cnt int64, mean_x, mean_y, M2x, M2y, Cxy float64), each [max(ngroups, 1)].
    ``sorted_gids``: group ids are non-decreasing (clustered keys)."""
    device = torch.device(device)
    assert x.dtype == torch.float64 and y.dtype == torch.float64 and x.numel() == n and y.numel() == n
    if device.type != "cpu":
        return _gpu(gid, ngroups, x, y, valid, n, device, sorted_gids)
    return _cpu(gid, ngroups, x, y, valid, n)


def _gpu(gid, ngroups, x, y, valid, n, device, sorted_gids) -> Moments:
    g = max(ngroups, 1)
    # the count and the five shifted sums in ONE zeroed buffer (one fill kernel;
    # slots padded to 512 bytes, the alignment of a fresh allocation)
    slot = -(-g // 64) * 64
    zbuf = torch.zeros(6 * slot, dtype=torch.int64, device=device)
    cnt = zbuf[:g]
    sums = zbuf[slot:].view(torch.float64)
    x, y = x.contiguous(), y.contiguous()
    gid = None if gid is None else gid.contiguous()
    if valid is not None:
        valid = valid.contiguous()
        assert valid.numel() == n and valid.element_size() == 1
    assert gid is None or (gid.dtype == torch.int32 and gid.numel() == n)
    rdt = idx_dtype(n)
    first = torch.full((g,), torch.iinfo(rdt).max, dtype=rdt, device=device)
    launch("agg_moments2").agg_moments2(ptr(gid), n, ngroups if gid is not None else 1, ptr(x), ptr(y), ptr(valid),
                                        ptr(cnt), ptr(first), rdt == torch.int64, ptr(sums), slot, bool(sorted_gids),
                                        stream(x))
    sx, sy, sxx, syy, sxy = (sums[k * slot: k * slot + g] for k in range(5))
    if n == 0:
        return cnt, sx, sy, sxx, syy, sxy
    # the finaliser: g elements. A group without a pair keeps first at its
    # maximum: its shift is some row's value, and its count of 0 tells the caller
    at = first.clamp(max=n - 1)
    kx, ky = gather_tensor(x, at), gather_tensor(y, at)
    c = cnt.to(torch.float64).clamp(min=1)
    return (cnt, kx + sx / c, ky + sy / c, (sxx - sx * sx / c).clamp(min=0), (syy - sy * sy / c).clamp(min=0),
            sxy - sx * sy / c)


def _cpu(gid, ngroups, x, y, valid, n) -> Moments:
    g = max(ngroups, 1)
    gi = torch.zeros(n, dtype=torch.int64) if gid is None else gid.to(torch.int64)
    sel = (gi >= 0) & (gi < g)
    if valid is not None:
        sel &= valid
    gi, x, y = gi[sel], x[sel], y[sel]

    def per_group(v):
        return torch.zeros(g, dtype=torch.float64).index_add_(0, gi, v)
    cnt = torch.bincount(gi, minlength=g)[:g].to(torch.int64) if gi.numel() else torch.zeros(g, dtype=torch.int64)
    c = cnt.to(torch.float64).clamp(min=1)
    mx, my = per_group(x) / c, per_group(y) / c
    # one refinement of the rounded mean: a constant column's mean is then the
    # constant itself, so its centred sum is exactly 0 (the NULL rule of regr_slope)
    mx, my = mx + per_group(x - mx[gi]) / c, my + per_group(y - my[gi]) / c
    dx, dy = x - mx[gi], y - my[gi]
    return cnt, mx, my, per_group(dx * dx), per_group(dy * dy), per_group(dx * dy)
