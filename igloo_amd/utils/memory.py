"""HBM accounting for resident columns and the structures derived from them.

Resident table columns carry derived structures built on first use and kept
with the column tensor like an index: the tags of kind "derived" declared in
utils/tags.py (narrow copies, secondary and dense indexes, sketches, search
fences, row-packed copies). The cache tier (cache/tiered.py) charges them to
the column that owns them, so the HBM budget covers what the table really
holds, and evicting a column drops its derived structures with it.
"""
from __future__ import annotations

from typing import Iterable

import torch

from . import tags

DERIVED_ATTRS = tags.DERIVED


def _tensor_bytes(x) -> int:
    if isinstance(x, torch.Tensor):
        return x.numel() * x.element_size()
    if isinstance(x, (tuple, list)):
        return sum(_tensor_bytes(v) for v in x)
    return 0


def derived_nbytes(t: torch.Tensor) -> int:
    """Bytes held by the derived structures attached to ``t``."""
    n = 0
    for tag in tags.CHARGED:
        v = tag.get(t)
        if v is None or v is t or v is False:
            continue
        n += _tensor_bytes(v)
        if tag is tags.PERM and isinstance(v, tuple) and v and isinstance(v[0], torch.Tensor):
            n += derived_nbytes(v[0])     # the index keys' own dense table
    return n


def column_nbytes(col) -> int:
    """Bytes of a Column including the derived structures of its data tensor."""
    return col.nbytes + derived_nbytes(col.data)


def batch_nbytes(cols: Iterable) -> int:
    return sum(column_nbytes(c) for c in cols)


def device_capacity(device) -> int:
    """Total memory of ``device`` in bytes (0 for the CPU)."""
    device = torch.device(device)
    if device.type != "cuda":
        return 0
    try:
        return torch.cuda.get_device_properties(device).total_memory
    except (RuntimeError, AssertionError):
        return 0
