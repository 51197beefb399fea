"""The tensor-tag registry (igloo_amd/utils/tags.py): every ``_igloo_*``
attribute the package uses is declared there, the refused-write guard lives in
``Tag.set`` alone, and the lineage / inheritance rules behave as the gather
paths relied on when each wrote them out itself."""
import pathlib
import re

import torch

from igloo_amd.utils import memory, tags

PKG = pathlib.Path(tags.__file__).resolve().parents[1]
DECLARED = {name: v for name, v in vars(tags).items() if isinstance(v, tags.Tag)}


def _sources():
    return {p: p.read_text() for p in PKG.rglob("*.py")}


def test_registry_closure():
    src = _sources()
    attrs = {t.attr for t in DECLARED.values()}
    assert len(attrs) == len(DECLARED) == 22
    found = set()
    for text in src.values():
        found |= set(re.findall(r"_igloo_[a-z0-9_]+", text))
    # _igloo_refs lives on expression objects (sql/expr.py), not tensors
    assert found - attrs == {"_igloo_refs"}, found - attrs
    assert attrs <= found
    # every declared tag is used outside the registry; ORIGIN is read and
    # written by the registry's own origin() / inherit_take(), which are
    outside = "\n".join(text for p, text in src.items() if p.name != "tags.py")
    for name in DECLARED:
        use = r"\btags\.(origin|inherit_take)\(" if name == "ORIGIN" else rf"\btags\.{name}\.(get|set|clear)\b"
        assert re.search(use, outside), name
    # and nothing outside it touches the attributes or guards a write itself
    assert not re.search(r"""[gs]etattr\([^)]*["']_igloo_|hasattr\([^)]*_igloo_|\._igloo_[a-z_]+ *=[^=]""",
                         re.sub(r".*_igloo_refs.*", "", outside))
    assert "except (AttributeError, RuntimeError)" not in outside


def test_charged_set():
    assert tags.DERIVED == ("_igloo_narrow", "_igloo_perm", "_igloo_dense", "_igloo_hll", "_igloo_fence",
                            "_igloo_packed")
    assert memory.DERIVED_ATTRS is tags.DERIVED
    assert set(tags.CHARGED) == {t for t in DECLARED.values() if t.kind == tags.DERIVED_KIND}
    assert all(t.doc and t.kind in (tags.FACT, tags.LINEAGE, tags.DERIVED_KIND, tags.MEMO) for t in DECLARED.values())


def test_refused_write():
    class Closed:
        __slots__ = ()
    assert tags.NDV.set(Closed(), 3) is False
    assert tags.NDV.set(None, 3) is False
    assert tags.NDV.get(Closed()) is None and tags.NDV.get(Closed(), 7) == 7
    t = torch.arange(4)
    v = (0, 3)
    assert tags.BOUND.get(t) is None
    assert tags.BOUND.set(t, v) is True
    assert tags.BOUND.get(t) is v and t._igloo_bound is v
    tags.BOUND.clear(t)
    assert not hasattr(t, "_igloo_bound") and tags.BOUND.get(t) is None
    tags.BOUND.clear(t)          # clearing an absent tag is a no-op


def _src8():
    src = torch.arange(8, dtype=torch.int64) * 3
    src._igloo_sorted = True
    src._igloo_distinct = True
    return src


def test_inherit_take():
    idx = torch.tensor([1, 4, 6])
    src = _src8()
    plain = src[idx]
    tags.inherit_take(plain, src, idx)                     # no incr tag on the index: nothing is known
    assert not hasattr(plain, "_igloo_sorted") and not hasattr(plain, "_igloo_distinct")
    idx._igloo_incr = True
    dst = src[idx]
    tags.inherit_take(dst, src, idx)
    assert dst._igloo_sorted is True and dst._igloo_distinct is True
    assert not hasattr(dst, "_igloo_origin")               # the source is no resident column
    only_sorted, only_distinct, compacted = src[idx], src[idx], src[idx]
    tags.inherit_take(only_sorted, src, idx, distinct=False)
    assert only_sorted._igloo_sorted is True and not hasattr(only_sorted, "_igloo_distinct")
    tags.inherit_take(only_distinct, src, idx, sorted=False)
    assert only_distinct._igloo_distinct is True and not hasattr(only_distinct, "_igloo_sorted")
    tags.inherit_take(compacted, src, True)                # rows kept in order without an index
    assert compacted._igloo_sorted is True and compacted._igloo_distinct is True
    src._igloo_sorted = False                              # a known-unsorted source never yields sorted
    for i in (idx, True):
        out = src[idx]
        tags.inherit_take(out, src, i)
        assert not hasattr(out, "_igloo_sorted") and out._igloo_distinct is True


def test_lineage():
    from igloo_amd import types as T
    from igloo_amd.columnar import Column
    res = torch.arange(8, dtype=torch.int64)
    res._igloo_resident = True
    assert tags.origin(res) is res
    assert tags.origin(torch.arange(8)) is None
    same = torch.arange(4, dtype=torch.int64)
    same._igloo_base = (Column(T.INT64, res), 8)
    assert tags.base_column(same) is res and tags.origin(same) is res
    other = torch.arange(4, dtype=torch.int32)
    other._igloo_base = (Column(T.INT64, res), 8)
    assert tags.base_column(other) is None and tags.origin(other) is None
    res2 = torch.arange(8, dtype=torch.int64)
    res2._igloo_resident = True
    same._igloo_origin = res2                              # an explicit origin wins over the base
    assert tags.origin(same) is res2
    dst = same[:2]
    tags.inherit_take(dst, same, None)                     # the origin carries over whatever the index
    assert dst._igloo_origin is res2 and not hasattr(dst, "_igloo_sorted")
    from igloo_amd.ops import gather
    assert gather.origin is tags.origin


def test_cpu_gather_end_to_end():
    """mask_to_indices -> take_many on CPU tensors: the index is tagged
    increasing, and the CPU gather passes NO tag on (only the device gather
    paths call inherit_take) -- as before the registry existed."""
    from igloo_amd import types as T
    from igloo_amd.columnar import Column
    from igloo_amd.ops.gather import take_many
    from igloo_amd.ops.select import mask_to_indices
    col = torch.arange(16, dtype=torch.int64) * 2
    col._igloo_resident = col._igloo_sorted = col._igloo_distinct = True
    mask = torch.zeros(16, dtype=torch.bool)
    mask[[0, 3, 4, 9, 15]] = True
    idx = mask_to_indices(mask)
    assert idx._igloo_incr is True and idx.tolist() == [0, 3, 4, 9, 15]
    out = take_many([Column(T.INT64, col)], idx)[0].data
    assert out.tolist() == [0, 6, 8, 18, 30]
    assert [hasattr(out, a) for a in ("_igloo_origin", "_igloo_sorted", "_igloo_distinct")] == [False] * 3


def test_derived_bytes():
    keys = torch.arange(10, dtype=torch.int64)
    perm = torch.arange(10, dtype=torch.int32)
    first = torch.zeros(11, dtype=torch.int32)
    keys._igloo_dense = (0, 9, first)
    t = torch.arange(10, dtype=torch.int64)
    t._igloo_perm = (keys, perm)
    assert memory.derived_nbytes(t) == 10 * 8 + 10 * 4 + 11 * 4
    hist = torch.arange(10, dtype=torch.int64)
    hist._igloo_key_hist = (0, 64, torch.zeros(64, dtype=torch.int64))
    assert memory.derived_nbytes(hist) == 0                # a memo: not charged to the column
