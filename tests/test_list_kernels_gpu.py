"""The list kernels (csrc/kernels/nested.hip) at op level, through
igloo_amd.ops.nested, against the CPU path of the same op.

Rows alias and overlap each other's child ranges, leave parts of the child
unreferenced and start near its end; 1 / 64 / 65 / 257 rows reach the tail
wave and the second block; lengths 0 / 1 / 63 / 64 / 65 / 200 reach both the
lane-per-row and the wave-per-row schedule. The quadratic functions (set
functions, sort) run three ways -- the LDS kernels, the generic path (bound
lowered to 8, or a 513-element row at the real bound of 512) and the CPU --
and must agree; KERNEL_CALLS tells which path ran."""
import random

import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
from igloo_amd import types as T
from igloo_amd.columnar import Column, Nested
from igloo_amd.ops import nested as NS
from igloo_amd.ops._lib import KERNEL_CALLS

pytestmark = pytest.mark.gpu

ROWS = [1, 64, 65, 257]
LENS = [0, 1, 63, 64, 65, 200]
CHILD_N = 300


def _list(n, seed, child_n=CHILD_N, lens=LENS, width=9, nulls=True):
    """CPU LIST<BIGINT> column of n rows over one shared child."""
    g = random.Random(seed)
    se, valid = [], []
    for _ in range(n):
        ln = g.choice(lens)
        st = g.choice([child_n - ln, g.randint(0, child_n - ln)])     # every other row ends at the child's end
        se.append([st, ln])
        valid.append(g.random() > 0.1)
    data = torch.tensor([g.randrange(width) for _ in range(child_n)], dtype=torch.int64)
    cvalid = torch.tensor([g.random() > 0.15 for _ in range(child_n)]) if nulls else None
    return Column(T.LIST(T.INT64), torch.tensor(se, dtype=torch.int64).reshape(n, 2), torch.tensor(valid),
                  dictionary=Nested(child=Column(T.INT64, data, cvalid)))


def _ints(n, seed, lo, hi, nulls=True):
    g = random.Random(seed)
    return Column(T.INT64, torch.tensor([g.randint(lo, hi) for _ in range(n)], dtype=torch.int64),
                  torch.tensor([g.random() > 0.1 for _ in range(n)]) if nulls else None)


def _dev(c, dev):
    if c is None:
        return None
    if c.dtype.kind == "list":
        return Column(c.dtype, c.data.to(dev), None if c.valid is None else c.valid.to(dev),
                      dictionary=Nested(child=_dev(c.nested.child, dev)))
    return Column(c.dtype, c.data.to(dev), None if c.valid is None else c.valid.to(dev))


def _py(c):
    return c.to_arrow().to_pylist()


def _both(gpu_device, fn, *cols):
    """fn over CPU columns and over their device copies."""
    return _py(fn(*cols)), _py(fn(*[_dev(c, gpu_device) for c in cols]))


LINEAR = {
    "slice": lambda l, m, x, k: NS.slice_(l, x.data, k.data, x.valid, k.valid),
    "slice_const": lambda l, m, x, k: NS.slice_(l, -70, -2),
    "pop_front": lambda l, m, x, k: NS.pop_front(l),
    "pop_back": lambda l, m, x, k: NS.pop_back(l),
    "append": lambda l, m, x, k: NS.append(l, x, l.dtype),
    "prepend": lambda l, m, x, k: NS.append(l, x, l.dtype, front=True),
    "concat": lambda l, m, x, k: NS.concat_lists([l, m, l], l.dtype),
    "reverse": lambda l, m, x, k: NS.reverse(l),
    "repeat": lambda l, m, x, k: NS.repeat(x, k.data, k.valid, l.dtype),
    "resize": lambda l, m, x, k: NS.resize(l, k.data, k.valid, x),
    "resize_null": lambda l, m, x, k: NS.resize(l, k.data, k.valid, None),
    "position": lambda l, m, x, k: NS.position(l, x),
    "position_from": lambda l, m, x, k: NS.position(l, x, k.data, k.valid),
    "has": lambda l, m, x, k: NS.has_value(l, x),
    "positions": lambda l, m, x, k: NS.positions(l, x),
    "remove": lambda l, m, x, k: NS.remove(l, x, 1),
    "remove_n": lambda l, m, x, k: NS.remove(l, x, k.data, k.valid),
    "remove_all": lambda l, m, x, k: NS.remove(l, x),
    "replace_n": lambda l, m, x, k: NS.replace(l, x, k, k.data, k.valid),
    "replace_all": lambda l, m, x, k: NS.replace(l, x, k),
    "max": lambda l, m, x, k: NS.extreme(l, True),
    "min": lambda l, m, x, k: NS.extreme(l, False),
}

QUADRATIC = {
    "distinct": lambda l, m: NS.distinct(l),
    "union": lambda l, m: NS.union(l, m),
    "intersect": lambda l, m: NS.intersect(l, m),
    "except": lambda l, m: NS.except_(l, m),
    "has_all": lambda l, m: NS.has_all(l, m),
    "has_any": lambda l, m: NS.has_any(l, m),
    "sort": lambda l, m: NS.sort(l),
    "sort_desc_last": lambda l, m: NS.sort(l, True, False),
}
FAST = ("list_set_count", "list_sort_idx")
GENERIC = ("list_set_generic", "list_sort_generic")


def _calls(names):
    return sum(KERNEL_CALLS[n] for n in names)


@pytest.mark.parametrize("n", ROWS)
def test_linear_kernels(gpu_device, n):
    l, m = _list(n, 1 + n), _list(n, 2 + n)
    x, k = _ints(n, 3 + n, 0, 9), _ints(n, 4 + n, -3, 70)
    before = _calls(["list_slice_se", "list_parts_write", "list_match_count", "list_match_write", "list_minmax_idx"])
    for name, fn in LINEAR.items():
        want, got = _both(gpu_device, fn, l, m, x, k)
        assert got == want, name
    assert _calls(["list_slice_se", "list_parts_write", "list_match_count", "list_match_write",
                   "list_minmax_idx"]) >= before + len(LINEAR)


@pytest.mark.parametrize("n", ROWS)
def test_flatten_kernel(gpu_device, n):
    inner = _list(90, 5 + n, lens=[0, 1, 5, 64, 70])
    g = random.Random(n)
    se = [[g.randint(0, 20), g.choice([0, 1, 3, 64, 70])] for _ in range(n)]
    outer = Column(T.LIST(inner.dtype), torch.tensor(se, dtype=torch.int64).reshape(n, 2),
                   torch.tensor([g.random() > 0.1 for _ in range(n)]), dictionary=Nested(child=inner))
    want = _py(NS.flatten(outer))
    dev_outer = Column(outer.dtype, outer.data.to(gpu_device), outer.valid.to(gpu_device),
                       dictionary=Nested(child=_dev(inner, gpu_device)))
    before = KERNEL_CALLS["list_flatten_write"]
    assert _py(NS.flatten(dev_outer)) == want
    assert KERNEL_CALLS["list_flatten_write"] == before + 1


@pytest.mark.parametrize("bound", [512, 8])
@pytest.mark.parametrize("n", ROWS)
def test_quadratic_kernels(gpu_device, monkeypatch, n, bound):
    monkeypatch.setattr(NS, "LIST_FAST_MAX", bound)
    l, m = _list(n, 6 + n, width=40), _list(n, 7 + n, width=40)
    for name, fn in QUADRATIC.items():
        fast, generic = _calls(FAST), _calls(GENERIC)
        want, got = _both(gpu_device, fn, l, m)
        assert got == want, name
        longest = max(int(NS._vlen(c).max()) for c in ((l,) if name in ("distinct",) or "sort" in name else (l, m)))
        if longest <= bound:
            assert _calls(FAST) > fast and _calls(GENERIC) == generic + 1, name     # + 1: the CPU run
        else:
            assert _calls(GENERIC) == generic + 2, name


@pytest.mark.parametrize("longest", [512, 513])
def test_quadratic_kernels_at_the_bound(gpu_device, longest):
    assert NS.LIST_FAST_MAX == 512 == NS.launch_bound()
    lens = [511, longest, 3, 0, 512]
    child_n = 1100
    l = _list(5, 31, child_n=child_n, lens=[0], width=300)
    m = _list(5, 32, child_n=child_n, lens=[0], width=300)
    for c, shift in ((l, 0), (m, 40)):
        c.data[:, 1] = torch.tensor(lens)
        c.data[:, 0] = torch.tensor([shift, child_n - longest, 17, 5, child_n - 512 - shift])
        c.valid[:] = True
    for name, fn in QUADRATIC.items():
        fast, generic = _calls(["list_set_write", "list_sort_idx"]), _calls(GENERIC)
        want, got = _both(gpu_device, fn, l, m)
        assert got == want, name
        if longest <= 512:
            assert _calls(GENERIC) == generic + 1, name
            if not name.startswith("has"):
                assert _calls(["list_set_write", "list_sort_idx"]) == fast + 1, name
        else:
            assert _calls(GENERIC) == generic + 2, name
            assert _calls(["list_set_write", "list_sort_idx"]) == fast, name


def test_string_lists(gpu_device):
    words = ["apple", "fig", "", "naïve café", "kiwi", None, "Zed"]
    g = random.Random(5)
    rows = [None if i % 7 == 0 else [g.choice(words) for _ in range(g.choice([0, 1, 5, 20, 70]))] for i in range(65)]
    needle = [g.choice(words) for _ in range(65)]
    cpu = Column.from_arrow(pa.array(rows, pa.list_(pa.string())), device="cpu")
    dev = Column.from_arrow(pa.array(rows, pa.list_(pa.string())), device=gpu_device)
    xc = Column.from_arrow(pa.array(needle, pa.string()), device="cpu")
    xd = Column.from_arrow(pa.array(needle, pa.string()), device=gpu_device)
    for fn in (NS.distinct, NS.sort, lambda c: NS.sort(c, True, False), lambda c: NS.extreme(c, True), NS.reverse,
               lambda c: NS.union(c, NS.reverse(c)), lambda c: NS.except_(c, NS.slice_(c, 1, 2))):
        assert _py(fn(dev)) == _py(fn(cpu))
    for fn in (NS.position, NS.positions, NS.has_value, NS.remove, lambda c, x: NS.replace(c, x, x),
               lambda c, x: NS.append(c, x, c.dtype)):
        assert _py(fn(dev, xd)) == _py(fn(cpu, xc))


def test_repeated_list_query_replays_and_graphs(gpu_device):
    """The output sizes of the list kernels reach the host through the
    speculation log: the recorded, the replayed and the graph-captured
    executions return the same rows."""
    g = random.Random(9)
    rows = [None if i % 13 == 0 else [g.choice([None, g.randint(0, 9)]) for _ in range(g.choice([0, 2, 5, 66, 130]))]
            for i in range(200)]
    e = ig.QueryEngine(device=gpu_device)
    e.graphs_disabled = False
    e.register_table("t", pa.table({"id": pa.array(range(200), pa.int64()),
                                    "l": pa.array(rows, pa.list_(pa.int64()))}))
    sql = ("select id, array_sort(array_distinct(l)) d, array_remove_all(l, id % 10) r, l[2:4] || l s, "
           "array_position(l, 3) p from t where id % 3 <> 1 order by id")
    first = e.sql(sql).table.to_pylist()
    assert len(first) == sum(1 for i in range(200) if i % 3 != 1)
    assert first[3]["d"] == (None if rows[first[3]["id"]] is None else
                             sorted(set(rows[first[3]["id"]]), key=lambda v: (v is not None, v)))
    for _ in range(3):
        assert e.sql(sql).table.to_pylist() == first
