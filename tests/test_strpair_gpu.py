"""The two-operand string kernels (csrc/kernels/strpair.hip) and substr_index
(strfunc.hip) on the device: SQL over a plain and a dictionary column
against plain-Python oracles, the op-level shapes of ``apply_pair``, the LDS
cap of the edit distance and its long-row kernel, and replay / graph capture
of a repeated query. Parity unpinned (see tests/test_strpair.py)."""
import random

import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
from igloo_amd.columnar import Column
from igloo_amd.ops import strfuncs as SF
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS, native

pytestmark = pytest.mark.gpu

LONG = "lorem9 ipsum42 " * 20          # one 300-byte row
WORDS = ["apple", "banana", "cherry", "Date", "elder-berry", "fig9", "grape_12", "Hello World", "", "naïve café",
         "order 66 and 7 of 12345", "aXa1 a22 A3", "ÉCOLE école 9é", "bananana an", "aaa", None, "a,b,,c", "an", ","]
_g = random.Random(23)
VALS = [_g.choice(WORDS) for _ in range(299)]
VALS.insert(130, LONG)
OTHER = [_g.choice(WORDS) for _ in range(300)]
OTHER[130] = LONG[7:] + "é"
N = len(VALS)


def lev(a, b):
    """Edit distance by the full matrix, kept as two rows of it."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def find_in_set(a, lst):
    parts = lst.split(",")
    return parts.index(a) + 1 if a in parts else 0


def substr_index(s, d, n):
    if s == "" or d == "" or n == 0:
        return ""
    return d.join(s.split(d)[:n]) if n > 0 else d.join(s.rsplit(d)[n:])


ORACLE = {
    "levenshtein": lev,
    "strpos": lambda a, b: a.find(b) + 1,
    "contains": lambda a, b: b in a,
    "starts_with": lambda a, b: a.startswith(b),
    "ends_with": lambda a, b: a.endswith(b),
    "find_in_set": find_in_set,
}
_WANT = {}


def want(name, xs, ys, key):
    """Oracle column, computed once per (function, operands)."""
    k = (name, key)
    if k not in _WANT:
        fn = ORACLE[name]
        _WANT[k] = [None if x is None or y is None else fn(x, y) for x, y in zip(xs, ys)]
    return _WANT[k]


def q(s):
    return "'" + s.replace("'", "''") + "'"


@pytest.fixture(scope="module")
def eng(gpu_device):
    e = ig.QueryEngine(device=gpu_device)
    cols = {"id": Column.from_arrow(pa.array(range(N), pa.int64()), device=gpu_device)}
    for nm, vals in (("p", VALS), ("d", VALS), ("o", OTHER), ("od", OTHER)):
        cols[nm] = Column.from_arrow(pa.array(vals, pa.string()), device=gpu_device, dict_encode=nm.endswith("d"))
    assert cols["p"].is_plain_string and cols["d"].is_dict and cols["od"].is_dict
    e.register_table("t", cols)
    return e


def run(e, sql):
    return e.sql(sql).table.to_pylist()


class device_only:
    """The block launches every kernel in ``kernels`` and takes no host step."""

    def __init__(self, *kernels):
        self.kernels = kernels

    def __enter__(self):
        self.calls = {k: KERNEL_CALLS[k] for k in self.kernels}
        self.host = sum(HOST_STEPS.values())

    def __exit__(self, et, ev, tb):
        if et is None:
            for k in self.kernels:
                assert KERNEL_CALLS[k] > self.calls[k], f"kernel {k} did not run"
            assert sum(HOST_STEPS.values()) == self.host, dict(HOST_STEPS)
        return False


CONST = "an"
CONST_HAY = "a,b,,c bananana an naïve café"


@pytest.mark.parametrize("col,other", [("p", "o"), ("d", "od")])
@pytest.mark.parametrize("name", sorted(ORACLE))
def test_sql_against_python(eng, name, col, other):
    kernel = "str_lev" if name == "levenshtein" else "str_pair"
    # (a literal second argument of strpos / starts_with / ends_with is the plan of old, checked all the same)
    with device_only(kernel):
        r = run(eng, f"select {name}({col}, {other}) cc, {name}({col}, {q(CONST)}) ck, "
                     f"{name}({q(CONST_HAY)}, {col}) kc, {name}({col}, reverse({other})) ce from t order by id")
    assert [x["cc"] for x in r] == want(name, VALS, OTHER, "cc")
    assert [x["ck"] for x in r] == want(name, VALS, [CONST] * N, "ck")
    assert [x["kc"] for x in r] == want(name, [CONST_HAY] * N, VALS, "kc")
    assert [x["ce"] for x in r] == want(name, VALS, [None if v is None else v[::-1] for v in OTHER], "ce")


@pytest.mark.parametrize("col", ["p", "d"])
def test_constant_operands_and_nulls(eng, col):
    with device_only("str_pair", "str_lev"):
        r = run(eng, f"select levenshtein({col}, 'banana') lv, contains({col}, 'an') ct, "
                     f"find_in_set({col}, 'an,apple,,aaa') fs, find_in_set('an', {col}) fr, "
                     f"strpos('bananana an', {col}) sp, levenshtein({col}, NULL) nl, "
                     f"contains(NULL, {col}) nc from t order by id")
    assert [x["lv"] for x in r] == want("levenshtein", VALS, ["banana"] * N, "banana")
    assert [x["ct"] for x in r] == want("contains", VALS, ["an"] * N, "an")
    assert [x["fs"] for x in r] == want("find_in_set", VALS, ["an,apple,,aaa"] * N, "set")
    assert [x["fr"] for x in r] == want("find_in_set", ["an"] * N, VALS, "rset")
    assert [x["sp"] for x in r] == want("strpos", ["bananana an"] * N, VALS, "hay")
    assert [x["nl"] for x in r] == [None] * N and [x["nc"] for x in r] == [None] * N


@pytest.mark.parametrize("col", ["p", "d"])
@pytest.mark.parametrize("delim,n", [(" ", 2), ("an", -2), ("aa", 1), ("aa", -1), ("é", -1), ("9 ", 19), ("", 1),
                                     ("a", 0)])
def test_substr_index(eng, col, delim, n):
    with device_only("str_fn"):
        r = run(eng, f"select substr_index({col}, {q(delim)}, {n}) v from t order by id")
    assert [x["v"] for x in r] == [None if v is None else substr_index(v, delim, n) for v in VALS]


def test_find_in_set_over_dictionary_touches_the_dictionary_only(gpu_device):
    col = Column.from_arrow(pa.array(VALS, pa.string()), device=gpu_device, dict_encode=True)
    assert col.is_dict and len(col.dictionary) < N
    k0 = KERNEL_CALLS["str_pair"]
    out, valid = SF.apply_pair(col, "an,apple,,aaa", "find_in_set")
    assert KERNEL_CALLS["str_pair"] == k0 + 1
    # the kernel saw the dictionary's rows: its result is what the codes gather from
    per_entry, _ = SF.apply_pair(col.dictionary, "an,apple,,aaa", "find_in_set")
    assert per_entry.numel() == len(col.dictionary)
    assert per_entry.tolist() == [find_in_set(v or "", "an,apple,,aaa") for v in col.dict_values()]
    codes = col.data.to(torch.int64).clamp(min=0)
    ok = valid if valid is not None else torch.ones(N, dtype=torch.bool, device=out.device)
    assert torch.equal(out[ok], per_entry[codes][ok])
    assert [v if m else None for v, m in zip(out.tolist(), ok.tolist())] == \
        want("find_in_set", VALS, ["an,apple,,aaa"] * N, "set")
    # the per-entry table is kept on the dictionary: the same call again launches nothing
    k1 = KERNEL_CALLS["str_pair"]
    SF.apply_pair(col, "an,apple,,aaa", "find_in_set")
    assert KERNEL_CALLS["str_pair"] == k1


# ------------------------------------------------------------------ op level
def _col(vals, dev):
    return Column.from_arrow(pa.array(vals, pa.large_string()), device=dev, dict_encode=False)


OP_SHAPES = {
    "0rows": ([], []),
    "1row": (["naïve"], ["naive"]),
    "empty": ([""], [""]),
    "left": ("a,b,,c", ["a", "", "c", "b,", None, "é"]),
    "right": (["banana", "", "an", None, "naïve", "bananana an"], "an"),
    "left1": (["é,e"], ["e", "é", "", ","]),         # a one-row column broadcast by n
}


@pytest.mark.parametrize("shape", sorted(OP_SHAPES))
@pytest.mark.parametrize("name", sorted(ORACLE))
def test_apply_pair_shapes(gpu_device, name, shape):
    a, b = OP_SHAPES[shape]
    n = max(len(x) for x in (a, b) if isinstance(x, list))
    xs = [a] * n if isinstance(a, str) else (a * n if len(a) == 1 and n != 1 else a)
    ys = [b] * n if isinstance(b, str) else b
    exp = [None if x is None or y is None else ORACLE[name](x, y) for x, y in zip(xs, ys)]

    def go(dev):
        out, valid = SF.apply_pair(a if isinstance(a, str) else _col(a, dev), b if isinstance(b, str) else _col(b, dev),
                                   name, n)
        assert out.numel() == n and out.dtype == (torch.bool if name in SF.PAIR_BOOL else torch.int32)
        ok = [True] * n if valid is None else valid.tolist()
        return [v if m else None for v, m in zip(out.tolist(), ok)]
    k = "str_lev" if name == "levenshtein" else "str_pair"
    k0 = KERNEL_CALLS[k]
    assert go(gpu_device) == exp
    assert KERNEL_CALLS[k] == k0 + (1 if n else 0)
    assert go("cpu") == exp


# -------------------------------------------------------------------- the cap
def _cap_rows():
    cap = native().LEV_FAST_MAX
    g = random.Random(5)

    def text(k):
        return "".join(g.choice("abcde ") for _ in range(k))
    straddle = text(cap - 1) + "é" + text(3)          # the 2-byte character is character number cap
    short = [("kitten", "sitting"), ("", "abc"), ("naïve", "naive"), (None, "a"), ("flaw", "lawn")] * 14
    head = text(cap - 1)
    edge = [(text(cap - 1), text(cap + 40)), (text(cap), text(cap)), (text(cap + 60), text(cap)),
            (head + "é", head + "e" + text(5))]       # cap characters in cap + 1 bytes
    long_ = [(text(cap + 1), text(cap + 30)), (text(2 * cap + 3), text(cap + 1)), (straddle, straddle[:cap - 1] + "e" + text(9)),
             (straddle + text(cap), "é" + straddle + text(cap - 7)), ("x" * 70000, "abc"), ("abc", "x" * 70000 + "c")]
    return cap, short, edge, long_


def test_levenshtein_cap_and_long_rows(gpu_device):
    cap, short, edge, long_ = _cap_rows()
    rows = short[:33] + long_[:3] + edge + short[33:] + long_[3:]
    a, b = _col([x for x, _ in rows], gpu_device), _col([y for _, y in rows], gpu_device)
    h0, k0 = sum(HOST_STEPS.values()), KERNEL_CALLS["str_lev"]
    out, valid = SF.apply_pair(a, b, "levenshtein")
    assert KERNEL_CALLS["str_lev"] == k0 + 2          # the LDS kernel and ONE launch for the long rows
    assert sum(HOST_STEPS.values()) == h0
    got = [v if m else None for v, m in zip(out.tolist(), valid.tolist())]
    assert got == [None if x is None or y is None else lev(x, y) for x, y in rows]
    assert got[rows.index(long_[4])] == 70000        # past 16 bits
    # without the long rows: everything fits LDS, one launch
    rows = short + edge
    a, b = _col([x for x, _ in rows], gpu_device), _col([y for _, y in rows], gpu_device)
    k0 = KERNEL_CALLS["str_lev"]
    out, valid = SF.apply_pair(a, b, "levenshtein")
    assert KERNEL_CALLS["str_lev"] == k0 + 1
    assert sum(HOST_STEPS.values()) == h0
    got = [v if m else None for v, m in zip(out.tolist(), valid.tolist())]
    assert got == [None if x is None or y is None else lev(x, y) for x, y in rows]


# ----------------------------------------------------------- replay / graphs
def test_repeated_query_replays_and_graphs(gpu_device):
    """The long-row counter reaches the host through the logged readback:
    recorded, replayed and graph-captured executions agree."""
    cap = native().LEV_FAST_MAX
    vals, other = list(VALS), list(OTHER)
    vals[7], other[7] = "ab" * cap, "ba" * (cap - 3) + "é"        # a long row that the WHERE keeps
    e = ig.QueryEngine(device=gpu_device)
    e.graphs_disabled = False
    e.register_table("t", {"id": Column.from_arrow(pa.array(range(N), pa.int64()), device=gpu_device),
                           "p": Column.from_arrow(pa.array(vals, pa.string()), device=gpu_device, dict_encode=False),
                           "o": Column.from_arrow(pa.array(other, pa.string()), device=gpu_device, dict_encode=False)})
    sql = ("select id, levenshtein(p, o) d, strpos(p, o) s, substr_index(p, 'an', 2) x from t "
           "where id % 3 <> 2 order by id")
    h0, k0 = sum(HOST_STEPS.values()), KERNEL_CALLS["str_lev"]
    first = run(e, sql)
    assert KERNEL_CALLS["str_lev"] >= k0 + 2          # the long row took the second kernel
    keep = [(i, v, w) for i, (v, w) in enumerate(zip(vals, other)) if i % 3 != 2]
    assert [x["id"] for x in first] == [i for i, _, _ in keep]
    for x, (_, v, w) in zip(first, keep):
        nul = v is None or w is None
        assert x["d"] == (None if nul else lev(v, w)), (v, w)
        assert x["s"] == (None if nul else v.find(w) + 1), (v, w)
        assert x["x"] == (None if v is None else substr_index(v, "an", 2)), v
    modes = []
    for _ in range(5):
        assert run(e, sql) == first
        modes.append(e.last_metrics["speculation"])
    assert sum(HOST_STEPS.values()) == h0
    assert modes[-1] in ("replayed", "graph"), modes


def test_explain_analyze_lists_no_host_step(eng):
    txt = eng.explain("select levenshtein(p, o), find_in_set(d, 'an,apple'), strpos(p, o), substr_index(p, ' ', -1), "
                      "contains(d, od) from t", analyze=True)
    assert "host steps: none" in txt, txt
