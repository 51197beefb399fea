"""The TRY_CAST kernels of csrc/kernels/trycast.hip on gfx950 against the plain
Python expectations of tests/trycast_cases.py, compared exactly: bits for
doubles, integers as integers, validity byte for byte. Every test asserts that
``try_parse`` / ``cast_checked`` was launched and that no host step was
noted, so neither a host fallback nor a readback can pass.

Shapes are the smallest that can go wrong: for cast_checked every n around a
lane's 8 rows, a wave and a block, each again on views that start 1 and 3
elements into their buffer (unaligned head, element-wise stores); for
try_parse sliced columns, empty strings, dictionaries, all-NULL input and
50 000 mixed rows per kind so that the grid-stride loop runs."""
import functools

import numpy as np
import pyarrow as pa
import pytest
import torch

import text_cases as C
import trycast_cases as K
import igloo_amd as ig
from igloo_amd import types as T
from igloo_amd.columnar import Column
from igloo_amd.ops import trycast as TC
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS
from test_text_values_gpu import utf8_column

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 8 * 256 + 3)
STARTS = (0, 1, 3)
N_RANDOM = 50_000


class launched:
    """The named kernel ran at least `times` and nothing left the device."""

    def __init__(self, name, times=1):
        self.name, self.times = name, times

    def __enter__(self):
        self.k0, self.h0 = KERNEL_CALLS[self.name], sum(HOST_STEPS.values())

    def __exit__(self, *exc):
        if exc[0] is None:
            assert KERNEL_CALLS[self.name] >= self.k0 + self.times, f"{self.name} was not launched"
            assert sum(HOST_STEPS.values()) == self.h0, dict(HOST_STEPS)


def dtype_of(kind):
    if kind[0] == "decimal":
        return T.DECIMAL(kind[1], kind[2])
    if kind[0] == "wide":
        return T.DECIMAL(38, kind[1])
    return T.DataType(kind[0])


_NP = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64, "float32": np.float32,
       "float64": np.float64, "decimal": np.int64}


def check(what, want, col):
    """want: ints / floats / bools with None for NULL; col: the kernel's column. Exact."""
    assert col.valid is not None and col.valid.dtype == torch.bool
    ok = col.valid.cpu().numpy()
    want_ok = np.array([v is not None for v in want], dtype=np.bool_)
    bad = np.flatnonzero(ok != want_ok)
    assert bad.size == 0, f"{what}: validity differs at {bad[:8]}, want {[want[i] for i in bad[:8]]}"
    got = col.data.cpu().numpy()
    if got.dtype.kind == "f":
        got = got.view(np.uint64 if got.dtype == np.float64 else np.uint32)
        w = np.array([0.0 if v is None else v for v in want], dtype=col.data.cpu().numpy().dtype).view(got.dtype)
    else:
        w = np.array([0 if v is None else v for v in want], dtype=got.dtype)
    bad = np.flatnonzero((got != w) & want_ok)
    assert bad.size == 0, f"{what}: values differ at {bad[:8]}: want {w[bad[:8]]}, got {got[bad[:8]]}"
    assert not got[~want_ok].any(), f"{what}: a NULL row holds a value"


# ---- cast_checked ---------------------------------------------------------------------

LONGEST = max(SIZES) + max(STARTS)


@functools.lru_cache(maxsize=None)
def numeric_case(i):
    """Case i of convert_cases, its edge values cycled to the longest shape, with expectations (computed once)."""
    src, dst, vals = K.convert_cases()[i]
    rows = [vals[j % len(vals)] for j in range(LONGEST)]
    by_value = {}
    for v in vals:
        by_value[repr(v)] = K.expect_convert(v, src, dst)
    return src, dst, rows, [by_value[repr(v)] for v in rows]


def source_tensor(src, rows, device, odd_words=False):
    if src[0] == "wide":
        flat = np.array([w for v in rows for w in K.wide_words(v)], dtype=np.int64)
        if odd_words:            # rows that start 8 bytes off a 16-byte boundary: never vector aligned
            buf = torch.from_numpy(np.concatenate([np.zeros(1, np.int64), flat])).to(device)
            return buf[1:].view(-1, 2)
        return torch.from_numpy(flat).to(device).view(-1, 2)
    return torch.from_numpy(np.array(rows, dtype=_NP[src[0]])).to(device)


@pytest.mark.parametrize("i", range(len(K.convert_cases())),
                         ids=["-".join(map(str, c[0] + c[1])) for c in K.convert_cases()])
def test_cast_checked_edges_at_every_shape(i, gpu_device):
    src, dst, rows, want = numeric_case(i)
    st, dt = dtype_of(src), dtype_of(dst)
    base = source_tensor(src, rows, gpu_device)
    mask = np.arange(LONGEST) % 5 != 2
    vbase = torch.from_numpy(mask).to(gpu_device)
    with launched("cast_checked", len(SIZES) * len(STARTS) * 2 - 6):
        for start in STARTS:
            for n in SIZES:
                x = base[start:start + n]
                got = TC.cast_checked(Column(st, x, None), dt)
                check(f"{src}->{dst} n={n} start={start}", want[start:start + n], got)
                got = TC.cast_checked(Column(st, x, vbase[start:start + n]), dt)
                check(f"{src}->{dst} n={n} start={start} masked",
                      [w if m else None for w, m in zip(want[start:start + n], mask[start:start + n])], got)
        if src[0] == "wide":
            got = TC.cast_checked(Column(st, source_tensor(src, rows, gpu_device, odd_words=True), None), dt)
            check(f"{src}->{dst} rows 8 bytes off", want, got)


def test_cast_checked_random_values(gpu_device):
    """Random magnitudes of every bit length, grouped per (source, target): more than one block each."""
    triples = K.random_convert_triples(200_000, 5)
    groups = {}
    for src, dst, v in triples:
        groups.setdefault((src, dst), []).append(v)
    with launched("cast_checked", 40):
        for (src, dst), vals in groups.items():
            if src[0] in K.INT_BITS and dst[0] in K.INT_BITS and K.INT_BITS[dst[0]] >= K.INT_BITS[src[0]]:
                continue
            want = [K.expect_convert(v, src, dst) for v in vals]
            got = TC.cast_checked(Column(dtype_of(src), source_tensor(src, vals, gpu_device), None), dtype_of(dst))
            check(f"random {src}->{dst}", want, got)


# ---- try_parse ---------------------------------------------------------------------------

def text_kinds():
    out = [(k, T.DataType(k), lambda t, k=k: K.expect_int_text(t, k), K.int_texts) for k in K.INT_BITS]
    for p, s in K.DECIMAL_TYPES:
        out.append((f"decimal{s}" if p == 18 else f"dec{p}_{s}", T.DECIMAL(p, s), lambda t, p=p, s=s: K.expect_decimal_text(t, p, s),
                    K.decimal_texts))
    out.append(("float", T.FLOAT64, C.expect_float, lambda: [t for t, _ in C.float_cases()]))
    out.append(("real", T.FLOAT32, lambda t: None if C.expect_float(t) is None else to_f32(C.expect_float(t)),
                lambda: [t for t, _ in C.float_cases()]))
    out.append(("date", T.DATE32, C.expect_date, lambda: [t for t, _ in C.date_cases()]))
    out.append(("bool", T.BOOL, K.expect_bool_text, lambda: [t for t, _ in K.BOOL_TEXTS]))
    return out


def to_f32(v):
    with np.errstate(over="ignore"):
        return float(np.float32(v))


TEXT_KINDS = text_kinds()


@pytest.mark.parametrize("name,t,expect,texts", TEXT_KINDS, ids=[k[0] for k in TEXT_KINDS])
def test_try_parse_fixed_cases_plain_sliced_masked(name, t, expect, texts, gpu_device):
    texts = list(texts()) + ["", ""]
    want = [expect(x) for x in texts]
    assert None in want and any(v is not None for v in want)
    with launched("try_parse", 4):
        check(f"{name} plain", want, TC.try_parse(utf8_column(texts, gpu_device), t))
        check(f"{name} sliced", want, TC.try_parse(utf8_column(texts, gpu_device, lead=["garbage", "12x", "", "\xff\xfe"]), t))
        valid = np.arange(len(texts)) % 7 != 0
        check(f"{name} masked", [w if m else None for w, m in zip(want, valid)],
              TC.try_parse(utf8_column(texts, gpu_device, valid=valid), t))
        check(f"{name} all NULL", [None] * len(texts),
              TC.try_parse(utf8_column(texts, gpu_device, valid=np.zeros(len(texts), dtype=np.bool_)), t))
    assert len(TC.try_parse(utf8_column([], gpu_device), t)) == 0


MIXED = [("int8", T.INT8), ("int16", T.INT16), ("int32", T.INT32), ("int64", T.INT64), ("float", T.FLOAT64), ("date", T.DATE32),
         ("decimal0", T.DECIMAL(18, 0)), ("decimal2", T.DECIMAL(18, 2)), ("decimal9", T.DECIMAL(18, 9)),
         ("decimal18", T.DECIMAL(18, 18)), ("timestamp", T.TIMESTAMP), ("bool", T.BOOL)]


@pytest.mark.parametrize("kind,t", MIXED, ids=[k for k, _ in MIXED])
def test_try_parse_mixed_random_rows(kind, t, gpu_device):
    cases = K.mixed_cases(kind, N_RANDOM, 101)
    texts, want = [c[0] for c in cases], [c[1] for c in cases]
    K.assert_quarters(want, kind)                     # on the host, before anything is sent to the device
    with launched("try_parse", 2):
        check(f"{kind} mixed", want, TC.try_parse(utf8_column(texts, gpu_device), t))
        check(f"{kind} mixed, sliced", want[5:], TC.try_parse(utf8_column(texts[5:], gpu_device, lead=texts[:5]), t))


def test_try_parse_timestamp_cases(gpu_device):
    cases = K.timestamp_cases()
    texts, want = [c[0] for c in cases] + [""], [c[1] for c in cases] + [None]
    assert sum(w is None for w in want) >= len(K.TS_REJECT)
    with launched("try_parse", 2):
        check("timestamp", want, TC.try_parse(utf8_column(texts, gpu_device), T.TIMESTAMP))
        check("timestamp sliced", want, TC.try_parse(utf8_column(texts, gpu_device, lead=["2024-01-02", "x"]), T.TIMESTAMP))


def test_try_parse_dictionary_column(gpu_device):
    """Parsed once per dictionary entry, gathered by code: the column is never decoded."""
    words = ["12", "x", "", "-7", "300", "12 ", None, "127"]
    rows = [words[(i * 5) % len(words)] for i in range(3000)]
    col = Column.from_arrow(pa.array(rows, pa.string()).dictionary_encode(), device=gpu_device)
    assert col.is_dict
    d0 = KERNEL_CALLS["str_gather"]
    with launched("try_parse", 2):
        check("dict int8", [None if r is None else K.expect_int_text(r, "int8") for r in rows], TC.try_parse(col, T.INT8))
        check("dict int32", [None if r is None else K.expect_int_text(r, "int32") for r in rows], TC.try_parse(col, T.INT32))
    assert KERNEL_CALLS["str_gather"] == d0, "the dictionary column was decoded"


# ---- a whole query, captured --------------------------------------------------------------

def test_query_with_try_cast_replays_as_a_graph(gpu_device):
    n = 5000
    cases = K.mixed_cases("int32", n, 7)
    texts, want = [c[0] for c in cases], [c[1] for c in cases]
    K.assert_quarters(want, "query input")
    xs = [(i * 7919) % 70000 - 35000 for i in range(n)]
    e = ig.QueryEngine(device=gpu_device)
    e.graphs_disabled = False
    e.register_table("t", {"id": Column.from_arrow(pa.array(range(n), pa.int64()), device=gpu_device),
                           "s": utf8_column(texts, gpu_device),
                           "x": Column.from_arrow(pa.array(xs, pa.int64()), device=gpu_device)})
    sql = "SELECT id, TRY_CAST(s AS INT) + id * 2 AS v, TRY_CAST(x AS SMALLINT) AS w FROM t"
    expect = [{"id": i, "v": None if want[i] is None else want[i] + 2 * i,
               "w": K.expect_convert(xs[i], ("int64",), ("int16",))} for i in range(n)]
    modes, reads = [], []
    with launched("try_parse"), launched("cast_checked"):
        for _ in range(4):
            assert e.sql(sql).table.to_pylist() == expect
            modes.append(e.last_metrics["speculation"])
            reads.append(e.last_metrics["readbacks"])
    print("speculation:", modes, "readbacks:", reads)
    assert modes[-1] == "graph", modes
    assert reads[-1] == 0, reads
