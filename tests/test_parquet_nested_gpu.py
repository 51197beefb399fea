"""LIST / MAP / STRUCT Parquet columns decoded on the GPU
(csrc/kernels/parquet_nested.hip + the entry-space leaves of parquet.hip) vs
pyarrow's decoder on the same file.

Shapes are the smallest at which the level kernels can go wrong: NULL, empty
and one-element lists next to each other, a first row that is NULL and a last
row that is empty, one 5,000-element list that spans several 512-byte pages
(and several 256-lane passes of one workgroup), three row groups with a
partial last one, two files in one table, data page v1 and v2, and every
codec whose levels sit in another place (v1 compressed pages keep them inside
the compressed payload).
"""
import datetime
import decimal

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from igloo_amd import types as T
from igloo_amd.connectors.gpu_parquet import GpuParquetReader
from igloo_amd.ops._lib import KERNEL_CALLS
from parquet_legacy_list import write_two_level_list

pytestmark = pytest.mark.gpu

N_EDGE = 2000


def _edge_lists(n=N_EDGE, big=5000):
    cycle = [[1, 2, None], None, [], [4]]
    rows = [cycle[i % 4] for i in range(n)]
    rows[0] = None                                   # first row NULL
    rows[n // 2 + 1] = list(range(big))              # one row across many pages
    rows[n - 1] = []                                 # last row empty
    return rows


@pytest.fixture(scope="module")
def edge_table():
    return pa.table({"l": pa.array(_edge_lists(), pa.list_(pa.int64()))})


def _read(paths, cols, device, groups=None):
    r = GpuParquetReader(list(paths))
    if groups is None:
        groups = [(fi, g) for fi, m in enumerate(r.metas) for g in range(len(m.row_groups))]
    got, rejected = r.read(cols, groups, device)
    assert rejected == {}, rejected
    return got


def _check(path, t, device, dtypes=None):
    schema = pq.read_schema(path)
    cols = [(f.name, (dtypes or {}).get(f.name) or T.from_arrow_type(f.type)) for f in schema]
    got = _read([path], cols, device)
    ref = pq.read_table(path)
    for name, _ in cols:
        assert got[name].to_arrow().to_pylist() == ref.column(name).to_pylist(), name
    return got


@pytest.mark.parametrize("use_dictionary", [True, False])
@pytest.mark.parametrize("compression", ["none", "snappy", "zstd"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_edge_lists(tmp_path, gpu_device, edge_table, version, compression, use_dictionary):
    path = str(tmp_path / "edge.parquet")
    pq.write_table(edge_table, path, data_page_version=version, compression=compression, data_page_size=512,
                   row_group_size=700, use_dictionary=use_dictionary)
    assert pq.ParquetFile(path).metadata.num_row_groups == 3
    before = KERNEL_CALLS["pq_list_rows"]
    got = _check(path, edge_table, gpu_device)
    assert KERNEL_CALLS["pq_list_rows"] > before
    col = got["l"]
    assert tuple(col.data.shape) == (N_EDGE, 2)
    # the child lives in entry space: one row per element, plus one per empty or NULL list
    want = sum(len(r) if r else 1 for r in edge_table.column("l").to_pylist())
    assert len(col.dictionary.child) == want


def test_two_files_accumulate_entry_bases(tmp_path, gpu_device, edge_table):
    a, b = str(tmp_path / "a.parquet"), str(tmp_path / "b.parquet")
    other = pa.table({"l": pa.array([[7, 8], [], None, [9]] * 300 + [[10]], pa.list_(pa.int64()))})
    pq.write_table(edge_table, a, data_page_size=512, row_group_size=700)
    pq.write_table(other, b, data_page_size=512, row_group_size=500, data_page_version="2.0", compression="zstd")
    got = _read([a, b], [("l", T.LIST(T.INT64))], gpu_device)
    want = edge_table.column("l").to_pylist() + other.column("l").to_pylist()
    assert got["l"].to_arrow().to_pylist() == want
    # a subset of the row groups, starting inside the second file
    got = _read([a, b], [("l", T.LIST(T.INT64))], gpu_device, groups=[(0, 2), (1, 1), (1, 2)])
    assert got["l"].to_arrow().to_pylist() == want[1400:2000] + other.column("l").to_pylist()[500:]


@pytest.mark.parametrize("rows", [[None] * 777, [[]] * 777], ids=["all-null", "all-empty"])
def test_degenerate_list_columns(tmp_path, gpu_device, rows):
    t = pa.table({"l": pa.array(rows, pa.list_(pa.int64()))})
    path = str(tmp_path / "d.parquet")
    pq.write_table(t, path, row_group_size=300)
    _check(path, t, gpu_device)


def test_zero_row_groups(tmp_path, gpu_device):
    t = pa.table({"l": pa.array([[1], None], pa.list_(pa.int64())),
                  "m": pa.array([[("a", 1)], None], pa.map_(pa.string(), pa.int64())),
                  "s": pa.array([{"a": 1}, None], pa.struct([("a", pa.int64())]))})
    path = str(tmp_path / "z.parquet")
    pq.write_table(t, path)
    cols = [(f.name, T.from_arrow_type(f.type)) for f in t.schema]
    got = _read([path], cols, gpu_device, groups=[])
    for name, _ in cols:
        assert got[name].to_arrow().to_pylist() == []


def _cycled(values, n=1500):
    """n list rows over ``values``: a NULL, an empty, a one-element and a three-element list (with a NULL) in turn."""
    k = len(values)
    shapes = [lambda i: None, lambda i: [], lambda i: [values[i % k]],
              lambda i: [values[i % k], None, values[(i + 1) % k]]]
    return [shapes[i % 4](i) for i in range(n)]


ELEMENTS = {
    "double": (pa.float64(), [0.5, -1.25, 3e300, 0.0], None),
    "bool": (pa.bool_(), [True, False, False, True, True], None),
    "date": (pa.date32(), [datetime.date(1970, 1, 1), datetime.date(2024, 2, 29), datetime.date(1969, 12, 31)], None),
    "decimal": (pa.decimal128(15, 2), [decimal.Decimal("1.25"), decimal.Decimal("-9999999999999.99"),
                                       decimal.Decimal("0.00")], None),
    "int32-as-bigint": (pa.int32(), [-2**31, 2**31 - 1, 0, 7], T.LIST(T.INT64)),
    "utf8-dict": (pa.string(), ["alpha", "", "beta", "gamma-" * 9], None),
    "utf8-plain": (pa.string(), [f"row-{i}-{'x' * (i % 23)}" for i in range(997)], None),
}


@pytest.mark.parametrize("kind", sorted(ELEMENTS))
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_element_types(tmp_path, gpu_device, kind, version):
    at, values, dt = ELEMENTS[kind]
    t = pa.table({"l": pa.array(_cycled(values), pa.list_(at))})
    path = str(tmp_path / "e.parquet")
    pq.write_table(t, path, data_page_version=version, data_page_size=2048, row_group_size=600,
                   use_dictionary=kind != "utf8-plain")
    if kind.startswith("utf8"):
        enc = pq.ParquetFile(path).metadata.row_group(0).column(0).encodings
        assert ("RLE_DICTIONARY" in enc or "PLAIN_DICTIONARY" in enc) == (kind == "utf8-dict")
    got = _check(path, t, gpu_device, {"l": dt} if dt else None)
    if dt:
        assert got["l"].dtype == dt
    if kind.startswith("utf8"):
        assert got["l"].dictionary.child.is_plain_string       # string children are plain columns


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_required_list_of_required_int32(tmp_path, gpu_device, version):
    f = pa.field("l", pa.list_(pa.field("element", pa.int32(), nullable=False)), nullable=False)
    rows = [[i, i + 1] if i % 3 == 0 else [] if i % 3 == 1 else [i] for i in range(1300)]
    t = pa.table([pa.array(rows, f.type)], schema=pa.schema([f]))
    path = str(tmp_path / "r.parquet")
    pq.write_table(t, path, data_page_version=version, data_page_size=512, row_group_size=500)
    leaf = GpuParquetReader([path]).metas[0].leaves[0]
    assert (leaf["max_def"], leaf["max_rep"]) == (1, 1)
    got = _check(path, t, gpu_device)
    assert got["l"].valid is None                               # a required list has no validity


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_legacy_two_level_list(tmp_path, gpu_device, version):
    """``optional group l (LIST) { repeated int32 element; }``: the leaf is the repeated node."""
    rows = [[i, -i] if i % 4 == 0 else None if i % 4 == 1 else [] if i % 4 == 2 else [i] for i in range(1300)]
    rows[650] = list(range(3000))
    path = str(tmp_path / "l2.parquet")
    t = write_two_level_list(path, rows, data_page_version=version, data_page_size=512, row_group_size=500,
                             compression="snappy")
    leaf = GpuParquetReader([path]).metas[0].leaves[0]
    assert (leaf["name"], leaf["kind"], leaf["max_rep"], leaf["rep_def"], leaf["max_def"]) == ("l.element", "list", 1, 2, 2)
    before = KERNEL_CALLS["pq_list_rows"]
    got = _check(path, t, gpu_device)
    assert KERNEL_CALLS["pq_list_rows"] > before
    assert got["l"].to_arrow().to_pylist() == rows


@pytest.mark.parametrize("compression", ["none", "snappy"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_map_utf8_int64(tmp_path, gpu_device, version, compression):
    rows = [None if i % 5 == 0 else [] if i % 5 == 1 else [("k%d" % (i % 7), i), ("b", None)] if i % 5 == 2
            else [("b", i)] if i % 5 == 3 else [("a", None), ("c", -i), ("k", 2**40 + i)] for i in range(1700)]
    t = pa.table({"m": pa.array(rows, pa.map_(pa.string(), pa.int64()))})
    path = str(tmp_path / "m.parquet")
    pq.write_table(t, path, data_page_version=version, compression=compression, data_page_size=512,
                   row_group_size=600)
    before = KERNEL_CALLS["pq_list_rows"]
    got = _check(path, t, gpu_device)
    assert KERNEL_CALLS["pq_list_rows"] == before + 1           # rows come from the key leaf alone
    kids = got["m"].dictionary.children
    assert len(kids["key"]) == len(kids["value"])


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_structs(tmp_path, gpu_device, version):
    st = pa.struct([pa.field("a", pa.int64()), pa.field("b", pa.string())])
    rq = pa.struct([pa.field("a", pa.int64(), nullable=False), pa.field("b", pa.string())])
    n = 1900
    s_rows = [None if i % 4 == 0 else {"a": None if i % 3 == 0 else i, "b": None if i % 5 == 0 else "s%d" % (i % 13)}
              for i in range(n)]
    r_rows = [{"a": i, "b": None if i % 2 else "r%d" % i} for i in range(n)]
    q_rows = [None if i % 7 == 0 else {"a": -i, "b": "q"} for i in range(n)]   # optional struct, required field
    schema = pa.schema([pa.field("s", st), pa.field("r", rq, nullable=False), pa.field("q", rq)])
    t = pa.table([pa.array(s_rows, st), pa.array(r_rows, rq), pa.array(q_rows, rq)], schema=schema)
    path = str(tmp_path / "s.parquet")
    pq.write_table(t, path, data_page_version=version, data_page_size=512, row_group_size=700)
    before = KERNEL_CALLS["pq_struct_valid"]
    got = _check(path, t, gpu_device)
    assert KERNEL_CALLS["pq_struct_valid"] == before + 2        # s and q; the required struct needs none
    assert got["r"].valid is None


def _sql_table(n=1200):
    ls = [[1, 2, None], None, [], [4], [4, 5, 6, 7]]
    ms = [[("a", 1), ("b", 2)], None, [], [("b", None)], [("c", 3)]]
    return pa.table({
        "id": pa.array(range(n), pa.int64()),
        "l": pa.array([ls[i % 5] if i % 11 else [i, 4] for i in range(n)], pa.list_(pa.int64())),
        "m": pa.array([ms[(i + 2) % 5] for i in range(n)], pa.map_(pa.string(), pa.int64())),
        "s": pa.array([None if i % 6 == 0 else {"a": None if i % 4 == 0 else i, "b": "s%d" % (i % 9)}
                       for i in range(n)], pa.struct([("a", pa.int64()), ("b", pa.string())])),
    })


QUERIES = [
    "select id, l[1], array_length(l), cardinality(m), m['b'], s.a from t order by id",
    "select id, unnest(l) from t",
    "select count(*) from t where array_has(l, 4)",
]


def test_sql_end_to_end(tmp_path, gpu_device):
    """Nested Parquet columns feed the device kernels without the host decoder:
    the same queries on the CPU engine give the same rows, and no column of the
    scan was left to the host. Repeated three times (replay / graph capture of
    the downstream plan over the decoded columns)."""
    import igloo_amd as ig
    path = str(tmp_path / "t.parquet")
    pq.write_table(_sql_table(), path, row_group_size=500, data_page_size=1024)
    cpu = ig.QueryEngine(device="cpu")
    cpu.register_parquet("t", path)
    gpu = ig.QueryEngine(device=gpu_device)
    src = gpu.register_parquet("t", path)
    for q in QUERIES:
        want = cpu.query(q).to_pylist()
        if "order by" not in q:
            want = sorted(want, key=repr)
        assert want, q
        for _ in range(3):
            have = gpu.query(q).to_pylist()
            if "order by" not in q:
                have = sorted(have, key=repr)
            assert have == want, q
            # every scan so far decoded all of its columns on the device
            assert src.last_gpu_stats and src.last_gpu_stats["host_columns"] == [], src.last_gpu_stats
