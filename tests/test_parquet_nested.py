"""Nested Parquet columns on the native metadata path (CPU): what the footer
decoder reports for LIST / MAP / STRUCT leaves (``rep_def``, ``anc_def``,
``top``, ``kind``) and how the page planner lays their pages out in entry
space (csrc/io/parquet_meta.cpp). The device decode is covered by
tests/test_parquet_nested_gpu.py."""
import struct

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from igloo_amd import types as T
from igloo_amd.connectors.gpu_parquet import FileMeta, GpuParquetReader
from igloo_amd.ops._lib import native
from parquet_legacy_list import write_two_level_list


def _list_type(list_nullable, elem_nullable, elem=pa.int64()):
    return pa.field("l", pa.list_(pa.field("element", elem, nullable=elem_nullable)), nullable=list_nullable)


def _write(path, fields, arrays, **kw):
    schema = pa.schema(fields)
    pq.write_table(pa.table(arrays, schema=schema), path, **kw)
    return FileMeta(path)


@pytest.mark.parametrize("list_nullable", [True, False])
@pytest.mark.parametrize("elem_nullable", [True, False])
def test_footer_list_levels(tmp_path, list_nullable, elem_nullable):
    f = _list_type(list_nullable, elem_nullable)
    m = _write(str(tmp_path / "l.parquet"), [f], [pa.array([[1, 2], [], [3]], f.type)])
    (leaf,) = m.leaves
    assert leaf["name"] == "l.list.element" and leaf["top"] == "l" and leaf["kind"] == "list"
    assert leaf["max_rep"] == 1
    assert leaf["anc_def"] == int(list_nullable)
    assert leaf["rep_def"] == int(list_nullable) + 1          # the repeated node adds a level
    assert leaf["max_def"] == leaf["rep_def"] + int(elem_nullable)


def test_footer_legacy_two_level_list(tmp_path):
    """``optional group l (LIST) { repeated int32 element; }``: the repeated node is the leaf
    (pyarrow reads this form but cannot write it: tests/parquet_legacy_list.py)."""
    path = str(tmp_path / "l2.parquet")
    rows = [[1, 2], None, [], [3]] * 300
    write_two_level_list(path, rows, data_page_size=512, row_group_size=500)
    ref = pq.ParquetFile(path).schema
    assert len(ref) == 1 and ref.column(0).path == "l.element"          # no middle group
    assert (ref.column(0).max_repetition_level, ref.column(0).max_definition_level) == (1, 2)
    assert pq.read_table(path).column("l").to_pylist() == rows
    m = FileMeta(path)
    (leaf,) = m.leaves
    assert leaf["name"] == "l.element" and leaf["top"] == "l" and leaf["kind"] == "list"
    assert leaf["max_rep"] == 1 and leaf["anc_def"] == 1
    assert leaf["rep_def"] == leaf["max_def"] == 2
    at = pq.read_schema(path).field("l").type
    assert GpuParquetReader([path]).supports("l", T.from_arrow_type(at)) is None
    host, chunks = _stage(path, m, 0)
    plan = native().pq_plan(host.ctypes.data, chunks, leaf["type"], leaf["max_def"], leaf["max_rep"])
    assert plan["unsupported"] == "" and plan["num_entries"] == sum(len(r) if r else 1 for r in rows)
    assert plan["num_level_pages"] >= len(m.row_groups) == 3


def test_list_of_one_field_structs_is_left_to_the_host(tmp_path):
    """A 3-level list whose element is a group of one field is a list of structs, not a list."""
    ls = pa.list_(pa.struct([("a", pa.int64())]))
    path = str(tmp_path / "ls1.parquet")
    pq.write_table(pa.table({"ls": pa.array([[{"a": 1}], None], ls)}), path)
    (leaf,) = FileMeta(path).leaves
    assert leaf["kind"] == "nested" and leaf["max_rep"] == 1
    assert GpuParquetReader([path]).supports("ls", T.from_arrow_type(ls)) is not None


def test_footer_map_struct_and_flat(tmp_path):
    mt = pa.map_(pa.string(), pa.int64())
    st = pa.struct([pa.field("a", pa.int64()), pa.field("b", pa.string(), nullable=False)])
    fields = [pa.field("id", pa.int64(), nullable=False), pa.field("m", mt), pa.field("s", st),
              pa.field("rs", st, nullable=False)]
    m = _write(str(tmp_path / "ms.parquet"), fields,
               [pa.array([1, 2]), pa.array([[("a", 1)], None], mt), pa.array([{"a": 1, "b": "x"}, None], st),
                pa.array([{"a": None, "b": "y"}, {"a": 2, "b": "z"}], st)])
    by = {l["name"]: l for l in m.leaves}
    assert [l["name"] for l in m.leaves] == ["id", "m.key_value.key", "m.key_value.value", "s.a", "s.b", "rs.a", "rs.b"]
    assert by["id"]["kind"] == "flat" and by["id"]["top"] == "id"
    assert (by["id"]["rep_def"], by["id"]["anc_def"], by["id"]["max_def"]) == (0, 0, 0)
    k, v = by["m.key_value.key"], by["m.key_value.value"]
    assert (k["kind"], v["kind"]) == ("map_key", "map_value") and k["top"] == v["top"] == "m"
    assert (k["rep_def"], k["anc_def"], k["max_def"], k["max_rep"]) == (2, 1, 2, 1)
    assert (v["rep_def"], v["anc_def"], v["max_def"], v["max_rep"]) == (2, 1, 3, 1)
    for name, anc, md in (("s.a", 1, 2), ("s.b", 1, 1), ("rs.a", 0, 1), ("rs.b", 0, 0)):
        l = by[name]
        assert l["kind"] == "struct_field" and l["top"] == name.split(".")[0]
        assert (l["rep_def"], l["anc_def"], l["max_def"], l["max_rep"]) == (0, anc, md, 0)


def _stage(path, m, li):
    """The leaf's chunks staged back to back: (buffer, chunk tuples with the footer's value counts)."""
    total = sum(g["chunks"][li]["length"] for g in m.row_groups)
    host = np.zeros(total + 64, dtype=np.uint8)
    chunks, off, row = [], 0, 0
    for g in m.row_groups:
        c = g["chunks"][li]
        native().pq_pread(path, [(c["start"], c["length"], host.ctypes.data + off)], 1)
        chunks.append((off, c["length"], c["codec"], row, g["num_rows"], c["num_values"]))
        off += c["length"]
        row += g["num_rows"]
    return host, chunks


def _nested_table(n=3000):
    lists = [[i, None, i + 1] if i % 4 == 0 else None if i % 4 == 1 else [] if i % 4 == 2 else [i] for i in range(n)]
    maps = [None if i % 5 == 0 else [] if i % 5 == 1 else [("k%d" % (i % 7), i), ("z", None)] for i in range(n)]
    structs = [None if i % 6 == 0 else {"a": None if i % 3 == 0 else i, "b": "s%d" % (i % 11)} for i in range(n)]
    return pa.table({"l": pa.array(lists, pa.list_(pa.int64())),
                     "m": pa.array(maps, pa.map_(pa.string(), pa.int64())),
                     "s": pa.array(structs, pa.struct([("a", pa.int64()), ("b", pa.string())]))})


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("compression", ["none", "snappy"])
def test_plan_nested_leaves(tmp_path, version, compression):
    t = _nested_table()
    path = str(tmp_path / "n.parquet")
    pq.write_table(t, path, row_group_size=1100, compression=compression, data_page_version=version,
                   data_page_size=512)
    m = FileMeta(path)
    N = native()
    LP = N.PQ_LEVEL_PAGE_BYTES
    for li, leaf in enumerate(m.leaves):
        host, chunks = _stage(path, m, li)
        plan = N.pq_plan(host.ctypes.data, chunks, leaf["type"], leaf["max_def"], leaf["max_rep"], levels=True)
        assert plan["unsupported"] == "", leaf["name"]
        assert plan["num_pages"] * 72 == len(plan["pages"])                  # sizeof(kern::PqPage) is unchanged
        assert len(plan["level_pages"]) % LP == 0 and len(plan["level_pages"]) == plan["num_level_pages"] * LP
        data_pages = plan["num_pages"] - plan["num_dict_pages"]
        assert plan["num_level_pages"] == data_pages > len(m.row_groups)     # small pages: several per chunk
        # level pages: (rep_off, def_off, entry_base, first_row, rep_len, def_len, num_entries, flags)
        lps = [struct.unpack_from("<qqqqiiii", plan["level_pages"], k * LP) for k in range(plan["num_level_pages"])]
        entries = sum(c[5] for c in chunks) if leaf["max_rep"] else t.num_rows
        assert sum(lp[6] for lp in lps) == entries                           # pages count entries
        if leaf["max_rep"]:
            assert plan["num_entries"] == entries > t.num_rows
        base = 0
        for lp in lps:
            assert lp[2] == base                                             # cumulative over pages and chunks
            base += lp[6]
        starts = [lp for lp in lps if lp[7] & 4]
        assert [lp[3] for lp in starts] == [c[3] for c in chunks]            # a chunk's first page knows its first row
        assert all(bool(lp[7] & 1) == (version == "1.0") for lp in lps)
        # the value pages are entry-counted too: out_row (offset 24) runs with the entries
        rows = [struct.unpack_from("<q", plan["pages"], k * 72 + 24)[0] for k in range(plan["num_pages"])]
        kinds = [struct.unpack_from("<i", plan["pages"], k * 72 + 56)[0] for k in range(plan["num_pages"])]
        assert [r for r, kd in zip(rows, kinds) if kd != 2] == [lp[2] for lp in lps]


def test_flat_plan_has_no_level_pages(tmp_path):
    path = str(tmp_path / "f.parquet")
    pq.write_table(pa.table({"x": pa.array([1, None, 3], pa.int64())}), path)
    m = FileMeta(path)
    host, chunks = _stage(path, m, 0)
    plan = native().pq_plan(host.ctypes.data, [c[:5] for c in chunks], m.leaves[0]["type"], 1, 0)
    assert plan["unsupported"] == "" and plan["level_pages"] == b"" and plan["num_entries"] == 0


@pytest.mark.parametrize("at", [pa.int64(), pa.list_(pa.int64())], ids=["flat", "list"])
def test_all_null_chunk_with_empty_dictionary_plans(tmp_path, at):
    """An all-NULL chunk has a dictionary page without entries and dictionary-encoded data
    pages without values: nothing is missing there."""
    path = str(tmp_path / "an.parquet")
    pq.write_table(pa.table({"x": pa.array([None] * 777, at)}), path)
    m = FileMeta(path)
    leaf = m.leaves[0]
    host, chunks = _stage(path, m, 0)
    plan = native().pq_plan(host.ctypes.data, chunks, leaf["type"], leaf["max_def"], leaf["max_rep"])
    assert plan["unsupported"] == "" and plan["num_dict_pages"] == 1 and plan["dict_entries"] == 0


def test_deeper_nesting_reports_a_reason(tmp_path):
    ll = pa.list_(pa.list_(pa.int64()))
    ls = pa.list_(pa.struct([("a", pa.int64()), ("b", pa.int64())]))
    ss = pa.struct([("in", pa.struct([("a", pa.int64())]))])
    ml = pa.map_(pa.string(), pa.list_(pa.int64()))
    path = str(tmp_path / "deep.parquet")
    pq.write_table(pa.table({"ll": pa.array([[[1], [2, 3]], None], ll), "ls": pa.array([[{"a": 1, "b": 2}], []], ls),
                             "ss": pa.array([{"in": {"a": 1}}, None], ss), "ml": pa.array([[("k", [1])], None], ml),
                             "ok": pa.array([[1], None], pa.list_(pa.int64()))}), path)
    m = FileMeta(path)
    assert {l["top"]: l["kind"] for l in m.leaves if l["top"] != "ok"} == {t: "nested" for t in ("ll", "ls", "ss", "ml")}
    r = GpuParquetReader([path])
    for name, at in (("ll", ll), ("ls", ls), ("ss", ss), ("ml", ml)):
        why = r.supports(name, T.from_arrow_type(at))
        assert isinstance(why, str) and why, name
    assert r.supports("ok", T.LIST(T.INT64)) is None
    assert r.supports("ok", T.LIST(T.UTF8)) is not None           # element type mismatch
    assert r.supports("ok", T.MAP(T.INT64, T.INT64)) is not None   # shape mismatch
    # the planner itself refuses more than one repetition level
    leaf = m.leaves[0]
    assert leaf["max_rep"] == 2
    host, chunks = _stage(path, m, 0)
    plan = native().pq_plan(host.ctypes.data, chunks, leaf["type"], leaf["max_def"], leaf["max_rep"])
    assert plan["unsupported"] != ""


def test_struct_field_order_is_checked(tmp_path):
    st = pa.struct([("a", pa.int64()), ("b", pa.string())])
    path = str(tmp_path / "s.parquet")
    pq.write_table(pa.table({"s": pa.array([{"a": 1, "b": "x"}], st)}), path)
    r = GpuParquetReader([path])
    assert r.supports("s", T.STRUCT([("a", T.INT64), ("b", T.UTF8)])) is None
    assert r.supports("s", T.STRUCT([("b", T.UTF8), ("a", T.INT64)])) is not None
    assert r.supports("s", T.STRUCT([("a", T.INT64)])) is not None


def test_plan_rejects_a_second_dictionary_page_after_an_empty_one(tmp_path):
    """An all-NULL chunk: [empty dictionary page][data page]. The dictionary page staged twice is refused."""
    path = str(tmp_path / "an2.parquet")
    pq.write_table(pa.table({"x": pa.array([None] * 100, pa.int64())}), path, compression="none")
    m = FileMeta(path)
    (c,) = [g["chunks"][0] for g in m.row_groups]
    raw = np.zeros(c["length"], dtype=np.uint8)
    native().pq_pread(path, [(c["start"], c["length"], raw.ctypes.data)], 1)
    heads = native().pq_page_headers(raw.ctypes.data, c["length"])
    assert heads[0]["type"] == 2 and heads[0]["num_values"] == 0
    dlen = heads[0]["header_len"] + heads[0]["compressed"]
    host = np.concatenate([raw[:dlen], raw, np.zeros(64, np.uint8)])
    with pytest.raises(RuntimeError, match="two dictionary pages"):
        native().pq_plan(host.ctypes.data, [(0, c["length"] + dlen, 0, 0, 100)], m.leaves[0]["type"], 1, 0)


def test_v2_plan_rejects_wrong_row_count(tmp_path):
    t = pa.table({"l": pa.array([[1, 2], None, [], [3]] * 250, pa.list_(pa.int64()))})
    path = str(tmp_path / "v2.parquet")
    pq.write_table(t, path, compression="none", data_page_version="2.0")
    m = FileMeta(path)
    leaf = m.leaves[0]
    host, chunks = _stage(path, m, 0)
    (c,) = chunks
    ok = native().pq_plan(host.ctypes.data, [c], leaf["type"], leaf["max_def"], leaf["max_rep"])
    assert ok["unsupported"] == "" and ok["num_entries"] == c[5]
    # the v2 page headers state their rows: one more than they hold is refused on the host
    with pytest.raises(RuntimeError):
        native().pq_plan(host.ctypes.data, [c[:4] + (c[4] + 1, c[5])], leaf["type"], leaf["max_def"], leaf["max_rep"])
    # and so is a value count the pages do not add up to
    with pytest.raises(RuntimeError):
        native().pq_plan(host.ctypes.data, [c[:5] + (c[5] + 1,)], leaf["type"], leaf["max_def"], leaf["max_rep"])


def test_struct_field_by_dotted_name(tmp_path):
    """``s.a`` names field ``a`` of the STRUCT column ``s`` (with or without the table's name in front)."""
    import igloo_amd as ig
    st = pa.struct([("a", pa.int64()), ("b", pa.string())])
    path = str(tmp_path / "t.parquet")
    pq.write_table(pa.table({"id": pa.array([1, 2, 3]),
                             "s": pa.array([{"a": 10, "b": "x"}, None, {"a": None, "b": "z"}], st)}), path)
    e = ig.QueryEngine(device="cpu")
    e.register_parquet("t", path)
    rows = e.query("select id, s.a, t.s.b as b, get_field(s, 'a') as g from t order by id").to_pylist()
    assert [(r["id"], r["s.a"], r["b"], r["g"]) for r in rows] == [(1, 10, "x", 10), (2, None, None, None), (3, None, "z", None)]
    with pytest.raises(Exception, match="not found"):
        e.query("select s.nope from t")
