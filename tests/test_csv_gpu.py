"""GPU CSV parsing (csrc/kernels/csv.hip) vs Arrow's CSV reader on the same
files: quoting with "" escapes and embedded delimiters/newlines, CRLF, empty
lines, NULLs, every type the engine parses (int32/int64/decimal/float64/
date/bool/utf8), and a value that does not parse (host fallback)."""
import decimal
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

import igloo_amd as ig
from igloo_amd import types as T
from igloo_amd.catalog import Field
from igloo_amd.columnar import Column
from igloo_amd.connectors.csv import CsvTable
from igloo_amd.connectors.gpu_csv import CsvParseError, read_csv_gpu
from igloo_amd.ops._lib import KERNEL_CALLS

pytestmark = pytest.mark.gpu

FIELDS = [Field("i32", T.INT32), Field("i64", T.INT64), Field("dec", T.DECIMAL(15, 2)), Field("f", T.FLOAT64),
          Field("d", T.DATE32), Field("b", T.BOOL), Field("s", T.UTF8)]


def _arrow_ref(path, fields, header=True):
    ro = pacsv.ReadOptions(autogenerate_column_names=False, column_names=None if header else [f.name for f in fields])
    co = pacsv.ConvertOptions(column_types={f.name: f.dtype.to_arrow() for f in fields})
    return pacsv.read_csv(path, read_options=ro, convert_options=co)


def _compare(got, ref, fields):
    for f in fields:
        want = Column.from_arrow(ref.column(f.name), device="cpu", dtype=f.dtype).to_arrow().to_pylist()
        have = got[f.name].to_arrow().to_pylist()
        if f.dtype.kind == "float64":
            # exact: the device parser is correctly rounded, like Arrow's
            bits = lambda xs: [None if x is None else struct.pack("<d", x) for x in xs]
            assert bits(have) == bits(want), f.name
        else:
            assert have == want, f.name


def test_csv_types_quotes_nulls(tmp_path, gpu_device):
    rng = np.random.default_rng(1)
    n = 20000
    words = ["plain", "with,comma", 'say "hi"', "multi\nline", "", "crlf\r\nin field", "naïve ünïcode"]
    rows = ["i32,i64,dec,f,d,b,s"]
    for i in range(n):
        i32 = "" if i % 97 == 0 else str(int(rng.integers(-2**31, 2**31 - 1)))
        i64 = str(int(rng.integers(-2**62, 2**62)))
        dec = f"{int(rng.integers(-10**12, 10**12)) / 100:.2f}"
        f = "" if i % 89 == 0 else repr(float(np.round(rng.standard_normal() * 1000, 6)))
        d = f"{1990 + i % 30:04d}-{1 + i % 12:02d}-{1 + i % 28:02d}"
        b = ["true", "false", "True", ""][i % 4]
        w = words[i % len(words)]
        s = '"' + w.replace('"', '""') + '"' if any(c in w for c in ',"\n\r') or i % 5 == 0 else w
        rows.append(",".join([i32, i64, dec, f, d, b, s]))
        if i % 1000 == 0:
            rows.append("")  # empty line (skipped)
    text = "\r\n".join(rows) + "\r\n"
    path = str(tmp_path / "t.csv")
    with open(path, "w", newline="") as fh:
        fh.write(text)
    got = read_csv_gpu(path, FIELDS, None, gpu_device)
    ref = _arrow_ref(path, FIELDS)
    assert len(got["i32"]) == ref.num_rows == n
    _compare(got, ref, FIELDS)


def test_csv_no_header_no_trailing_newline(tmp_path, gpu_device):
    path = str(tmp_path / "t.csv")
    with open(path, "w") as fh:
        fh.write("1,a\n2,b\n3,c")
    fields = [Field("x", T.INT64), Field("y", T.UTF8)]
    got = read_csv_gpu(path, fields, None, gpu_device, has_header=False)
    assert got["x"].to_arrow().to_pylist() == [1, 2, 3]
    assert got["y"].to_arrow().to_pylist() == ["a", "b", "c"]


def test_csv_bad_value_raises(tmp_path, gpu_device):
    path = str(tmp_path / "t.csv")
    with open(path, "w") as fh:
        fh.write("a,b\n1,x\n2.5,y\n")
    with pytest.raises(CsvParseError):
        read_csv_gpu(path, [Field("a", T.INT64), Field("b", T.UTF8)], None, gpu_device)


def test_csv_table_query_gpu_vs_cpu(tmp_path, gpu_device):
    rng = np.random.default_rng(2)
    n = 100000
    t = pa.table({"k": pa.array(rng.integers(0, 50, n)), "v": pa.array(rng.integers(-1000, 1000, n)),
                  "name": pa.array([f"n{i % 13}" for i in range(n)])})
    path = str(tmp_path / "t.csv")
    pacsv.write_csv(t, path)
    q = "SELECT name, count(*) AS c, sum(v) AS s FROM t WHERE k < 25 GROUP BY name ORDER BY name"
    cpu = ig.QueryEngine(device="cpu")
    cpu.register_csv("t", path)
    g = ig.QueryEngine(device=gpu_device)
    src = g.register_csv("t", path)
    before = KERNEL_CALLS["csv_parse"]
    assert g.query(q).to_pylist() == cpu.query(q).to_pylist()
    assert src.last_scan == "gpu" and KERNEL_CALLS["csv_parse"] > before


def test_reference_fixture_on_gpu(gpu_device):
    # reference crates/connectors/filesystem/test_data.csv via the coordinator's explicit schema
    path = os.path.join(os.path.dirname(__file__), "data", "test_data.csv")
    e = ig.QueryEngine(device=gpu_device)
    e.register_csv("test_table", path, schema=[Field("col_a", T.INT64), Field("col_b", T.UTF8)])
    r = e.query("SELECT col_a, col_b FROM test_table LIMIT 5")
    assert r.to_pylist() == [{"col_a": 1, "col_b": "foo"}, {"col_a": 2, "col_b": "bar"}]
