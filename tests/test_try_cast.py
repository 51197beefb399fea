"""TRY_CAST and arrow_cast on the CPU engine, statement level: every row of the
semantics table over small Arrow tables with NULLs mixed in, literal folding
(with the statement-template case), TRY_CAST inside WHERE / join keys /
COALESCE / GROUP BY / NOT IN, plan serde, EXPLAIN, the errors, and equality
with CAST wherever CAST succeeds. Expectations come from tests/trycast_cases.py
(Python int / Decimal / math / datetime), never from the engine."""
import datetime
from decimal import Decimal

import pyarrow as pa
import pytest

import igloo_amd as ig
import text_cases as C
import trycast_cases as K
from igloo_amd.utils.errors import NotSupported, PlanError

SQL_INT = {"int8": "TINYINT", "int16": "SMALLINT", "int32": "INT", "int64": "BIGINT"}


def engine(**tables):
    e = ig.QueryEngine(device="cpu")
    for name, t in tables.items():
        e.register_table(name, t)
    return e


def column(e, sql):
    t = e.sql(sql).table
    return t.column(0).to_pylist()


def with_nulls(values):
    """Every fifth row NULL (the NULL rows hold no value at all)."""
    return [None if i % 5 == 4 else v for i, v in enumerate(values)]


def as_engine_value(v, t):
    """An Arrow result value in the oracle's representation (unscaled decimal, days, microseconds)."""
    if v is None:
        return None
    if isinstance(v, Decimal):
        return int(v.scaleb(t[2]))
    if isinstance(v, datetime.datetime):
        return K.micros(v)
    if isinstance(v, datetime.date):
        return v.toordinal() - 719163
    return v


# ---- text sources ---------------------------------------------------------------

@pytest.mark.parametrize("kind", list(SQL_INT))
def test_text_to_integer(kind):
    texts = with_nulls(K.int_texts())
    e = engine(t=pa.table({"s": pa.array(texts, pa.string())}))
    want = [None if t is None else K.expect_int_text(t, kind) for t in texts]
    assert any(v is None for v in want) and any(v is not None for v in want)
    assert column(e, f"SELECT TRY_CAST(s AS {SQL_INT[kind]}) FROM t") == want


@pytest.mark.parametrize("p,s", K.DECIMAL_TYPES)
def test_text_to_decimal(p, s):
    texts = with_nulls(K.decimal_texts())
    e = engine(t=pa.table({"s": pa.array(texts, pa.string())}))
    want = [None if t is None else K.expect_decimal_text(t, p, s) for t in texts]
    got = column(e, f"SELECT TRY_CAST(s AS DECIMAL({p},{s})) FROM t")
    assert [as_engine_value(v, ("decimal", p, s)) for v in got] == want


def test_text_to_double_and_real():
    import numpy as np
    cases = C.float_cases()
    texts = with_nulls([t for t, _ in cases])
    e = engine(t=pa.table({"s": pa.array(texts, pa.string())}))
    want = [None if t is None else C.expect_float(t) for t in texts]
    got = column(e, "SELECT TRY_CAST(s AS DOUBLE) FROM t")
    assert [None if v is None else C.bits(v) for v in got] == [None if v is None else C.bits(v) for v in want]
    got = column(e, "SELECT TRY_CAST(s AS REAL) FROM t")
    with np.errstate(over="ignore"):
        want32 = [None if v is None else float(np.float32(v)) for v in want]
    assert [None if v is None else C.bits(v) for v in got] == [None if v is None else C.bits(v) for v in want32]


def test_text_to_date_bool_timestamp():
    dates = with_nulls([t for t, _ in C.date_cases()][::9])
    bools = with_nulls([t for t, _ in K.BOOL_TEXTS])
    ts = K.timestamp_cases(400, 23)
    stamps = with_nulls([t for t, _ in ts])
    e = engine(d=pa.table({"s": pa.array(dates, pa.string())}), b=pa.table({"s": pa.array(bools, pa.string())}),
               ts=pa.table({"s": pa.array(stamps, pa.string())}))
    got = column(e, "SELECT TRY_CAST(s AS DATE) FROM d")
    assert [as_engine_value(v, None) for v in got] == [None if t is None else C.expect_date(t) for t in dates]
    assert column(e, "SELECT TRY_CAST(s AS BOOLEAN) FROM b") == [None if t is None else K.expect_bool_text(t) for t in bools]
    got = column(e, "SELECT TRY_CAST(s AS TIMESTAMP) FROM ts")
    want = [None if t is None else v for t, (_, v) in zip(stamps, ts)]
    assert sum(v is None for v in want) > len(K.TS_REJECT) // 2
    assert [as_engine_value(v, None) for v in got] == want


# ---- numeric sources --------------------------------------------------------------

def _arrow_type(kind):
    if kind[0] == "decimal":
        return pa.decimal128(kind[1], kind[2])
    if kind[0] == "wide":
        return pa.decimal128(38, kind[1])
    return {"int8": pa.int8(), "int16": pa.int16(), "int32": pa.int32(), "int64": pa.int64(), "float32": pa.float32(),
            "float64": pa.float64()}[kind[0]]


def _sql_type(kind):
    return f"DECIMAL({kind[1]},{kind[2]})" if kind[0] == "decimal" else SQL_INT[kind[0]]


@pytest.mark.parametrize("src,dst,vals", K.convert_cases(), ids=lambda x: "-".join(map(str, x)) if isinstance(x, tuple) else "")
def test_numeric_conversion(src, dst, vals):
    if src[0] in ("decimal", "wide"):      # what an Arrow decimal of the source's precision can hold
        vals = [v for v in vals if abs(v) < 10 ** (18 if src[0] == "decimal" else 38)]
    rows = with_nulls(vals)
    if src[0] in ("decimal", "wide"):
        scale = src[2] if src[0] == "decimal" else src[1]
        arr = pa.array([None if v is None else Decimal(v).scaleb(-scale, context=C._CTX) for v in rows], _arrow_type(src))
    else:
        arr = pa.array(rows, _arrow_type(src))
    e = engine(t=pa.table({"x": arr}))
    want = [None if v is None else K.expect_convert(v, src, dst) for v in rows]
    got = column(e, f"SELECT TRY_CAST(x AS {_sql_type(dst)}) FROM t")
    assert [as_engine_value(v, dst) for v in got] == want


def test_conversions_that_cannot_fail_follow_cast():
    t = pa.table({"i": pa.array([1, None, -7], pa.int32()), "d": pa.array([datetime.date(2024, 2, 29), None, datetime.date(1969, 12, 31)]),
                  "b": pa.array([True, False, None]), "m": pa.array([Decimal("1.50"), None, Decimal("-2.25")], pa.decimal128(9, 2))})
    e = engine(t=t)
    for expr in ("i AS BIGINT", "i AS DOUBLE", "i AS VARCHAR", "d AS TIMESTAMP", "d AS VARCHAR", "b AS VARCHAR", "m AS DOUBLE",
                 "m AS VARCHAR", "CAST(d AS TIMESTAMP) AS DATE", "NULL AS INT", "i AS INT"):
        assert column(e, f"SELECT TRY_CAST({expr}) FROM t") == column(e, f"SELECT CAST({expr}) FROM t"), expr


def test_equals_cast_where_cast_succeeds():
    import re
    # spellings the CPU engine's CAST (pyarrow) reads as well: canonical integers, 'T' / ' ' and microseconds
    rng_ints = [t for t, v in C.int_cases() if v is not None and abs(v) < 2 ** 31 and str(v) == t]
    ts = [t for t, v in K.timestamp_cases(300, 29, False) if v is not None and re.fullmatch(r"[^t]{10,26}", t)]
    assert len(rng_ints) > 50 and len(ts) > 100
    e = engine(i=pa.table({"s": pa.array(rng_ints, pa.string())}), ts=pa.table({"s": pa.array(ts, pa.string())}),
               f=pa.table({"s": pa.array([repr(float(t)) for t in C.random_float_texts(500, 3)], pa.string())}),
               n=pa.table({"x": pa.array([0, 1, -1, 127, -128, 5], pa.int64()), "y": pa.array([0.5, -0.9, 126.99, -128.5, 2.5, 1e2])}))
    for q in ("SELECT {}(s AS INT) FROM i", "SELECT {}(s AS BIGINT) FROM i", "SELECT {}(s AS DOUBLE) FROM f",
              "SELECT {}(s AS TIMESTAMP) FROM ts", "SELECT {}(x AS TINYINT) FROM n", "SELECT {}(y AS TINYINT) FROM n",
              "SELECT {}(y AS DECIMAL(6,1)) FROM n", "SELECT {}(x AS DECIMAL(5,2)) FROM n"):
        a, b = column(e, q.format("TRY_CAST")), column(e, q.format("CAST"))
        assert a == b and None not in a, q


# ---- literals ------------------------------------------------------------------------

def test_literals_fold_with_a_range_check():
    e = engine()
    assert column(e, "SELECT TRY_CAST('abc' AS INT)") == [None]
    assert column(e, "SELECT TRY_CAST(300 AS TINYINT)") == [None]
    assert column(e, "SELECT TRY_CAST('2024-02-30' AS DATE)") == [None]
    assert column(e, "SELECT TRY_CAST(1e30 AS BIGINT)") == [None]
    assert column(e, "SELECT TRY_CAST(127 AS TINYINT)") == [127]
    assert column(e, "SELECT TRY_CAST('70000' AS SMALLINT)") == [None]
    assert column(e, "SELECT TRY_CAST('70000' AS INT)") == column(e, "SELECT CAST('70000' AS INT)") == [70000]
    assert column(e, "SELECT TRY_CAST(1234.5 AS DECIMAL(5,2))") == [None]
    assert column(e, "SELECT TRY_CAST(123.455 AS DECIMAL(5,2))") == column(e, "SELECT CAST(123.455 AS DECIMAL(5,2))")
    assert column(e, "SELECT TRY_CAST('2024-01-02T03:04:05+01:00' AS TIMESTAMP)") == [datetime.datetime(2024, 1, 2, 2, 4, 5)]
    assert column(e, "SELECT TRY_CAST(NULL AS INT)") == [None]
    assert e.sql("SELECT TRY_CAST('abc' AS INT) AS x").table.schema.field("x").type == pa.int32()


def test_one_template_does_not_answer_for_another_literal():
    e = engine()
    assert column(e, "SELECT TRY_CAST('12' AS INT)") == [12]
    assert column(e, "SELECT TRY_CAST('ab' AS INT)") == [None]
    assert column(e, "SELECT TRY_CAST('13' AS INT)") == [13]
    assert column(e, "SELECT TRY_CAST(100 AS TINYINT)") == [100]
    assert column(e, "SELECT TRY_CAST(200 AS TINYINT)") == [None]


# ---- inside queries ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dirty():
    t = pa.table({"s": pa.array(["1", "2", "x", None, "3", "2 ", "300", "2"], pa.string()), "k": pa.array(range(8), pa.int64())})
    u = pa.table({"n": pa.array([1, 2, 300, None], pa.int64()), "name": pa.array(["one", "two", "big", "none"])})
    return engine(t=t, u=u)


def test_in_where_join_coalesce_group_by(dirty):
    e = dirty
    assert column(e, "SELECT k FROM t WHERE TRY_CAST(s AS INT) >= 2 ORDER BY k") == [1, 4, 6, 7]
    assert column(e, "SELECT k FROM t WHERE TRY_CAST(s AS TINYINT) IS NULL ORDER BY k") == [2, 3, 5, 6]
    got = e.sql("SELECT t.k, u.name FROM t JOIN u ON TRY_CAST(t.s AS BIGINT) = u.n ORDER BY t.k").table.to_pylist()
    assert got == [{"k": 0, "name": "one"}, {"k": 1, "name": "two"}, {"k": 6, "name": "big"}, {"k": 7, "name": "two"}]
    assert column(e, "SELECT COALESCE(TRY_CAST(s AS INT), -1) FROM t ORDER BY k") == [1, 2, -1, -1, 3, -1, 300, 2]
    got = e.sql("SELECT TRY_CAST(s AS INT) AS v, count(*) AS c FROM t GROUP BY TRY_CAST(s AS INT) ORDER BY v NULLS LAST").table.to_pylist()
    assert got == [{"v": 1, "c": 1}, {"v": 2, "c": 2}, {"v": 3, "c": 1}, {"v": 300, "c": 1}, {"v": None, "c": 3}]
    assert column(e, "SELECT TRY_CAST(s AS INT) + k * 2 FROM t ORDER BY k") == [1, 4, None, None, 11, None, 312, 16]


def test_not_in_sees_the_nulls(dirty):
    """The subquery column is nullable whatever its input: a NULL among the values empties NOT IN."""
    e = dirty
    assert column(e, "SELECT n FROM u WHERE n NOT IN (SELECT TRY_CAST(s AS BIGINT) FROM t WHERE k IN (0, 2))") == []
    assert column(e, "SELECT n FROM u WHERE n NOT IN (SELECT TRY_CAST(s AS BIGINT) FROM t WHERE k IN (0, 1)) ORDER BY n") == [300]
    # a NOT NULL input column still gives a nullable TRY_CAST
    from igloo_amd.sql.expr import ColRef, Func
    from igloo_amd import types as T
    f = Func("try_cast", [ColRef(1, "c", T.UTF8, nullable=False)], T.INT32)
    assert f.nullable and not f.args[0].nullable


def test_plan_serde_and_explain(dirty):
    from igloo_amd.sql import serde
    e = dirty
    sql = "SELECT k, TRY_CAST(s AS SMALLINT) AS v FROM t WHERE TRY_CAST(s AS INT) < 100"
    plan, _ = e.logical_plan(sql)
    back = serde.loads(serde.dumps(plan), e.catalog)
    assert "try_cast" in serde.dumps(plan)
    assert e.execute_logical(back, ["k", "v"]).to_pylist() == e.sql(sql).table.to_pylist() == \
        [{"k": 0, "v": 1}, {"k": 1, "v": 2}, {"k": 4, "v": 3}, {"k": 7, "v": 2}]
    text = "\n".join(e.sql("EXPLAIN " + sql).table.column("plan").to_pylist())
    assert "TRY_CAST(s#" in text and " AS Int16)" in text and " AS Int32)" in text
    assert e.sql("SELECT TRY_CAST(s AS INT) FROM t").table.column_names == ["TRY_CAST(s AS INT)"]
    # x::t stays a plain cast
    assert "TRY_CAST" not in "\n".join(e.sql("EXPLAIN SELECT k::INT FROM t").table.column("plan").to_pylist())


def test_errors(dirty):
    e = dirty
    e.register_table("nest", pa.table({"l": pa.array([[1], None]), "st": pa.array([{"a": 1}, None]),
                                       "b": pa.array([b"x", None], pa.binary()), "ts": pa.array([datetime.datetime(2024, 1, 1), None])}))
    for q, word in (("SELECT TRY_CAST(l AS INT) FROM nest", "List"), ("SELECT TRY_CAST(st AS VARCHAR) FROM nest", "Struct"),
                    ("SELECT TRY_CAST(b AS VARCHAR) FROM nest", "Binary"), ("SELECT TRY_CAST(s AS BYTEA) FROM t", "Binary"),
                    ("SELECT TRY_CAST(INTERVAL '1' DAY AS INT)", "interval"),
                    ("SELECT TRY_CAST(s AS TIMESTAMPTZ) FROM t", "Timestamp(us,")):
        with pytest.raises(NotSupported) as ex:
            e.sql(q)
        assert word in str(ex.value), q
    # an impossible pair stays the PlanError it is for CAST
    for q in ("SELECT {}(CAST(ts AS TIMESTAMPTZ) AS BOOLEAN) FROM nest",):
        for form in ("CAST", "TRY_CAST"):
            with pytest.raises(PlanError):
                e.sql(q.format(form))
    with pytest.raises(Exception):
        e.sql("SELECT TRY_CAST(s, INT) FROM t")


# ---- arrow_cast ------------------------------------------------------------------------------

def test_arrow_cast_round_trips_every_scalar_name():
    t = pa.table({"i8": pa.array([1, None], pa.int8()), "i16": pa.array([1, None], pa.int16()), "i32": pa.array([1, None], pa.int32()),
                  "i64": pa.array([1, None], pa.int64()), "f32": pa.array([1.5, None], pa.float32()), "f64": pa.array([1.5, None]),
                  "b": pa.array([True, None]), "s": pa.array(["1", None]), "d": pa.array([datetime.date(2024, 1, 2), None]),
                  "ts": pa.array([datetime.datetime(2024, 1, 2, 3), None]), "m": pa.array([Decimal("1.25"), None], pa.decimal128(12, 2)),
                  "z": pa.array([datetime.datetime(2024, 1, 2, 3), None], pa.timestamp("us", tz="Europe/Berlin")),
                  "bin": pa.array([b"1", None], pa.binary())})
    e = engine(t=t)
    names = {c: column(e, f"SELECT arrow_typeof({c}) FROM t")[0] for c in t.column_names}
    assert names["ts"] == "Timestamp(Microsecond, None)" and names["m"] == "Decimal128(12, 2)" and names["i8"] == "Int8"
    for c, name in names.items():
        lit = name.replace("'", "''")
        assert column(e, f"SELECT arrow_typeof(arrow_cast({c}, '{lit}')) FROM t")[0] == name
        assert column(e, f"SELECT arrow_cast({c}, '{lit}') FROM t") == t.column(c).to_pylist()
    # from another type: the semantics of CAST, errors included
    assert column(e, "SELECT arrow_cast(i64, 'Int32') FROM t") == [1, None]
    assert column(e, "SELECT arrow_typeof(arrow_cast(s, 'Decimal128(10, 3)')) FROM t")[0] == "Decimal128(10, 3)"
    assert column(e, "SELECT arrow_cast(s, 'Float64') FROM t") == [1.0, None]
    assert column(e, "SELECT arrow_typeof(arrow_cast(NULL, 'Null'))") == ["Null"]
    assert column(e, "SELECT arrow_cast('7', 'Int64')") == [7]
    e.register_table("bad", pa.table({"s": pa.array(["x"])}))
    with pytest.raises(Exception):
        e.sql("SELECT arrow_cast(s, 'Int32') FROM bad")


def test_arrow_cast_rejects_other_names():
    e = engine(t=pa.table({"n": pa.array([1], pa.int64())}))
    for bad in ("Foo", "int32", "INT", "List(Int32)", "Decimal128(40, 2)", "Decimal128(5)", ""):
        with pytest.raises(PlanError) as ex:
            e.sql(f"SELECT arrow_cast(n, '{bad}') FROM t")
        assert repr(bad) in str(ex.value)
    with pytest.raises(PlanError):
        e.sql("SELECT arrow_cast(n, n) FROM t")
