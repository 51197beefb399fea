"""TIMESTAMP WITH TIME ZONE on the CPU engine: the own TZif reader and the
compiled zone tables (igloo_amd/utils/tzdb.py), the CPU twins of the tz kernels
(igloo_amd/ops/timezone.py), parser, binder, Arrow / Parquet / plan serde.

Expected values come from the standard library's independent reader
(tests/tz_cases.py); they are integers and compare exactly."""
import struct

import numpy as np
import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
import tz_cases as TC
from igloo_amd import types as T
from igloo_amd.ops import timezone as TZ
from igloo_amd.utils import tzdb
from igloo_amd.utils.errors import PlanError


@pytest.fixture(scope="module", autouse=True)
def _tz_dir():
    old = tzdb._tz_dir
    tzdb.set_tz_dir(TC.TZ_DIR)
    yield
    tzdb.set_tz_dir(old)


def t64(vals):
    return torch.tensor(vals, dtype=torch.int64)


# ------------------------------------------------------------------ tables and CPU twins
@pytest.mark.parametrize("zone", TC.ZONES)
def test_to_local_matches_oracle(zone):
    us = TC.instants(zone)
    local, offs = TZ.to_local(t64(us), zone, want_offsets=True)
    assert local.tolist() == [TC.o_to_local(v, zone) for v in us]
    assert offs.dtype == torch.int32 and offs.tolist() == [TC.o_offset(v, zone) for v in us]


@pytest.mark.parametrize("zone", TC.ZONES)
def test_to_utc_matches_oracle(zone):
    w = TC.wall_times(zone)
    assert TZ.to_utc(t64(w), zone).tolist() == [TC.o_to_utc(v, zone) for v in w]


@pytest.mark.parametrize("zone", TC.ZONES)
def test_trunc_and_part_match_oracle(zone):
    us = TC.instants(zone)
    for unit in TC.UNITS:
        assert TZ.trunc(t64(us), zone, unit).tolist() == [TC.o_trunc(v, zone, unit) for v in us], unit
    for field in TC.FIELDS:
        got = TZ.part(t64(us), zone, field)
        assert got.dtype == torch.int32 and got.tolist() == [TC.o_part(v, zone, field) for v in us], field


def test_new_york_gap_and_fold_rule():
    """PEP 495 fold=0: 01:30 on the autumn night is its first occurrence, 02:30 on the spring night
    lands one hour later."""
    import datetime as dt
    ny = "America/New_York"
    fold = TC.us_of(dt.datetime(2024, 11, 3, 1, 30))
    gap = TC.us_of(dt.datetime(2024, 3, 10, 2, 30))
    assert TZ.to_utc_py(fold, ny) == TC.us_of(dt.datetime(2024, 11, 3, 5, 30))      # EDT, not EST
    assert TZ.to_utc_py(gap, ny) == TC.us_of(dt.datetime(2024, 3, 10, 7, 30))
    assert TZ.to_local_py(TZ.to_utc_py(gap, ny), ny) == gap + 3_600_000_000


def test_table_shape():
    ny = tzdb.zone_table("America/New_York")
    explicit = len(TC.explicit_transitions("America/New_York"))
    assert explicit == 175 and explicit + 790 < ny.trans.size < explicit + 810     # + one 400-year cycle
    assert ny.offs.dtype == np.int32 and ny.trans.dtype == np.int64 and ny.wall.dtype == np.int64
    assert ny.offs[0] == -17762                       # LMT: not a whole minute
    assert bool(np.all(np.diff(ny.trans) > 0)) and bool(np.all(np.diff(ny.wall) >= 0))
    p = 1 << ny.log2p
    buf = ny.padded()
    assert p == 1024 and buf.size == 2 * p + p // 2 and buf[ny.trans.size] == np.iinfo(np.int64).max
    assert tzdb.zone_table("America/New_York") is ny                      # compiled once
    assert tzdb.zone_table("Africa/Casablanca").utc_lo == tzdb._NO_FOLD   # 197 transitions, no rule
    assert tzdb.zone_table("Asia/Kathmandu").trans.size == 2
    assert tzdb.zone_table("UTC").fixed and tzdb.zone_table("UTC").log2p == -1


@pytest.mark.parametrize("name,seconds", sorted(TC.FIXED.items()))
def test_fixed_offsets_need_no_database(name, seconds, monkeypatch):
    monkeypatch.setattr(tzdb, "_search_dirs", lambda: pytest.fail("a fixed offset looked for a file"))
    tzdb._tables.pop((name, tzdb.tz_dir()), None)
    zt = tzdb.zone_table(name)
    assert zt.fixed and int(zt.offs[0]) == seconds
    us = TC.instants("UTC")
    assert TZ.to_local(t64(us), name).tolist() == [TC.o_to_local(v, name) for v in us]
    assert TZ.to_utc(t64(us), name).tolist() == [TC.o_to_utc(v, name) for v in us]
    assert TZ.trunc(t64(us), name, "day").tolist() == [TC.o_trunc(v, name, "day") for v in us]
    assert TZ.part(t64(us), name, "hour").tolist() == [TC.o_part(v, name, "hour") for v in us]


# -------------------------------------------------------------------------- the TZif reader
def _tzif(transitions, types, idx, footer, version=b"2"):
    """A slim TZif file: empty v1 block, 64-bit block, footer."""
    abbr = b"LMT\x00STD\x00DST\x00"

    def header(timecnt, typecnt, charcnt):
        return b"TZif" + version + b"\x00" * 15 + struct.pack(">6l", 0, 0, 0, timecnt, typecnt, charcnt)
    v1 = header(0, 1, 4) + struct.pack(">lBB", 0, 0, 0) + b"UTC\x00"
    body = struct.pack(f">{len(transitions)}q", *transitions) + bytes(idx)
    for off, isdst, ab in types:
        body += struct.pack(">lBB", off, isdst, ab)
    return v1 + header(len(transitions), len(types), len(abbr)) + body + abbr + b"\n" + footer + b"\n"


SYN_TYPES = [(3420, 0, 0), (3600, 0, 4), (7200, 1, 8)]          # LMT +0:57, STD +1, DST +2
SYN_TRANS = [-2000000000, 323226000, 341370000]                # LMT->STD, 1980-03-30 01:00Z ->DST, 1980-10-26 01:00Z ->STD
SYN = _tzif(SYN_TRANS, SYN_TYPES, [1, 2, 1], b"STD-1DST,M3.5.0,M10.5.0/3")


def test_synthetic_file_with_rule(tmp_path):
    import datetime as dt
    import zoneinfo
    (tmp_path / "Syn").mkdir()
    (tmp_path / "Syn" / "Zone").write_bytes(SYN)
    zt = tzdb.compile_tzif(SYN, "Syn/Zone", "syn")
    assert zt.trans[:3].tolist() == SYN_TRANS and zt.offs[:4].tolist() == [3420, 3600, 7200, 3600]
    assert zt.trans.size == 3 + 800 and zt.utc_lo == TC.us_of(dt.datetime(1981, 1, 1)) // 1_000_000
    with open(tmp_path / "Syn" / "Zone", "rb") as f:
        zi = zoneinfo.ZoneInfo.from_file(f)
    us = [t * 1_000_000 + d for t in SYN_TRANS for d in (-1, 0, 1)]
    us += [TC.us_of(dt.datetime(y, m, d, h)) for y in (1981, 2024, 2380, 2381, 2900, 5555)
           for m, d, h in ((3, 29, 0), (3, 29, 1), (7, 1, 12), (10, 25, 0), (10, 25, 1), (12, 31, 23))]
    want = [int((TC.EPOCH_UTC + TC.dt.timedelta(microseconds=v)).astimezone(zi).utcoffset().total_seconds()) for v in us]
    assert zt.offsets_utc(np.array(us, dtype=np.int64)).tolist() == want
    wall = [v + o * 1_000_000 + d for v, o in zip(us, want) for d in (0, 1_800_000_000, -1_800_000_000)]
    want_w = [int(TC.naive(w).replace(tzinfo=zi, fold=0).utcoffset().total_seconds()) for w in wall]
    assert zt.offsets_wall(np.array(wall, dtype=np.int64)).tolist() == want_w
    # through the lookup path
    old = tzdb.tz_dir()
    try:
        tzdb.set_tz_dir(str(tmp_path))
        assert TZ.to_local_py(us[5], "Syn/Zone") == us[5] + want[5] * 1_000_000
    finally:
        tzdb.set_tz_dir(old)


def _blocks(raw):
    """Offsets of the block boundaries of a slim TZif file."""
    v1_end = 44 + 6 + 4
    timecnt, typecnt, charcnt = struct.unpack_from(">3l", raw, v1_end + 32)
    data_end = v1_end + 44 + timecnt * 9 + typecnt * 6 + charcnt
    return [0, 20, 44, v1_end, v1_end + 20, v1_end + 44, v1_end + 44 + timecnt * 8, data_end, len(raw) - 1]


@pytest.mark.parametrize("cut", range(9))
def test_truncated_file_names_the_file(cut):
    raw = SYN[:_blocks(SYN)[cut]]
    with pytest.raises(PlanError, match="some/path.*(truncated|bad magic)"):
        tzdb.compile_tzif(raw, "X", "some/path")


def test_broken_files():
    with pytest.raises(PlanError, match="the/file.*bad magic"):
        tzdb.compile_tzif(b"TZjf" + SYN[4:], "X", "the/file")
    with pytest.raises(PlanError, match="the/file.*bad magic"):
        tzdb.compile_tzif(SYN[:54] + b"XXXX" + SYN[58:], "X", "the/file")
    swapped = _tzif([SYN_TRANS[1], SYN_TRANS[0], SYN_TRANS[2]], SYN_TYPES, [1, 2, 1], b"STD-1")
    with pytest.raises(PlanError, match="the/file.*not increasing"):
        tzdb.compile_tzif(swapped, "X", "the/file")
    with pytest.raises(PlanError, match="the/file.*out of range"):
        tzdb.compile_tzif(_tzif(SYN_TRANS, SYN_TYPES, [1, 7, 1], b"STD-1"), "X", "the/file")
    with pytest.raises(PlanError, match="the/file.*version 1"):
        tzdb.compile_tzif(_tzif(SYN_TRANS, SYN_TYPES, [1, 2, 1], b"STD-1", version=b"\x00"), "X", "the/file")
    with pytest.raises(PlanError, match="the/file.*footer"):
        tzdb.compile_tzif(_tzif(SYN_TRANS, SYN_TYPES, [1, 2, 1], b"STD-1DST,M13.1.0,M10.5.0"), "X", "the/file")


def test_unknown_zone_says_where_it_looked():
    with pytest.raises(PlanError, match="unknown time zone 'Mars/Olympus'.*looked in.*golden"):
        tzdb.zone_table("Mars/Olympus")
    with pytest.raises(PlanError, match="invalid time zone name"):
        tzdb.zone_table("../etc/passwd")


def test_lookup_order(tmp_path, monkeypatch):
    """tz_dir / IGLOO_TZDIR first, then zoneinfo.TZPATH, then the tzdata package."""
    import zoneinfo
    monkeypatch.setattr(zoneinfo, "TZPATH", (str(tmp_path / "sys"),))
    monkeypatch.setenv("IGLOO_TZDIR", str(tmp_path / "env"))
    old = tzdb._tz_dir
    try:
        tzdb.set_tz_dir(None)
        dirs = tzdb._search_dirs()
        assert dirs[:2] == [str(tmp_path / "env"), str(tmp_path / "sys")]
        tzdb.set_tz_dir(str(tmp_path / "opt"))
        assert tzdb._search_dirs()[:2] == [str(tmp_path / "opt"), str(tmp_path / "sys")]
        from igloo_amd.utils import switches
        assert "IGLOO_TZDIR" in switches.ENV and "IGLOO_TZDIR" in switches.__doc__
    finally:
        tzdb.set_tz_dir(old)


# ----------------------------------------------------------------------------------- types
def test_type_names_and_arrow():
    assert T.parse_type_name("TIMESTAMPTZ") == T.TIMESTAMPTZ("UTC")
    assert T.parse_type_name("TIMESTAMP WITH TIME ZONE", "Europe/Berlin") == T.TIMESTAMPTZ("Europe/Berlin")
    assert T.parse_type_name("TIMESTAMP WITHOUT TIME ZONE", "Europe/Berlin") == T.TIMESTAMP == T.parse_type_name("TIMESTAMP")
    t = T.from_arrow_type(pa.timestamp("ns", tz="Europe/Berlin"))
    assert t == T.DataType("timestamp", tz="Europe/Berlin") and t.is_zoned and t != T.TIMESTAMP
    assert t.to_arrow() == pa.timestamp("us", tz="Europe/Berlin") and str(t) == 'Timestamp(us, "Europe/Berlin")'
    assert T.from_arrow_type(pa.timestamp("ms")) == T.TIMESTAMP and not T.TIMESTAMP.is_zoned
    assert T.common_numeric(T.TIMESTAMPTZ("UTC"), t) == T.TIMESTAMPTZ("UTC")      # the first zone
    with pytest.raises(PlanError, match="AT TIME ZONE"):
        T.common_numeric(t, T.TIMESTAMP)


def test_parser():
    from igloo_amd.ops._lib import native
    ast = native().parse_sql("select a at time zone 'UTC'::varchar, b::timestamp with time zone, "
                             "cast(c as timestamp without time zone), cast(d as timestamptz) from t")[0]
    text = repr(ast)
    assert "at_time_zone" in text and "TIMESTAMP WITH TIME ZONE" in text and "TIMESTAMP WITHOUT TIME ZONE" in text
    st = native().parse_sql("set time zone 'Europe/Berlin'")[0]
    assert st["k"] == "set" and st["s"] == "time_zone"
    assert native().parse_sql("show time zone")[0]["s"] == "time_zone"
    # a column called "at" and an alias still parse
    assert native().parse_sql("select x at from t")[0]["k"] == "query"


def test_plan_serde_round_trips_the_zone():
    from igloo_amd.sql import serde
    e = ig.QueryEngine(device="cpu")
    e.register_table("t", TC.sql_table(pa))
    plan, names = e.logical_plan("select k, date_trunc('day', ts at time zone 'Pacific/Apia') d, ts from t where "
                                 "ts > '2024-03-10 00:00:00'")
    text = serde.dumps(plan)
    back = serde.loads(text, e.catalog)
    assert serde.dumps(back) == text and "Pacific/Apia" in text and "America/New_York" in text
    assert [c.dtype for c in back.schema] == [c.dtype for c in plan.schema]
    assert back.schema[1].dtype == T.TIMESTAMPTZ("Pacific/Apia") and back.schema[2].dtype == T.TIMESTAMPTZ("America/New_York")
    assert e.execute_logical(back, names).equals(e.sql("select k, date_trunc('day', ts at time zone 'Pacific/Apia') d, "
                                                       "ts from t where ts > '2024-03-10 00:00:00'").table)


# ------------------------------------------------------------------------------------- SQL
@pytest.fixture(scope="module")
def engine():
    e = ig.QueryEngine(device="cpu")
    e.register_table("t", TC.sql_table(pa))
    return e


@pytest.mark.parametrize("check", TC.SQL_CHECKS, ids=lambda f: f.__name__)
def test_sql(engine, check):
    check(engine, pa)


def test_string_column_cast(engine):
    TC.check_string_column_cast(engine, pa)


def test_parquet_host_reader_and_native_footer(engine, tmp_path):
    path = TC.check_parquet(engine, pa, tmp_path)
    from igloo_amd.connectors.gpu_parquet import FileMeta, conversion
    leaves = {l["name"]: l for l in FileMeta(path).leaves}
    assert leaves["ts"]["logical"] == "timestamp_us" and leaves["ts"]["tz"] == "UTC"     # isAdjustedToUTC = true
    assert leaves["nv"]["logical"] == "timestamp_us" and leaves["nv"]["tz"] == ""         # false stays naive
    assert conversion(leaves["ts"], T.TIMESTAMPTZ("America/New_York")) == ("copy", 8, 1)
    assert conversion(leaves["nv"], T.TIMESTAMPTZ("UTC")) is None        # local time is no instant
    assert conversion(leaves["nv"], T.TIMESTAMP) == ("copy", 8, 1)


def test_flight_schema_and_registry(engine):
    from igloo_amd.sql import functions as F
    assert "date_bin" in F.DATETIME and "to_local_time" in F.DATETIME
    plan, names = engine.logical_plan("select ts, ts at time zone 'Europe/Berlin' b from t")
    assert [c.dtype.to_arrow() for c in plan.schema] == [pa.timestamp("us", tz="America/New_York"),
                                                         pa.timestamp("us", tz="Europe/Berlin")]


def test_naive_timestamps_are_untouched(engine):
    """Nothing that worked before changes: naive columns stay naive through the same functions."""
    r = engine.sql("select date_trunc('hour', nv) h, hour(nv) p, nv + interval '1 day' a, cast(nv as date) d, "
                   "to_char(nv, '%H:%M %z') c, arrow_typeof(nv) y from t order by k").table
    us = TC.sql_rows()
    assert r.schema.field("h").type == pa.timestamp("us") == r.schema.field("a").type
    assert r.column("h").cast(pa.int64()).to_pylist() == [None if v is None else v // 3_600_000_000 * 3_600_000_000 for v in us]
    assert r.column("p").to_pylist() == [None if v is None else TC.o_part(v, "UTC", "hour") for v in us]
    assert r.column("c")[0].as_py() == "03:00 %z"
