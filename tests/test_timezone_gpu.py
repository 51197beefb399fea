"""TIMESTAMP WITH TIME ZONE on the device (csrc/kernels/tz.hip): the four
kernels equal the standard library's oracle and the CPU twins at every
transition of ten zones, at row counts around the wave, the workgroup and the
two-row tile, with NULL rows that hold INT64_MIN and with a column sliced off
its 16-byte alignment; each kernel ran (KERNEL_CALLS) and no host step was
taken (HOST_STEPS). The SQL checks of tests/tz_cases.py run on the GPU engine;
statements that differ only in a zone keep their own plans, and a repeated
zoned query replays as a graph."""
import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
import tz_cases as TC
from igloo_amd.ops import timezone as TZ
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS
from igloo_amd.utils import tzdb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _tz_dir():
    old = tzdb._tz_dir
    tzdb.set_tz_dir(TC.TZ_DIR)
    yield
    tzdb.set_tz_dir(old)


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


def dev(vals, gpu_device, misalign=False):
    """The values on the device; ``misalign``: a view from row 1 of a longer buffer, so the column
    starts 8 bytes past a 16-byte boundary."""
    if misalign:
        t = torch.tensor([0] + list(vals), dtype=torch.int64, device=gpu_device)[1:]
        assert t.data_ptr() % 16 == 8 or not len(vals)
        return t
    t = torch.tensor(list(vals), dtype=torch.int64, device=gpu_device)
    assert t.data_ptr() % 16 == 0
    return t


def host(t):
    return t.cpu().tolist()


@pytest.mark.parametrize("zone", TC.ZONES)
def test_kernels_at_every_transition(zone, gpu_device):
    """All four kernels over every probe of the zone (aligned and misaligned), against the oracle
    and the CPU twins."""
    us, wall = TC.instants(zone), TC.wall_times(zone)
    want_local = [TC.o_to_local(v, zone) for v in us]
    want_off = [TC.o_offset(v, zone) for v in us]
    want_utc = [TC.o_to_utc(v, zone) for v in wall]
    cpu_us, cpu_wall = torch.tensor(us, dtype=torch.int64), torch.tensor(wall, dtype=torch.int64)
    with device_only("tz_to_local", "tz_to_utc", "tz_trunc", "tz_part"):
        for mis in (False, True):
            local, offs = TZ.to_local(dev(us, gpu_device, mis), zone, want_offsets=True)
            assert host(local) == want_local and host(offs) == want_off and offs.dtype == torch.int32
            assert host(TZ.to_local(dev(us, gpu_device, mis), zone)) == want_local
            assert host(TZ.to_utc(dev(wall, gpu_device, mis), zone)) == want_utc
        for unit in TC.UNITS:
            got = host(TZ.trunc(dev(us, gpu_device, unit in ("day", "month")), zone, unit))
            assert got == [TC.o_trunc(v, zone, unit) for v in us], unit
            assert got == TZ.trunc(cpu_us, zone, unit).tolist(), unit
        for field in TC.FIELDS:
            got = TZ.part(dev(us, gpu_device, field in ("hour", "week")), zone, field)
            assert got.dtype == torch.int32 and host(got) == [TC.o_part(v, zone, field) for v in us], field
            assert host(got) == TZ.part(cpu_us, zone, field).tolist(), field
    assert want_local == TZ.to_local(cpu_us, zone).tolist() and want_utc == TZ.to_utc(cpu_wall, zone).tolist()


@pytest.mark.parametrize("n", TC.ROW_COUNTS)
@pytest.mark.parametrize("zone", ["America/New_York", "Asia/Kathmandu", "+05:30"])
def test_row_counts_nulls_and_alignment(zone, n, gpu_device):
    """Row counts around the wave, the workgroup and the tile; every 7th row a NULL holding
    INT64_MIN; aligned and sliced from row 1. A table zone, a two-transition zone and a fixed
    offset (the path without LDS)."""
    src = TC.instants(zone if zone in TC.ZONES else "UTC")
    us, valid = TC.rows(src, n)
    wall, _ = TC.rows(TC.wall_times(zone if zone in TC.ZONES else "UTC"), n)
    keep = [i for i, k in enumerate(valid) if k]

    def live(t):
        v = host(t)
        assert len(v) == n
        return [v[i] for i in keep]
    for mis in (False, True):
        local, offs = TZ.to_local(dev(us, gpu_device, mis), zone, want_offsets=True)
        assert live(local) == [TC.o_to_local(us[i], zone) for i in keep]
        assert live(offs) == [TC.o_offset(us[i], zone) for i in keep]
        assert live(TZ.to_utc(dev(wall, gpu_device, mis), zone)) == [TC.o_to_utc(wall[i], zone) for i in keep]
        assert live(TZ.trunc(dev(us, gpu_device, mis), zone, "day")) == [TC.o_trunc(us[i], zone, "day") for i in keep]
        assert live(TZ.trunc(dev(us, gpu_device, mis), zone, "quarter")) == \
            [TC.o_trunc(us[i], zone, "quarter") for i in keep]
        assert live(TZ.part(dev(us, gpu_device, mis), zone, "hour")) == [TC.o_part(us[i], zone, "hour") for i in keep]
        assert live(TZ.part(dev(us, gpu_device, mis), zone, "doy")) == [TC.o_part(us[i], zone, "doy") for i in keep]


@pytest.mark.parametrize("name", sorted(TC.FIXED))
def test_fixed_offset_zones(name, gpu_device):
    us = TC.instants("UTC") + TC.instants("Asia/Kathmandu")
    with device_only("tz_to_local", "tz_to_utc", "tz_trunc", "tz_part"):
        assert host(TZ.to_local(dev(us, gpu_device), name)) == [TC.o_to_local(v, name) for v in us]
        assert host(TZ.to_utc(dev(us, gpu_device, True), name)) == [TC.o_to_utc(v, name) for v in us]
        assert host(TZ.trunc(dev(us, gpu_device), name, "week")) == [TC.o_trunc(v, name, "week") for v in us]
        assert host(TZ.part(dev(us, gpu_device, True), name, "minute")) == [TC.o_part(v, name, "minute") for v in us]
    assert TZ.device_table(name, gpu_device)[1] is None         # no table on the device at all


def test_device_table_is_cached(gpu_device):
    a = TZ.device_table("Europe/Berlin", torch.device(gpu_device))[1]
    b = TZ.device_table("Europe/Berlin", torch.device(gpu_device))[1]
    assert a is b and a.data_ptr() == b.data_ptr() and a.is_cuda


# ------------------------------------------------------------------------------------- SQL
@pytest.fixture(scope="module")
def engines(gpu_device):
    tab = TC.sql_table(pa)
    g, c = ig.QueryEngine(device=gpu_device), ig.QueryEngine(device="cpu")
    g.register_table("t", tab)
    c.register_table("t", tab)
    return g, c


@pytest.mark.parametrize("check", TC.SQL_CHECKS, ids=lambda f: f.__name__)
def test_sql(engines, check):
    h0 = sum(HOST_STEPS.values())
    check(engines[0], pa)
    assert sum(HOST_STEPS.values()) == h0, dict(HOST_STEPS)


def test_sql_equals_cpu_engine_and_runs_the_kernels(engines):
    g, c = engines
    sql = ("select k, ts at time zone 'Europe/Dublin' a, to_local_time(ts) l, nv at time zone 'Australia/Lord_Howe' u, "
           "date_trunc('week', ts at time zone 'Pacific/Apia') w, extract(dow from ts) d, cast(ts as varchar) s, "
           "ts + interval '1 month' m, date_bin(interval '15 minutes', ts) b from t order by k")
    with device_only("tz_to_local", "tz_to_utc", "tz_trunc", "tz_part", "strfmt"):
        got = g.sql(sql).table
    assert got.equals(c.sql(sql).table)
    assert got.schema.field("w").type == pa.timestamp("us", tz="Pacific/Apia")


def test_zoned_keys_group_join_window_on_device(engines):
    g, c = engines
    for sql in (
        "select date_trunc('hour', ts) h, g, count(*) n, min(ts) lo, max(ts at time zone 'Asia/Kathmandu') hi "
        "from t group by 1, 2 order by 1 nulls last, 2",
        "select a.k, b.k bk from t a join t b on a.ts = b.ts at time zone 'Europe/Berlin' and a.g = b.g order by 1, 2",
        "select distinct date_trunc('day', ts) d from t order by 1 nulls first",
        "select k, row_number() over (partition by date_trunc('day', ts) order by ts, k) r, "
        "lag(ts) over (order by k) p from t order by k",
    ):
        assert g.sql(sql).table.equals(c.sql(sql).table), sql


def test_string_column_cast(engines):
    TC.check_string_column_cast(engines[0], pa)


def test_naive_to_char_is_unchanged(engines):
    """A naive value has no offset: %z and %:z are copied as before, on the device as on the CPU."""
    g, c = engines
    sql = "select to_char(nv, '%H:%M %z|%:z|%%z') a, to_char(cast(nv as date), '%Y %z') d from t order by k"
    got = g.sql(sql).table
    assert got.equals(c.sql(sql).table)
    assert got.column("a")[0].as_py() == "03:00 %z|%:z|%z" and got.column("d")[0].as_py() == "2024 %z"


def test_generated_temporal_casts(engines):
    """CAST between timestamp and date inside a generated expression kernel (exec/expr_jit.py)
    floors to the day and scales back, over negative instants too."""
    g, c = engines
    sql = ("select k, cast(nv as date) d, cast(cast(nv as date) as timestamp) m, cast(to_local_time(ts) as date) z, "
           "cast(ts as date) l from t order by k")
    got = g.sql(sql).table
    assert got.equals(c.sql(sql).table)
    us = TC.sql_rows()
    assert got.column("d").cast(pa.int32()).to_pylist() == [None if v is None else v // 86_400_000_000 for v in us]
    assert got.column("l").cast(pa.int32()).to_pylist() == \
        [None if v is None else TC.o_to_local(v, "America/New_York") // 86_400_000_000 for v in us]


def test_parquet_native_reader(engines, tmp_path):
    g, c = engines
    before = KERNEL_CALLS["pq_decode"]
    TC.check_parquet(g, pa, tmp_path)
    assert KERNEL_CALLS["pq_decode"] > before          # the zoned column decoded on the device
    TC.check_parquet(c, pa, tmp_path)


def test_arrow_device_export(engines):
    g, _ = engines
    r = g.sql_device("select k, ts, ts at time zone 'Europe/Berlin' b, nv from t order by k")
    got = r.to_arrow()
    assert got.schema.field("ts").type == pa.timestamp("us", tz="America/New_York")
    assert got.schema.field("b").type == pa.timestamp("us", tz="Europe/Berlin")
    assert got.schema.field("nv").type == pa.timestamp("us")
    assert got.column("b").cast(pa.int64()).to_pylist() == TC.sql_rows() == got.column("ts").cast(pa.int64()).to_pylist()


def test_repeated_zoned_query_replays_as_a_graph(gpu_device):
    e = ig.QueryEngine(device=gpu_device)
    e.graphs_disabled = False
    e.register_table("t", TC.sql_table(pa))
    sql = ("select date_trunc('day', ts at time zone 'Pacific/Apia') d, hour(ts) h, count(*) n, "
           "max(to_local_time(ts)) hi, min(nv at time zone 'Europe/Dublin') lo from t where k % 3 <> 2 "
           "group by 1, 2 order by 1 nulls last, 2")
    h0 = sum(HOST_STEPS.values())
    first = e.sql(sql).table
    us = TC.sql_rows()
    want = sorted({(TC.o_trunc(v, "Pacific/Apia", "day"), TC.o_part(v, "America/New_York", "hour"))
                   for i, v in enumerate(us) if v is not None and i % 3 != 2})
    got = list(zip(first.column("d").cast(pa.int64()).to_pylist(), first.column("h").to_pylist()))
    assert [x for x in got if x[0] is not None] == want
    modes = []
    for _ in range(6):
        assert e.sql(sql).table.equals(first)
        modes.append(e.last_metrics["speculation"])
    assert sum(HOST_STEPS.values()) == h0
    assert modes[-1] == "graph", modes
