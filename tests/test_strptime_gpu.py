"""The strptime kernel (csrc/kernels/strptime.hip) on gfx950 against the cases of
tests/strptime_cases.py, at the operator and through SQL. Values are integers and compare
exactly. Every operator call on a plain column must advance KERNEL_CALLS["strptime"] by exactly
one, so a host fallback cannot pass.

Shapes: the case groups as they come, every row count around a wave and a block, and
256 * 16384 + 300 rows -- the first count at which the grid-stride loop takes a second trip --
tiled on the device from a 300-row column. Malformed text is ordinary input; no test feeds the
kernel corrupt offsets (that guard is exercised in tests/test_strptime_host.py only)."""
import re

import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
import strptime_cases as K
from igloo_amd import types as T
from igloo_amd.columnar import Column
from igloo_amd.ops import strptime as SP
from igloo_amd.ops._lib import HOST_STEPS, KERNEL_CALLS
from igloo_amd.utils.errors import ExecutionError
from test_strptime import bytes_column, call, groups, ints

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_UNITS = ("timestamp", "millis", "seconds", "date")


def run(col, formats, unit="timestamp", launches=1):
    k0, h0 = KERNEL_CALLS["strptime"], sum(HOST_STEPS.values())
    out = SP.strptime(col, formats, unit)
    assert KERNEL_CALLS["strptime"] == k0 + launches and sum(HOST_STEPS.values()) == h0
    assert out.data.is_cuda and out.data.dtype == (torch.int32 if unit == "date" else torch.int64)
    assert out.dtype == (T.DATE32 if unit == "date" else T.TIMESTAMP)
    return out


def values(col):
    ok = col.valid.cpu().tolist() if col.valid is not None else [True] * len(col)
    return [v if k else None for v, k in zip(col.data.cpu().tolist(), ok)]


def test_every_matching_case_in_every_unit():
    total = 0
    for formats, rows in groups(K.all_cases()).items():
        good = [(t, v) for t, v in rows if v is not None]
        if not good:
            continue
        col = bytes_column([t for t, _ in good] + [b"\xffNULL"], valid=[True] * len(good) + [False], device=DEV)
        for unit in OP_UNITS:
            assert values(run(col, formats, unit)) == [K.expect_unit(v, unit) for _, v in good] + [None], (formats, unit)
        total += len(good)
    assert total > 50_000


def test_every_rejected_case_is_named_in_row_order():
    """Each text no format matches, among texts that match: the error names the smallest bad row;
    that row is then made NULL (a NULL row never raises) and the next one is named."""
    n_bad = 0
    for formats, rows in groups(K.table_cases()).items():
        bad = [k for k, (_, v) in enumerate(rows) if v is None]
        if not bad:
            continue
        col = bytes_column([t for t, _ in rows], valid=[True] * len(rows), device=DEV)
        for k in bad:
            with pytest.raises(ExecutionError) as ex:
                SP.strptime(col, formats, "millis")
            m = re.match(r"to_timestamp_millis\(\): row (\d+): ", str(ex.value))
            assert m and int(m.group(1)) == k, (formats, rows[k][0], str(ex.value))
            col.valid[k] = False
        want = [None if v is None else K.expect_unit(v, "millis") for _, v in rows]
        assert values(run(col, formats, "millis")) == want, formats
        n_bad += len(bad)
    assert n_bad > 1000


@pytest.fixture(scope="module")
def base300():
    """300 texts of mixed shapes that four formats read between them, and their instants."""
    formats = ("%Y-%m-%dT%H:%M:%S%.f%#z", "%d/%b/%Y:%I:%M:%S %p %z", "%A, %B %d, %Y", "%Y-%m-%dT%H:%M:%S%.f")
    pool = [c for c in K.round_trip_cases() if c[0][0] in ("%Y-%m-%dT%H:%M:%S%.f", "%d/%b/%Y:%I:%M:%S %p %z",
                                                           "%Y-%m-%dT%H:%M:%S%#z", "%A, %B %d, %Y")]
    step = len(pool) // 300
    picked = [pool[i * step + (i % 7)] for i in range(300)]
    assert len({c[0] for c in picked}) == 4
    return formats, [t for _, t, _ in picked], [v for _, _, v in picked]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_row_counts_around_a_wave_and_a_block(base300, n):
    formats, texts, vals = base300
    col = bytes_column(texts[:n], device=DEV)
    for unit in ("timestamp", "date"):
        out = run(col, formats, unit, launches=1 if n else 0)          # n == 0 launches nothing
        assert values(out) == [K.expect_unit(v, unit) for v in vals[:n]]


def test_second_trip_of_the_grid_stride_loop(base300):
    formats, texts, vals = base300
    n = 256 * 16384 + 300
    reps = -(-n // 300)
    base = bytes_column(texts, device=DEV)
    nb = base.data.numel()
    data = base.data.repeat(reps)
    off = (base.offsets[:-1].unsqueeze(0) + torch.arange(reps, dtype=torch.int64, device=DEV).unsqueeze(1) * nb).reshape(-1)
    off = torch.cat([off, torch.tensor([reps * nb], dtype=torch.int64, device=DEV)])[:n + 1]
    want = torch.tensor(vals, dtype=torch.int64, device=DEV).repeat(reps)[:n]
    col = Column(T.UTF8, data, None, offsets=off)
    out = run(col, formats)
    assert len(out) == n and torch.equal(out.data, want)
    # one bad row in the second trip: its first byte is no digit and starts no name
    bad = 256 * 16384 + 150
    lo = int(off[bad].item())
    data[lo] = ord("#")
    with pytest.raises(ExecutionError, match=rf"to_timestamp\(\): row {bad}: '#"):
        SP.strptime(col, formats)


def test_dictionary_column():
    d = bytes_column([b"2024-04-03", b"not a date", b"2000-02-29", b"never used"], device=DEV)
    codes = torch.tensor([0, 2, 1, 0, 2, 3], dtype=torch.int32, device=DEV)
    valid = torch.tensor([True, True, False, True, True, False], device=DEV)
    a, b = K.us(2024, 4, 3), K.us(2000, 2, 29)
    # an unparsable entry that no non-NULL row uses does not raise: the rows decide (entries, then rows)
    out = run(Column(T.UTF8, codes, valid, dictionary=d), ("%F",), launches=2)
    assert values(out) == [a, b, None, a, b, None]
    # every entry parses: one launch over the entries, gathered by code; NULL rows stay NULL
    good = bytes_column([b"2024-04-03", b"2000-02-29"], device=DEV)
    codes2 = torch.tensor([1, 0, 0, 1, 1], dtype=torch.int32, device=DEV)
    valid2 = torch.tensor([True, False, True, True, False], device=DEV)
    out = run(Column(T.UTF8, codes2, valid2, dictionary=good), ("%F",), "date")
    assert values(out) == [b // K.US_DAY, None, a // K.US_DAY, b // K.US_DAY, None]
    assert out.data.cpu().tolist()[1] == 0 and out.data.cpu().tolist()[4] == 0      # 0 under NULL rows, as on a plain column
    assert values(run(Column(T.UTF8, codes2, None, dictionary=good), ("%F",))) == [b, a, a, b, b]
    # a used unparsable entry raises and names the row, not the entry
    with pytest.raises(ExecutionError, match=r"to_timestamp\(\): row 2: 'not a date'"):
        SP.strptime(Column(T.UTF8, codes, None, dictionary=d), ("%F",))


def test_slice_whose_first_offset_is_not_zero(base300):
    formats, texts, vals = base300
    full = bytes_column(texts, device=DEV)
    sl = Column(T.UTF8, full.data, None, offsets=full.offsets[37:37 + 101])
    assert int(sl.offsets[0].item()) > 0 and len(sl) == 100
    assert values(run(sl, formats)) == vals[37:137]


def test_last_row_ends_at_the_end_of_the_buffer():
    """The last text's one-digit day is the buffer's last byte: the greedy second digit must not be read."""
    col = bytes_column([b"2024-04-03", b"2024-4-3"], device=DEV)
    assert int(col.offsets[-1].item()) == col.data.numel()
    assert values(run(col, ("%Y-%m-%d",))) == [K.us(2024, 4, 3)] * 2
    col = bytes_column([b"13:05 3.4.2024 7"], device=DEV)
    assert values(run(col, ("%H:%M %d.%m.%Y %S",))) == [K.us(2024, 4, 3, 13, 5, 7)]


def test_error_names_the_smallest_bad_row_and_null_rows_never_raise():
    texts = [b"2024-04-03"] * 400
    texts[70], texts[300] = b"2024-04-31", b"junk"
    with pytest.raises(ExecutionError, match=r"to_date\(\): row 70: '2024-04-31' matches none of the formats \('%F', '%s'\)"):
        SP.strptime(bytes_column(texts, device=DEV), ("%F", "%s"), to_date=True)
    valid = [True] * 400
    valid[70] = valid[300] = False
    out = run(bytes_column(texts, valid=valid, device=DEV), ("%F", "%s"), "date")
    assert values(out) == [None if k in (70, 300) else K.us(2024, 4, 3) // K.US_DAY for k in range(400)]
    assert out.data[70].item() == 0 and out.data[300].item() == 0


def test_through_sql_on_the_device():
    """The six functions over the table and a sample of the generated cases; the expression paths that
    generate kernels decline the call, so the operator's kernel runs."""
    e = ig.QueryEngine(device=DEV)
    k0, h0 = KERNEL_CALLS["strptime"], sum(HOST_STEPS.values())
    n = 0
    for formats, rows in groups(K.round_trip_cases()[::20] + K.python_cases()[0][::10] + K.table_cases()).items():
        good = []
        for t, v in rows:
            if v is not None and b"\x00" not in t:
                good.append((t.decode("utf-8"), v))
        if not good:
            continue
        texts = [t for t, _ in good] + [None]
        e.register_table("c", pa.table({"k": pa.array(range(len(texts)), pa.int64()), "s": pa.array(texts, pa.string())}))
        sel = ", ".join(call(u, "s", formats) for u in K.UNITS)
        r = e.sql(f"select {sel} from c order by k").table
        for i, unit in enumerate(K.UNITS):
            assert ints(r, i) == [K.expect_unit(v, unit) for _, v in good] + [None], (formats, unit)
        n += len(good)
    assert n > 2500 and KERNEL_CALLS["strptime"] > k0 and sum(HOST_STEPS.values()) == h0
    # inside a filter and an aggregate
    texts = ["03/04/2024 13:05", "04/04/2024 00:00", None, "1/1/1999 0:0"] * 50
    e.register_table("c", pa.table({"s": pa.array(texts, pa.string()), "g": pa.array(list(range(200)), pa.int64())}))
    k0 = KERNEL_CALLS["strptime"]
    r = e.sql("select count(*) n, max(to_date(s, '%d/%m/%Y %H:%M')) d from c "
              "where to_timestamp(s, '%d/%m/%Y %H:%M') >= timestamp '2024-04-03 13:05:00' and g >= 4").table.to_pylist()
    assert r[0]["n"] == 98 and str(r[0]["d"]) == "2024-04-04" and KERNEL_CALLS["strptime"] > k0
    texts[130] = "31/04/2024 00:00"
    e.register_table("c", pa.table({"s": pa.array(texts, pa.string()), "g": pa.array(list(range(200)), pa.int64())}))
    with pytest.raises(ExecutionError, match=r"to_timestamp_seconds\(\): row 130: '31/04/2024 00:00'"):
        e.sql("select to_timestamp_seconds(s, '%d/%m/%Y %H:%M') from c")
