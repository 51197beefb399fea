"""The text <-> value kernels on gfx950 against plain Python expectations, at
the inputs of tests/text_cases.py: CAST(varchar AS ...) (strexpr.hip
parse_kernel), the CSV and NDJSON parsers (csv.hip, json.hip), CAST(... AS
VARCHAR) (fmt kernels), md5 / sha2 (digest.hip) and to_char (strfmt.hip).

Every comparison is exact: bit equality for doubles, byte equality for text.
Each test asserts that the native launch counter moved, so a host fallback
cannot pass. tests/test_textparse_host.py proves the same parsing routines on
two million floats on the CPU; the float slow path is integer only, so the
device must agree bit for bit, which is what is checked here."""
import datetime
import functools
import hashlib

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.csv as pacsv
import pytest
import torch

import text_cases as C
from igloo_amd import types as T
from igloo_amd.catalog import Field
from igloo_amd.columnar import Column
from igloo_amd.connectors.gpu_csv import CsvParseError, read_csv_gpu
from igloo_amd.connectors.gpu_json import JsonParseError, read_json_gpu
from igloo_amd.ops import digest as D
from igloo_amd.ops import strings as S
from igloo_amd.ops._lib import KERNEL_CALLS
from igloo_amd.utils.errors import ExecutionError

pytestmark = pytest.mark.gpu

N_RANDOM = 50_000          # > 256 threads x the blocks of a small grid: the grid-stride loop runs
KINDS = ["float", "int", "date"] + [f"decimal{s}" for s in C.DECIMAL_SCALES]


def _dtype(kind):
    if kind.startswith("decimal"):
        return T.DECIMAL(18, int(kind[7:]))
    return {"float": T.FLOAT64, "int": T.INT64, "date": T.DATE32}[kind]


@functools.lru_cache(maxsize=None)
def accepted(kind):
    """(texts, expected numpy array): the accepted fixed cases plus N_RANDOM random ones.
    Doubles are expected as their bit patterns."""
    if kind == "float":
        texts = [t for t, v in C.float_cases() if v is not None] + C.random_float_texts(N_RANDOM, 77)
        return texts, np.array([C.bits(float(t)) for t in texts], dtype=np.uint64)
    if kind == "int":
        texts = [t for t, v in C.int_cases() if v is not None] + C.random_int_texts(N_RANDOM, 78)
        return texts, np.array([C.expect_int(t) for t in texts], dtype=np.int64)
    if kind == "date":
        texts = [t for t, v in C.date_cases() if v is not None] + C.random_date_texts(N_RANDOM, 79)
        return texts, np.array([C.expect_date(t) for t in texts], dtype=np.int32)
    s = int(kind[7:])
    texts = [t for t, sc, v in C.decimal_cases() if sc == s and v is not None] + C.random_decimal_texts(N_RANDOM, s, 80 + s)
    return texts, np.array([C.expect_decimal(t, s) for t in texts], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def rejected(kind):
    if kind == "float":
        return [t for t, v in C.float_cases() if v is None]
    if kind == "int":
        return [t for t, v in C.int_cases() if v is None]
    if kind == "date":
        return [t for t, v in C.date_cases() if v is None]
    s = int(kind[7:])
    return [t for t, sc, v in C.decimal_cases() if sc == s and v is None]


def utf8_column(texts, device, valid=None, lead=()):
    """A plain Utf8 column of `texts`; with `lead`, a slice of a longer one:
    its offsets start past the bytes of the leading rows."""
    raw = [t.encode("utf-8") if isinstance(t, str) else t for t in list(lead) + list(texts)]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in raw], out=off[1:])
    chars = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8).copy())[:int(off[-1])].to(device)
    offsets = torch.from_numpy(off).to(device)[len(lead):]
    v = None if valid is None else torch.from_numpy(np.asarray(valid, dtype=np.bool_)).to(device)
    return Column(T.UTF8, chars, v, offsets=offsets)


def values_of(col, kind):
    x = col.data.cpu().numpy()
    return x.view(np.uint64) if kind == "float" else x


def text_rows(col):
    """The rows of a plain Utf8 column as bytes (None for NULL)."""
    off = col.offsets.cpu().numpy()
    chars = col.data.cpu().numpy().tobytes()
    valid = None if col.valid is None else col.valid.cpu().numpy()
    return [None if valid is not None and not valid[i] else chars[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def assert_same(texts, want, got, what):
    bad = np.flatnonzero(np.asarray(want) != np.asarray(got))
    assert bad.size == 0, f"{what}: {bad.size} of {len(texts)} differ, first: " + \
        str([(texts[i][:60], want[i], got[i]) for i in bad[:8]])


# ---- CAST(varchar AS ...) ---------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_parse_plain_sliced_and_masked(kind, gpu_device):
    texts, want = accepted(kind)
    t = _dtype(kind)
    before = KERNEL_CALLS["str_parse"]
    got = S.parse(utf8_column(texts, gpu_device), t)
    assert got.valid is None
    assert_same(texts, want, values_of(got, kind), f"{kind} plain")
    # the same rows as a slice of a longer column: offsets start past garbage rows
    got = S.parse(utf8_column(texts, gpu_device, lead=["garbage", "12x", "", "\xff\xfe"]), t)
    assert_same(texts, want, values_of(got, kind), f"{kind} sliced")
    # NULL rows hold text that does not parse: they neither raise nor disturb their neighbours
    valid = np.ones(len(texts), dtype=np.bool_)
    valid[::7] = False
    masked = [("not a value" if i % 14 else "") if not valid[i] else x for i, x in enumerate(texts)]
    got = S.parse(utf8_column(masked, gpu_device, valid=valid), t)
    assert got.valid is not None and bool((got.valid.cpu().numpy() == valid).all())
    assert_same(texts, np.where(valid, want, 0), np.where(valid, values_of(got, kind), 0), f"{kind} masked")
    assert KERNEL_CALLS["str_parse"] == before + 3


@pytest.mark.parametrize("kind", KINDS)
def test_parse_rejects_one_string_at_a_time(kind, gpu_device):
    texts, _ = accepted(kind)
    t = _dtype(kind)
    before = KERNEL_CALLS["str_parse"]
    bad = rejected(kind)
    assert bad
    for i, x in enumerate(bad):
        rows = texts[:300] if i % 2 == 0 else []       # among valid neighbours (two blocks), and alone
        with pytest.raises(ExecutionError):
            S.parse(utf8_column(rows + [x] + rows[:5], gpu_device), t)
    assert KERNEL_CALLS["str_parse"] == before + len(bad)


def test_parse_int32_range(gpu_device):
    ok = ["2147483647", "-2147483648", "+5", "-0", "007"]
    got = S.parse(utf8_column(ok, gpu_device), T.INT32)
    assert got.data.cpu().tolist() == [2147483647, -2147483648, 5, 0, 7]
    for x in ("2147483648", "-2147483649", "9223372036854775807", "1.0", ""):
        with pytest.raises(ExecutionError):
            S.parse(utf8_column(["1", x, "2"], gpu_device), T.INT32)


def test_cpu_and_gpu_agree_where_both_accept(gpu_device):
    """The CPU path is Arrow's cast: where it accepts a text the contract accepts, the value is the same."""
    for kind in ("float", "int", "date"):
        texts, want = accepted(kind)
        texts, want = texts[:4000], want[:4000]
        t = _dtype(kind)
        agree = 0
        for x, w in zip(texts, want):
            try:
                cpu = pc.cast(pa.array([x], pa.large_string()), t.to_arrow())[0].as_py()
            except pa.ArrowInvalid:
                continue
            if kind == "float":
                assert C.bits(cpu) == int(w), (x, cpu)
            elif kind == "date":
                assert cpu.toordinal() - 719163 == int(w), (x, cpu)
            else:
                assert cpu == int(w), (x, cpu)
            agree += 1
        assert agree > len(texts) // 2, (kind, agree)


# ---- CSV ---------------------------------------------------------------------

# accepted by the contract of text_cases.py, not by Arrow's CSV reader (asserted below)
PYARROW_CANNOT_READ = {"int": lambda x: x.startswith("+"),
                       "decimal": lambda x: x in ("1.0000000000000000000000000000000000000000", "0" * 40 + "." + "0" * 40)}


def _csv_file(path, texts, tail_newline):
    """k,v,w: row r holds texts[r] in v (every third one quoted) and another case as the row's
    last field w (every fifth quoted); line ends alternate between \\n and \\r\\n."""
    n = len(texts)
    rows = ["k,v,w\n"]
    for r in range(n):
        v, w = texts[r], texts[(r * 7 + 3) % n]
        if r % 3 == 0:
            v = '"' + v + '"'
        if r % 5 == 0:
            w = '"' + w + '"'
        end = "" if (r == n - 1 and not tail_newline) else ("\r\n" if r % 2 else "\n")
        rows.append(f"{r},{v},{w}{end}")
    with open(path, "w", newline="") as fh:
        fh.write("".join(rows))


@pytest.mark.parametrize("kind", KINDS)
def test_csv_fields_exact(kind, gpu_device, tmp_path):
    texts, want = accepted(kind)
    keep = [i for i, x in enumerate(texts) if x != ""]
    assert len(keep) == len(texts)                     # nothing is dropped: no accepted case is empty
    t = _dtype(kind)
    fields = [Field("k", T.INT64), Field("v", t), Field("w", t)]
    n = len(texts)
    perm = (np.arange(n) * 7 + 3) % n
    for tail_newline in (True, False):
        path = str(tmp_path / f"{kind}_{tail_newline}.csv")
        _csv_file(path, texts, tail_newline)
        before = KERNEL_CALLS["csv_parse"]
        got = read_csv_gpu(path, fields, None, gpu_device)
        assert KERNEL_CALLS["csv_parse"] == before + 1
        assert got["k"].data.cpu().tolist() == list(range(n))
        assert got["v"].valid is None and got["w"].valid is None
        assert_same(texts, want, values_of(got["v"], kind), f"csv {kind} v")
        assert_same([texts[i] for i in perm], want[perm], values_of(got["w"], kind), f"csv {kind} w (last field)")
    # Arrow's reader on the same texts (minus the spellings it cannot read, each asserted)
    base = "decimal" if kind.startswith("decimal") else kind
    cannot = PYARROW_CANNOT_READ.get(base, lambda x: False)
    skip = {x for x in texts if cannot(x)}
    atype = pa.decimal128(38, t.scale) if base == "decimal" else t.to_arrow()
    co = pacsv.ConvertOptions(column_types={"v": atype})
    for x in sorted(skip)[:25]:
        with pytest.raises(pa.ArrowInvalid):
            pacsv.read_csv(pa.BufferReader(f"v\n{x}\n".encode()), convert_options=co)
    rows = [i for i, x in enumerate(texts) if x not in skip]
    ref = pacsv.read_csv(pa.BufferReader(("v\n" + "".join(f'"{texts[i]}"\n' for i in rows)).encode()),
                         convert_options=co).column("v").combine_chunks()
    if base == "float":
        ref_vals = ref.to_numpy(zero_copy_only=False).view(np.uint64)
    elif base == "date":
        ref_vals = ref.cast(pa.int32()).to_numpy()
    elif base == "int":
        ref_vals = ref.to_numpy()
    else:
        ref_vals = np.array([int(d.scaleb(t.scale)) for d in ref.to_pylist()], dtype=np.int64)
    assert_same([texts[i] for i in rows], ref_vals, want[rows], f"arrow csv {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_csv_rejects_one_field_per_file(kind, gpu_device, tmp_path):
    texts, _ = accepted(kind)
    t = _dtype(kind)
    fields = [Field("k", T.INT64), Field("v", t, nullable=False)]
    path = str(tmp_path / "bad.csv")
    bad = [x for x in rejected(kind) if x != ""]       # an empty field is NULL, not a parse error (below)
    for i, x in enumerate(bad):
        q = '"' if ("," in x or i % 2) else ""
        with open(path, "w", newline="") as fh:
            fh.write("k,v\n" + "".join(f"{r},{texts[r]}\n" for r in range(3)) + f"3,{q}{x}{q}\r\n4,{texts[4]}")
        with pytest.raises(CsvParseError):
            read_csv_gpu(path, fields, None, gpu_device)
    # the empty field: NULL in a nullable column
    with open(path, "w", newline="") as fh:
        fh.write(f"k,v\n0,{texts[0]}\n1,\n2,{texts[2]}\n")
    got = read_csv_gpu(path, [Field("k", T.INT64), Field("v", t)], None, gpu_device)
    assert got["v"].valid.cpu().tolist() == [True, False, True]


# ---- NDJSON ------------------------------------------------------------------

JSON_SCHEMA = [Field("i", T.INT64), Field("f", T.FLOAT64), Field("s", T.UTF8), Field("t", T.UTF8), Field("b", T.BOOL)]


@pytest.mark.parametrize("nrows", [1, 64, 65, 257, 2000])
def test_ndjson_records(nrows, gpu_device, tmp_path):
    lines, rows = C.json_records(nrows, 100 + nrows)
    path = str(tmp_path / "t.json")
    with open(path, "w", newline="", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + ("\n" if nrows % 2 else ""))
    before = KERNEL_CALLS["json_parse"], KERNEL_CALLS["json_str_copy"]
    got = read_json_gpu(path, JSON_SCHEMA, None, gpu_device)
    assert KERNEL_CALLS["json_parse"] == before[0] + 1
    for name in ("i", "f", "b"):
        col = got[name]
        valid = np.ones(nrows, dtype=np.bool_) if col.valid is None else col.valid.cpu().numpy()
        vals = col.data.cpu().numpy()
        for r in range(nrows):
            w = rows[r][name]
            assert bool(valid[r]) == (w is not None), (name, r, lines[r])
            if w is None:
                continue
            if name == "f":
                assert C.bits(float(vals[r])) == C.bits(float(w)), (r, lines[r], w, vals[r])
            else:
                assert vals[r] == w, (name, r, lines[r])
    for name in ("s", "t"):
        have = text_rows(got[name])
        for r in range(nrows):
            w = rows[r][name]
            assert have[r] == (None if w is None else w.encode("utf-8")), (name, r, lines[r], have[r])
    if any(rows[r]["s"] or rows[r]["t"] for r in range(nrows)):
        assert KERNEL_CALLS["json_str_copy"] > before[1]


@pytest.mark.parametrize("what", sorted(C.JSON_ERROR_LINES))
def test_ndjson_errors(what, gpu_device, tmp_path):
    good, _ = C.json_records(70, 5)
    path = str(tmp_path / "bad.json")
    for lines in ([C.JSON_ERROR_LINES[what]], good + [C.JSON_ERROR_LINES[what]] + good[:3]):
        with open(path, "w", newline="", encoding="utf-8") as fh:
            fh.write("\n".join(lines) + "\n")
        with pytest.raises(JsonParseError):
            read_json_gpu(path, JSON_SCHEMA, None, gpu_device)


# ---- digests -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _digest_inputs():
    rows = C.digest_strings(300) + ["x" * 10_000, "é" * 5_000]
    return rows


@pytest.mark.parametrize("algo", ["md5", "sha224", "sha256", "sha384", "sha512"])
def test_digests_every_length(algo, gpu_device):
    rows = _digest_inputs()
    assert sorted(len(s.encode()) for s in rows[:301]) == list(range(301))     # every padding boundary is present
    want = [hashlib.new(algo, s.encode("utf-8")).hexdigest().encode() for s in rows]
    before = KERNEL_CALLS["digest_hex"]
    assert text_rows(D.hex_digest(utf8_column(rows, gpu_device), algo)) == want
    # NULL rows stay NULL
    valid = np.ones(len(rows), dtype=np.bool_)
    valid[::5] = False
    got = text_rows(D.hex_digest(utf8_column(rows, gpu_device, valid=valid), algo))
    assert got == [w if v else None for w, v in zip(want, valid)]
    # a slice of a longer column
    got = text_rows(D.hex_digest(utf8_column(rows, gpu_device, lead=["lead", "", "é" * 33]), algo))
    assert got == want
    assert KERNEL_CALLS["digest_hex"] == before + 3
    # the same data as a dictionary column: each distinct value hashed once, the codes pick
    codes = np.array([(i * 37) % len(rows) for i in range(1000)], dtype=np.int32)
    dic = Column(T.UTF8, torch.from_numpy(codes).to(gpu_device), None, dictionary=utf8_column(rows, gpu_device))
    got = D.hex_digest(dic, algo)
    assert KERNEL_CALLS["digest_hex"] == before + 4
    assert [None if x is None else x.encode() for x in got.to_arrow().to_pylist()] == [want[c] for c in codes]


# ---- to_char -------------------------------------------------------------------

DAYS = ["Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday", "Sunday"]
MONTHS = ["January", "February", "March", "April", "May", "June", "July", "August", "September", "October", "November",
          "December"]


def _h12(t):
    return t.hour % 12 or 12


# every supported specifier alone, then the combined patterns; (t: datetime, us: microseconds since the epoch)
TO_CHAR = {
    "%Y": lambda t, us: f"{t.year:04d}", "%C": lambda t, us: f"{t.year // 100:02d}", "%y": lambda t, us: f"{t.year % 100:02d}",
    "%m": lambda t, us: f"{t.month:02d}", "%d": lambda t, us: f"{t.day:02d}", "%e": lambda t, us: f"{t.day:2d}",
    "%j": lambda t, us: f"{(t.date() - datetime.date(t.year, 1, 1)).days + 1:03d}",
    "%H": lambda t, us: f"{t.hour:02d}", "%k": lambda t, us: f"{t.hour:2d}", "%I": lambda t, us: f"{_h12(t):02d}",
    "%l": lambda t, us: f"{_h12(t):2d}", "%M": lambda t, us: f"{t.minute:02d}", "%S": lambda t, us: f"{t.second:02d}",
    "%p": lambda t, us: "AM" if t.hour < 12 else "PM", "%P": lambda t, us: "am" if t.hour < 12 else "pm",
    "%f": lambda t, us: f"{t.microsecond:06d}000", "%.3f": lambda t, us: f".{t.microsecond // 1000:03d}",
    "%.6f": lambda t, us: f".{t.microsecond:06d}", "%.9f": lambda t, us: f".{t.microsecond:06d}000",
    "%.f": lambda t, us: f".{t.microsecond:06d}000",
    "%a": lambda t, us: DAYS[t.weekday()][:3], "%A": lambda t, us: DAYS[t.weekday()],
    "%b": lambda t, us: MONTHS[t.month - 1][:3], "%h": lambda t, us: MONTHS[t.month - 1][:3],
    "%B": lambda t, us: MONTHS[t.month - 1], "%u": lambda t, us: f"{t.isoweekday()}", "%w": lambda t, us: f"{t.isoweekday() % 7}",
    "%F": lambda t, us: f"{t.year:04d}-{t.month:02d}-{t.day:02d}", "%T": lambda t, us: f"{t.hour:02d}:{t.minute:02d}:{t.second:02d}",
    "%D": lambda t, us: f"{t.month:02d}/{t.day:02d}/{t.year % 100:02d}", "%R": lambda t, us: f"{t.hour:02d}:{t.minute:02d}",
    "%s": lambda t, us: f"{us // 1_000_000}", "%%": lambda t, us: "%",
    # combined, and what is not a specifier is copied
    "%Y-%m-%d %H:%M:%S%.6f": lambda t, us: f"{t.year:04d}-{t.month:02d}-{t.day:02d} {t.hour:02d}:{t.minute:02d}:"
                                            f"{t.second:02d}.{t.microsecond:06d}",
    "%F %T": lambda t, us: f"{t.year:04d}-{t.month:02d}-{t.day:02d} {t.hour:02d}:{t.minute:02d}:{t.second:02d}",
    "%A, %B %e, %Y at %l:%M %p (day %j, week day %u) 100%%": lambda t, us: (
        f"{DAYS[t.weekday()]}, {MONTHS[t.month - 1]} {t.day:2d}, {t.year:04d} at {_h12(t):2d}:{t.minute:02d} "
        f"{'AM' if t.hour < 12 else 'PM'} (day {(t.date() - datetime.date(t.year, 1, 1)).days + 1:03d}, "
        f"week day {t.isoweekday()}) 100%"),
    "%d/%m/%y %I%P %a %b é€ %q %": lambda t, us: (
        f"{t.day:02d}/{t.month:02d}/{t.year % 100:02d} {_h12(t):02d}{'am' if t.hour < 12 else 'pm'} "
        f"{DAYS[t.weekday()][:3]} {MONTHS[t.month - 1][:3]} é€ %q %"),
    "%.4f %.": lambda t, us: "%.4f %.",
}


@functools.lru_cache(maxsize=None)
def _date_values():
    return [v for _, v in C.date_cases() if v is not None]


@functools.lru_cache(maxsize=None)
def _timestamp_values():
    day = 86_400_000_000
    vals = [-1, 0, 999_999, 1, 1_000_000, -1_000_000, -1_000_001, day - 1, day, 12 * 3600 * 1_000_000,
            -day, -day - 1, -day + 1, 43_200_000_000 - 1, 86_399_999_999, -86_399_999_999,
            -2_208_988_800_000_000 + 123_456, -2_208_988_800_000_000 - 1,          # around 1900-01-01
            -62_135_596_800_000_000, 253_402_300_799_999_999,                      # 0001-01-01 .. 9999-12-31 23:59:59.999999
            951_782_400_000_000 + 86_399_999_999, 1_709_164_800_000_000 + 500_000]  # 2000-02-29, 2024-02-29
    for d in _date_values()[::37]:
        vals += [d * day, d * day + 43_200_000_000, d * day + 86_399_999_999, d * day + 3_723_000_004]
    return vals


def _to_char_check(col, us_values, device_calls_before):
    epoch = datetime.datetime(1970, 1, 1)
    ts = [epoch + datetime.timedelta(microseconds=u) for u in us_values]
    for fmt, ref in TO_CHAR.items():
        want = [ref(t, u) for t, u in zip(ts, us_values)]
        got = [b.decode("utf-8") for b in text_rows(D.to_char(col, fmt))]
        bad = [(u, w, g) for u, w, g in zip(us_values, want, got) if w != g]
        assert not bad, (fmt, len(bad), bad[:5])
        # the CPU twin is pinned to the same reference
        step = max(1, len(us_values) // 200)
        assert [D.py_strftime(u, fmt) for u in us_values[::step]] == want[::step], fmt
    assert KERNEL_CALLS["strfmt"] == device_calls_before + len(TO_CHAR)


def test_to_char_dates(gpu_device):
    days = _date_values()
    col = Column(T.DATE32, torch.tensor(days, dtype=torch.int32, device=gpu_device))
    _to_char_check(col, [d * 86_400_000_000 for d in days], KERNEL_CALLS["strfmt"])


def test_to_char_timestamps(gpu_device):
    us = _timestamp_values()
    col = Column(T.TIMESTAMP, torch.tensor(us, dtype=torch.int64, device=gpu_device))
    _to_char_check(col, us, KERNEL_CALLS["strfmt"])


def test_to_char_format_length_limit(gpu_device):
    """The format travels to the kernel in a 128-byte argument: 128 bytes work, 129 raise (never truncated)."""
    col = Column(T.DATE32, torch.tensor([0, 19782], dtype=torch.int32, device=gpu_device))
    fmt = "%Y-%m-%d|" * 14 + "%%"
    assert len(fmt.encode()) == 128
    assert text_rows(D.to_char(col, fmt)) == [b"1970-01-01|" * 14 + b"%", b"2024-02-29|" * 14 + b"%"]
    assert D.py_strftime(0, fmt) == "1970-01-01|" * 14 + "%"
    with pytest.raises(RuntimeError, match="longer than 128 bytes"):
        D.to_char(col, fmt + "x")


# ---- CAST(... AS VARCHAR) ------------------------------------------------------

def test_to_string_fixed_point(gpu_device):
    cases = C.fixed_format_cases()
    before = KERNEL_CALLS["fmt"]
    for s in range(19):
        rows = [(v, t) for v, sc, t in cases if sc == s]
        col = Column(T.DECIMAL(18, s) if s else T.INT64, torch.tensor([v for v, _ in rows], dtype=torch.int64, device=gpu_device))
        assert text_rows(S.to_string(col)) == [t.encode() for _, t in rows], s
    assert KERNEL_CALLS["fmt"] == before + 19


def test_to_string_int32_date_bool(gpu_device):
    before = KERNEL_CALLS["fmt"]
    ints = [0, 1, -1, 9, 10, -10, 2147483647, -2147483648, 1000000000, -999999999]
    col = Column(T.INT32, torch.tensor(ints, dtype=torch.int32, device=gpu_device))
    assert text_rows(S.to_string(col)) == [str(v).encode() for v in ints]
    cases = C.date_format_cases()
    col = Column(T.DATE32, torch.tensor([v for v, _ in cases], dtype=torch.int32, device=gpu_device))
    got = text_rows(S.to_string(col))
    bad = [(v, t, g) for (v, t), g in zip(cases, got) if t.encode() != g]
    assert not bad, (len(bad), bad[:8])
    valid = torch.tensor([True, False, True, True, False], device=gpu_device)
    col = Column(T.BOOL, torch.tensor([True, True, False, True, False], device=gpu_device), valid)
    assert text_rows(S.to_string(col)) == [b"true", None, b"false", b"true", None]
    assert KERNEL_CALLS["fmt"] == before + 3
