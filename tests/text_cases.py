"""Hard inputs for the text <-> value routines (csrc/kernels/textparse.h,
json.hip, digest.hip, strfmt.hip), shared by tests/test_textparse_host.py
(the routines compiled as host C++ under sanitizers) and
tests/test_text_values_gpu.py (the gfx950 kernels). A plain helper module:
seeded generators that return ``(text, expected)`` lists, where ``expected``
is ``None`` for a text that must be rejected. Expectations come from Python
alone: ``float()`` (correctly rounded), ``decimal.Decimal``, ``int()``,
``datetime.date``, ``hashlib`` and ``json.loads``.

Every comparison made with these cases is exact: bits for doubles, bytes for
text.
"""
import datetime
import decimal
import functools
import json
import random
import re
import struct
from decimal import Decimal

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
DBL_MAX = 1.7976931348623157e308
DECIMAL_SCALES = (0, 2, 9, 18)
_CTX = decimal.Context(prec=2500, Emin=-999999, Emax=999999)

# ---- the accept / reject contract, written down once -----------------------
# A text is accepted exactly when it matches its kind's grammar in full (no
# surrounding whitespace, ASCII digits only) and the value condition holds;
# everything else raises.
#   float    any magnitude is accepted: overflow is +-inf, underflow is +-0
#   int      the value fits int64 ("+5", "-0" and leading zeros are fine)
#   decimal  the value is exact at the column's scale (extra fractional digits
#            must be zeros) and the scaled value fits int64, however many
#            leading zeros or digits the text has
#   date     YYYY-MM-DD, a real day of the proleptic Gregorian calendar
CONTRACT = {
    "float": re.compile(r"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?"
                        r"|[nN][aA][nN])"),
    "int": re.compile(r"[+-]?[0-9]+"),
    "decimal": re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)"),
    "date": re.compile(r"[0-9]{4}-[0-9]{2}-[0-9]{2}"),
}


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def expect_float(text: str):
    return float(text) if CONTRACT["float"].fullmatch(text) else None


def expect_int(text: str):
    if not CONTRACT["int"].fullmatch(text):
        return None
    v = int(text)
    return v if INT64_MIN <= v <= INT64_MAX else None


def expect_decimal(text: str, scale: int):
    """The scaled int64, or None."""
    if not CONTRACT["decimal"].fullmatch(text):
        return None
    v = _CTX.scaleb(Decimal(text), scale)
    if v != v.to_integral_value(context=_CTX):
        return None
    n = int(v)
    return n if INT64_MIN <= n <= INT64_MAX else None


def expect_date(text: str):
    """Days since 1970-01-01, or None."""
    if not CONTRACT["date"].fullmatch(text):
        return None
    y, m, d = int(text[:4]), int(text[5:7]), int(text[8:])
    try:
        return datetime.date(y, m, d).toordinal() - 719163
    except ValueError:
        return None


# ---- floats ----------------------------------------------------------------

def random_double(rng) -> float:
    """Bit pattern uniform over every finite exponent, subnormals included."""
    while True:
        b = rng.getrandbits(64)
        if (b >> 52) & 0x7FF != 0x7FF:
            return from_bits(b)


def float_forms(x: float):
    return [repr(x), "%.17e" % x, "%.6e" % x, "%.2f" % x]


def _midpoint_texts(a: Decimal, b: Decimal):
    """The exact decimal midpoint of two adjacent doubles, and the same
    string with its last digit moved one up and one down."""
    mid = _CTX.divide(_CTX.add(a, b), Decimal(2))
    unit = Decimal(1).scaleb(mid.as_tuple().exponent)
    return [str(mid), str(_CTX.add(mid, unit)), str(_CTX.subtract(mid, unit)),
            format(mid, "f") if -400 < mid.adjusted() < 40 else str(mid)]


def float_midpoints(n_random: int = 150, seed: int = 11):
    rng = random.Random(seed)
    lows = [float(2 ** 53 - 2), float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2), 1.0, from_bits(bits(1.0) - 1),
            0.0, 5e-324, from_bits(0x000FFFFFFFFFFFFE), from_bits(0x000FFFFFFFFFFFFF), 2.2250738585072014e-308,
            from_bits(bits(DBL_MAX) - 1), 0.1, 1e22, 1e23, 8.98846567431158e307]
    for _ in range(n_random):
        lows.append(abs(random_double(rng)))
    for _ in range(n_random // 3):
        lows.append(from_bits(rng.getrandbits(52)))                      # subnormal
    out = []
    for a in lows:
        if a >= DBL_MAX:
            continue
        b = from_bits(bits(a) + 1)
        out += _midpoint_texts(Decimal(a), Decimal(b))
    # DBL_MAX and the overflow midpoint 2^1024 - 2^970
    out += _midpoint_texts(Decimal(DBL_MAX), Decimal(2 ** 1024))
    out.append("9007199254740993")
    out.append("2.4703282292062327208051355972539e-324")                 # just below / above half the min subnormal
    out.append("2.4703282292062327208051355972540e-324")
    out += ["-" + t for t in out[::7]]
    return [(t, expect_float(t)) for t in out]


def float_mantissa_cases(n: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rng.randint(1, 25)
        m = rng.randrange(10 ** (nd - 1), 10 ** nd)
        out.append("%de%d" % (m, rng.randint(-350, 350)))
    return out


FLOAT_HAND = [
    # syntax
    "1.", ".5", "+.5", "-.5", "1e+5", "1E5", "1e-5", "1.5e3", "-0.0", "0", "-0", "+0", "0.0e0", "0e999999",
    # leading and trailing zeros
    "000123.4500", "0000000000000000000000000001", "0.0000000000000000000000000001", "1.0000000000000000000000000000",
    "00.00", "100000000000000000000000", "1" + "0" * 400, "0." + "0" * 400 + "1", "0" * 50 + "." + "0" * 50 + "7e52",
    "1e0000000000000000000005", "1e-0000000000000000000005",
    # range
    "1e400", "1e-400", "-1e400", "-1e-400", "1e99999", "-1e-99999", "1e99999999999999999999", "1e-99999999999999999999",
    "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1.8e308", "179769313486231580793e289",
    "4.9e-324", "5e-324", "2.5e-324", "2.4e-324", "2.2250738585072011e-308", "2.2250738585072014e-308",
    "0." + "0" * 330 + "1", "123456789012345678901234567890e-360", "0.00000001e-330",
    # the issue's examples and more than 19 significant digits
    "0.9680488278733529", "9007199254740993", "9007199254740992.9999999999999999999", "9007199254740993.0000000000000000001",
    "1.00000000000000011102230246251565404236316680908203125",
    "1.00000000000000011102230246251565404236316680908203124",
    "1.00000000000000011102230246251565404236316680908203126",
    "12345678901234567890", "1234567890123456789012345", "0.12345678901234567890123456789",
    "9" * 19, "9" * 20, "9" * 25 + "e-10", "18446744073709551615", "18446744073709551616", "9999999999999999999e289",
    # more than 800 significant digits
    "1" * 850, "0." + "3" * 900, "1." + "0" * 850 + "1", "1." + "0" * 850 + "1e-300", "9" * 1200 + "e-1000",
    # special values, any case
    "inf", "-inf", "+inf", "Infinity", "-Infinity", "INF", "iNfInItY", "nan", "NaN", "NAN",
]
FLOAT_REJECT = ["", ".", "-", "+", "e5", "1e", "1e+", "1e-", "1.2.3", " 1", "1 ", "0x10", "1_0", "1d5", "-.", "+.e1", ".e1",
                "1e5.0", "1e 5", "--1", "+-1", "in", "infi", "infinityy", "na", "nan0", "1inf", "1,5", "1f", "١"]


@functools.lru_cache(maxsize=None)
def float_cases():
    """The fixed float list: [(text, float or None)]."""
    rng = random.Random(7)
    texts = list(FLOAT_HAND)
    for _ in range(600):
        texts += float_forms(random_double(rng))
    for b in (1, 2, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x0010000000000001, 0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000,
              0x4340000000000000, 0x433FFFFFFFFFFFFF, 0x4340000000000001):
        texts += float_forms(from_bits(b))
        texts += float_forms(-from_bits(b))
    texts += float_mantissa_cases(1500, 8)
    out = [(t, expect_float(t)) for t in texts]
    out += float_midpoints()
    assert all(v is not None for _, v in out)
    out += [(t, expect_float(t)) for t in FLOAT_REJECT]
    assert all(v is None for _, v in out[-len(FLOAT_REJECT):])
    return out


def random_float_texts(n: int, seed: int):
    """n accepted float texts of the families above (no expectations: the
    caller maps ``float`` over them)."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        k = rng.randrange(8)
        x = random_double(rng)
        if k == 0:
            out.append(repr(x))
        elif k == 1:
            out.append("%.17e" % x)
        elif k == 2:
            out.append("%.6e" % x)
        elif k == 3:
            out.append("%.2f" % (x if abs(x) < 1e22 else rng.uniform(-1e6, 1e6)))
        elif k == 4:
            out.append(repr(rng.uniform(-1e6, 1e6)))
        elif k == 5:
            out.append(repr(rng.random()))
        elif k == 6:
            nd = rng.randint(1, 25)
            out.append("%de%d" % (rng.randrange(10 ** (nd - 1), 10 ** nd), rng.randint(-350, 350)))
        else:
            # a double's neighbourhood with more digits than fit 64 bits: often within the parser's bracket
            out.append("%.24e" % x if rng.random() < 0.5 else "%.30f" % rng.uniform(-1e3, 1e3))
    return out


# ---- integers --------------------------------------------------------------

INT_REJECT = ["", "-", "+", "1.0", "10000000000000000000", "99999999999999999999", "-10000000000000000000",
              "1234567890123456789012345", "9223372036854775808", "-9223372036854775809", "18446744073709551616",
              "18446744073709551617", "1e3", " 1", "1 ", "0x1", "--1", "1-", "٣"]


@functools.lru_cache(maxsize=None)
def int_cases():
    texts = ["0", "-0", "+0", "+5", "007", "-007", "000000000000000000000000000007", "1", "-1"]
    for lim in (1 << 31, 1 << 63):
        for d in (-2, -1, 0, 1, 2):
            texts += [str(lim + d), str(-lim + d)]
    rng = random.Random(5)
    for _ in range(300):
        nd = rng.randint(1, 19)
        texts.append(("-" if rng.random() < 0.5 else "") + str(rng.randrange(10 ** (nd - 1), 10 ** nd)))
    out = [(t, expect_int(t)) for t in texts] + [(t, expect_int(t)) for t in INT_REJECT]
    assert all(v is None for _, v in out[-len(INT_REJECT):])
    return out


def random_int_texts(n: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rng.randint(1, 19)
        v = rng.randrange(10 ** (nd - 1), min(10 ** nd, INT64_MAX + 1))    # every one is accepted
        out.append(("-" if rng.random() < 0.5 else "+" if rng.random() < 0.05 else "") + "0" * rng.randrange(3) + str(v))
    return out


# ---- decimals --------------------------------------------------------------

def _point(digits: str, scale: int) -> str:
    """The digits of a scaled integer as text with the point `scale` from the right."""
    if scale == 0:
        return digits
    digits = digits.rjust(scale + 1, "0")
    return digits[:-scale] + "." + digits[-scale:]


@functools.lru_cache(maxsize=None)
def decimal_cases():
    """[(text, scale, scaled int or None)] for the scales of DECIMAL_SCALES."""
    out = []
    for s in DECIMAL_SCALES:
        texts = ["0", "-0", "1", "-1", "1.000", ".5", "5.", "-.5", "+.5", "+5", "007.10", ".", "-.", "+.", "", "-", "+", "1.2.3",
                 "1e2", " 1", "1 ", "1.005", "0.0000000000000000001", "1.0000000000000000000000000000000000000000",
                 "0" * 40 + "1", "0" * 40 + "." + "0" * 40, "-" + "0" * 40 + "12.50", "1" * 36, "-" + "1" * 36, "1" * 60,
                 "9" * 37, "0." + "0" * 17 + "1", "123456789012345678.000000000000000001"]
        for edge in (INT64_MAX, INT64_MIN):
            for d in (-1, 0, 1, 2):
                v = edge + (d if edge > 0 else -d)
                texts.append(("-" if v < 0 else "") + _point(str(abs(v)), s))
            texts.append(("-" if edge < 0 else "") + _point(str(abs(edge)), s) + "000")
        out += [(t, s, expect_decimal(t, s)) for t in texts]
    return out


def random_decimal_texts(n: int, scale: int, seed: int):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rng.randint(1, 18)
        v = rng.randrange(10 ** (nd - 1), 10 ** nd)
        t = _point(str(v), scale)
        k = rng.randrange(4)
        if k == 0 and scale:
            t = t.rstrip("0")                 # fewer fractional digits ("5." when all are zeros)
        elif k == 1 and scale:
            t += "0" * rng.randrange(4)       # zeros past the scale are exact
        out.append(("-" if rng.random() < 0.5 else "") + t)
    return out


# ---- dates -----------------------------------------------------------------

FULL_YEARS = (1900, 2000, 2023, 2024)


@functools.lru_cache(maxsize=None)
def date_cases():
    texts = ["0001-01-01", "9999-12-31", "1970-01-01", "1969-12-31", "1600-02-29", "2100-02-28"]
    for y in FULL_YEARS:
        d = datetime.date(y, 1, 1)
        while d.year == y:
            texts.append(d.isoformat())
            d += datetime.timedelta(days=1)
    out = [(t, expect_date(t)) for t in texts]
    assert all(v is not None for _, v in out)
    bad = ["2023-2-03", "2023/02/03", "2023-02-3", "20230203", "2023-00-10", "2023-13-01", "2023-01-00", "", "2023-02-03 ",
           "+023-02-03", "2023-02-03T00", "1900-02-29", "2100-02-29"]
    for y in (2023, 2024):
        for m in range(1, 13):
            last = (datetime.date(y + (m == 12), m % 12 + 1, 1) - datetime.timedelta(days=1)).day
            bad += ["%04d-%02d-%02d" % (y, m, d) for d in range(last + 1, 32)] + ["%04d-%02d-32" % (y, m)]
    out += [(t, expect_date(t)) for t in bad]
    assert all(v is None for _, v in out[-len(bad):])
    return out


def random_date_texts(n: int, seed: int):
    rng = random.Random(seed)
    return [datetime.date.fromordinal(rng.randint(1, 3652059)).isoformat() for _ in range(n)]


# ---- value -> text ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixed_format_cases():
    """[(int64 value, scale, text)] against Decimal's plain notation."""
    rng = random.Random(3)
    out = []
    for s in range(19):
        vals = [INT64_MIN, INT64_MAX, INT64_MIN + 1, 0, 1, -1, 5, -5, 10 ** s, -(10 ** s), 10 ** s - 1, -(10 ** s - 1),
                10 ** s + 1, 10 ** max(s - 1, 0), -(10 ** max(s - 1, 0)), 9, -9, 10, -10, 99, 100, -100]
        vals += [rng.randrange(-(10 ** k), 10 ** k) for k in range(1, 19)]
        for v in vals:
            out.append((v, s, format(_CTX.scaleb(Decimal(v), -s), "f")))
    return out


def _leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def civil_from_days(days: int):
    """Proleptic Gregorian (year, month, day) of a day count from 1970-01-01:
    whole 400-year cycles, then a walk over years and months. Year 0 and
    negative years are astronomical (year 0 is leap)."""
    cycles, n = divmod(days + 719162, 146097)        # days from 0001-01-01
    y = 1 + 400 * cycles
    while n >= (366 if _leap(y) else 365):
        n -= 366 if _leap(y) else 365
        y += 1
    m = 1
    for dim in (31, 29 if _leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31):
        if n < dim:
            break
        n -= dim
        m += 1
    return y, m, n + 1


def date_text(days: int) -> str:
    """YYYY-MM-DD for years 0..9999, the plain decimal year outside."""
    y, m, d = civil_from_days(days)
    return ("%04d" % y if 0 <= y <= 9999 else str(y)) + "-%02d-%02d" % (m, d)


@functools.lru_cache(maxsize=None)
def date_format_cases():
    """[(date32 value, text)]: datetime.date inside years 1..9999 (its first,
    last and February/March days of every year, every day of FULL_YEARS), the
    integer calendar above outside."""
    out = []
    for y in range(1, 10000):
        for d in (datetime.date(y, 1, 1), datetime.date(y, 2, 28), datetime.date(y, 3, 1), datetime.date(y, 12, 31)):
            for dd in (d, d + datetime.timedelta(days=1) if d < datetime.date.max else d):
                out.append((dd.toordinal() - 719163, dd.isoformat()))
    for t, v in date_cases():
        if v is not None:
            out.append((v, t))
    first, last = datetime.date.min.toordinal() - 719163, datetime.date.max.toordinal() - 719163
    # the integer calendar agrees with datetime where both exist
    for v, t in out[::97]:
        assert date_text(v) == t
    rng = random.Random(4)
    outside = [first - 1, first - 365, first - 366, first - 367, first - 730, last + 1, last + 365, last + 366, last + 367,
               -(1 << 31), (1 << 31) - 1, first - 146097, first - 146097 - 1, last + 146097]
    outside += [rng.randint(-(1 << 31), first - 1) for _ in range(300)] + [rng.randint(last + 1, (1 << 31) - 1) for _ in range(300)]
    out += [(v, date_text(v)) for v in outside]
    return out


# ---- NDJSON ----------------------------------------------------------------

JSON_FIELDS = ("i", "f", "s", "t", "b")      # int64, float64, utf8, utf8, bool; all nullable


def _json_string(rng, s: str) -> str:
    """A JSON spelling of s: a mix of raw characters and every escape form."""
    simple = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t"}
    parts = []
    for ch in s:
        o = ord(ch)
        if ch in simple:
            parts.append(simple[ch])
        elif ch == "/" and rng.random() < 0.5:
            parts.append("\\/")
        elif o < 0x20:
            parts.append("\\u%04x" % o)
        elif o >= 0x10000 and rng.random() < 0.6:
            o -= 0x10000
            parts.append("\\u%04X\\u%04x" % (0xD800 + (o >> 10), 0xDC00 + (o & 0x3FF)))
        elif o < 0x10000 and rng.random() < 0.3:
            parts.append("\\u%04x" % o if rng.random() < 0.5 else "\\u%04X" % o)
        else:
            parts.append(ch)
    return '"' + "".join(parts) + '"'


def _json_text(rng, nbytes=None) -> str:
    alphabet = ["a", "Z", "0", " ", '"', "\\", "/", "\b", "\f", "\n", "\r", "\t", "\x01", "\x1f", "}", "{", "]", ",", ":",
                "\u00e9", "\u00df", "\u20ac", "\u6f22", "\u07ff", "\u0800", "\uffff", "\ud7ff", "\ue000",
                "\U0001f600", "\U00010000", "\U0010ffff"]
    if nbytes is None:
        return "".join(rng.choice(alphabet) for _ in range(rng.randrange(12)))
    s = ""
    while len(s.encode()) < nbytes:
        ch = rng.choice(alphabet)
        if len((s + ch).encode()) <= nbytes:
            s += ch
    return s


def json_records(n: int, seed: int):
    """n NDJSON lines over JSON_FIELDS and what json.loads makes of them:
    (lines, rows) with rows[r][field] the expected value (None: NULL)."""
    rng = random.Random(seed)
    floats = [t for t, v in float_cases() if v is not None and re.fullmatch(r"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?", t)]
    ints = [t for t, v in int_cases() if v is not None and re.fullmatch(r"-?(0|[1-9][0-9]*)", t)]
    sizes = [0, 1, 63, 64, 65]
    lines, rows = [], []
    for r in range(n):
        ws = (lambda: rng.choice(["", "", " ", "  ", "\t", " \t "])) if r % 3 else (lambda: "")
        members = []
        s_val = _json_text(rng, sizes[r % 5] if r % 2 == 0 else None)
        t_val = _json_text(rng)
        # escapes at the very start and end of a string
        if r % 7 == 0:
            t_val = "\n" + t_val + "\t"
        if r % 11 == 0:
            t_val = "€" + t_val + "😀"
        vals = {"i": rng.choice(ints), "f": rng.choice(floats), "s": _json_string(rng, s_val), "t": _json_string(rng, t_val),
                "b": rng.choice(["true", "false"])}
        if r % 13 == 0:
            vals["t"] = '"\\u20ac' + vals["t"][1:-1] + '\\ud83d\\ude00"'
        keys = list(JSON_FIELDS)
        rng.shuffle(keys)
        for k in keys:
            p = rng.random()
            if p < 0.08:
                continue                                            # absent
            if p < 0.16:
                members.append((k, "null"))
                continue
            if p < 0.22:                                            # duplicate key: the last one wins
                other = {"i": "17", "f": "0.5", "s": '"first"', "t": "null", "b": "true"}[k]
                members.append((k, other))
            members.append((k, vals[k]))
        # unknown keys with nested values to skip, '}' and ']' inside their strings
        for _ in range(rng.randrange(3)):
            junk = rng.choice(['{"a":"}","b":[1,{"c":"]}"}],"d":{}}', '["}", "]", "\\"}", {"k": "\\\\"}]', '"plain"', "12.5e3", "null",
                               '{"i": 1, "f": 2}', "[]", "{}", '"\\ud83d\\ude00}"'])
            members.insert(rng.randrange(len(members) + 1), ("x%d" % rng.randrange(3), junk))
        line = ws() + "{" + ",".join(ws() + json.dumps(k) + ws() + ":" + ws() + v + ws() for k, v in members) + "}" + ws()
        obj = json.loads(line)
        lines.append(line)
        row = {k: obj.get(k) for k in JSON_FIELDS}
        if isinstance(row["f"], int):            # an integer literal in the float column
            row["f"] = float(str(row["f"]))
        rows.append(row)
    return lines, rows


JSON_ERROR_LINES = {
    "lone high surrogate": '{"s":"a\\ud800b"}',
    "lone low surrogate": '{"s":"\\udc00"}',
    "surrogates in the wrong order": '{"s":"\\udc00\\ud800"}',
    "high surrogate then a BMP escape": '{"s":"\\ud83d\\u0041"}',
    "lone surrogate in a skipped value": '{"x":["\\ud800"],"s":"a"}',
    "truncated record": '{"i":1,"s":"abc',
    "truncated after a key": '{"i":1,"s"',
    "wrong type: string for an int": '{"i":"1"}',
    "wrong type: number for a bool": '{"b":1}',
    "wrong type: fraction for an int": '{"i":1.5}',
    "unknown escape": '{"s":"\\q"}',
    "escaped key": '{"\\u0069":1}',
}


# ---- digests ---------------------------------------------------------------

def digest_strings(max_len: int = 300, seed: int = 9):
    """One string of every UTF-8 byte length 0..max_len: a seeded mix of ASCII
    and 2-, 3- and 4-byte characters, cut at character boundaries."""
    rng = random.Random(seed)
    alphabet = "abcXYZ019 ~\x00\x7f" + "éßñ" + "€漢￿" + "😀\U0010ffff"
    out = []
    for n in range(max_len + 1):
        s = ""
        left = n
        while left:
            ch = rng.choice(alphabet)
            k = len(ch.encode())
            if k <= left:
                s += ch
                left -= k
        assert len(s.encode()) == n
        out.append(s)
    return out
