"""Inputs and expectations for TRY_CAST, shared by tests/test_try_cast.py (CPU
engine), tests/test_try_cast_gpu.py (the gfx950 kernels of trycast.hip) and
tests/test_trycast_host.py (the same routines as host C++ under sanitizers).
A plain helper module like text_cases.py, whose accepted / rejected lists and
``expect_*`` oracles it reuses for int, decimal, float and date text.

Every expectation comes from Python ``int`` / ``Decimal`` / ``math`` /
``datetime`` alone; none of it shares code with the engine. ``None`` stands
for NULL. Comparisons made with these cases are exact.
"""
import datetime
import functools
import math
import random
import struct
from decimal import ROUND_HALF_EVEN, Decimal

import text_cases as C

INT_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64}
INT64_MIN, INT64_MAX = C.INT64_MIN, C.INT64_MAX


def int_range(kind):
    b = INT_BITS[kind]
    return -(1 << (b - 1)), (1 << (b - 1)) - 1


# ---- text -> integer at the target's own width -------------------------------

INT_EDGE_TEXTS = ["127", "128", "-128", "-129", "32767", "32768", "-32768", "-32769", "2147483647", "2147483648",
                  "-2147483648", "-2147483649", "9223372036854775807", "9223372036854775808", "-9223372036854775808",
                  "-9223372036854775809", "+127", "0128", "-0", "", " 1", "1 ", "12x"]


def expect_int_text(text, kind):
    v = C.expect_int(text)
    lo, hi = int_range(kind)
    return v if v is not None and lo <= v <= hi else None


@functools.lru_cache(maxsize=None)
def int_texts():
    return INT_EDGE_TEXTS + [t for t, _ in C.int_cases()]


# ---- text -> decimal(p, s) -----------------------------------------------------

DECIMAL_TYPES = ((5, 2), (18, 0), (18, 9), (18, 18), (38, 2))     # (precision, scale)
DECIMAL_EDGE_TEXTS = ["999.99", "-999.99", "1000.00", "-1000.00", "999.990", "999.995", "1000", "0.01", "0.001", "99999",
                      "100000", "999999999999999999", "1000000000000000000", "-999999999999999999", "0.999999999999999999",
                      "1.000000000000000000", "92233720368547758.07", "92233720368547758.08", "1e2", "", "."]


def expect_decimal_text(text, p, s):
    v = C.expect_decimal(text, s)
    if v is None or (p <= 18 and abs(v) >= 10 ** p):
        return None
    return v


@functools.lru_cache(maxsize=None)
def decimal_texts():
    return DECIMAL_EDGE_TEXTS + sorted({t for t, _, _ in C.decimal_cases()})


# ---- text -> bool ---------------------------------------------------------------

BOOL_TEXTS = [("true", True), ("TRUE", True), ("True", True), ("tRuE", True), ("t", True), ("T", True), ("1", True),
              ("false", False), ("FALSE", False), ("False", False), ("f", False), ("F", False), ("0", False),
              ("yes", None), ("no", None), ("", None), (" true", None), ("true ", None), ("tru", None), ("truee", None),
              ("01", None), ("2", None), ("y", None), ("on", None), ("fals", None), ("t1", None)]


# ---- text -> timestamp ------------------------------------------------------------

TS_REJECT = [
    "", " ", "2024", "2024-01", "2024-1-02", "24-01-02", "024-01-02", "2024/01/02", "20240102", "0000-01-01", "2024-00-10",
    "2024-13-01", "2023-02-29", "2024-02-30", "2024-04-31", "2024-01-00", "2024-01-32",
    " 2024-01-02", "2024-01-02 ", "x2024-01-02", "2024-01-02x", "2024-01-02 03:04:05 ", " 2024-01-02 03:04:05",
    "2024-01-02T", "2024-01-02 03", "2024-01-02T03", "2024-01-02 3:04", "2024-01-02 03:4", "2024-01-02 03:04:5",
    "2024-01-02 03:", "2024-01-02 03:04:", "2024-01-02 03:04:05.", "2024-01-02 03:04:05.1234567890",
    "2024-01-02 03:04.5", "2024-01-02  03:04", "2024-01-02_03:04", "2024-01-02t03:04:05x",
    "2024-01-02 24:00", "2024-01-02 23:60", "2024-01-02 23:59:60", "2024-01-02 23:59:61", "2024-01-02 99:00:00",
    "2024-01-02 03:04:05+", "2024-01-02 03:04:05+1", "2024-01-02 03:04:05+123", "2024-01-02 03:04:05+24",
    "2024-01-02 03:04:05+24:00", "2024-01-02 03:04:05+01:60", "2024-01-02 03:04:05+0160", "2024-01-02 03:04:05+01:0",
    "2024-01-02 03:04:05+01:000", "2024-01-02 03:04:05+01-00", "2024-01-02 03:04:05 +01:00", "2024-01-02 03:04:05ZZ",
    "2024-01-02 03:04:05Z ", "2024-01-02 03:04:05 Z", "2024-01-02 03:04:05UTC", "2024-01-02 03:04:05+01:00Z",
    "2024-01-02 03:04:05.12x", "2024-01-02 0३:04", "2024-01-02+1", "2024-01-02Zx", "2024-01-02 +01:00", "12:34:56", "03:04",
]
TS_HAND = [("0001-01-01", datetime.datetime(1, 1, 1)), ("9999-12-31 23:59:59.999999", datetime.datetime(9999, 12, 31, 23, 59, 59, 999999)),
           ("1970-01-01T00:00:00Z", datetime.datetime(1970, 1, 1)), ("1969-12-31 23:59:59.5", datetime.datetime(1969, 12, 31, 23, 59, 59, 500000)),
           ("2024-02-29t12:00", datetime.datetime(2024, 2, 29, 12)), ("2024-01-02 03:04:05.1234569", datetime.datetime(2024, 1, 2, 3, 4, 5, 123456)),
           ("2024-01-02 03:04:05.123456999", datetime.datetime(2024, 1, 2, 3, 4, 5, 123456)),
           ("2024-01-02 03:04:05.1", datetime.datetime(2024, 1, 2, 3, 4, 5, 100000)),
           ("2024-01-02+05:30", datetime.datetime(2024, 1, 1, 18, 30)), ("2024-01-02-05", datetime.datetime(2024, 1, 2, 5)),
           ("2024-01-02z", datetime.datetime(2024, 1, 2)), ("2024-01-02 03:04-0130", datetime.datetime(2024, 1, 2, 4, 34)),
           ("2024-01-02T03:04:05+23:59", datetime.datetime(2024, 1, 1, 3, 5, 5)),
           ("2024-12-31 23:30:00-01:00", datetime.datetime(2025, 1, 1, 0, 30))]
_EPOCH = datetime.datetime(1970, 1, 1)


def micros(dt: datetime.datetime) -> int:
    return (dt - _EPOCH) // datetime.timedelta(microseconds=1)


def print_timestamp(rng, dt: datetime.datetime, offsets=True):
    """`dt` (a naive UTC instant) in a randomly chosen accepted spelling; returns (text, the value that was
    printed). With an offset the wall time printed is dt + offset, so the instant is still dt."""
    off = 0
    form = rng.randrange(5)
    zone = rng.randrange(5) if offsets else 0
    if zone >= 2:
        off = rng.randrange(-(23 * 60 + 59), 23 * 60 + 60)
        lo, hi = datetime.datetime(1, 1, 2), datetime.datetime(9999, 12, 30)
        if not lo <= dt <= hi:
            off = 0
    wall = dt + datetime.timedelta(minutes=off)
    date = "%04d-%02d-%02d" % (wall.year, wall.month, wall.day)
    sep = rng.choice(["T", "t", " "])
    value = wall
    if form == 0:
        text, value = date, wall.replace(hour=0, minute=0, second=0, microsecond=0)
    elif form == 1:
        text, value = date + sep + "%02d:%02d" % (wall.hour, wall.minute), wall.replace(second=0, microsecond=0)
    elif form == 2:
        text, value = date + sep + "%02d:%02d:%02d" % (wall.hour, wall.minute, wall.second), wall.replace(microsecond=0)
    else:
        nd = rng.randint(1, 9)
        digits = ("%06d" % wall.microsecond + "".join(rng.choice("0123456789") for _ in range(3)))[:nd]
        value = wall.replace(microsecond=int(digits[:6].ljust(6, "0")))
        text = date + sep + "%02d:%02d:%02d.%s" % (wall.hour, wall.minute, wall.second, digits)
    if zone == 1:
        text += rng.choice("Zz")
    elif zone >= 2:
        sign = "-" if off < 0 else "+"
        h, m = divmod(abs(off), 60)
        text += sign + ("%02d" % h if m == 0 and zone == 2 else "%02d:%02d" % (h, m) if zone == 3 else "%02d%02d" % (h, m))
    return text, micros(value - datetime.timedelta(minutes=off))


@functools.lru_cache(maxsize=None)
def timestamp_cases(n=3000, seed=17, offsets=True):
    """[(text, microseconds or None)]: accepted texts printed from values, the hand list, the rejected list."""
    rng = random.Random(seed)
    out = [(t, micros(dt)) for t, dt in TS_HAND] if offsets else []
    span = (datetime.datetime(9999, 12, 31, 23, 59, 59) - datetime.datetime(1, 1, 1)).total_seconds()
    for _ in range(n):
        dt = datetime.datetime(1, 1, 1) + datetime.timedelta(seconds=rng.randrange(int(span)), microseconds=rng.randrange(10 ** 6))
        out.append(print_timestamp(rng, dt, offsets))
    out += [(t, None) for t in TS_REJECT]
    return out


# ---- mixed text columns: accepted texts interleaved with mutated ones ------------------

def mutate(rng, text, kind):
    """A text of `kind` made unreadable: a digit replaced by x, a trailing space, month 13."""
    k = rng.randrange(3)
    if k == 0 or not any(c.isdigit() for c in text):
        return text + " "
    if k == 1 and kind in ("date", "timestamp"):
        return text[:5] + "13" + text[7:]
    pos = [i for i, c in enumerate(text) if c.isdigit()]
    i = rng.choice(pos)
    return text[:i] + "x" + text[i + 1:]


def mixed_cases(kind, n, seed):
    """n (text, expected) pairs, every other text mutated; `kind`: int8 .. int64 / float / date /
    decimal<scale> (precision 18) / timestamp / bool. Expectations by the oracles above; a timestamp
    that was printed from a value expects that value, a mutated one NULL."""
    rng = random.Random(seed)
    if kind in INT_BITS:
        good = C.random_int_texts(n, seed)
        if kind != "int64":        # half of them inside the narrower range
            lo, hi = int_range(kind)
            good = [str(rng.randint(lo, hi)) if i % 4 < 2 else t for i, t in enumerate(good)]
        expect = lambda t: expect_int_text(t, kind)
    elif kind == "float":
        good, expect = C.random_float_texts(n, seed), C.expect_float
    elif kind == "date":
        good, expect = C.random_date_texts(n, seed), C.expect_date
    elif kind.startswith("decimal"):
        good, expect = C.random_decimal_texts(n, int(kind[7:]), seed), lambda t: expect_decimal_text(t, 18, int(kind[7:]))
    elif kind == "timestamp":
        printed = dict(c for c in timestamp_cases(n, seed) if c[1] is not None)
        good, expect = list(printed)[:n], printed.get
    else:
        good, expect = [rng.choice([t for t, v in BOOL_TEXTS if v is not None]) for _ in range(n)], expect_bool_text
    texts = [mutate(rng, t, kind) if i % 2 else t for i, t in enumerate(good)]
    return [(t, expect(t)) for t in texts]


def expect_bool_text(text):
    return {"true": True, "t": True, "1": True, "false": False, "f": False, "0": False}.get(
        "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in text))


def assert_quarters(expected, what):
    """At least a quarter of a mixed column is rejected and at least a quarter accepted, by the oracle alone."""
    n = len(expected)
    nulls = sum(v is None for v in expected)
    assert nulls * 4 >= n and (n - nulls) * 4 >= n, f"{what}: {nulls} of {n} rejected"


# ---- cast_checked: numeric edge inputs ----------------------------------------------------

def f64_next(x, up):
    return math.nextafter(x, math.inf if up else -math.inf)


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_next(x, up):
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    if x == 0:
        return struct.unpack("<f", struct.pack("<i", 1))[0] * (1 if up else -1)
    b += 1 if (x > 0) == up else -1
    return struct.unpack("<f", struct.pack("<i", b))[0]


POW2 = (7, 15, 31, 63)


def int_edges(bits):
    """Integers around +-2^7 / 2^15 / 2^31 / 2^63 that fit a `bits`-wide source."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = {0, 1, -1, lo, hi}
    for p in POW2:
        for d in (-2, -1, 0, 1, 2):
            vals |= {(1 << p) + d, -(1 << p) + d}
    return sorted(v for v in vals if lo <= v <= hi)


def float_edges(single=False):
    nxt, rnd = (f32_next, f32) if single else (f64_next, float)
    vals = [0.0, -0.0, 0.5, -0.5, -0.9, 0.9, 1.5, 2.5, -1.5, -2.5, 126.5, 127.5, -128.5, float("nan"), float("inf"), float("-inf"),
            2147483647.9, -2147483648.9, 2147483648.0, 1e10, -1e10, 1e19, -1e19, 1e30, 9.995, 999.995, 999.994, 0.005, 0.015,
            1.005, 123456789.125, 1e-320 if not single else 1e-40]
    for p in POW2:
        for b in (float(2 ** p), -float(2 ** p)):
            vals += [b, nxt(b, True), nxt(b, False), b - 1, b + 1, b - 0.5, b + 0.5]
    return [rnd(v) for v in vals]


def wide_edges():
    """int128 values whose high word is and is not the sign extension of the low word."""
    vals = set(int_edges(64))
    for p in (63, 64, 65, 100, 126):
        for d in (-1, 0, 1):
            vals |= {(1 << p) + d, -(1 << p) + d}
    vals |= {(1 << 127) - 1, -(1 << 127), 10 ** 38 - 1, -(10 ** 38) + 1, 10 ** 20 + 5, -(10 ** 20) - 5,
             99999500000000000000, 99999499999999999999, 5 * 10 ** 19, 5 * 10 ** 19 - 1}
    return sorted(vals)


def wide_words(v):
    lo = v & 0xFFFFFFFFFFFFFFFF
    hi = (v >> 64) & 0xFFFFFFFFFFFFFFFF
    s = lambda w: w - (1 << 64) if w >> 63 else w
    return s(lo), s(hi)


def decimal_edges(scale):
    """Unscaled int64 values of a DECIMAL(18, scale) source: rounding ties, precision edges, int64 edges."""
    vals = {0, 1, -1, 5, -5, 49, 50, -49, -50, 99999, 100000, -99999, -100000, 999995, 999994, -999995, 999985,
            INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, INT64_MAX // 10, INT64_MAX // 10 + 1, 10 ** 18, -(10 ** 18)}
    for k in (1, 2, 3, 9, 17, 18):
        vals |= {10 ** k, 10 ** k - 1, 10 ** k // 2, 10 ** k // 2 - 1, -(10 ** k // 2), -(10 ** k // 2) + 1, 127 * 10 ** k,
                 128 * 10 ** k - 1, 128 * 10 ** k}
    return sorted(v for v in vals if INT64_MIN <= v <= INT64_MAX)


def expect_convert(v, src, dst):
    """src / dst: ("int8".."int64",) | ("float32",) | ("float64",) | ("decimal", p, s) | ("wide", s).
    v: a Python int (unscaled for decimal / wide) or float. Returns the int result or None."""
    sk, dk = src[0], dst[0]
    s_scale = src[2] if sk == "decimal" else src[1] if sk == "wide" else 0
    if dk in INT_BITS:
        lo, hi = int_range(dk)
        if sk in ("float32", "float64"):
            if math.isnan(v) or math.isinf(v):
                return None
            r = math.trunc(v)
        else:
            r = abs(v) // 10 ** s_scale * (-1 if v < 0 else 1)         # toward zero
        return r if lo <= r <= hi else None
    p, s = dst[1], dst[2]
    if sk in ("float32", "float64"):
        if math.isnan(v) or math.isinf(v):
            return None
        if sk == "float32":
            prod = f32(v) * f32(float(10 ** s))       # exact in a double: 24 x 24 bits
            if abs(prod) > 3.4028235677973366e38:     # past the float32 range (and its rounding boundary)
                return None
            prod = f32(prod)                          # CAST multiplies in the source's precision
        else:
            prod = v * float(10 ** s)
        if math.isinf(prod):
            return None
        r = int(Decimal(prod).to_integral_value(rounding=ROUND_HALF_EVEN))
    else:
        up = s - s_scale
        if up >= 0:
            r = v * 10 ** up
        else:                                                          # half away from zero
            q, rem = divmod(abs(v), 10 ** -up)
            r = (q + (2 * rem >= 10 ** -up)) * (-1 if v < 0 else 1)
    if not INT64_MIN <= r <= INT64_MAX or (p <= 18 and abs(r) >= 10 ** p):
        return None
    return r


INT_SRCS = (("int8",), ("int16",), ("int32",), ("int64",))
INT_DSTS = INT_SRCS
DEC_DSTS = (("decimal", 5, 2), ("decimal", 18, 0), ("decimal", 18, 6), ("decimal", 38, 10), ("decimal", 3, 0))


@functools.lru_cache(maxsize=None)
def convert_cases():
    """[(src, dst, [values])] over every source kind and both target families."""
    out = []
    for src in INT_SRCS:
        vals = int_edges(INT_BITS[src[0]])
        for dst in INT_DSTS:
            if INT_BITS[dst[0]] < INT_BITS[src[0]]:
                out.append((src, dst, vals))
        out += [(src, dst, vals) for dst in DEC_DSTS]
    for src, vals in ((("float64",), float_edges()), (("float32",), float_edges(True))):
        out += [(src, dst, vals) for dst in INT_DSTS + DEC_DSTS]
    for s in (0, 2, 6, 18):
        src = ("decimal", 18, s)
        out += [(src, dst, decimal_edges(s)) for dst in INT_DSTS + DEC_DSTS]
    for s in (0, 2, 20, 38):
        src = ("wide", s)
        out += [(src, dst, wide_edges()) for dst in INT_DSTS + DEC_DSTS]
    return out


def random_convert_triples(n, seed):
    """n random (src, dst, value) triples: magnitudes spread over every bit length."""
    rng = random.Random(seed)
    srcs = [c[0] for c in convert_cases()]
    dsts = INT_DSTS + DEC_DSTS
    out = []
    for _ in range(n):
        src = rng.choice(srcs)
        dst = rng.choice(dsts)
        sk = src[0]
        if sk in ("float32", "float64"):
            v = rng.choice((-1, 1)) * rng.random() * 2.0 ** rng.randint(-4, 70)
            v = f32(v) if sk == "float32" else v
        else:
            bits = INT_BITS.get(sk, 128 if sk == "wide" else 64)
            v = rng.getrandbits(rng.randint(1, bits - 1)) * rng.choice((-1, 1))
        out.append((src, dst, v))
    return out
