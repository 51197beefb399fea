"""Shared inputs and plain-Python oracles of the BINARY tests
(test_binary.py on the CPU engine, test_binary_gpu.py on the device,
test_binary_host.py for the stand-alone sanitizer program).

The oracles are Python's own: binascii, base64, hashlib, strict
``bytes.decode``. base64 is the standard alphabet without padding on output
(parity unpinned: the reference has no fixture); input may be unpadded or
correctly padded.
"""
import base64
import binascii
import hashlib
import random

#: every residue mod 3 and mod 4, both blake2 block sizes (64 / 128) +- 1
LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
ROW_COUNTS = [1, 255, 256, 257, 1000]          # kBlock is 256
EDGE = [b"", b"\x00", b"a", b"a\x00", b"a\x00\x00"]
#: ORDER BY must give exactly this (byte-wise, shorter prefix first)
TRAILING_ZERO_ORDER = [b"", b"\x00", b"a", b"a\x00", b"a\x00\x00", b"b"]


def byte_string(n: int, seed: int = 0) -> bytes:
    return random.Random(1000 * seed + n).randbytes(n)


def base_values():
    """One value per length, all 256 byte values, the edge values."""
    return [byte_string(n) for n in LENGTHS] + [bytes(range(256))] + EDGE


def rows(n: int, nulls: bool = True):
    """n rows cycling through base_values() (every 7th NULL when ``nulls``)."""
    base = base_values()
    if n < len(base):
        # few rows: the short and the edge values (the long ones have rows of their own elsewhere)
        base = EDGE[::-1] + base
    out = [base[i % len(base)] if i < len(base) else byte_string(i % 70, seed=i) for i in range(n)]
    if nulls:
        out = [None if i % 7 == 3 else v for i, v in enumerate(out)]
    return out


def alignment_rows():
    """Row starts hit every alignment mod 8 (lengths 1 x 8), then longer rows from each of them."""
    out = [bytes([65 + i]) for i in range(8)]
    for i in range(8):
        out += [byte_string(9 + i, seed=77), byte_string(24, seed=78 + i)]
    return out


def sliced_array(pa, values, typ=None, lead=3):
    """An Arrow array whose offsets do not start at 0: ``values`` behind ``lead`` rows that are sliced off."""
    arr = pa.array([b"skipped-%d" % i for i in range(lead)] + list(values), typ or pa.binary())
    return arr.slice(lead)


# ------------------------------------------------------------------ oracles
def hex_of(v: bytes) -> str:
    return binascii.hexlify(v).decode("ascii")


def b64_of(v: bytes) -> str:
    return base64.b64encode(v).rstrip(b"=").decode("ascii")


_ALPHABET = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")


def b64_strict(v: bytes):
    """The decode contract, independent of the engine's twin: bytes, or None when v must be rejected."""
    pad = 2 if v.endswith(b"==") else 1 if v.endswith(b"=") else 0
    body = v[:len(v) - pad]
    if pad and len(v) % 4:
        return None
    if len(body) % 4 == 1 or any(c not in _ALPHABET for c in body):
        return None
    out = base64.b64decode(body + b"=" * (-len(body) % 4))
    return out if base64.b64encode(out).rstrip(b"=") == body else None


def utf8_ok(v: bytes) -> bool:
    try:
        v.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def blake2(v: bytes, algo: str) -> str:
    return hashlib.new(algo, v).hexdigest()


# ------------------------------------------------------------ invalid inputs
HEX_INVALID = [b"0", b"abc", b"0g", b"zz", b" 0a", b"0a ", b"0x0a", b"\xff\xff", b"0a0b0c0d0e0f0g0a", b"0A0B0"]
HEX_VALID = [b"", b"0a", b"0A", b"fF", b"00112233445566778899aAbBcCdDeEfF"]
B64_INVALID = [
    b"Q",            # length 1 (mod 4)
    b"QUJDR",        # length 1 (mod 4)
    b"QQ!A", b"QQ A", b"QQ-_", b"QQ\n", b"\xff\xff",      # outside the alphabet
    b"Q=QQ", b"=QQQ", b"QQ=Q", b"QUJD=QUI",               # '=' anywhere but the end
    b"QQ=", b"QQQ==", b"Q===", b"QUJD=", b"QUJD==", b"=", b"==",     # more padding than the length allows
    b"QR", b"QUJ", b"QR==", b"QUJ=",                      # non-zero trailing bits
]
B64_VALID = [b"", b"QQ", b"QQ==", b"QUI", b"QUI=", b"QUJD", b"+/+/", b"AAAA", b"QUJDRA", b"QUJDRA=="]
UTF8_INVALID = [
    b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",   # overlong
    b"\xed\xa0\x80", b"\xed\xbf\xbf",                     # surrogates
    b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\xfe",     # above U+10FFFF
    b"\x80", b"\xbf", b"a\x80b", b"\xc3\xa9\xa9",         # stray continuation bytes
    b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"abc\xc3", b"\xc3a", b"\xe2\x82a",     # truncated
]
UTF8_VALID = [b"", b"abc", "é".encode(), "€".encode(), "\U0001F600".encode(), b"\xf4\x8f\xbf\xbf", b"\xed\x9f\xbf",
              b"\xee\x80\x80", b"\xe0\xa0\x80", b"\xf0\x90\x80\x80", b"\xc2\x80", b"\x7f", ("aé" * 40).encode()]
#: a sequence split across a row boundary is invalid in both rows
UTF8_SPLIT = [b"\xc3", b"\xa9"]


def placements(bad: bytes, good: bytes):
    """(rows, first bad row | None): the bad value first, last in a block of
    256, as the only row, and under a NULL (which must not raise). The rows
    under NULLs travel as (value, False) pairs: see ``with_nulls``."""
    return [
        ([bad] + [good] * 300, 0),
        ([good] * 255 + [bad] + [good] * 44, 255),
        ([bad], 0),
        ([good, (bad, False), good], None),
        ([(bad, False)], None),
    ]


def with_nulls(pa, rows_, typ):
    """An Arrow array of ``typ`` in which a (value, False) row is NULL but keeps the value's bytes underneath."""
    vals = [r[0] if isinstance(r, tuple) else r for r in rows_]
    ok = [not isinstance(r, tuple) and r is not None for r in rows_]
    arr = pa.array([v if v is not None else b"" for v in vals], typ)
    if all(ok):
        return arr
    import numpy as np
    validity = pa.array(np.array(ok), pa.bool_()).buffers()[1]
    bufs = arr.buffers()
    return pa.Array.from_buffers(typ, len(arr), [validity, bufs[1], bufs[2]], null_count=ok.count(False))
