"""A Parquet file whose LIST column has the legacy 2-level form

    optional group l (LIST) { repeated int32 element; }

which pyarrow reads but cannot write. A 3-level list with a REQUIRED element

    optional group l (LIST) { repeated group list { required int32 element; } }

carries the same repetition / definition levels in its pages (the element adds
no level), so the file pyarrow writes is kept byte for byte and only its footer
is re-emitted with the middle group taken out: the schema loses that element,
the leaf becomes the repeated node, and the chunks' ``path_in_schema`` loses the
group's name. The footer goes through a small generic Thrift compact-protocol
reader / writer (values as (type, value) trees, nothing Parquet-specific).
"""
import struct

import pyarrow as pa
import pyarrow.parquet as pq

STOP, TRUE, FALSE, BYTE, I16, I32, I64, DOUBLE, BINARY, LIST, SET, MAP, STRUCT = range(13)


class _Reader:
    def __init__(self, buf):
        self.b, self.p = buf, 0

    def byte(self):
        self.p += 1
        return self.b[self.p - 1]

    def varint(self):
        v = sh = 0
        while True:
            c = self.byte()
            v |= (c & 0x7F) << sh
            if not c & 0x80:
                return v
            sh += 7

    def zigzag(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t):
        if t in (TRUE, FALSE):              # a bool inside a list / map: one byte
            return self.byte() == TRUE
        if t == BYTE:
            return self.byte()
        if t in (I16, I32, I64):
            return self.zigzag()
        if t == DOUBLE:
            self.p += 8
            return self.b[self.p - 8:self.p]
        if t == BINARY:
            n = self.varint()
            self.p += n
            return self.b[self.p - n:self.p]
        if t in (LIST, SET):
            h = self.byte()
            n, et = h >> 4, h & 15
            if n == 15:
                n = self.varint()
            return et, [self.value(et) for _ in range(n)]
        if t == MAP:
            n = self.varint()
            if n == 0:
                return 0, 0, []
            kv = self.byte()
            return kv >> 4, kv & 15, [(self.value(kv >> 4), self.value(kv & 15)) for _ in range(n)]
        assert t == STRUCT, t
        fields, last = [], 0
        while True:
            h = self.byte()
            if h == STOP:
                return fields
            ft, delta = h & 15, h >> 4
            fid = last + delta if delta else self.zigzag()
            last = fid
            fields.append([fid, ft, ft == TRUE if ft in (TRUE, FALSE) else self.value(ft)])


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zigzag(v):
    return _varint((v << 1) ^ (v >> 63))


def _write(t, v):
    if t in (TRUE, FALSE):
        return bytes([TRUE if v else FALSE])
    if t == BYTE:
        return bytes([v])
    if t in (I16, I32, I64):
        return _zigzag(v)
    if t == DOUBLE:
        return bytes(v)
    if t == BINARY:
        return _varint(len(v)) + bytes(v)
    if t in (LIST, SET):
        et, items = v
        head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + _varint(len(items))
        return head + b"".join(_write(et, x) for x in items)
    if t == MAP:
        kt, vt, items = v
        if not items:
            return b"\x00"
        return _varint(len(items)) + bytes([(kt << 4) | vt]) + b"".join(_write(kt, k) + _write(vt, x) for k, x in items)
    out, last = bytearray(), 0
    for fid, ft, fv in v:
        if ft in (TRUE, FALSE):
            ft = TRUE if fv else FALSE
        delta = fid - last
        out += bytes([(delta << 4) | ft]) if 0 < delta <= 15 else bytes([ft]) + _zigzag(fid)
        if ft not in (TRUE, FALSE):
            out += _write(ft, fv)
        last = fid
    return bytes(out) + b"\x00"


def _field(struct_fields, fid):
    return next(f for f in struct_fields if f[0] == fid)


def write_two_level_list(path, rows, **kw):
    """Write ``rows`` (lists of ints, None = NULL list; no NULL elements) as the column
    ``l`` in the legacy 2-level form. Returns the table pyarrow wrote."""
    at = pa.list_(pa.field("element", pa.int32(), nullable=False))
    t = pa.table([pa.array(rows, at)], schema=pa.schema([pa.field("l", at)]))
    pq.write_table(t, path, **kw)
    raw = open(path, "rb").read()
    assert raw[-4:] == b"PAR1"
    flen = struct.unpack("<I", raw[-8:-4])[0]
    meta = _Reader(raw[-8 - flen:-8]).value(STRUCT)
    assert _write(STRUCT, meta) == raw[-8 - flen:-8]        # the writer round-trips pyarrow's footer
    et, schema = _field(meta, 2)[2]                         # FileMetaData.schema
    root, top, mid, leaf = schema                           # root, l (LIST), repeated group, required leaf
    assert _field(mid, 3)[2] == 2 and _field(leaf, 3)[2] == 0 and _field(mid, 5)[2] == 1
    _field(leaf, 3)[2] = 2                                  # SchemaElement.repetition_type = REPEATED
    _field(meta, 2)[2] = (et, [root, top, leaf])
    for rg in _field(meta, 4)[2][1]:                        # row_groups[].columns[].meta_data.path_in_schema
        for chunk in _field(rg, 1)[2][1]:
            path_f = _field(_field(chunk, 3)[2], 3)
            st, names = path_f[2]
            assert len(names) == 3
            path_f[2] = (st, [names[0], names[2]])
    meta[:] = [f for f in meta if f[0] != 5]                # key_value_metadata: the stored Arrow schema
    footer = _write(STRUCT, meta)
    with open(path, "wb") as f:
        f.write(raw[:-8 - flen] + footer + struct.pack("<I", len(footer)) + b"PAR1")
    return t
