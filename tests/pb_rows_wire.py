"""Shared by the rows tests (not a test module): a numpy serializer of ragged
rows written from the wire rules alone, and the .proto / JSON that make the
project's own host serializer (native.json_proto_roundtrip) emit the same
batch."""
import base64
import json

import numpy as np

BYTES, FIXED32, FIXED64 = 7, 8, 9
# kind -> (numpy dtype of the source array, wire value of each element; None: the memory image)
KINDS = {
    0: ("int32", lambda a: a.astype("int64").view("uint64")),        # int32: sign-extended, 10 bytes if < 0
    1: ("uint32", lambda a: a.astype("uint64")),
    2: ("int32", lambda a: ((a.astype("int64") << 1) ^ (a.astype("int64") >> 63)).view("uint64") & 0xFFFFFFFF),
    3: ("int64", lambda a: a.view("uint64")),
    4: ("uint64", lambda a: a),
    5: ("int64", lambda a: ((a << 1) ^ (a >> 63)).view("uint64")),
    6: ("uint8", lambda a: (a != 0).astype("uint64")),               # any nonzero byte is true
    BYTES: ("uint8", None),
    FIXED32: ("float32", None),
    FIXED64: ("float64", None),
}
PROTO_TYPES = {0: "int32", 1: "uint32", 2: "sint32", 3: "int64", 4: "uint64", 5: "sint64", 6: "bool",
               FIXED32: "float", FIXED64: "double"}


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def varints(wire):
    """Vectorized protobuf varint encoding of a uint64 array."""
    wire = wire.astype(np.uint64)
    nbytes = np.ones(wire.shape, dtype=np.int64)
    for k in range(1, 10):
        nbytes += (wire >> np.uint64(7 * k)) > 0
    start = np.cumsum(nbytes) - nbytes
    out = np.zeros(int(nbytes.sum()), dtype=np.uint8)
    for k in range(10):
        m = nbytes > k
        byte = ((wire[m] >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8)
        byte |= np.where(nbytes[m] > k + 1, 0x80, 0).astype(np.uint8)
        out[start[m] + k] = byte
    return out.tobytes()


def values(kind, n, seed):
    """Every varint length 1..10 next to each other: small values, full-width
    ones, negative int32 (10 bytes), both signs under zigzag; bools and bytes
    are any byte; floats are multiples of 1/8 (exact as JSON text)."""
    rng = np.random.default_rng(seed)
    if kind in (6, BYTES):
        v = rng.integers(0, 256, n).astype(np.uint8)
        if kind == 6:
            v[::2] = 0
        return v
    if kind in (FIXED32, FIXED64):
        return (rng.integers(-2**20, 2**20, n) / 8.0).astype(KINDS[kind][0])
    if kind in (0, 2):
        v = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        v[::3] = rng.integers(-100, 100, len(v[::3]))
        return v
    if kind == 1:
        return rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 32, n).astype(np.uint32)
    if kind in (3, 5):
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) >> rng.integers(0, 63, n)
    return rng.integers(0, 2**64 - 1, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)


def reference(number, inner, kind, arr, ends):
    """The rows as the wire format says, row by row: tag, size of the
    sub-message, inner tag, payload size, payload. A row without elements of
    a packed kind is an empty sub-message; one of kind bytes keeps its (empty)
    inner field; inner 0 is a bare length-delimited element."""
    wire = KINDS[kind][1]
    tag, itag = varint((number << 3) | 2), varint((inner << 3) | 2)
    out, at = bytearray(), 0
    for end in ends:
        end = int(end)
        row = arr[at:end]
        p = varints(wire(row)) if wire else row.tobytes()
        if inner == 0:
            out += tag + varint(len(p)) + p
        elif end == at and kind != BYTES:
            out += tag + b"\x00"
        else:
            sub = itag + varint(len(p)) + p
            out += tag + varint(len(sub)) + sub
        at = end
    return bytes(out)


def proto_text(kind, number, inner):
    """A Batch whose field `number` is what one rows job builds."""
    if inner == 0:
        return 'syntax = "proto2";\nmessage Batch { repeated bytes rows = %d; }\n' % number
    field = "optional bytes v = %d" % inner if kind == BYTES else \
        "repeated %s v = %d [packed = true]" % (PROTO_TYPES[kind], inner)
    return 'syntax = "proto2";\nmessage Row { %s; }\nmessage Batch { repeated Row rows = %d; }\n' % (field, number)


def batch_json(kind, inner, arr, ends):
    """The JSON of the same batch (bytes as base64)."""
    rows, at = [], 0
    for end in ends:
        end = int(end)
        row = arr[at:end]
        at = end
        if kind == BYTES:
            text = base64.b64encode(row.tobytes()).decode()
            rows.append(text if inner == 0 else {"v": text})
        elif len(row) == 0:
            rows.append({})
        elif kind == 6:
            rows.append({"v": [bool(x) for x in row]})
        elif kind in (FIXED32, FIXED64):
            rows.append({"v": [float(x) for x in row]})
        else:
            rows.append({"v": [int(x) for x in row]})
    return json.dumps({"rows": rows}).encode()


def host_wire(native, tmp_path, kind, number, inner, arr, ends):
    """(wire bytes, JSON of the parsed-back message) from the project's host
    serializer, the type parsed from a .proto at run time."""
    name = "rows_%d_%d_%d.proto" % (kind, number, inner)
    (tmp_path / name).write_text(proto_text(kind, number, inner))
    _, wire, back = native.json_proto_roundtrip(str(tmp_path), name, "Batch", batch_json(kind, inner, arr, ends),
                                                base64_to_bytes=True)
    return wire, back, name
