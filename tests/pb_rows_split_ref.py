"""Shared by the rows-split tests (not a test module): a pure-python splitter
written from the wire rules alone (the protobuf encoding, and what the issue
of the splitter calls a row), with the outputs and codes of pb::SplitRows, and
the messages the host and the GPU tests both run."""
import numpy as np

import pb_rows_wire as W

NONE = 2**64 - 1
ELEM = {0: "<u4", 1: "<u4", 2: "<u4", 3: "<u8", 4: "<u8", 5: "<u8", 6: "u1", W.BYTES: "u1",
        W.FIXED32: "<u4", W.FIXED64: "<u8"}


def _varint(b, p, end):
    """(value, next offset) or None: at most ten bytes, the tenth at most 1."""
    v = 0
    for i in range(10):
        if p + i >= end:
            return None
        c = b[p + i]
        v |= (c & 0x7F) << (7 * i)
        if not c & 0x80:
            return (v, p + i + 1) if i < 9 or c <= 1 else None
    return None


def field(b, p, end):
    """(tag, next, value offset, value length) of the field at p, or None."""
    t = _varint(b, p, end)
    if t is None or t[0] > 0xFFFFFFFF or t[0] >> 3 == 0:
        return None
    tag, q = t
    wire = tag & 7
    if wire == 0:
        v = _varint(b, q, end)
        return None if v is None else (tag, v[1], 0, 0)
    if wire in (1, 5):
        size = 8 if wire == 1 else 4
        return None if end - q < size else (tag, q + size, 0, 0)
    if wire == 2:
        v = _varint(b, q, end)
        if v is None or v[0] > 0xFFFFFFFF or v[0] > end - v[1]:
            return None
        return tag, v[1] + v[0], v[1], v[0]
    return None


def _row(b, v, s, inner, kind):
    """(code, elements as a list of ints or bytes) of one row's value."""
    po, pl = v, s
    if inner != 0 and s > 0:
        f = field(b, v, v + s)
        if f is None:
            return 1, None
        if f[0] != (inner << 3 | 2) or f[1] != v + s:
            p = f[1]
            while p < v + s:
                g = field(b, p, v + s)
                if g is None:
                    return 1, None
                p = g[1]
            return 6, None
        po, pl = f[2], f[3]
    pay = bytes(b[po:po + pl])
    if kind == W.BYTES:
        return 0, list(pay)
    if kind in (W.FIXED32, W.FIXED64):
        w = 4 if kind == W.FIXED32 else 8
        if pl % w:
            return 1, None
        return 0, [int.from_bytes(pay[i:i + w], "little") for i in range(0, pl, w)]
    if pl and pay[-1] & 0x80:
        return 1, None
    out, p = [], 0
    while p < pl:
        e = _varint(pay, p, pl)
        if e is None:
            return 1, None
        x, p = e
        if kind in (0, 1):
            x &= 0xFFFFFFFF
        elif kind == 2:
            x &= 0xFFFFFFFF
            x = ((x >> 1) ^ -(x & 1)) & 0xFFFFFFFF
        elif kind == 5:
            x = ((x >> 1) ^ -(x & 1)) & (2**64 - 1)
        elif kind == 6:
            x = 1 if x else 0
        out.append(x)
    return 0, out


def split(number, inner, kind, msg, cap=None, row_cap=None):
    """(err, count, rows, others, first_bad, values bytes, row_ends list) as
    native.pb_split_rows returns them."""
    b = bytes(msg)
    n = len(b)
    if not (1 <= number < 2**29 and 0 <= inner < 2**29 and 0 <= kind <= 9 and (inner or kind == W.BYTES)):
        return 2, 0, 0, 0, NONE, b"", []
    if cap is None:
        cap = n // (1 if kind <= W.BYTES else (4 if kind == W.FIXED32 else 8))
    if row_cap is None:
        row_cap = n // 2
    vals, ends, others, p = [], [], 0, 0
    while p < n:
        f = field(b, p, n)
        if f is None:
            return 1, 0, 0, 0, p, b"", []
        tag, nxt, v, s = f
        if tag >> 3 != number:
            others += 1
        elif tag & 7 != 2:
            return 6, 0, 0, 0, p, b"", []
        else:
            code, elems = _row(b, v, s, inner, kind)
            if code:
                return code, 0, 0, 0, p, b"", []
            vals += elems
            ends.append(len(vals))
        p = nxt
    if len(vals) > cap or len(ends) > row_cap:
        return 5, len(vals), len(ends), others, NONE, b"", []
    return 0, len(vals), len(ends), others, NONE, np.array(vals, dtype=np.uint64).astype(ELEM[kind]).tobytes(), ends


# ---- the messages of the tests

ALL = [(k, 2) for k in sorted(W.KINDS)] + [(W.BYTES, 0)]
NUMBERS = (1, 15, 16, 2047, 2048, 2**29 - 1)
# empty rows at the start and the end, 300 of them in a run, one row over
# three 4 KiB chunks for every kind (5000 elements), 4100 one-element rows
BOUNDARY_ENDS = np.concatenate([[0, 0, 0, 2047, 2048], np.full(300, 2048), [2049, 7049],
                                7049 + 1 + np.arange(4100), np.full(3, 7049 + 4100)]).astype(np.uint32)


def tag(number, wire):
    return W.varint(number << 3 | wire)


def bytes_field(number, payload):
    return tag(number, 2) + W.varint(len(payload)) + bytes(payload)


def long_varint(v, nbytes):
    """v in exactly nbytes bytes (over-long)."""
    out = bytearray()
    for _ in range(nbytes - 1):
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v & 0x7F)
    return bytes(out)


def boundary_message(kind, inner, number=4, seed=None):
    arr = W.values(kind, int(BOUNDARY_ENDS[-1]), 100 + kind if seed is None else seed)
    return W.reference(number, inner, kind, arr, BOUNDARY_ENDS), arr


def small_message(kind, inner, number=4, sizes=(3, 0, 70, 1, 0, 129), seed=7):
    arr = W.values(kind, sum(sizes), seed)
    return W.reference(number, inner, kind, arr, np.cumsum(sizes)), arr


def wire_like_cases():
    """Payload that looks like wire: (kind, inner, message)."""
    inner_msg, _ = small_message(1, 2, number=4, sizes=(5, 0, 9))
    out = []
    for payload in (inner_msg + b"\x00" * (-len(inner_msg) % 4), b"\x0a\x01" * 3000, b"\xff" * 5000):
        arr = np.frombuffer(payload, dtype=np.uint8)
        ends = [len(payload) // 2, len(payload)]
        out.append((W.BYTES, 0, W.reference(4, 0, W.BYTES, arr, ends)))
        out.append((W.BYTES, 3, W.reference(4, 3, W.BYTES, arr, ends)))
        f = np.frombuffer(payload[:len(payload) // 4 * 4], dtype=np.float32)
        out.append((W.FIXED32, 2, W.reference(4, 2, W.FIXED32, f, [f.size // 3, f.size])))
    return out


def foreign_cases():
    """Foreign fields of wire types 0, 1, 2 and 5 before, between and after
    the rows: (kind, inner, message, others)."""
    foreign = [tag(1, 0) + W.varint(300), tag(9, 1) + b"\x01" * 8, bytes_field(3, b"model-7"), tag(2000, 5) + b"\xff" * 4,
               bytes_field(7, b"\x22\x00" * 40), tag(5, 0) + b"\x00"]
    out = []
    for kind, inner in ((1, 2), (W.FIXED64, 2), (W.BYTES, 0)):
        arr = W.values(kind, 700, 31)
        rows = [W.reference(4, inner, kind, arr[a:b], [b - a]) for a, b in ((0, 3), (3, 3), (3, 600), (600, 700))]
        msg = foreign[0] + foreign[1] + rows[0] + foreign[2] + rows[1] + rows[2] + foreign[3] + foreign[4] + rows[3] + \
            foreign[5]
        out.append((kind, inner, msg, 6))
    return out


def noncanonical_cases():
    """Over-long varints in a row length, an inner length and a foreign
    field's value: (kind, inner, message)."""
    pay = W.varints(np.array([1, 300, 70000], dtype=np.uint64))
    sub = tag(2, 2) + long_varint(len(pay), 3) + pay
    row_a = tag(4, 2) + long_varint(len(sub), 5) + sub
    sub_b = tag(2, 2) + W.varint(len(pay)) + pay
    row_b = tag(4, 2) + long_varint(len(sub_b), 10) + sub_b
    return [(1, 2, row_a + tag(6, 0) + long_varint(5, 10) + row_b + tag(4, 2) + long_varint(0, 2))]


def cut_cases():
    """The boundary message of kind 1 cut at each of its last 24 lengths:
    code 1 with the offset of the field that is cut, or a shorter whole
    message where the cut falls between two rows."""
    base, _ = boundary_message(1, 2)
    return [(1, 2, base[:len(base) - k]) for k in range(1, 25)]


def malformed_cases():
    """(kind, inner, message) that give code 1."""
    out = []
    good, _ = small_message(1, 2)
    fgood, _ = small_message(W.FIXED32, 2)
    for wire in (3, 4, 6, 7):
        out.append((1, 2, good + tag(9, wire) + good))
    out.append((1, 2, good + b"\x02\x00" + good))                                  # field number 0
    out.append((1, 2, good + tag(4, 2) + W.varint(50) + b"\x12\x01\x05"))          # a length past the end
    out.append((1, 2, good + tag(9, 0) + b"\x80" * 10 + b"\x00" + good))           # an 11-byte varint
    out.append((1, 2, good + tag(9, 0) + b"\xff" * 9 + b"\x02" + good))            # a tenth byte above 1
    out.append((W.FIXED32, 2, fgood + tag(4, 2) + b"\x07\x12\x05" + b"\x01" * 5 + fgood))  # 5 bytes of floats
    out.append((W.FIXED64, 2, tag(4, 2) + b"\x0e\x12\x0c" + b"\x01" * 12))
    out.append((1, 2, good + tag(4, 2) + b"\x04\x12\x02\x01\x81" + good))          # payload ends inside a varint
    out.append((3, 2, good + tag(4, 2) + b"\x0e\x12\x0c\x05" + b"\x80" * 10 + b"\x01" + good))  # 11-byte element
    out.append((3, 2, tag(4, 2) + b"\x0d\x12\x0b\x05" + b"\xff" * 9 + b"\x02"))    # element's tenth byte above 1
    out.append((1, 2, good + tag(4, 2) + b"\x03\x12\x05\x01" + good))              # the inner length leaves the row
    # two offenders: the lower one wins
    out.append((1, 2, good + tag(9, 3) + good + b"\x02\x00"))
    out.append((1, 2, good + tag(4, 2) + b"\x04\x12\x02\x01\x81" + good + tag(9, 7)))
    return out


def unsupported_cases():
    """(kind, inner, message, code): code 6 unless a malformed field lies lower."""
    good, _ = small_message(1, 2)
    two = tag(4, 2) + b"\x05\x12\x01\x07\x18\x01"                    # a second field in the row
    unpacked = tag(4, 2) + b"\x02\x10\x07"                           # the inner field with wire 0
    twice = tag(4, 2) + b"\x06\x12\x01\x07\x12\x01\x08"              # the packed field in two occurrences
    other = tag(4, 2) + b"\x03\x1a\x01\x07"                          # another field in its place
    scalar = tag(4, 0) + b"\x07"                                     # `number` with wire 0
    bad = tag(9, 3)
    out = [(1, 2, good + x + good, 6) for x in (two, unpacked, twice, other, scalar)]
    out.append((1, 2, good + two + good + bad, 6))
    out.append((1, 2, good + bad + good + two, 1))
    out.append((1, 2, good + tag(4, 2) + b"\x05\x12\x01\x07\x1b\x01" + good, 1))  # the second field is no wire
    return out
