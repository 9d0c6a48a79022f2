"""Shared by the records-split tests (not a test module): a pure-python
splitter of records written from the wire rules alone (the protobuf encoding,
and the rules of a taken field as the README's record splitter paragraph
states them), with the outputs and codes of pb::SplitRecords, and the messages
the host and the GPU tests both run.

A split column is (inner, kind, scalar). A case is a dict: number, cols, msg
and optionally row_cap, caps (one capacity per column) and what the test
expects of it (code, rows, others, absent, values)."""
import numpy as np

import pb_records_wire as RW
import pb_rows_split_ref as R
import pb_rows_wire as W

NONE = R.NONE
EB = {0: 4, 1: 4, 2: 4, 3: 8, 4: 8, 5: 8, 6: 1, W.BYTES: 1, W.FIXED32: 4, W.FIXED64: 8}
RAGGED_KINDS = tuple(range(10))
SCALAR_KINDS = (0, 1, 2, 3, 4, 5, 6, W.FIXED32, W.FIXED64)
INNERS = (1, 2, 3, 15, 16, 2047, 2048, 2**29 - 1)


def wire_type(kind, scalar):
    if not scalar:
        return 2
    return 0 if kind <= 6 else (5 if kind == W.FIXED32 else 1)


def _element(kind, x):
    """A varint's value as the element of the kind's vector layout."""
    if kind in (0, 1):
        return x & 0xFFFFFFFF
    if kind == 2:
        x &= 0xFFFFFFFF
        return ((x >> 1) ^ -(x & 1)) & 0xFFFFFFFF
    if kind == 5:
        return ((x >> 1) ^ -(x & 1)) & (2**64 - 1)
    if kind == 6:
        return 1 if x else 0
    return x


def _elements(kind, pay):
    """The elements of a ragged payload that passed the payload rule, or None
    when one of its varints is longer than ten bytes (or its tenth is above 1)."""
    if kind == W.BYTES:
        return list(pay)
    if kind in (W.FIXED32, W.FIXED64):
        w = EB[kind]
        return [int.from_bytes(pay[i:i + w], "little") for i in range(0, len(pay), w)]
    out, p = [], 0
    while p < len(pay):
        e = R._varint(pay, p, len(pay))
        if e is None:
            return None
        out.append(_element(kind, e[0]))
        p = e[1]
    return out


def _record(b, v, s, cols):
    """(code, {column: (offset, bytes)}) of the record whose value is b[v, v+s)."""
    end, p, code, taken = v + s, v, 0, {}
    while p < end:
        f = R.field(b, p, end)
        if f is None:
            return 1, taken
        tag, nxt, vo, vl = f
        c = next((i for i, col in enumerate(cols) if col[0] == tag >> 3), None)
        if c is None or tag & 7 != wire_type(cols[c][1], cols[c][2]) or c in taken:
            code = 6
        elif cols[c][2]:
            size = {0: nxt - R._varint(b, p, end)[1], 1: 8, 5: 4}[tag & 7]
            taken[c] = (nxt - size, size)
        else:
            kind = cols[c][1]
            if kind <= 6 and vl and b[vo + vl - 1] & 0x80:
                return 1, taken
            if kind > 6 and vl % EB[kind]:
                return 1, taken
            taken[c] = (vo, vl)
        p = nxt
    return code, taken


def _columns_ok(number, cols):
    if not (1 <= number < 2**29 and 1 <= len(cols) <= 8):
        return False
    for inner, kind, scalar in cols:
        if not (1 <= inner < 2**29 and 0 <= kind <= 9) or (scalar and kind == W.BYTES):
            return False
    return len({c[0] for c in cols}) == len(cols)


def split(number, cols, msg, row_cap=None, caps=None):
    """(err, rows, others, first_bad, [(count, absent, values bytes, row_ends
    list or None)]) as native.pb_split_records returns them."""
    b = bytes(msg)
    n = len(b)
    blank = [(0, 0, b"", None if c[2] else []) for c in cols]
    if not _columns_ok(number, cols) or n > 2**32 - 1:
        return 2, 0, 0, NONE, blank
    if row_cap is None:
        row_cap = n // 2
    if caps is None:
        caps = [row_cap if scalar else n // (EB[kind] if kind >= 8 else 1) for _, kind, scalar in cols]
    vals = [[] for _ in cols]
    ends = [[] for _ in cols]
    absent = [0] * len(cols)
    rows = others = p = 0
    while p < n:
        f = R.field(b, p, n)
        if f is None:
            return 1, 0, 0, p, blank
        tag, nxt, v, s = f
        if tag >> 3 != number:
            others += 1
        elif tag & 7 != 2:
            return 6, 0, 0, p, blank
        else:
            code, taken = _record(b, v, s, cols)
            elems = {}
            for c, (off, size) in taken.items():
                if code != 1 and not cols[c][2]:
                    elems[c] = _elements(cols[c][1], b[off:off + size])
                    if elems[c] is None:
                        code = 1
            if code:
                return code, 0, 0, p, blank
            for c, (_, kind, scalar) in enumerate(cols):
                if not scalar:
                    vals[c] += elems.get(c, [])
                    ends[c].append(len(vals[c]))
                elif c not in taken:
                    absent[c] += 1
                    vals[c].append(0)
                elif kind <= 6:
                    vals[c].append(_element(kind, R._varint(b, taken[c][0], taken[c][0] + taken[c][1])[0]))
                else:
                    vals[c].append(int.from_bytes(b[taken[c][0]:taken[c][0] + taken[c][1]], "little"))
            rows += 1
        p = nxt
    if rows > row_cap:
        return 5, rows, others, NONE, blank
    if any(len(v) > cap for v, cap in zip(vals, caps)):
        return 5, rows, others, NONE, [(len(v), a, b"", None if c[2] else []) for v, a, c in zip(vals, absent, cols)]
    return 0, rows, others, NONE, [
        (len(v), a, np.array(v, dtype=np.uint64).astype(R.ELEM[c[1]]).tobytes(), None if c[2] else e)
        for v, a, e, c in zip(vals, absent, ends, cols)]


# ---- the messages of the tests

tag = R.tag
bytes_field = R.bytes_field


def fld(inner, wire, payload):
    """One field of a record: wire 2 gets its length."""
    payload = bytes(payload)
    return tag(inner, wire) + (W.varint(len(payload)) if wire == 2 else b"") + payload


def rec(sub, number=4):
    return bytes_field(number, sub)


def make_columns(specs, rows, seed, per_row=6):
    """Wire columns (pb_records_wire.column) for specs [(kind, scalar)]: column
    c has inner INNERS[c]; a ragged one has 0 .. 2 * per_row elements per
    record, with records of none at the start, in the middle and at the end."""
    rng = np.random.default_rng(seed)
    out = []
    for c, (kind, scalar) in enumerate(specs):
        if scalar:
            out.append(RW.column(INNERS[c], kind, W.values(kind, rows, seed * 16 + c)))
            continue
        sizes = rng.integers(0, 2 * per_row + 1, rows)
        sizes[[0, rows // 2, rows - 1]] = 0
        out.append(RW.column(INNERS[c], kind, W.values(kind, int(sizes.sum()), seed * 16 + c), np.cumsum(sizes)))
    return out


def split_columns(columns):
    return [(c["inner"], c["kind"], c["ends"] is None) for c in columns]


def expected(columns):
    """[(values bytes, row_ends list or None)] a split gives back: bools 0 / 1."""
    return [(((c["arr"] != 0).astype(np.uint8) if c["kind"] == 6 else c["arr"]).tobytes(),
             None if c["ends"] is None else [int(e) for e in c["ends"]]) for c in columns]


def case(columns, rows, msg=None, number=4, **more):
    return dict(number=number, cols=split_columns(columns), msg=RW.reference(number, columns, rows) if msg is None else msg,
                rows=rows, values=expected(columns), **more)


EXAMPLE = [(3, False), (W.FIXED32, False), (0, True), (W.BYTES, False)]  # ids, weights, label, blob


def round_trip_sets():
    """Column sets of 1, 2, 4 and 8 columns in which every kind comes as a
    ragged and as a scalar column: (specs, rows, per_row) with messages of
    about three chunks of 4096 bytes."""
    pool = [(k, False) for k in RAGGED_KINDS] + [(k, True) for k in SCALAR_KINDS]
    # wire bytes of an element of pb_rows_wire.values(), about
    wire = {0: 7, 1: 2.5, 2: 3.5, 3: 7, 4: 4.3, 5: 4, 6: 1, W.BYTES: 1, W.FIXED32: 4, W.FIXED64: 8}
    out = []
    for ncols in (1, 2, 4, 8):
        for at in range(0, len(pool), ncols):
            specs = [pool[(at + c) % len(pool)] for c in range(ncols)]
            fixed = 2 + sum(1.5 + wire[k] for k, s in specs if s)  # a record's header and scalars
            ragged = sum(wire[k] for k, s in specs if not s)
            if not ragged:
                out.append((specs, int(12288 / fixed), 0))
            else:
                out.append((specs, 48, max(1, round((12288 / 48 - fixed) / ragged))))
    return out


def round_trip_cases():
    return [case(make_columns(specs, rows, 300 + i, per_row), rows) for i, (specs, rows, per_row) in
            enumerate(round_trip_sets())]


def seam_message():
    """Four columns, about three chunks: records, field headers and payloads
    straddle the chunk ends."""
    columns = make_columns(EXAMPLE, 48, 41, 18)
    return columns, RW.reference(4, columns, 48)


def seam_cases():
    """A foreign bytes field of every length 0..40 in front: every byte of a
    tag, a length, a field header and a payload's end falls on a chunk end."""
    columns, msg = seam_message()
    return [case(columns, 48, msg=bytes_field(9, b"\x22" * length) + msg, others=1) for length in range(41)]


def record_count_cases():
    return [case(make_columns(EXAMPLE, rows, 50 + rows, 1), rows) for rows in (255, 256, 257, 513)]


def element_count_cases():
    """2047, 2048 and 2049 elements in a varint, a fixed-width and a bytes
    column of the same job."""
    out = []
    for count in (2047, 2048, 2049):
        rows = 33
        columns = []
        for c, kind in enumerate((1, W.FIXED64, W.BYTES)):
            rng = np.random.default_rng(count + c)
            cuts = np.sort(rng.integers(0, count + 1, rows - 1))
            columns.append(RW.column(c + 1, kind, W.values(kind, count, count + c), np.append(cuts, count)))
        out.append(case(columns, rows))
    return out


def long_record_case():
    """One record longer than eight chunks: a blob of 40 KiB, so the skip
    table hops inside a record."""
    columns = make_columns(EXAMPLE, 9, 77, 3)
    sizes = np.array([3, 0, 5, 40 * 1024, 1, 0, 7, 2, 0])
    columns[3] = RW.column(INNERS[3], W.BYTES, W.values(W.BYTES, int(sizes.sum()), 78), np.cumsum(sizes))
    return case(columns, 9)


def skip_cases():
    """The jobs of the count, element and long-record tests and three of the
    seam ones, for every span of the serial hops."""
    seams = seam_cases()
    return record_count_cases() + element_count_cases() + [long_record_case(), seams[0], seams[17], seams[40]]


def _with_records(columns, rows, subs, between=None, number=4):
    out = bytearray()
    for r, sub in enumerate(subs):
        if between:
            out += between[r % len(between)]
        out += rec(sub, number)
    return bytes(out)


def shape_cases():
    """Fields reversed; a packed, a bytes and a scalar column absent from every
    other record; an empty record; foreign top-level fields between records."""
    rows = 40
    columns = make_columns(EXAMPLE, rows, 91, 5)
    out = []
    # reversed: the last column's field first
    subs = [RW.record_fields(columns[::-1], r) for r in range(rows)]
    out.append(case(columns, rows, msg=_with_records(columns, rows, subs)))
    # column `gone` absent from the odd records: an empty row, or a scalar that reads as 0
    for gone in range(4):
        subs = [RW.record_fields([c for i, c in enumerate(columns) if i != gone or r % 2 == 0], r) for r in range(rows)]
        want = []
        for i, c in enumerate(columns):
            if i != gone:
                want.append(c)
            elif c["ends"] is None:
                arr = c["arr"].copy()
                arr[1::2] = 0
                want.append(RW.column(c["inner"], c["kind"], arr))
            else:
                ends = np.concatenate([[0], c["ends"]]).astype(np.int64)
                sizes = np.diff(ends)
                keep = np.concatenate([c["arr"][ends[r]:ends[r + 1]] for r in range(0, rows, 2)])
                sizes[1::2] = 0
                want.append(RW.column(c["inner"], c["kind"], keep, np.cumsum(sizes)))
        absent = [rows // 2 if i == gone and c["ends"] is None else 0 for i, c in enumerate(columns)]
        out.append(dict(case(want, rows, msg=_with_records(columns, rows, subs)), absent=absent))
    # empty records: every column absent
    subs = [RW.record_fields(columns, r) if r % 3 else b"" for r in range(rows)]
    blank = []
    for c in columns:
        if c["ends"] is None:
            arr = c["arr"].copy()
            arr[0::3] = 0
            blank.append(RW.column(c["inner"], c["kind"], arr))
        else:
            ends = np.concatenate([[0], c["ends"]]).astype(np.int64)
            sizes = np.diff(ends)
            keep = [c["arr"][ends[r]:ends[r + 1]] for r in range(rows) if r % 3]
            sizes[0::3] = 0
            blank.append(RW.column(c["inner"], c["kind"], np.concatenate(keep), np.cumsum(sizes)))
    out.append(dict(case(blank, rows, msg=_with_records(columns, rows, subs)),
                    absent=[0, 0, len(range(0, rows, 3)), 0]))
    # foreign top-level fields of wire types 0, 1, 2 and 5 between the records
    foreign = [tag(1, 0) + W.varint(300), tag(9, 1) + b"\x01" * 8, bytes_field(3, b"model-7"), tag(2000, 5) + b"\xff" * 4,
               bytes_field(7, b"\x22\x00" * 40)]
    subs = [RW.record_fields(columns, r) for r in range(rows)]
    out.append(case(columns, rows, msg=_with_records(columns, rows, subs, between=foreign) + foreign[0], others=rows + 1))
    return out


def wire_like_case():
    """A blob whose bytes are themselves serialized records of the same number."""
    inner_columns = make_columns(EXAMPLE, 30, 5, 4)
    blob = np.frombuffer(RW.reference(4, inner_columns, 30), dtype=np.uint8)
    rows = 3
    columns = make_columns(EXAMPLE, rows, 6, 4)
    columns[3] = RW.column(INNERS[3], W.BYTES, np.concatenate([blob, blob[:100], blob]),
                           [blob.size, blob.size + 100, 2 * blob.size + 100])
    return case(columns, rows)


EXAMPLE_COLS = [(1, 3, False), (2, W.FIXED32, False), (3, 0, True), (15, W.BYTES, False)]


def good_example(seed=7, rows=6):
    columns = make_columns(EXAMPLE, rows, seed, 3)
    return RW.reference(4, columns, rows)


def code_cases():
    """Messages of the EXAMPLE columns that give codes 1 and 6, with the
    offset each names. Where two offenders exist, the lowest wins."""
    good = good_example()
    g = len(good)
    long_elem = b"\x05" + b"\x80" * 10 + b"\x01"
    one = {
        "a fixed payload that is not whole elements": rec(fld(2, 2, b"\x01" * 5)),
        "a varint payload that ends in a continuation bit": rec(fld(1, 2, b"\x01\x81")),
        "an 11-byte varint in a taken payload": rec(fld(1, 2, long_elem)),
        "a tenth byte above 1 in a taken payload": rec(fld(1, 2, b"\xff" * 9 + b"\x02")),
        "both 6 and 1: an unknown field, then an 11-byte element": rec(fld(9, 0, b"\x07") + fld(1, 2, long_elem)),
        "both 6 and 1: an 11-byte element, then a column twice": rec(fld(1, 2, long_elem) + fld(1, 2, b"\x01")),
        "both 6 and 1: an unknown field, then no wire": rec(fld(9, 0, b"\x07") + tag(9, 3)),
        "a field that leaves the record": rec(fld(3, 0, b"\x07") + tag(1, 2) + b"\x05\x01"),
        "a scalar of eleven bytes": rec(tag(3, 0) + b"\x80" * 10 + b"\x01"),
    }
    six = {
        "an unknown field": rec(fld(1, 2, b"\x07") + fld(9, 0, b"\x07")),
        "a column twice": rec(fld(1, 2, b"\x07") + fld(1, 2, b"\x08")),
        "a scalar twice": rec(fld(3, 0, b"\x07") + fld(3, 0, b"\x08")),
        "a packed field where a scalar is expected": rec(fld(3, 2, b"\x01\x02")),
        "an unpacked element where a packed field is expected": rec(fld(1, 0, b"\x07")),
        "a fixed32 where the varint scalar is expected": rec(fld(3, 5, b"\x01\x02\x03\x04")),
        "`number` with wire type 0": tag(4, 0) + b"\x07",
    }
    out = []
    for code, group in ((1, one), (6, six)):
        for what, bad in group.items():
            out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good + bad + good, code=code, first_bad=g, what=what))
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good[:-1], code=1, what="a truncated message"))
    bad1, bad6 = one["an 11-byte varint in a taken payload"], six["an unknown field"]
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good + bad6 + good + bad1, code=6, first_bad=g, what="6 below 1"))
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good + bad1 + good + bad6, code=1, first_bad=g, what="1 below 6"))
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good + bad6 + good + b"\x0b", code=6, first_bad=g,
                    what="6 below a top-level field that is no wire"))
    # an 11-byte element a few chunks behind an unsupported record
    far = good_example(8, 700)
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=good + bad6 + far + bad1, code=6, first_bad=g, what="6 far below 1"))
    out.append(dict(number=4, cols=EXAMPLE_COLS, msg=far + bad1 + far + bad6, code=1, first_bad=len(far),
                    what="1 far below 6"))
    return out


def capacity_cases():
    """The seam message with every capacity exact, each column's cap short by
    one, and row_cap short by one (every count is then 0)."""
    columns, msg = seam_message()
    rows = 48
    exact = [rows if c["ends"] is None else c["arr"].size for c in columns]
    out = [dict(case(columns, rows, msg=msg, row_cap=rows, caps=list(exact)), code=0, counts=exact)]
    for c in range(len(columns)):
        caps = list(exact)
        caps[c] -= 1
        out.append(dict(number=4, cols=split_columns(columns), msg=msg, row_cap=rows, caps=caps, code=5, rows=rows,
                        counts=exact))
    out.append(dict(number=4, cols=split_columns(columns), msg=msg, row_cap=rows - 1, caps=list(exact), code=5, rows=rows,
                    counts=[0] * len(columns)))
    # an 11-byte element in a record beyond row_cap still wins over 5
    bad = rec(fld(1, 2, b"\x05" + b"\x80" * 10 + b"\x01"))
    out.append(dict(number=4, cols=split_columns(columns), msg=msg + bad, row_cap=3, caps=list(exact), code=1,
                    first_bad=len(msg)))
    return out


def refused_cases():
    """Jobs the twin refuses (code 2): (number, cols)."""
    good = EXAMPLE_COLS
    return [(0, good), (2**29, good), (4, [(0, 3, False)]), (4, [(2**29, 3, False)]), (4, [(1, 10, False)]),
            (4, [(1, W.BYTES, True)]), (4, []), (4, [(i + 1, 0, True) for i in range(9)]),
            (4, [(1, 3, False), (2, 0, True), (1, W.FIXED32, False)]), (4, [(3, 0, True), (3, 0, False)])]


def all_cases():
    """Every message the GPU file splits, for the host comparison."""
    return (round_trip_cases() + seam_cases() + record_count_cases() + element_count_cases() + [long_record_case()] +
            shape_cases() + [wire_like_case()] + code_cases() + capacity_cases())
