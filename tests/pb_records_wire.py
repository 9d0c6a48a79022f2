"""Shared by the records tests (not a test module): a numpy serializer of
records (a repeated sub-message with several fields, each field a column)
written from the wire rules alone, and the .proto / JSON that make the
project's own host serializer (native.json_proto_roundtrip) emit the same
batch.

A column is a dict: inner, kind (pb_rows_wire.KINDS), arr (the numpy array of
all its elements) and ends (the row ends, or None for a scalar column: one
element per record)."""
import base64
import json

import numpy as np

import pb_rows_wire as W


def column(inner, kind, arr, ends=None):
    return dict(inner=inner, kind=kind, arr=arr, ends=None if ends is None else np.asarray(ends, dtype=np.uint32))


def _payload(col, lo, hi):
    wire = W.KINDS[col["kind"]][1]
    part = col["arr"][lo:hi]
    if wire is None:
        return part.tobytes()
    if col["kind"] == 6:  # one byte, 0 or 1
        return (part != 0).astype(np.uint8).tobytes()
    return W.varints(wire(part))


def record_fields(columns, r):
    """The fields of record r, in column order: a packed field without
    elements is omitted, a bytes field and a scalar one are always there."""
    sub = bytearray()
    for col in columns:
        inner, kind = col["inner"], col["kind"]
        if col["ends"] is None:
            wire_type = 0 if kind <= 6 else (5 if kind == W.FIXED32 else 1)
            sub += W.varint((inner << 3) | wire_type) + _payload(col, r, r + 1)
            continue
        lo, hi = (int(col["ends"][r - 1]) if r else 0), int(col["ends"][r])
        if hi == lo and kind != W.BYTES:
            continue
        p = _payload(col, lo, hi)
        sub += W.varint((inner << 3) | 2) + W.varint(len(p)) + p
    return bytes(sub)


def reference_records(number, columns, rows):
    """[the sub-message bytes of each record]."""
    return [record_fields(columns, r) for r in range(rows)]


def reference(number, columns, rows):
    tag = W.varint((number << 3) | 2)
    out = bytearray()
    for sub in reference_records(number, columns, rows):
        out += tag + W.varint(len(sub)) + sub
    return bytes(out)


def twin_columns(columns):
    """The columns as native.pb_serialize_records takes them."""
    return [(c["inner"], c["kind"], c["arr"].tobytes(), None if c["ends"] is None else [int(e) for e in c["ends"]])
            for c in columns]


def proto_text(number, columns, model_field=None):
    """A Batch whose field `number` is what the records job builds; field
    names are f<inner>. Columns must have distinct inner numbers."""
    fields = []
    for c in columns:
        inner, kind = c["inner"], c["kind"]
        if kind == W.BYTES:
            fields.append("optional bytes f%d = %d;" % (inner, inner))
        elif c["ends"] is None:
            fields.append("optional %s f%d = %d;" % (W.PROTO_TYPES[kind], inner, inner))
        else:
            fields.append("repeated %s f%d = %d [packed = true];" % (W.PROTO_TYPES[kind], inner, inner))
    model = "optional string model = %d; " % model_field if model_field else ""
    return 'syntax = "proto2";\nmessage Example { %s }\nmessage Batch { %srepeated Example examples = %d; }\n' % (
        " ".join(fields), model, number)


def _json_value(kind, x):
    if kind == 6:
        return bool(x)
    if kind in (W.FIXED32, W.FIXED64):
        return float(x)
    return int(x)


def batch_json(columns, rows, model=None):
    """The JSON of the same batch (bytes as base64)."""
    out = []
    for r in range(rows):
        rec = {}
        for c in columns:
            name, kind = "f%d" % c["inner"], c["kind"]
            if c["ends"] is None:
                rec[name] = _json_value(kind, c["arr"][r])
                continue
            lo, hi = (int(c["ends"][r - 1]) if r else 0), int(c["ends"][r])
            if kind == W.BYTES:
                rec[name] = base64.b64encode(c["arr"][lo:hi].tobytes()).decode()
            elif hi > lo:
                rec[name] = [_json_value(kind, x) for x in c["arr"][lo:hi]]
        out.append(rec)
    doc = {"examples": out}
    if model is not None:
        doc = {"model": model, "examples": out}
    return json.dumps(doc).encode()


def host_wire(native, tmp_path, number, columns, rows, name="records.proto"):
    """(wire bytes, JSON of the parsed-back message, proto file name) from the
    project's host serializer, the type parsed from a .proto at run time."""
    (tmp_path / name).write_text(proto_text(number, columns))
    _, wire, back = native.json_proto_roundtrip(str(tmp_path), name, "Batch", batch_json(columns, rows),
                                                base64_to_bytes=True)
    return wire, back, name
