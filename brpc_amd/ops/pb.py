"""Batched protobuf wire scan on the GPU (``gpu/pb_kernels.hip``): decode the
top-level fields of many small serialized messages (RpcMeta-sized) packed in
one device buffer, one lane per message, one launch."""
import torch

from ..native import native
from ._common import require_gpu_tensor, stream_handle

WIRE_VARINT, WIRE_FIXED64, WIRE_LEN, WIRE_FIXED32 = 0, 1, 2, 5
ERRORS = {-1: "truncated or malformed", -2: "too many fields", -3: "field number 0", -4: "unsupported wire type",
          -5: "offsets outside the buffer or descending"}


def pb_scan(buf, offsets, max_fields=16):
    """buf: uint8 device tensor; offsets: int64 device tensor of n+1 message
    boundaries. Returns (fields, nfields): fields is an int64 (n, max_fields,
    2) tensor of [tag, value] rows (tag = field << 3 | wire; value = varint,
    fixed bits, or offset << 32 | length for wire 2, offset relative to the
    message), nfields an int32 (n,) tensor of field counts (negative = error,
    see ERRORS)."""
    require_gpu_tensor(buf, "buf")
    require_gpu_tensor(offsets, "offsets")
    if buf.dtype != torch.uint8 or offsets.dtype != torch.int64:
        raise TypeError("buf must be uint8 and offsets int64")
    if offsets.device != buf.device:
        raise ValueError("offsets must live on the same device as buf (%s vs %s)" % (offsets.device, buf.device))
    if not buf.is_contiguous() or not offsets.is_contiguous():
        raise ValueError("buf and offsets must be contiguous")
    n = offsets.numel() - 1
    dev = buf.device
    fields = torch.zeros((max(n, 1), max_fields, 2), dtype=torch.int64, device=dev)
    nfields = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    if n > 0:
        with torch.cuda.device(dev):
            # the kernel bounds every message by buf.numel() (code -5)
            native.gpu.pb_scan_launch(buf.data_ptr(), buf.numel(), offsets.data_ptr(), n, int(max_fields),
                                      fields.data_ptr(), nfields.data_ptr(), stream_handle(dev))
    return fields[:n], nfields[:n]


# kind_name -> (PbRunKind / kDeviceFieldBytes, tensor dtypes whose memory is the kind's vector layout)
_KINDS = {
    "int32": (0, (torch.int32,)),
    "uint32": (1, (torch.int32, getattr(torch, "uint32", torch.int32))),
    "sint32": (2, (torch.int32,)),
    "int64": (3, (torch.int64,)),
    "uint64": (4, (torch.int64, getattr(torch, "uint64", torch.int64))),
    "sint64": (5, (torch.int64,)),
    "bool": (6, (torch.bool, torch.uint8)),
    "bytes": (7, None),
}
BUILD_ERRORS = {2: "refused (field number, kind, alignment or size)", 3: "longer than the destination",
                4: "a source tensor changed while the message was built"}


def pb_build_message(fields):
    """Serialize device tensors into one protobuf message in device memory
    (``gpu::DeviceBuildMessages``): the values never leave HBM, the host
    learns only lengths.

    fields: [(number, tensor, kind_name)] in wire order, kind_name one of
    int32, uint32, sint32, int64, uint64, sint64, bool (a packed repeated
    field of the tensor's elements; the unsigned kinds take the signed tensor
    of the same width, its bits read as unsigned) or bytes (a length-delimited
    field holding the tensor's memory image: bytes / string, and packed
    float / double / fixed32 / fixed64). An empty packed field is omitted, as
    the host serializer does; an empty bytes field is emitted.

    Returns (message, positions): a uint8 device tensor trimmed to the
    message's length, and [(offset, length)] of every field's payload in it.

    The codec batch runs on its own stream, not on torch's: the caller's
    current stream is synchronized before the call, so tensors produced by
    kernels queued just before are complete when the builder reads them, and
    the message is complete when this returns."""
    if not fields:
        raise ValueError("no fields")
    dev = fields[0][1].device
    rows, keep = [], []
    for number, t, kind_name in fields:
        if kind_name not in _KINDS:
            raise ValueError("unknown kind %r (one of %s)" % (kind_name, ", ".join(_KINDS)))
        kind, dtypes = _KINDS[kind_name]
        require_gpu_tensor(t, "field %d" % number)
        if t.device != dev:
            raise ValueError("all fields must live on one device (%s vs %s)" % (t.device, dev))
        if dtypes is not None and t.dtype not in dtypes:
            raise TypeError("field %d: kind %s takes a tensor of %s, not %s" % (number, kind_name, dtypes[0], t.dtype))
        t = t.contiguous()
        keep.append(t)
        count = t.numel() * t.element_size() if kind == 7 else t.numel()
        rows.append((int(number), kind, t.data_ptr() if count else 0, count))
    cap = native.gpu.device_message_worst_case(rows)
    if cap == 0 and any(r[3] or r[1] == 7 for r in rows):
        raise ValueError("fields refused: " + BUILD_ERRORS[2])
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        n, err, pos = native.gpu.device_build_message(rows, out.data_ptr(), cap, dev.index or 0)
    if err:
        raise ValueError("pb_build_message: " + BUILD_ERRORS.get(err, "code %d" % err))
    return out[:n], [tuple(p) for p in pos]


# the kinds of pb_build_rows: those above plus the fixed widths (8: 4-byte
# elements, 9: 8-byte elements)
_ROW_KINDS = dict(_KINDS)
_ROW_KINDS.update({
    "float32": (8, (torch.float32,)),
    "fixed32": (8, (torch.int32, getattr(torch, "uint32", torch.int32))),
    "float64": (9, (torch.float64,)),
    "fixed64": (9, (torch.int64, getattr(torch, "uint64", torch.int64))),
})
ROWS_ERRORS = dict(BUILD_ERRORS)
ROWS_ERRORS[1] = "row_ends decreases or does not end at the number of values"
ROWS_ERRORS[2] = "refused (field number, inner, kind, alignment, rows or size)"


def pb_build_rows(number, values, row_ends, kind_name, inner=None):
    """Serialize a ragged batch in device memory as the occurrences of one
    repeated field (``gpu::DeviceBuildRows``): row r holds the elements
    ``values[row_ends[r-1]:row_ends[r]]`` (equal neighbours: an empty row).

    With ``inner`` each row is a sub-message whose packed field ``inner``
    holds the row (``repeated Row rows = number`` with ``message Row
    {repeated T v = inner [packed = true];}``); without it (kind bytes only)
    each row is one ``repeated bytes`` / ``repeated string`` element.
    kind_name: a kind of ``pb_build_message``, or float32, float64, fixed32,
    fixed64. row_ends: an int32 or uint32 device tensor, or the int64 one
    ``json_parse_float_rows(..., ragged=True)`` returns next to values. A
    2-D values tensor with ``row_ends=None`` means equal rows.

    Returns a uint8 device tensor trimmed to the serialized length: a valid
    message by itself, and (protobuf concatenation being merge) a part of a
    larger one when concatenated with a ``pb_build_message`` result.

    The builder runs on its own stream: the caller's current stream is
    synchronized before the call, as in ``pb_build_message``."""
    if kind_name not in _ROW_KINDS:
        raise ValueError("unknown kind %r (one of %s)" % (kind_name, ", ".join(_ROW_KINDS)))
    kind, dtypes = _ROW_KINDS[kind_name]
    require_gpu_tensor(values, "values")
    dev = values.device
    if dtypes is not None and values.dtype not in dtypes:
        raise TypeError("kind %s takes a tensor of %s, not %s" % (kind_name, dtypes[0], values.dtype))
    if row_ends is None:
        if values.dim() != 2:
            raise ValueError("row_ends=None needs a 2-D values tensor (equal rows)")
        per = values.shape[1] * (values.element_size() if kind == 7 else 1)
        row_ends = torch.arange(per, per * values.shape[0] + 1, max(per, 1), dtype=torch.int32, device=dev) \
            if per else torch.zeros(values.shape[0], dtype=torch.int32, device=dev)
    require_gpu_tensor(row_ends, "row_ends")
    if row_ends.device != dev:
        raise ValueError("row_ends must live on the same device as values (%s vs %s)" % (row_ends.device, dev))
    if row_ends.dtype == torch.int64:
        # what json_parse_float_rows(ragged=True) returns: narrowed on the device
        row_ends = row_ends.to(torch.int32)
    if row_ends.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or row_ends.dim() != 1:
        raise TypeError("row_ends must be a 1-D int32, uint32 or int64 tensor, not %s" % row_ends.dtype)
    values = values.contiguous()
    row_ends = row_ends.contiguous()
    count = values.numel() * values.element_size() if kind == 7 else values.numel()
    rows = row_ends.numel()
    inner = int(inner or 0)
    cap = native.gpu.device_rows_worst_case(int(number), inner, kind, count, rows)
    if cap == 0:
        raise ValueError("pb_build_rows: " + ROWS_ERRORS[2])
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (n, err, first_bad), = native.gpu.device_build_rows(
            [(int(number), inner, kind, values.data_ptr() if count else 0, count, row_ends.data_ptr(), rows,
              out.data_ptr(), cap)], dev.index or 0)
    if err == 1:
        raise ValueError("pb_build_rows: %s (row %d)" % (ROWS_ERRORS[1], first_bad))
    if err:
        raise ValueError("pb_build_rows: " + ROWS_ERRORS.get(err, "code %d" % err))
    return out[:n]


RECORDS_ERRORS = dict(ROWS_ERRORS)
RECORDS_ERRORS[2] = "refused (field number, inner, kind, columns, a scalar column's length, alignment, rows or size)"


def pb_build_records(number, columns, scalar=False):
    """Serialize a batch of records in device memory as the occurrences of one
    repeated sub-message with several fields (``gpu::DeviceBuildRecords``):
    ``repeated Example examples = number``, every field of ``Example`` one
    column.

    columns: [(inner, values, row_ends_or_None, kind_name)], written into
    every record in this order (at most 8). A column takes the tensor and
    dtype rules of ``pb_build_rows``. With ``row_ends`` it is ragged: a packed
    field ``inner`` (omitted in a record without elements) or, for kind bytes,
    a bytes / string field (always present); an int64 ``row_ends`` is narrowed
    on the device. With ``row_ends=None`` a 1-D tensor is a scalar column: one
    element per record, written with explicit presence (a zero stays); a 2-D
    tensor means equal rows of a ragged column, unless ``scalar=True`` flattens
    it into a scalar column.

    Returns a uint8 device tensor trimmed to the serialized length, which
    composes with a ``pb_build_message`` result by concatenation.

    The builder runs on its own stream: the caller's current stream is
    synchronized before the call, as in ``pb_build_message``."""
    if not columns:
        raise ValueError("no columns")
    dev = columns[0][1].device
    rows, cols, keep = None, [], []
    for c, (inner, values, row_ends, kind_name) in enumerate(columns):
        if kind_name not in _ROW_KINDS:
            raise ValueError("column %d: unknown kind %r (one of %s)" % (c, kind_name, ", ".join(_ROW_KINDS)))
        kind, dtypes = _ROW_KINDS[kind_name]
        require_gpu_tensor(values, "column %d" % c)
        if values.device != dev:
            raise ValueError("all columns must live on one device (%s vs %s)" % (values.device, dev))
        if dtypes is not None and values.dtype not in dtypes:
            raise TypeError("column %d: kind %s takes a tensor of %s, not %s" % (c, kind_name, dtypes[0], values.dtype))
        if row_ends is None and values.dim() == 2 and not scalar:
            per = values.shape[1] * (values.element_size() if kind == 7 else 1)
            row_ends = torch.arange(per, per * values.shape[0] + 1, max(per, 1), dtype=torch.int32, device=dev) \
                if per else torch.zeros(values.shape[0], dtype=torch.int32, device=dev)
        values = values.contiguous()
        count = values.numel() * values.element_size() if kind == 7 else values.numel()
        ends_ptr, nrows = 0, count
        if row_ends is not None:
            require_gpu_tensor(row_ends, "column %d row_ends" % c)
            if row_ends.device != dev:
                raise ValueError("column %d: row_ends must live on the same device as values" % c)
            if row_ends.dtype == torch.int64:
                row_ends = row_ends.to(torch.int32)
            if row_ends.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or row_ends.dim() != 1:
                raise TypeError("column %d: row_ends must be a 1-D int32, uint32 or int64 tensor, not %s"
                                % (c, row_ends.dtype))
            row_ends = row_ends.contiguous()
            if row_ends.numel() == 0:
                raise ValueError("column %d: row_ends is empty" % c)
            ends_ptr, nrows = row_ends.data_ptr(), row_ends.numel()
            keep.append(row_ends)
        elif kind == 7:
            raise ValueError("column %d: a bytes column needs row_ends" % c)
        if rows is None:
            rows = nrows
        elif nrows != rows:
            raise ValueError("column %d holds %d records, the columns before it %d" % (c, nrows, rows))
        keep.append(values)
        cols.append((int(inner), kind, values.data_ptr() if count else 0, count, ends_ptr))
    cap = native.gpu.device_records_worst_case(int(number), cols, rows)
    if cap == 0:
        raise ValueError("pb_build_records: " + RECORDS_ERRORS[2])
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (n, err, first_bad, bad_column), = native.gpu.device_build_records(
            [(int(number), cols, rows, out.data_ptr(), cap)], dev.index or 0)
    if err == 1:
        raise ValueError("pb_build_records: %s (row %d, column %d)" % (RECORDS_ERRORS[1], first_bad, bad_column))
    if err:
        raise ValueError("pb_build_records: " + RECORDS_ERRORS.get(err, "code %d" % err))
    return out[:n]


SPLIT_ERRORS = {
    1: "malformed wire",
    2: "refused (field number, inner, kind or size)",
    5: "more elements or rows than max_elems / max_rows",
    6: "well-formed, but a row is not one packed field (or the field is no sub-message): use the host parser",
}


def pb_split_rows(message, number, kind_name, inner=None, max_elems=None, max_rows=None):
    """The inverse of ``pb_build_rows`` (``gpu::DeviceSplitRows``): every
    occurrence of field ``number`` in ``message`` (a uint8 device tensor) is a
    row; other top-level fields are skipped, so a whole ``Batch { string
    model = 1; repeated Row rows = 4; }`` splits as it is.

    Returns ``(values, row_ends)``, both trimmed: values holds the elements
    of all rows in the dtype of the kind (the first one ``pb_build_rows``
    takes for it; uint8 for bytes), row_ends is int32 with ``row_ends[r]`` the
    elements in rows 0..r. ``pb_build_rows(number, values, row_ends, ...)``
    gives a canonical message of rows alone back byte for byte.

    max_elems / max_rows size the outputs; without them they hold what any
    message of this size can: ``n // wire-minimum`` elements, ``n // 2`` rows.
    The splitter runs on its own stream: the caller's current stream is
    synchronized first, as in ``pb_build_rows``."""
    if kind_name not in _ROW_KINDS:
        raise ValueError("unknown kind %r (one of %s)" % (kind_name, ", ".join(_ROW_KINDS)))
    kind, dtypes = _ROW_KINDS[kind_name]
    dtype = dtypes[0] if dtypes else torch.uint8
    require_gpu_tensor(message, "message")
    if message.dtype != torch.uint8 or message.dim() != 1:
        raise TypeError("message must be a 1-D uint8 tensor")
    message = message.contiguous()
    dev = message.device
    n = message.numel()
    if n > native.gpu.device_split_max_bytes():
        raise ValueError("pb_split_rows: a message of %d bytes is above device_split_max_bytes()" % n)
    eb = torch.empty(0, dtype=dtype).element_size()
    cap = n // (eb if kind >= 8 else 1) if max_elems is None else int(max_elems)
    row_cap = n // 2 if max_rows is None else int(max_rows)
    values = torch.empty(max(cap, 1), dtype=dtype, device=dev)
    row_ends = torch.empty(max(row_cap, 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (count, rows, _, err, first_bad), = native.gpu.device_split_rows(
            [(int(number), int(inner or 0), kind, message.data_ptr() if n else 0, n, values.data_ptr(), cap,
              row_ends.data_ptr(), row_cap)], dev.index or 0)
    if err in (1, 6):
        raise ValueError("pb_split_rows: %s (offset %d)" % (SPLIT_ERRORS[err], first_bad))
    if err == 5:
        raise ValueError("pb_split_rows: %s (%d elements, %d rows)" % (SPLIT_ERRORS[5], count, rows))
    if err:
        raise ValueError("pb_split_rows: " + SPLIT_ERRORS.get(err, "code %d" % err))
    return values[:count], row_ends[:rows]


RECORDS_SPLIT_ERRORS = dict(SPLIT_ERRORS)
RECORDS_SPLIT_ERRORS[2] = "refused (field number, columns, a duplicate inner, a scalar bytes column or size)"
RECORDS_SPLIT_ERRORS[5] = "more records or elements than max_rows / max_elems"
RECORDS_SPLIT_ERRORS[6] = ("well-formed, but a record holds a field that is no column (or a column twice, or "
                           "unpacked): use the host parser")


def pb_split_records(message, number, columns, max_rows=None, max_elems=None):
    """The inverse of ``pb_build_records`` (``gpu::DeviceSplitRecords``):
    every occurrence of field ``number`` in ``message`` (a uint8 device
    tensor) is a record; other top-level fields are skipped.

    columns: [(inner, kind_name, scalar)] with distinct ``inner`` numbers (at
    most 8). A record's fields may come in any order. A ragged column absent
    from a record is a row of no element; a scalar absent from one reads as 0.

    Returns ``[(values, row_ends_or_None)]`` per column, trimmed, in the
    dtypes ``pb_split_rows`` uses: a ragged column's values and its int32
    ``row_ends``, a scalar column's one element per record and None.
    ``pb_build_records(number, ...)`` of the result gives canonical builder
    output back byte for byte.

    max_rows sizes every ``row_ends`` and the scalar columns, max_elems (one
    number, or one per column) the ragged values; without them they hold what
    any message of this size can (``n // 2`` records; the device keeps a table
    of 8 bytes per record and column, which for a message of several MB with
    many columns no longer fits one arena block: such a call is refused and
    needs ``max_rows``). The splitter runs on its own stream: the
    caller's current stream is synchronized first, as in ``pb_split_rows``."""
    if not columns:
        raise ValueError("no columns")
    require_gpu_tensor(message, "message")
    if message.dtype != torch.uint8 or message.dim() != 1:
        raise TypeError("message must be a 1-D uint8 tensor")
    message = message.contiguous()
    dev = message.device
    n = message.numel()
    if n > native.gpu.device_split_max_bytes():
        raise ValueError("pb_split_records: a message of %d bytes is above device_split_max_bytes()" % n)
    row_cap = n // 2 if max_rows is None else int(max_rows)
    if max_elems is not None and not isinstance(max_elems, (list, tuple)):
        max_elems = [max_elems] * len(columns)
    if max_elems is not None and len(max_elems) != len(columns):
        raise ValueError("max_elems must hold one capacity per column")
    outs, table = [], []
    for c, (inner, kind_name, scalar) in enumerate(columns):
        if kind_name not in _ROW_KINDS:
            raise ValueError("column %d: unknown kind %r (one of %s)" % (c, kind_name, ", ".join(_ROW_KINDS)))
        kind, dtypes = _ROW_KINDS[kind_name]
        dtype = dtypes[0] if dtypes else torch.uint8
        eb = torch.empty(0, dtype=dtype).element_size()
        if scalar:
            cap = row_cap
        else:
            cap = n // (eb if kind >= 8 else 1) if max_elems is None else int(max_elems[c])
        values = torch.empty(max(cap, 1), dtype=dtype, device=dev)
        row_ends = None if scalar else torch.empty(max(row_cap, 1), dtype=torch.int32, device=dev)
        outs.append((values, row_ends))
        table.append((int(inner), kind, bool(scalar), values.data_ptr(), cap,
                      0 if scalar else row_ends.data_ptr()))
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (rows, _, err, first_bad, counts), = native.gpu.device_split_records(
            [(int(number), table, message.data_ptr() if n else 0, n, row_cap)], dev.index or 0)
    if err in (1, 6):
        raise ValueError("pb_split_records: %s (offset %d)" % (RECORDS_SPLIT_ERRORS[err], first_bad))
    if err == 5:
        raise ValueError("pb_split_records: %s (%d records, elements per column: %s)"
                         % (RECORDS_SPLIT_ERRORS[5], rows, ", ".join(str(c[0]) for c in counts)))
    if err:
        raise ValueError("pb_split_records: " + RECORDS_SPLIT_ERRORS.get(err, "code %d" % err))
    return [(values[:count], None if row_ends is None else row_ends[:rows])
            for (values, row_ends), (count, _) in zip(outs, counts)]


def pb_scan_host(msg, max_fields=16):
    """Pure-python reference of one message's scan (tests)."""
    out, p = [], 0

    def varint():
        nonlocal p
        v, shift = 0, 0
        while True:
            if p >= len(msg) or shift >= 70:
                raise ValueError("truncated")
            c = msg[p]
            p += 1
            v |= (c & 0x7F) << shift
            if not c & 0x80:
                return v
            shift += 7

    while p < len(msg):
        tag = varint()
        field, wire = tag >> 3, tag & 7
        if field == 0:
            return out, -3
        if wire == 0:
            val = varint()
        elif wire in (1, 5):
            nb = 8 if wire == 1 else 4
            if len(msg) - p < nb:
                return out, -1
            val = int.from_bytes(msg[p:p + nb], "little")
            p += nb
        elif wire == 2:
            ln = varint()
            if ln > len(msg) - p:
                return out, -1
            val = (p << 32) | ln
            p += ln
        else:
            return out, -4
        if len(out) >= max_fields:
            return out, -2
        out.append((tag, val))
    return out, len(out)
