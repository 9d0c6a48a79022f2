"""JSON structural index on the GPU: the stage-1 tokenizer pass of
http+json bodies (the reference parses them on the CPU through rapidjson,
src/json2pb/json_to_pb.cpp). Returns the byte offsets of every unescaped
quote and of every ``{ } [ ] : ,`` outside strings, in order."""
import re

import torch

from ..native import native
from ._common import require_gpu_tensor, stream_handle

_STRUCTURAL = frozenset(b"{}[]:,")


def json_index(buf, max_positions=None):
    """uint8 device tensor of JSON text -> int64 device tensor of positions.

    Raises ValueError when a string is left open at the end of the input."""
    require_gpu_tensor(buf, "buf")
    if buf.dtype != torch.uint8:
        raise TypeError("buf must be uint8")
    n = buf.numel()
    if n >= 1 << 32:
        raise ValueError("json_index handles inputs below 4 GiB")
    dev = buf.device
    cap = n if max_positions is None else int(max_positions)
    out = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int64, device=dev)  # [count, err]
    scratch = torch.empty(native.gpu.json_index_scratch_bytes(max(n, 1)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        native.gpu.json_index_launch(buf.data_ptr(), n, out.data_ptr(), cap, meta.data_ptr(), meta.data_ptr() + 8,
                                     scratch.data_ptr(), stream_handle(dev))
    count, err = meta.tolist()
    err &= 0xFFFFFFFF
    if err & 1:
        raise ValueError("unterminated JSON string")
    if err & 2:
        raise ValueError("more than %d structural positions (found %d)" % (cap, count))
    return out[:count].to(torch.int64)


def json_index_host(data):
    """Pure-python reference of json_index (for tests): (positions, open).

    Like the kernel, a backslash escapes the next byte wherever it stands
    (outside strings it is invalid JSON either way)."""
    out, in_str, esc = [], False, False
    for i, c in enumerate(bytes(data)):
        escaped, esc = esc, (c == 0x5C and not esc)
        if c == 0x22 and not escaped:
            in_str = not in_str
            out.append(i)
        elif not in_str and c in _STRUCTURAL:
            out.append(i)
    return out, in_str


_FLOAT_KINDS = {torch.float32: 8, torch.float64: 9}
PRINT_ERRORS = {2: "refused (bad arguments)", 3: "longer than the output buffer", 4: "the source changed while printing"}


def json_print_floats(values):
    """float32 / float64 device tensor -> uint8 device tensor of JSON text
    ``v,v,...,v`` (no brackets), every element exactly as the host's pb2json
    prints a double: the shortest digits that convert back, ``2.0`` /
    ``123.45`` / ``0.000123`` / ``1.5e-7`` layouts, ``"NaN"`` / ``"Infinity"``
    / ``"-Infinity"`` quoted; a float32 is widened first (0.1f prints as
    0.10000000149011612). The values never leave HBM
    (``gpu::DevicePrintFloatArrays``).

    The printer runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the text is complete when
    this returns."""
    require_gpu_tensor(values, "values")
    if values.dtype not in _FLOAT_KINDS:
        raise TypeError("values must be float32 or float64, not %s" % values.dtype)
    dev = values.device
    t = values.contiguous().view(-1)
    n = t.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    cap = native.gpu.json_float_worst_case(n)
    if cap >= 1 << 32:
        raise ValueError("json_print_floats handles outputs below 4 GiB")
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err), = native.gpu.device_json_print_floats([t.data_ptr()], [n], [_FLOAT_KINDS[t.dtype]],
                                                            [out.data_ptr()], [cap], dev.index or 0)
    if err:
        raise ValueError("json_print_floats: " + PRINT_ERRORS.get(err, "code %d" % err))
    return out[:length]


_PARSE_MODES = {torch.float64: 1, torch.float32: 2}
_INT_RANGES = {torch.int32: (-(1 << 31), (1 << 31) - 1), torch.int64: (-(1 << 63), (1 << 63) - 1)}
_REDO_CAP = 64


def _redo_text(t, offset):
    """The number in the piece of `t` that starts at byte `offset`: fetched
    in windows that double until the piece's comma (or the end) is in one."""
    n, size = t.numel(), 256
    while True:
        piece = bytes(t[offset:offset + size].cpu().numpy())
        cut = piece.find(b",")
        if cut >= 0 or offset + size >= n:
            return (piece if cut < 0 else piece[:cut]).strip(b" \t\n\r[]")
        size *= 2


def _parse_number_text(name, text, dtype, max_elems, nested, ints=False):
    """One call of gpu::DeviceParseNumberText on `text`: (values, depth,
    row_ends or None). The redo elements are repaired from their offsets.
    ints: the `numbers` mode, every element checked to be an integer of
    `dtype`."""
    require_gpu_tensor(text, "text")
    if text.dtype != torch.uint8:
        raise TypeError("text must be uint8")
    if dtype not in (_INT_RANGES if ints else _PARSE_MODES):
        raise TypeError("dtype must be %s, not %s" % ("int32 or int64" if ints else "float32 or float64", dtype))
    mode = 0 if ints else _PARSE_MODES[dtype]
    dev = text.device
    t = text.contiguous().view(-1)
    n = t.numel()
    if n >= (1 << 32) - 1:
        raise ValueError("%s handles inputs below 4 GiB" % name)
    if n == 0:
        return torch.empty(0, dtype=dtype, device=dev), 0, None
    # an element and its comma take two bytes at least; a row "[v]," four
    cap = (n + 1) // 2 if max_elems is None else int(max_elems)
    row_cap = min(n // 4 + 1, cap) if nested else 0
    # numbers mode: 8 bytes of payload per element and a class byte
    out = torch.empty(max(cap, 1), dtype=torch.int64 if ints else dtype, device=dev)
    classes = torch.zeros(max(cap, 1) if ints else 0, dtype=torch.uint8, device=dev)
    row_ends = torch.empty(max(row_cap, 1), dtype=torch.int32, device=dev) if nested else None
    redo_cap = _REDO_CAP
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        while True:
            redo = torch.empty(2 * redo_cap, dtype=torch.int32, device=dev)
            (err, depth, count, rows, n_redo, first_bad), = native.gpu.device_json_parse_text(
                [t.data_ptr()], [n], [mode], [out.data_ptr()], [classes.data_ptr() if ints else 0], [cap],
                [row_ends.data_ptr() if nested else 0], [row_cap], [redo.data_ptr()], [redo_cap], dev.index or 0)
            if err != 3:
                break
            redo_cap = n_redo  # every listed element is repaired below: list them all
    if err == 1:
        raise ValueError("%s: element %d is not a JSON number" % (name, first_bad))
    if err == 5:
        raise ValueError("%s: more than max_elems=%d elements (the text holds %d)" % (name, cap, count))
    if err:
        raise ValueError("%s: refused (bad arguments, code %d)" % (name, err))
    if ints:
        pairs = (redo[:2 * n_redo].view(-1, 2).cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
        _check_ints(name, t, dtype, out[:count], classes[:count], pairs)
        if dtype != torch.int64:
            return out[:count].to(dtype), depth, (row_ends[:rows] if depth == 2 else None)
    elif n_redo:
        pairs = redo[:2 * n_redo].view(-1, 2).cpu().to(torch.int64) & 0xFFFFFFFF
        vals = [native.json_parse_double(_redo_text(t, off)) for off in pairs[:, 1].tolist()]
        out[pairs[:, 0].to(dev)] = torch.tensor(vals, dtype=torch.float64).to(dtype).to(dev)  # narrowed on the host
    # the worst case is many times the result: do not pin it behind a view
    values = out[:count] if 2 * count >= out.numel() else out[:count].clone()
    return values, depth, (row_ends[:rows] if depth == 2 else None)


_INTEGER_TEXT = re.compile(rb"-?(0|[1-9][0-9]*)\Z")


def _check_ints(name, t, dtype, payload, classes, redo_pairs):
    """The int64 payloads and class bytes of a numbers-mode parse: ValueError
    naming the lowest element that is not an integer of `dtype`. The redo
    elements are classed, and the integers among them filled in, from their
    text."""
    lo, hi = _INT_RANGES[dtype]
    if redo_pairs:
        idx, vals, cls = [], [], []
        for i, off in redo_pairs:
            piece = _redo_text(t, off)
            v = int(piece) if _INTEGER_TEXT.match(piece) else None
            c = 2 if v is None or v >= 1 << 64 or v < -(1 << 63) else (1 if v >= 1 << 63 else 0)
            idx.append(i)
            vals.append(v if c == 0 else 0)
            cls.append(c)
        at = torch.tensor(idx, dtype=torch.int64, device=payload.device)
        payload[at] = torch.tensor(vals, dtype=torch.int64, device=payload.device)
        classes[at] = torch.tensor(cls, dtype=torch.uint8, device=payload.device)
    wrong = classes != 0
    if dtype == torch.int32:
        wrong |= (payload < lo) | (payload > hi)
    first = torch.nonzero(wrong).view(-1)[:1]
    if first.numel():
        i = int(first[0])
        c = int(classes[i])
        why = ("is not an integer" if c == 2 else "is above INT64_MAX" if c == 1 else "does not fit int32")
        raise ValueError("%s: element %d %s" % (name, i, why))


def _shape_rows(name, values, depth, row_ends, ragged):
    """What the row parsers return for the (values, depth, row_ends) of one
    nested parse: a 2-D tensor, or (values, int64 row_ends) when ragged."""
    if depth != 2:
        if values.numel():
            raise ValueError(name + ": the text is not an array of arrays")
        row_ends = torch.empty(0, dtype=torch.int32, device=values.device)
    if ragged:
        return values, row_ends.to(torch.int64)
    rows = row_ends.numel()
    if rows == 0:
        return values.view(0, 0)
    ends = row_ends.cpu().to(torch.int64)
    sizes = torch.diff(ends, prepend=torch.zeros(1, dtype=torch.int64))
    odd = torch.nonzero(sizes != sizes[0]).view(-1)
    if odd.numel():
        r = int(odd[0])
        raise ValueError("%s: row %d has %d elements, row 0 has %d" % (name, r, int(sizes[r]), int(sizes[0])))
    return values.view(rows, int(sizes[0]))


def json_parse_floats(text, dtype=torch.float64, max_elems=None):
    """uint8 device tensor of JSON text ``v,v,...,v`` (or ``[v,v,...]``,
    whitespace allowed wherever JSON allows it) -> float64 / float32 device
    tensor, the inverse of ``json_print_floats``. Every element is converted
    exactly as the host's json2pb converts it: the correctly rounded double
    (``base/decimal_to_double.h``, the code the host reader runs; an integer
    literal becomes the double of its value), and for float32 ``(float)`` of
    that double. The text never leaves HBM and the device finds the elements
    itself (``gpu::DeviceParseNumberText``): one call, no separator table.

    The output is sized for the worst case, ``(n + 1) // 2`` elements, unless
    ``max_elems`` bounds it (ValueError when the text holds more).

    The rare elements a device lane does not decide (more than 19
    significant digits whose truncation leaves the rounding open) are
    fetched as text, converted with ``native.json_parse_double`` and written
    back. Raises ValueError naming the first element that is not a number of
    the RFC 8259 grammar (quoted ``"NaN"`` / ``"Infinity"`` among them).

    The parser runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the values are complete when
    this returns."""
    return _parse_number_text("json_parse_floats", text, dtype, max_elems, False)[0]


def json_parse_float_rows(text, dtype=torch.float64, ragged=False, max_elems=None):
    """uint8 device tensor of JSON text ``[[v,...],[v,...],...]`` -> a 2-D
    float64 / float32 device tensor, one row per inner array: the batch shape
    of http+json model APIs, parsed in HBM by the same single call as
    ``json_parse_floats`` (the device finds the row boundaries too). It
    round-trips with ``json_print_numbers``, which prints the rows back in
    one call.

    Rows of different lengths raise ValueError naming the first row that
    differs from row 0; with ``ragged=True`` the result is ``(values,
    row_ends)`` instead: all elements in order and an int64 tensor with the
    number of elements in rows 0..r. ``[ ]`` is a tensor of shape (0, 0)."""
    name = "json_parse_float_rows"
    values, depth, row_ends = _parse_number_text(name, text, dtype, max_elems, True)
    return _shape_rows(name, values, depth, row_ends, ragged)


def json_parse_ints(text, dtype=torch.int64, max_elems=None):
    """uint8 device tensor of JSON text ``v,v,...,v`` or ``[v,v,...]`` -> int64
    / int32 device tensor, the inverse of ``json_print_numbers`` on integers:
    ``json_parse_floats`` in the parser's ``numbers`` mode, which keeps an
    integer literal as its int64 instead of making a double of it. The text
    never leaves HBM.

    Raises ValueError naming the lowest element that is not an integer of
    ``dtype``: one with a fraction or an exponent (1.5, 1e3), one above
    INT64_MAX, or with ``dtype=torch.int32`` one outside int32; and, as
    ``json_parse_floats``, the first element that is not a JSON number. The
    elements a device lane does not decide (a 25-digit integer) are fetched as
    text and judged on the host.

    Stream discipline and ``max_elems`` as in ``json_parse_floats``."""
    return _parse_number_text("json_parse_ints", text, dtype, max_elems, False, ints=True)[0]


def json_parse_int_rows(text, dtype=torch.int64, ragged=False, max_elems=None):
    """uint8 device tensor of JSON text ``[[v,...],[v,...],...]`` of integers
    -> a 2-D int64 / int32 device tensor, or ``(values, row_ends)`` with
    ``ragged=True``: ``json_parse_float_rows`` for token ids, labels and
    masks. It round-trips with ``json_print_numbers``. Refusals as in
    ``json_parse_ints``."""
    name = "json_parse_int_rows"
    values, depth, row_ends = _parse_number_text(name, text, dtype, max_elems, True, ints=True)
    return _shape_rows(name, values, depth, row_ends, ragged)


_NUMBER_KINDS = {torch.int32: 0, torch.int64: 3, torch.bool: 6, torch.float32: 8, torch.float64: 9}
for _name, _kind in (("uint32", 1), ("uint64", 4)):  # where this torch has them
    if hasattr(torch, _name):
        _NUMBER_KINDS[getattr(torch, _name)] = _kind


def json_print_numbers(values, row_ends=None, brackets=True):
    """Device tensor of numbers -> uint8 device tensor of JSON text, the
    inverse of ``json_parse_float_rows`` / ``json_parse_int_rows``
    (``gpu::DevicePrintNumbers``); neither the values nor the row ends leave
    HBM, and the device checks the row ends itself.

    * 1-D ``values``, ``row_ends=None``: ``[v,v,...,v]``, or ``v,v,...,v``
      with ``brackets=False``.
    * ``row_ends`` (1-D int32 / int64 device tensor, ``row_ends[r]`` = the
      elements in rows 0..r, as ``json_parse_float_rows(..., ragged=True)``
      and ``pb_build_rows`` have it): ``[[v,..],[v,..],..]`` over the
      flattened values. Rows are not empty. No rows and no values: ``[]``.
    * 2-D ``values``, ``row_ends=None``: equal rows, one per ``values[r]``.

    int32 / int64 (uint32 / uint64 where torch has them) print as decimal
    integers, bool as ``true`` / ``false``, float32 / float64 exactly as
    ``json_print_floats`` prints them. No whitespace is written.

    Raises ValueError naming the lowest bad row when ``row_ends`` does not
    ascend strictly to ``values.numel()``.

    Stream discipline as in ``json_print_floats``: the printer runs on a pool
    stream, the caller's current stream is synchronized before the call, and
    the text is complete when this returns."""
    name = "json_print_numbers"
    if isinstance(values, torch.Tensor):
        values = values.contiguous()  # a transposed batch or a slice of one is welcome
    require_gpu_tensor(values, "values")
    if values.dtype not in _NUMBER_KINDS:
        raise TypeError("values must be one of %s, not %s"
                        % (", ".join(str(d) for d in _NUMBER_KINDS), values.dtype))
    dev = values.device
    kind = _NUMBER_KINDS[values.dtype]
    if row_ends is None and values.dim() == 2:
        rows, cols = values.shape
        if rows and not cols:
            raise ValueError(name + ": rows must not be empty")
        row_ends = torch.arange(1, rows + 1, dtype=torch.int64, device=dev) * cols
    elif row_ends is None and values.dim() != 1:
        raise ValueError(name + ": values must be 1-D, or 2-D without row_ends")
    t = values.view(-1)
    n = t.numel()
    ends = None
    if row_ends is not None:
        if isinstance(row_ends, torch.Tensor):
            row_ends = row_ends.contiguous()
        require_gpu_tensor(row_ends, "row_ends")
        if row_ends.dim() != 1 or row_ends.device != dev or row_ends.dtype not in (torch.int32, torch.int64):
            raise TypeError("row_ends must be a 1-D int32 or int64 tensor on the device of values")
        if row_ends.numel() == 0 and n:
            raise ValueError(name + ": %d values in no rows" % n)
        if row_ends.numel():
            # as uint32: what does not fit becomes an end the device refuses
            ends = row_ends if row_ends.dtype == torch.int32 else row_ends.clamp(0, 0xFFFFFFFF).to(torch.int32)
        else:
            brackets = True
    nrows = ends.numel() if ends is not None else 0
    if n == 0 and ends is None and not brackets:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    cap = native.gpu.json_number_print_worst_case(kind, n, nrows)
    if cap >= 1 << 32:
        raise ValueError(name + " handles outputs below 4 GiB")
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, first_bad, err), = native.gpu.device_json_print_numbers(
            [t.data_ptr() if n else 0], [n], [kind], [ends.data_ptr() if nrows else 0], [nrows], [bool(brackets)],
            [out.data_ptr()], [cap], dev.index or 0)
    if err == 1:
        raise ValueError("%s: row_ends[%d] does not ascend strictly to the %d values" % (name, first_bad, n))
    if err:
        raise ValueError(name + ": " + PRINT_ERRORS.get(err, "code %d" % err))
    return out[:length]


# kind_name -> (kind, text form, dtypes): the names ops.pb uses for its
# columns, plus the two text forms of uint8 data. fixed32 / fixed64 and bytes
# are wire notions: a JSON cell needs to know what the bits mean.
_RECORD_KINDS = {
    "int32": (0, 0, (torch.int32,)),
    "uint32": (1, 0, (torch.int32, getattr(torch, "uint32", torch.int32))),
    "sint32": (2, 0, (torch.int32,)),
    "int64": (3, 0, (torch.int64,)),
    "uint64": (4, 0, (torch.int64, getattr(torch, "uint64", torch.int64))),
    "sint64": (5, 0, (torch.int64,)),
    "bool": (6, 0, (torch.bool, torch.uint8)),
    "float32": (8, 0, (torch.float32,)),
    "float64": (9, 0, (torch.float64,)),
    "string": (7, 1, (torch.uint8,)),
    "base64": (7, 2, (torch.uint8,)),
}
RECORD_PRINT_ERRORS = dict(PRINT_ERRORS)
RECORD_PRINT_ERRORS[2] = "refused (columns, kinds, a scalar column's length, keys, alignment or size)"


def json_print_records(columns, brackets=True):
    """Columns of a batch in device memory -> uint8 device tensor of the JSON
    text ``[{"k0":cell,"k1":cell,...},...]`` (``gpu::DevicePrintRecordObjects``),
    the shape http+json model APIs return; no column and no table leaves HBM.

    columns: [(key, values, row_ends_or_None, kind_name)], at most 8, printed
    into every record in this order: every key appears in every record and
    nothing is omitted (this is not pb2json's omission rule). ``key`` is str
    (its UTF-8) or bytes. ``kind_name`` is one of the names ``pb_build_records``
    uses for numbers (int32, uint32, sint32, int64, uint64, sint64, bool,
    float32, float64), or ``"string"`` / ``"base64"`` for uint8 data. The
    ``(values, row_ends)`` pairs of ``pb_split_records`` are taken unchanged: an
    int64 ``row_ends`` is narrowed on the device, rows may be empty. With
    ``row_ends=None`` a 1-D tensor is a scalar column (one element per record),
    a 2-D one means equal rows.

    A cell is the element as ``json_print_numbers`` prints it, ``[v,...,v]``
    for a ragged number column, the escaped row in quotes for ``"string"``
    (no UTF-8 verdict) and the padded base64 of the row in quotes for
    ``"base64"``. ``brackets=False`` leaves the outer ``[`` ``]`` away.

    Raises ValueError naming the lowest bad row and its column when a table of
    row ends is malformed. Stream discipline as in ``json_print_numbers``."""
    name = "json_print_records"
    if not columns:
        raise ValueError("no columns")
    dev = columns[0][1].device
    rows, cols, keep = None, [], []
    for c, (key, values, row_ends, kind_name) in enumerate(columns):
        if kind_name not in _RECORD_KINDS:
            raise ValueError("column %d: unknown kind %r (one of %s)" % (c, kind_name, ", ".join(_RECORD_KINDS)))
        kind, text, dtypes = _RECORD_KINDS[kind_name]
        require_gpu_tensor(values, "column %d" % c)
        if values.device != dev:
            raise ValueError("all columns must live on one device (%s vs %s)" % (values.device, dev))
        if values.dtype not in dtypes:
            raise TypeError("column %d: kind %s takes a tensor of %s, not %s" % (c, kind_name, dtypes[0], values.dtype))
        if row_ends is None and values.dim() == 2:
            per = values.shape[1]
            row_ends = torch.arange(1, values.shape[0] + 1, dtype=torch.int32, device=dev) * per
        elif row_ends is None and values.dim() != 1:
            raise ValueError("column %d: values must be 1-D, or 2-D without row_ends" % c)
        values = values.contiguous()
        count = values.numel()
        ends_ptr, nrows = 0, count
        if row_ends is not None:
            require_gpu_tensor(row_ends, "column %d row_ends" % c)
            if row_ends.device != dev:
                raise ValueError("column %d: row_ends must live on the same device as values" % c)
            if row_ends.dtype == torch.int64:
                # as uint32: what does not fit becomes an end the device refuses
                row_ends = row_ends.clamp(0, 0xFFFFFFFF).to(torch.int32)
            if row_ends.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or row_ends.dim() != 1:
                raise TypeError("column %d: row_ends must be a 1-D int32, uint32 or int64 tensor, not %s"
                                % (c, row_ends.dtype))
            row_ends = row_ends.contiguous()
            nrows = row_ends.numel()
            ends_ptr = row_ends.data_ptr() if nrows else 0
            if nrows == 0 and count:
                raise ValueError("column %d: %d values in no rows" % (c, count))
            keep.append(row_ends)
        elif kind == 7:
            raise ValueError("column %d: a %s column needs row_ends" % (c, kind_name))
        if rows is None:
            rows = nrows
        elif nrows != rows:
            raise ValueError("column %d holds %d records, the columns before it %d" % (c, nrows, rows))
        keep.append(values)
        key = key.encode("utf-8") if isinstance(key, str) else bytes(key)
        cols.append((key, kind, text, values.data_ptr() if count else 0, count, ends_ptr))
    if rows == 0:  # no record: "[]" or nothing, and nothing to launch
        return torch.tensor(list(b"[]" if brackets else b""), dtype=torch.uint8, device=dev)
    cap = native.gpu.json_records_worst_case(cols, rows, bool(brackets))
    if cap == 0:
        raise ValueError(name + ": " + RECORD_PRINT_ERRORS[2])
    if cap >= 1 << 32:
        raise ValueError(name + " handles outputs below 4 GiB")
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err, first_bad, bad_column), = native.gpu.device_json_print_records(
            [(cols, rows, bool(brackets), out.data_ptr(), cap)], dev.index or 0)
    if err == 1:
        raise ValueError("%s: column %d: row_ends[%d] does not ascend to the column's %d values"
                         % (name, bad_column, first_bad, cols[bad_column][4]))
    if err:
        raise ValueError(name + ": " + RECORD_PRINT_ERRORS.get(err, "code %d" % err))
    return out[:length]


def base64_encode(data):
    """Any contiguous device tensor -> uint8 device tensor of the base64 text
    of its bytes (standard alphabet, ``=`` padded): the form pb2json gives a
    ``bytes`` field, 4/3 the size of the data. The bytes never leave HBM
    (``gpu::DeviceBase64Encode``).

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the text is complete when
    this returns."""
    require_gpu_tensor(data, "data")
    if not data.is_contiguous():
        raise ValueError("data must be contiguous")
    dev = data.device
    n = data.numel() * data.element_size()
    cap = (n + 2) // 3 * 4
    if cap >= 1 << 32:
        raise ValueError("base64_encode handles outputs below 4 GiB")
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err), = native.gpu.device_base64_encode([data.data_ptr()], [n], [out.data_ptr()], [cap],
                                                        dev.index or 0)
    if err:
        raise ValueError("base64_encode: refused (code %d)" % err)
    return out[:length]


def base64_decode(text):
    """uint8 device tensor of base64 text -> uint8 device tensor of the bytes,
    the inverse of ``base64_encode``. Canonical text (alphabet symbols and up
    to two trailing ``=``, padded or not) is decoded in HBM
    (``gpu::DeviceBase64Decode``). Anything else is fetched and given to the
    host decoder ``native.base64_decode``, which skips line breaks and
    spaces: its result is returned, or ValueError raised naming the offset of
    the first byte the device found odd.

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the bytes are complete when
    this returns."""
    require_gpu_tensor(text, "text")
    if text.dtype != torch.uint8:
        raise TypeError("text must be uint8")
    dev = text.device
    t = text.contiguous().view(-1)
    n = t.numel()
    if n >= (1 << 32) - 1:
        raise ValueError("base64_decode handles inputs below 4 GiB")
    cap = n // 4 * 3 + (n % 4) * 3 // 4
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err, first_odd), = native.gpu.device_base64_decode([t.data_ptr()], [n], [out.data_ptr()], [cap],
                                                                   dev.index or 0)
    if err == 1:
        lax = native.base64_decode(bytes(t.cpu().numpy()))
        if lax is None:
            raise ValueError("base64_decode: not base64 text (offset %d)" % first_odd)
        if not lax:
            return out[:0]
        return torch.frombuffer(bytearray(lax), dtype=torch.uint8).to(dev)
    if err:
        raise ValueError("base64_decode: refused (code %d)" % err)
    return out[:length]


_STRING_ERRORS = {2: "refused (bad arguments)", 3: "longer than the output buffer",
                  4: "the source changed during the call"}


def _flat_bytes(t, name):
    require_gpu_tensor(t, name)
    if t.dtype != torch.uint8:
        raise TypeError("%s must be uint8" % name)
    t = t.contiguous().view(-1)
    if t.numel() >= (1 << 32) - 1:
        raise ValueError("%s must be below 4 GiB" % name)
    return t


def json_escape_string(data, row_ends=None, quote=True, max_bytes=None):
    """uint8 device tensor of text -> uint8 device tensor of its JSON string:
    exactly what the host's ``json::EscapeString`` writes (``\\"`` ``\\\\``
    ``\\n`` ``\\r`` ``\\t`` ``\\b`` ``\\f``, ``\\u00xx`` for the other control
    bytes, everything else copied), with the surrounding quotes unless
    ``quote=False``. With ``row_ends`` (an integer device tensor, the bytes in
    rows 0..r, as ``pb_split_rows`` returns it for a ``repeated string``) the
    result is ``"r0","r1",...,"rk"``: a whole repeated field in one call. The
    text never leaves HBM (``gpu::DeviceEscapeJsonStrings``).

    The output is sized for the worst case (six bytes per byte) unless
    ``max_bytes`` bounds it (ValueError naming the size needed when the text
    is longer). ValueError names the first row whose end lies below its
    predecessor's, or the last row when it does not end at ``len(data)``.

    The escaper runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the text is complete when
    this returns."""
    t = _flat_bytes(data, "data")
    dev = t.device
    n = t.numel()
    rows, ends = 0, None
    if row_ends is not None:
        require_gpu_tensor(row_ends, "row_ends")
        ends = row_ends.contiguous().view(-1).to(torch.int32)
        rows = ends.numel()
        if rows == 0:
            if n:
                raise ValueError("json_escape_string: bytes without rows")
            return torch.empty(0, dtype=torch.uint8, device=dev)
    worst = native.gpu.json_escape_worst_case(n, rows) if rows else n * 6 + (2 if quote else 0)
    cap = worst if max_bytes is None else min(int(max_bytes), worst)
    if cap >= 1 << 32:
        raise ValueError("json_escape_string: the worst case must be below 4 GiB (pass max_bytes)")
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    if n == 0 and not rows and not quote:
        return out[:0]
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err, first_bad), = native.gpu.device_json_escape(
            [t.data_ptr() if n else 0], [n], [out.data_ptr()], [cap], [ends.data_ptr()] if rows else [],
            [rows] if rows else [], quote, dev.index or 0)
    if err == 1:
        raise ValueError("json_escape_string: row_ends is not ascending to len(data) (row %d)" % first_bad)
    if err == 3:
        raise ValueError("json_escape_string: max_bytes=%d is too small (the text takes %d)" % (cap, length))
    if err:
        raise ValueError("json_escape_string: " + _STRING_ERRORS.get(err, "code %d" % err))
    return out[:length] if 2 * length >= out.numel() else out[:length].clone()


def json_unescape_string(text):
    """uint8 device tensor of a JSON string's body (what stands between the
    quotes) -> uint8 device tensor of its bytes, the inverse of
    ``json_escape_string(..., quote=False)``. Escapes are resolved in HBM
    (``gpu::DeviceUnescapeJsonStrings``): the one-letter escapes, ``\\uXXXX``
    to UTF-8, a surrogate pair to its four bytes. A body the device leaves to
    the host (an unescaped quote, a bad or cut-off escape, a lone surrogate)
    is fetched and given to ``native.json_unescape`` and then to the reader
    itself (``native.json_reader_string``), which is looser about surrogates:
    its result is returned, or ValueError raised naming the offset the device
    reported.

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the bytes are complete when
    this returns."""
    t = _flat_bytes(text, "text")
    dev = t.device
    n = t.numel()
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err, first_bad), = native.gpu.device_json_unescape([t.data_ptr()], [n], [out.data_ptr()], [n],
                                                                   dev.index or 0)
    if err == 1:
        body = bytes(t.cpu().numpy())
        lax, _ = native.json_unescape(body)
        if lax is None:
            lax = native.json_reader_string(body)
        if lax is None:
            raise ValueError("json_unescape_string: not the body of a JSON string (offset %d)" % first_bad)
        if not lax:
            return out[:0]
        return torch.frombuffer(bytearray(lax), dtype=torch.uint8).to(dev)
    if err:
        raise ValueError("json_unescape_string: " + _STRING_ERRORS.get(err, "code %d" % err))
    return out[:length]


def _string_rows_tensors(rows, dev):
    data = b"".join(rows)
    ends, total = [], 0
    for r in rows:
        total += len(r)
        ends.append(total)
    values = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data \
        else torch.empty(0, dtype=torch.uint8, device=dev)
    return values, torch.tensor(ends, dtype=torch.int32).to(dev)


def json_unescape_string_rows(text, max_bytes=None, max_rows=None):
    """uint8 device tensor holding the text of an array of JSON strings,
    ``"r0","r1",...,"rk"`` or ``["r0","r1",...,"rk"]`` with JSON whitespace
    wherever JSON allows it -> ``(bytes, row_ends)``: a uint8 device tensor of
    the decoded strings one after the other and an int32 one with
    ``row_ends[r]`` the bytes in strings 0..r. The inverse of
    ``json_escape_string(data, row_ends)``, and what
    ``pb_build_rows(number, bytes, row_ends, "bytes")`` takes for a ``repeated
    string``. The text never leaves HBM
    (``gpu::DeviceUnescapeJsonStringRows``); empty text, whitespace and ``[ ]``
    give no rows. The bytes are not checked for UTF-8: run ``utf8_validate``
    on them (a concatenation can validate where a row alone would not).

    The outputs are sized for the worst case (``len(text) - 2`` bytes,
    ``(len(text) + 1) // 3`` rows) unless ``max_bytes`` / ``max_rows`` bound
    them (ValueError naming what the text takes when it holds more). A text
    the device leaves to the host (a lone surrogate, a bad escape, anything
    that is not an array of strings) is fetched and given to the reader
    (``native.json_reader_string_array``): its result is returned as device
    tensors, or ValueError raised naming the offset the device reported.

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and both tensors are complete
    when this returns."""
    t = _flat_bytes(text, "text")
    dev = t.device
    n = t.numel()
    worst_bytes = native.gpu.json_string_rows_max_bytes(n)
    worst_rows = native.gpu.json_string_rows_max_rows(n)
    cap = worst_bytes if max_bytes is None else min(int(max_bytes), worst_bytes)
    row_cap = worst_rows if max_rows is None else min(int(max_rows), worst_rows)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    ends = torch.empty(max(row_cap, 1), dtype=torch.int32, device=dev)
    if n == 0:
        return out[:0], ends[:0]
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, rows, _, err, first_bad), = native.gpu.device_json_unescape_rows(
            [t.data_ptr()], [n], [out.data_ptr() if cap else 0], [cap], [ends.data_ptr() if row_cap else 0], [row_cap],
            dev.index or 0)
    if err == 1:
        lax = native.json_reader_string_array(bytes(t.cpu().numpy()))
        if lax is None:
            raise ValueError("json_unescape_string_rows: not an array of JSON strings (offset %d)" % first_bad)
        return _string_rows_tensors(lax, dev)
    if err == 3:
        raise ValueError("json_unescape_string_rows: max_bytes=%d, max_rows=%d is too small (the text takes %d bytes "
                         "in %d rows)" % (cap, row_cap, length, rows))
    if err:
        raise ValueError("json_unescape_string_rows: " + _STRING_ERRORS.get(err, "code %d" % err))
    return out[:length], ends[:rows]


def base64_encode_rows(data, row_ends=None, brackets=True):
    """uint8 device tensor of bytes and an int32 / int64 device tensor
    ``row_ends`` (the bytes in rows 0..r, as ``pb_split_rows(..., "bytes")`` and
    a bytes column of ``pb_split_records`` return them) -> uint8 device tensor
    of the text ``["b0","b1",...,"bk"]``, every row as its ``=``-padded base64:
    a ``repeated bytes`` field, or a bytes column, as http+json carries it.
    ``brackets=False`` leaves the ``[`` ``]`` away. A 2-D ``data`` with
    ``row_ends=None`` means equal rows. The bytes never leave HBM
    (``gpu::DeviceBase64EncodeRows``); int64 ends are narrowed on the device.

    ValueError names the first row whose end lies below its predecessor's or
    above ``len(data)``, or the last row when it does not end at ``len(data)``.

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and the text is complete when
    this returns."""
    require_gpu_tensor(data, "data")
    if data.dtype != torch.uint8:
        raise TypeError("data must be uint8")
    dev = data.device
    if row_ends is None:
        if data.dim() != 2:
            raise ValueError("base64_encode_rows: row_ends is needed unless data is 2-D")
        rows, width = data.shape
        ends = torch.arange(1, rows + 1, dtype=torch.int64, device=dev).mul_(width).to(torch.int32)
    else:
        require_gpu_tensor(row_ends, "row_ends")
        if row_ends.dtype not in (torch.int32, torch.int64):
            raise TypeError("row_ends must be int32 or int64")
        ends = row_ends.contiguous().view(-1).to(torch.int32)
        rows = ends.numel()
    t = _flat_bytes(data, "data")
    n = t.numel()
    if rows == 0 and n:
        raise ValueError("base64_encode_rows: bytes without rows")
    cap = native.gpu.base64_rows_worst_case(n, rows, brackets)
    if cap >= 1 << 32:
        raise ValueError("base64_encode_rows: the worst case must be below 4 GiB")
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    if cap == 0:
        return out[:0]
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, err, first_bad), = native.gpu.device_base64_encode_rows(
            [t.data_ptr() if n else 0], [n], [ends.data_ptr() if rows else 0], [rows], brackets, [out.data_ptr()], [cap],
            dev.index or 0)
    if err == 1:
        raise ValueError("base64_encode_rows: row_ends is not ascending to len(data) (row %d)" % first_bad)
    if err:
        raise ValueError("base64_encode_rows: " + _STRING_ERRORS.get(err, "code %d" % err))
    return out[:length]


def base64_decode_rows(text, max_bytes=None, max_rows=None):
    """uint8 device tensor holding the text of an array of base64 strings,
    ``"b0","b1",...,"bk"`` or ``["b0","b1",...,"bk"]`` with JSON whitespace
    wherever JSON allows it -> ``(bytes, row_ends)``: a uint8 device tensor of
    the decoded rows one after the other and an int32 one with ``row_ends[r]``
    the bytes in rows 0..r. The inverse of ``base64_encode_rows``, and what
    ``pb_build_rows(number, bytes, row_ends, "bytes")`` and a bytes column of
    ``pb_build_records`` take. The text never leaves HBM
    (``gpu::DeviceBase64DecodeRows``); empty text, whitespace and ``[ ]`` give
    no rows.

    The outputs are sized for the worst case unless ``max_bytes`` /
    ``max_rows`` bound them (ValueError naming what the text takes when it
    holds more). A text the device leaves to the host (anything but canonical
    base64 inside the strings: a line break, an escape, URL-safe symbols; or
    anything that is not an array of strings) is fetched and given to the
    reader (``native.json_reader_string_array``) and then, row by row, to
    ``native.base64_decode``: their result is returned as device tensors, or
    ValueError raised naming the offset the device reported.

    The coder runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call, and both tensors are complete
    when this returns."""
    t = _flat_bytes(text, "text")
    dev = t.device
    n = t.numel()
    worst_bytes = native.gpu.base64_rows_max_bytes(n)
    worst_rows = native.gpu.base64_rows_max_rows(n)
    cap = worst_bytes if max_bytes is None else min(int(max_bytes), worst_bytes)
    row_cap = worst_rows if max_rows is None else min(int(max_rows), worst_rows)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    ends = torch.empty(max(row_cap, 1), dtype=torch.int32, device=dev)
    if n == 0:
        return out[:0], ends[:0]
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (length, rows, _, err, first_bad), = native.gpu.device_base64_decode_rows(
            [t.data_ptr()], [n], [out.data_ptr() if cap else 0], [cap], [ends.data_ptr() if row_cap else 0], [row_cap],
            dev.index or 0)
    if err == 1:
        strings = native.json_reader_string_array(bytes(t.cpu().numpy()))
        lax = None if strings is None else [native.base64_decode(s) for s in strings]
        if lax is None or any(r is None for r in lax):
            raise ValueError("base64_decode_rows: not an array of base64 strings (offset %d)" % first_bad)
        return _string_rows_tensors(lax, dev)
    if err == 3:
        raise ValueError("base64_decode_rows: max_bytes=%d, max_rows=%d is too small (the text takes %d bytes in %d "
                         "rows)" % (cap, row_cap, length, rows))
    if err:
        raise ValueError("base64_decode_rows: " + _STRING_ERRORS.get(err, "code %d" % err))
    return out[:length], ends[:rows]


def utf8_validate(data):
    """uint8 device tensor -> None when it is well-formed UTF-8 (the rule a
    protobuf ``string`` and a JSON text carry), else the first offset at which
    no well-formed sequence starts: what ``bytes.decode`` reports as
    ``UnicodeDecodeError.start``. The bytes never leave HBM
    (``gpu::DeviceValidateUtf8``).

    The check runs on a pool stream, not on torch's: the caller's current
    stream is synchronized before the call."""
    t = _flat_bytes(data, "data")
    dev = t.device
    n = t.numel()
    if n == 0:
        return None
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        (err, first_bad), = native.gpu.device_utf8_validate([t.data_ptr()], [n], dev.index or 0)
    if err == 1:
        return first_bad
    if err:
        raise ValueError("utf8_validate: " + _STRING_ERRORS.get(err, "code %d" % err))
    return None
