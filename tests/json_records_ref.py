"""Shared by the JSON records tests (not a test module): a pure-Python
composer of [{"k0":cell,...},...] whose every cell comes from a printer that
other tests already pin (native.json_format_number_rows, native.json_escape,
native.base64_encode), the Python structure json.loads must give back, and the
verdict on a table of row ends written out from the rule.

A column is a dict: key (bytes), kind (0..6, 8, 9 or BYTES), text (NUMBER,
STRING, BASE64), arr (the numpy array of all its elements) and ends (the row
ends, or None for a scalar column: one element per record)."""
import numpy as np

INT32, UINT32, SINT32, INT64, UINT64, SINT64, BOOL, BYTES, FLOAT, DOUBLE = range(10)
NUMBER, STRING, BASE64 = 0, 1, 2
DTYPES = {INT32: np.int32, UINT32: np.uint32, SINT32: np.int32, INT64: np.int64, UINT64: np.uint64, SINT64: np.int64,
          BOOL: np.uint8, BYTES: np.uint8, FLOAT: np.float32, DOUBLE: np.float64}
NUMBER_KINDS = [k for k in sorted(DTYPES) if k != BYTES]
NONE = 0xFFFFFFFF


def column(key, kind, arr, ends=None, text=NUMBER):
    key = key.encode("utf-8") if isinstance(key, str) else bytes(key)
    return dict(key=key, kind=kind, text=text, arr=np.ascontiguousarray(arr, dtype=DTYPES.get(kind, np.uint8)),
                ends=None if ends is None else np.asarray(ends, dtype=np.uint32))


def twin_columns(columns):
    """The columns as native.json_format_record_objects takes them."""
    return [(c["key"], c["kind"], c["text"], c["arr"].tobytes(), None if c["ends"] is None else c["ends"].tobytes())
            for c in columns]


def values(kind, n, seed=0, nonfinite=True):
    """n elements of `kind`: text lengths from 1 byte to the kind's widest side
    by side, the extremes first; floats with NaN and both infinities."""
    rng = np.random.default_rng(seed * 16 + kind)
    dt = np.dtype(DTYPES[kind])
    if kind == BOOL:
        return rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), n)
    if kind == BYTES:
        a = rng.integers(0, 256, n).astype(np.uint8)
        special = np.frombuffer(b'"\\\n\r\t\b\f\x00\x01\x1f/\x7f\x80\xff', dtype=np.uint8)
        pick = rng.integers(0, 3, n) == 0
        a[pick] = rng.choice(special, int(pick.sum()))
        return a
    if kind in (FLOAT, DOUBLE):
        a = rng.standard_normal(n) * np.power(10.0, rng.integers(-30, 30, n))
        a[::5] = np.round(a[::5])
        a = a.astype(dt)
        if nonfinite and n > 3:
            a[1], a[2], a[3] = np.nan, np.inf, -np.inf
        return a
    info = np.iinfo(dt)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)
    a = (bits & np.uint64(info.max)).astype(dt)
    if info.min < 0:
        a = np.where(rng.integers(0, 2, n) == 1, a, -a).astype(dt)
    a[:2] = [info.min, info.max][:len(a[:2])]
    return a


def ragged(rows, seed, longest=5, empty=3):
    """Row ends of `rows` rows of 0..longest elements, about one in `empty` empty."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, longest + 1, rows) * (rng.integers(0, empty, rows) > 0)
    return np.cumsum(sizes).astype(np.uint32)


def first_bad(columns, rows):
    """(row, column) of the lowest offender, None when every table is good: an
    end below its predecessor, an end above the column's count, or a last end
    that is not the count; the lowest row over all columns, then the lowest
    column that offends there."""
    best = None
    for c, col in enumerate(columns):
        if col["ends"] is None:
            continue
        prev = 0
        for r in range(rows):
            end = int(col["ends"][r])
            if end < prev or end > col["arr"].size or (r + 1 == rows and end != col["arr"].size):
                if best is None or (r, c) < best:
                    best = (r, c)
                break
            prev = end
    return best


def _elem_texts(native, col):
    """The text of every element of a number column, printed in one call."""
    n = col["arr"].size
    if n == 0:
        return []
    err, _, text = native.json_format_number_rows(col["arr"].tobytes(), n, col["kind"], None, False)
    assert err == 0
    parts = text.split(b",")  # no number, and no quoted NaN / Infinity, holds a comma
    assert len(parts) == n
    return parts


def reference(native, columns, rows, brackets=True):
    """The text, composed record by record. The tables must be good."""
    if rows == 0:
        return b"[]" if brackets else b""
    texts = [None if c["text"] != NUMBER else _elem_texts(native, c) for c in columns]
    records = []
    for r in range(rows):
        cells = []
        for c, col in enumerate(columns):
            key = native.json_escape(col["key"], None, True)
            if col["ends"] is None:
                cell = texts[c][r]
            else:
                lo, hi = (int(col["ends"][r - 1]) if r else 0), int(col["ends"][r])
                if col["text"] == STRING:
                    cell = native.json_escape(col["arr"][lo:hi].tobytes(), None, True)
                elif col["text"] == BASE64:
                    cell = b'"' + native.base64_encode(col["arr"][lo:hi].tobytes()) + b'"'
                else:
                    cell = b"[" + b",".join(texts[c][lo:hi]) + b"]"
            cells.append(key + b":" + cell)
        records.append(b"{" + b",".join(cells) + b"}")
    body = b",".join(records)
    return b"[" + body + b"]" if brackets else body


def _py_value(kind, x):
    if kind == BOOL:
        return bool(x)
    if kind in (FLOAT, DOUBLE):
        x = float(x)  # of a float32: its exact value
        if x != x:
            return "NaN"
        if x in (float("inf"), float("-inf")):
            return "Infinity" if x > 0 else "-Infinity"
        return x
    return int(x)


def structure(columns, rows):
    """What json.loads(text.decode("latin-1")) must equal: bytes map to code
    points one to one, so keys and strings of any bytes compare exactly."""
    import base64
    out = []
    for r in range(rows):
        rec = {}
        for col in columns:
            key = col["key"].decode("latin-1")
            if col["ends"] is None:
                rec[key] = _py_value(col["kind"], col["arr"][r])
                continue
            lo, hi = (int(col["ends"][r - 1]) if r else 0), int(col["ends"][r])
            if col["text"] == STRING:
                rec[key] = col["arr"][lo:hi].tobytes().decode("latin-1")
            elif col["text"] == BASE64:
                rec[key] = base64.b64encode(col["arr"][lo:hi].tobytes()).decode()
            else:
                rec[key] = [_py_value(col["kind"], x) for x in col["arr"][lo:hi]]
        out.append(rec)
    return out


def random_columns(rng, rows, ncols, first_kind=0, nonfinite=True):
    """ncols columns of every kind and shape over `rows` records, with empty
    rows, now and then a column without any element, keys that need escaping."""
    keys = [b"label", b'i"ds', b"sc\\ores", b"te\x01xt", b"bl\xc3\xa9ob", b"k\x80\xff", b"", b"\tz"]
    cols = []
    for c in range(ncols):
        kind = (first_kind + c) % 11
        text = NUMBER
        if kind >= 10 or kind == BYTES:
            text = STRING if kind == BYTES else BASE64
            kind = BYTES
        seed = int(rng.integers(0, 1 << 30))
        if kind != BYTES and rng.integers(0, 3) == 0:
            cols.append(column(keys[c], kind, values(kind, rows, seed, nonfinite)))
            continue
        ends = ragged(rows, seed, longest=int(rng.integers(1, 9)))
        if rng.integers(0, 6) == 0:
            ends[:] = 0
        n = int(ends[-1]) if rows else 0
        cols.append(column(keys[c], kind, values(kind, n, seed, nonfinite), ends, text))
    return cols
