"""json::FormatNumberRows (native.json_format_number_rows), the host twin of
the device printer gpu::DevicePrintNumbers, against Python's own json module:
integers and bools byte for byte with json.dumps, floats element by element
with native.json_shortest_double (the oracle of the float printers), and
json.loads of every text gives the values back. The C++ side is
brpc_amd/csrc/tests/number_print_unittest.cc; the device printer is compared
byte for byte with this twin in tests/test_gpu_json_number_rows.py."""
import json
import math

import pytest

np = pytest.importorskip("numpy")

NONE = 0xFFFFFFFF
INT32, UINT32, SINT32, INT64, UINT64, SINT64, BOOL, FLOAT, DOUBLE = 0, 1, 2, 3, 4, 5, 6, 8, 9
DTYPES = {INT32: np.int32, UINT32: np.uint32, SINT32: np.int32, INT64: np.int64, UINT64: np.uint64, SINT64: np.int64,
          BOOL: np.uint8, FLOAT: np.float32, DOUBLE: np.float64}


def _values(kind, n, seed):
    """n elements of `kind` of every width and both signs, the extremes among them."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(DTYPES[kind])
    if kind == BOOL:
        return rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), n)
    if kind in (FLOAT, DOUBLE):
        a = rng.standard_normal(n) * np.power(10.0, rng.integers(-30, 30, n))
        a[::5] = np.round(a[::5])
        return a.astype(dt)
    info = np.iinfo(dt)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)
    a = (bits & np.uint64(info.max)).astype(dt)
    if info.min < 0:
        a = np.where(rng.integers(0, 2, n) == 1, a, -a).astype(dt)
    a[:2] = [info.min, info.max][:len(a[:2])]
    return a


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    ends, at = [], 0
    while at < n:
        at = min(n, at + int(rng.integers(1, 6)))
        ends.append(at)
    return ends


def _nest(items, ends):
    return [items[a:b] for a, b in zip([0] + ends[:-1], ends)]


def _py(a, kind):
    if kind == BOOL:
        return [bool(x) for x in a]
    return a.tolist()


@pytest.mark.parametrize("kind", [INT32, UINT32, SINT32, INT64, UINT64, SINT64, BOOL])
@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_ints_and_bools_equal_json_dumps(native, kind, n):
    a = _values(kind, n, seed=kind * 1000 + n)
    items, ends = _py(a, kind), _rows(n, seed=n)
    dumps = lambda v: json.dumps(v, separators=(",", ":")).encode()  # noqa: E731
    err, bad, text = native.json_format_number_rows(a.tobytes(), n, kind, None, True)
    assert (err, bad) == (0, NONE) and text == dumps(items)
    assert json.loads(text) == items
    err, bad, bare = native.json_format_number_rows(a.tobytes(), n, kind, None, False)
    assert (err, bad) == (0, NONE) and bare == text[1:-1]
    for table in (ends, np.array(ends, dtype=np.uint32).tobytes()):
        err, bad, nested = native.json_format_number_rows(a.tobytes(), n, kind, table, False)
        assert (err, bad) == (0, NONE) and nested == dumps(_nest(items, ends))
    assert json.loads(nested) == _nest(items, ends)
    assert b" " not in nested


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_floats_equal_the_shortest_double_per_element(native, kind, n):
    a = _values(kind, n, seed=kind * 1000 + n)
    ends = _rows(n, seed=n)
    elems = [native.json_shortest_double(float(x)) for x in a]
    err, bad, text = native.json_format_number_rows(a.tobytes(), n, kind, None, False)
    assert (err, bad) == (0, NONE) and text == b",".join(elems)
    assert text == native.json_format_floats(a.tobytes(), kind)
    err, bad, nested = native.json_format_number_rows(a.tobytes(), n, kind, ends, True)
    want = b"[" + b",".join(b"[" + b",".join(row) + b"]" for row in _nest(elems, ends)) + b"]"
    assert (err, bad) == (0, NONE) and nested == want
    back = json.loads(nested)
    assert [len(r) for r in back] == [len(r) for r in _nest(elems, ends)]
    flat = np.array([x for r in back for x in r], dtype=np.float64).astype(DTYPES[kind])
    assert flat.tobytes() == a.tobytes()  # bit for bit, through Python's own parser


def test_non_finite_floats_are_quoted(native):
    a = np.array([math.nan, math.inf, -math.inf, -0.0], dtype=np.float32)
    err, _, text = native.json_format_number_rows(a.tobytes(), 4, FLOAT, [1, 4], True)
    assert err == 0 and text == b'[["NaN"],["Infinity","-Infinity",-0.0]]'
    assert json.loads(text) == [["NaN"], ["Infinity", "-Infinity", -0.0]]


def test_empty_forms(native):
    for kind in DTYPES:
        assert native.json_format_number_rows(b"", 0, kind, None, True) == (0, NONE, b"[]")
        assert native.json_format_number_rows(b"", 0, kind, None, False) == (0, NONE, b"")


def test_first_bad_and_refusals(native):
    a = np.arange(10, dtype=np.int32).tobytes()
    fmt = lambda ends: native.json_format_number_rows(a, 10, INT32, ends, True)  # noqa: E731
    assert fmt([3, 5, 10]) == (0, NONE, b"[[0,1,2],[3,4],[5,6,7,8,9]]")
    assert fmt([3, 2, 10]) == (1, 1, b"")     # a decrease
    assert fmt([3, 3, 10]) == (1, 1, b"")     # two equal neighbours
    assert fmt([0, 5, 10]) == (1, 0, b"")     # row_ends[0] == 0
    assert fmt([3, 11, 12]) == (1, 1, b"")    # an end above count
    assert fmt([3, 5, 9]) == (1, 2, b"")      # a last end below count
    assert fmt([]) == (2, NONE, b"")          # row ends without rows
    assert native.json_format_number_rows(a, 10, 7, None, True) == (2, NONE, b"")
    assert native.json_format_number_rows(a, 10, 10, None, True) == (2, NONE, b"")
    with pytest.raises(ValueError):
        native.json_format_number_rows(a, 11, INT32, None, True)  # fewer bytes than elements
