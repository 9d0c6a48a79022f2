"""json::ParseNumberText (native.json_parse_number_text), the host twin of
the device parser of number text without a separator table, against
Python: every value is float() of its element (correctly rounded), rows are
json.loads', and every malformed text is refused at the piece it should be.
The C++ side is brpc_amd/csrc/tests/number_text_unittest.cc; the device
side, compared byte for byte with this twin, is
tests/test_gpu_json_number_text.py."""
import json
import random
import struct

import pytest

np = pytest.importorskip("numpy")

NUMBERS, FLOAT64, FLOAT32 = 0, 1, 2
INT64, UINT64, DOUBLE, NEEDS_EXACT = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def _mixed(n, seed=0):
    """Elements of 1 to 25 characters side by side, every class among them
    (the pattern of tests/test_gpu_json_float_parse.py)."""
    pattern = ["1", "-1.2345678901234567e-0006", "0.5", "-0", "1e300", "18446744073709551615", "2.5E+0", "-0.0",
               "123456.0", "9223372036854775807", "4.9e-324", "0.1234567890123456789", "-7", "1e22", "3.4028235e38",
               "-9223372036854775808", "1.7976931348623157e308", "6", "1e-400", "0.000001"]
    rng = random.Random(seed)
    out = [pattern[i % len(pattern)] for i in range(n)]
    for i in range(0, n, 7):
        out[i] = repr(rng.gauss(0.0, 1.0))
    return out


def _powers_and_subnormals():
    pows = (np.arange(1, 2047, dtype=np.uint64) << np.uint64(52))  # the 2046 powers of two
    sub = np.array([1, 2, 3, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 51), (1 << 51) - 1], dtype=np.uint64)
    a = np.concatenate([pows, sub, sub | np.uint64(1 << 63)]).view(np.float64)
    return [repr(float(x)) for x in a]


def _nest(elems, sizes):
    """'[[..],[..],..]' with rows of the given sizes, cycled until the elements run out."""
    rows, i, k = [], 0, 0
    while i < len(elems):
        rows.append(elems[i:i + sizes[k % len(sizes)]])
        i += len(rows[-1])
        k += 1
    return "[" + ",".join("[" + ",".join(r) + "]" for r in rows) + "]", rows


def _values(elems):
    """float() of each element; "-0" is the integer 0 and so +0.0, as json2pb (and json.loads) make it."""
    return np.array([0.0 if e == "-0" else float(e) for e in elems], dtype=np.float64)


@pytest.mark.parametrize("source", ["mixed", "powers"])
def test_flat_values_are_float_of_each_element(native, source):
    elems = _mixed(1500, seed=1) if source == "mixed" else _powers_and_subnormals()
    want = _values(elems)
    for depth, text in ((0, ",".join(elems)), (1, "[" + ",".join(elems) + "]"), (1, " [ " + " ,\n".join(elems) + "\t]\r\n")):
        err, got_depth, count, rows, bad, out, classes, row_ends = native.json_parse_number_text(text.encode(), FLOAT64)
        assert (err, got_depth, count, rows, bad, row_ends) == (0, depth, len(elems), 0, NONE, [])
        assert out == want.tobytes() and classes == b""
        err, _, count, _, _, out32, _, _ = native.json_parse_number_text(text.encode(), FLOAT32)
        with np.errstate(all="ignore"):
            assert (err, count) == (0, len(elems)) and out32 == want.astype(np.float32).tobytes()
    # numbers mode is the separator twin's payload and classes
    text = ",".join(elems).encode()
    payload, want_cls = native.json_parse_numbers(text)
    err, _, _, _, _, out, classes, _ = native.json_parse_number_text(text, NUMBERS)
    assert err == 0 and out == payload and classes == want_cls


@pytest.mark.parametrize("sizes", [[1], [3], [300], [1, 5, 2, 64, 3]])
def test_rows_are_json_loads(native, sizes):
    elems = _mixed(700, seed=len(sizes)) + _powers_and_subnormals()[::40]
    text, rows = _nest(elems, sizes)
    loaded = json.loads(text)
    assert [len(r) for r in loaded] == [len(r) for r in rows]
    for t in (text, text.replace(",", " ,\n ").replace("[", "[ ").replace("]", "\t]")):
        err, depth, count, nrows, bad, out, _, row_ends = native.json_parse_number_text(t.encode(), FLOAT64)
        assert (err, depth, count, nrows, bad) == (0, 2, len(elems), len(rows), NONE)
        assert row_ends == list(np.cumsum([len(r) for r in rows]))
        # json.loads makes ints of integer literals and inf of overflows: float() of both is the double
        assert out == np.array([float(v) for r in loaded for v in r], dtype=np.float64).tobytes()
        assert out == _values(elems).tobytes()
    err, _, _, _, bad, _, _, _ = native.json_parse_number_text(text.encode(), FLOAT64, True, False)
    assert (err, bad) == (1, 0)  # no room for row ends: nested text is refused


def test_empty_texts(native):
    for t, depth in ((b"", 0), (b" \t\r\n ", 0), (b"[]", 1), (b" [\n] ", 1)):
        assert native.json_parse_number_text(t, NUMBERS) == (0, depth, 0, 0, NONE, b"", b"", [])


MALFORMED = [
    (b"[[],[1]]", 0), (b"[[1],[]]", 1), (b"[[]]", 0), (b"[[[1]]]", 0), (b"[1,2", 1), (b"[1", 0), (b"1,2]", 1),
    (b"[1,2]]", 1), (b"[[1,2],[3]", 2), (b"[[1,2]],[3]]", 1), (b"[1,[2]]", 1), (b"[[1],2]", 1), (b"[1],[2]", 0),
    (b"[[1][2]]", 0), (b'["NaN"]', 0), (b'1,"NaN",3', 1), (b"1,2,", 2), (b"[1,2,]", 2), (b",1", 0), (b",,,,", 0),
    (b"1,,2", 1), (b"1.", 0), (b"1,2,01", 2), (b"1 2", 0), (b"[1,2] x", 1), (b"x[1,2]", 0), (b"[1,]2]", 1),
    (b'1,1.,"NaN"', 1), (b"[1,2]\x00", 1), (b"{}", 0), (b"[1,null]", 1), (b"[true]", 0), (b"[1,+2]", 1),
    (b"[0x10]", 0), (b"[1,2e]", 1), (b"[[1,2],[3,4],]", 4), (b"[ [1] [2] ]", 0),
]


@pytest.mark.parametrize("text,first_bad", MALFORMED)
def test_malformed_text_is_refused_at_its_piece(native, text, first_bad):
    for mode in (NUMBERS, FLOAT64, FLOAT32):
        err, _, count, _, bad, out, classes, row_ends = native.json_parse_number_text(text, mode)
        assert (err, bad) == (1, first_bad)
        assert count == text.count(b",") + 1 and (out, classes, row_ends) == (b"", b"", [])
    # the same piece is blamed far into a long text, after and before good ones
    good = ",".join(_mixed(900, seed=5)).encode()
    if not text.startswith((b"[", b"x", b"{", b" ", b",")) and not text.endswith((b"]", b"x", b"\x00", b",")):
        err, _, _, _, bad, _, _, _ = native.json_parse_number_text(good + b"," + text + b"," + good, FLOAT64)
        assert (err, bad) == (1, 900 + first_bad)


def test_json_agrees_on_what_is_malformed(native):
    """Every malformed case (bare text wrapped in brackets first) is either
    no JSON at all or JSON that is no array of numbers / of non-empty arrays
    of numbers."""
    def number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool)

    def numbers(v):
        if not isinstance(v, list):
            return False
        return all(number(x) for x in v) or all(isinstance(r, list) and r and all(number(x) for x in r) for r in v)

    for text, _ in MALFORMED:
        t = text if text.lstrip()[:1] in (b"[", b"{", b"x") else b"[" + text + b"]"
        try:
            value = json.loads(t.decode("latin-1"))
        except ValueError:
            continue
        assert not numbers(value), text


def test_inexact_leaves_class_3_where_the_exact_route_is_needed(native):
    longer = "0." + "3" * native.json_max_device_number_chars()
    elems = _mixed(300, seed=2)
    elems[7] = elems[290] = longer
    text = ("[" + ",".join(elems) + "]").encode()
    err, _, count, _, _, out, classes, _ = native.json_parse_number_text(text, NUMBERS, False)
    assert err == 0 and count == 300
    assert [i for i, c in enumerate(classes) if c == NEEDS_EXACT] == [7, 290]
    assert out[56:64] == bytes(8)
    err, _, _, _, _, out, classes, _ = native.json_parse_number_text(text, NUMBERS)
    assert err == 0 and classes[7] == DOUBLE and out[56:64] == struct.pack("<d", float(longer))
    # shortest-printed normals never need it
    rng = np.random.default_rng(3)
    a = rng.standard_normal(5000)
    text = native.json_format_floats(a.tobytes(), 9)
    err, _, count, _, _, out, classes, _ = native.json_parse_number_text(text, NUMBERS, False)
    assert (err, count) == (0, 5000) and NEEDS_EXACT not in set(classes) and out == a.tobytes()
    assert native.json_parse_number_text(b"1", 3)[0] == 2  # a mode there is not
