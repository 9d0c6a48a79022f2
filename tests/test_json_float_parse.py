"""The JSON number parser (base/decimal_to_double.h) behind json::Reader's
packed number arrays, against an independent oracle: Python's float() is
correctly rounded. The C++ side (strtod, std::from_chars, the DOM) is in
brpc_amd/csrc/tests/decimal_to_double_unittest.cc."""
import importlib.util
import json
import os
import random
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64, UINT64, DOUBLE, NEEDS_EXACT = 0, 1, 2, 3

HARD = [
    "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "1.8e308", "1e400", "-1e+400",
    "2.4703282292062327e-324", "2.4703282292062328e-324", "4.9e-324", "2.2250738585072011e-308",
    "2.2250738585072014e-308", "2.225073858507201e-308", "9007199254740993.0", "9007199254740995.0",
    "9007199254740992.5", "0e999999999999", "1e-999999999999", "-0.0", "0.0", "1e23", "8.41e21", "1e22", "1e-22",
    "3.4028235677973366e38", "1.401298464324817e-45", "7.006492321624085e-46", "123456789012345678901234567890.5",
    "0.1000000000000000055511151231257827021181583404541015625", "1.00000000000000011102230246251565404236316680908203125",
    "1.00000000000000011102230246251565404236316680908203124", "1.00000000000000011102230246251565404236316680908203126",
    "18446744073709551616", "-9223372036854775809", "100000000000000000000", "179769313486231570000e288",
]


def _bits(x):
    return struct.pack("<d", x)


def _texts(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        kind = rng.randrange(6)
        if kind == 0:  # the digits of a double, 1 to 17 of them
            d = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
            if d != d or d in (float("inf"), float("-inf")):
                continue
            out.append("%.*e" % (rng.randrange(17), d))
        elif kind == 1:
            out.append(repr(rng.gauss(0.0, 1.0)))
        elif kind == 2:  # digits of no double in particular, up to 40 of them
            digits = "".join(rng.choice("0123456789") for _ in range(rng.randrange(1, 40)))
            out.append("%s%d.%se%d" % (rng.choice(["", "-"]), rng.randrange(1, 10), digits, rng.randrange(-330, 310)))
        elif kind == 3:  # plain decimals
            out.append("%s%d.%0*d" % (rng.choice(["", "-"]), rng.randrange(10 ** rng.randrange(1, 19)),
                                      rng.randrange(1, 19), rng.randrange(10 ** 18) % 10 ** rng.randrange(1, 19)))
        elif kind == 4:  # near the ends of the range
            out.append("%d.%dE%s%d" % (rng.randrange(1, 10), rng.randrange(10 ** 16), rng.choice(["+", "-", ""]),
                                       rng.randrange(300, 330)))
        else:  # a subnormal
            d = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(52)))[0]
            out.append("%.*e" % (rng.randrange(17), d))
    return out


def test_table_generator_is_in_step_with_the_header():
    path = os.path.join(ROOT, "tools", "gen_decimal_to_double_table.py")
    spec = importlib.util.spec_from_file_location("gen_decimal_to_double_table", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.OUT) as f:
        assert f.read() == gen.render()


def test_parse_double_matches_python_float(native):
    texts = _texts(20000, 8259) + HARD
    for t in texts:
        assert _bits(native.json_parse_double(t.encode())) == _bits(float(t)), t
    assert native.json_parse_double(b"-0") == 0.0 and _bits(native.json_parse_double(b"-0")) == _bits(0.0)
    assert native.json_parse_double(b"18446744073709551615") == float(2 ** 64 - 1)
    for bad in [b"01", b"1.", b".5", b"+1", b"1e", b"1e+", b"--1", b"1.2.3", b"0x10", b"NaN", b"Infinity", b"", b" 1"]:
        with pytest.raises(ValueError):
            native.json_parse_double(bad)


def test_parse_numbers_matches_python_float(native):
    texts = _texts(20000, 950) + HARD
    payload, classes = native.json_parse_numbers(("[" + " ,\n".join(texts) + " ]").encode())
    assert len(classes) == len(texts) and len(payload) == 8 * len(texts)
    for i, t in enumerate(texts):
        assert classes[i] == DOUBLE, t
        assert payload[8 * i:8 * i + 8] == _bits(float(t)), t
    # bare text, and the integer classes
    payload, classes = native.json_parse_numbers(b"1,-0,2.5,9223372036854775807,9223372036854775808,-9223372036854775808")
    assert list(classes) == [INT64, INT64, DOUBLE, INT64, UINT64, INT64]
    assert struct.unpack("<6Q", payload) == (1, 0, struct.unpack("<Q", _bits(2.5))[0], 2 ** 63 - 1, 2 ** 63, 2 ** 63)
    with pytest.raises(ValueError, match="element 2"):
        native.json_parse_numbers(b"[1.5,2,1.,3]")
    # what a device lane hands back: decided by the exact route here
    longer = "1." + "3" * native.json_max_device_number_chars()
    _, classes = native.json_parse_numbers(("1.5,%s" % longer).encode(), False)
    assert list(classes) == [DOUBLE, NEEDS_EXACT]
    payload, classes = native.json_parse_numbers(("1.5,%s" % longer).encode())
    assert list(classes) == [DOUBLE, DOUBLE] and payload[8:] == _bits(float(longer))


def test_narrow_double_bits(native):
    np = pytest.importorskip("numpy")
    rng = np.random.default_rng(32)
    bits = rng.integers(0, 2 ** 64, 20000, dtype=np.uint64)
    bits[::2] = (bits[::2] & np.uint64(0x800FFFFFFFFFFFFF)) | (rng.integers(1023 - 160, 1023 + 140, 10000).astype(np.uint64) << np.uint64(52))
    doubles = bits.view(np.float64)
    with np.errstate(all="ignore"):
        want = doubles.astype(np.float32).view(np.uint32)
    for b, w, d in zip(bits.tolist(), want.tolist(), doubles.tolist()):
        if d == d:  # a NaN's payload is the hardware's business; the C++ suite pins it to the cast
            assert native.narrow_double_bits(b) == w, hex(b)


def test_float_arrays_round_trip_through_json2pb(native):
    rng = random.Random(5000)
    fs = [struct.unpack("<f", struct.pack("<f", rng.gauss(0.0, 1.0)))[0] for _ in range(5000)]
    ds = [rng.gauss(0.0, 1.0) for _ in range(5000)]
    ds[7], ds[8], fs[9] = 5e-324, 1.7976931348623157e308, 1.401298464324817e-45  # the smallest float
    body = '{"name":"e","fs":[%s],"ds":[%s]}' % (
        native.json_format_floats(struct.pack("<5000f", *fs), 8).decode(),
        native.json_format_floats(struct.pack("<5000d", *ds), 9).decode())
    out = native.json_to_pb_to_json("mrpc.test.FloatArrays", body.encode())
    assert out == body
    back = json.loads(out)
    assert [_bits(x) for x in back["ds"]] == [_bits(x) for x in ds]
    assert back["fs"] == fs
    # the packed route and the element-wise route give one DOM
    assert native.json_parse_check(body.encode(), True) == (True, "")
    assert native.json_parse_check(body.encode(), False) == (True, "")
    assert native.json_parse_check(b"[1.5,1e5.3]", True) == native.json_parse_check(b"[1.5,1e5.3]", False)
