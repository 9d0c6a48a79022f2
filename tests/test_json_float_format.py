"""The shortest round-trip double formatter (base/shortest_double.h) on the
host: its generated table, and the pb2json host printer of float / double
arrays against the element-wise oracle (json::AppendShortestDouble). The
byte-for-byte sweep over doubles lives in
brpc_amd/csrc/tests/shortest_double_unittest.cc."""
import importlib.util
import math
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT, DOUBLE = 8, 9


def _generator():
    path = os.path.join(ROOT, "tools", "gen_shortest_double_table.py")
    spec = importlib.util.spec_from_file_location("gen_shortest_double_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generated_table_equals_a_regeneration():
    gen = _generator()
    with open(gen.OUT) as f:
        committed = f.read()
    assert committed == gen.render()
    # spot checks of the definition, independent of the generator's helpers
    assert gen.pow5(0) == 1 << 124 and gen.pow5(1) == 5 << 122
    assert gen.pow5(325) == 5 ** 325 >> ((5 ** 325).bit_length() - 125)
    assert gen.pow5_inv(0) == (1 << 125) + 1
    q = 291
    assert gen.pow5_inv(q) == (1 << ((5 ** q).bit_length() - 1 + 125)) // 5 ** q + 1
    assert "{0x%016xull, 0x%016xull}," % (gen.pow5(325) & (2 ** 64 - 1), gen.pow5(325) >> 64) in committed


def _mixed():
    vals = [1.0, 2.0, -0.0, 0.0, 0.1, 123.45, 0.000123, 1.5e-7, 1e21, 1e22, 1e300, 5e-324, 2.2250738585072014e-308,
            1.7976931348623157e308, math.ldexp(1.0, -1017), 9007199254740993.0, -1.2345678901234567e-6,
            float("nan"), float("inf"), float("-inf")]
    return vals + [math.sin(i) * 10.0 ** (i % 40 - 20) for i in range(500)]


def test_format_floats_equals_joined_shortest_double(native):
    ds = _mixed()
    want = b",".join(native.json_shortest_double(d) for d in ds)
    assert native.json_format_floats(struct.pack("<%dd" % len(ds), *ds), DOUBLE) == want
    assert native.json_shortest_double(0.1) == b"0.1"
    assert native.json_shortest_double(float("nan")) == b'"NaN"'
    # floats: widened first, so 0.1f shows its float rounding error
    fs = [struct.unpack("<f", struct.pack("<f", d if abs(d) < 3e38 or d != d else math.copysign(math.inf, d)))[0]
          for d in ds]
    want_f = b",".join(native.json_shortest_double(f) for f in fs)
    got_f = native.json_format_floats(struct.pack("<%df" % len(fs), *fs), FLOAT)
    assert got_f == want_f
    assert native.json_format_floats(struct.pack("<f", 0.1), FLOAT) == b"0.10000000149011612"
    assert native.json_format_floats(b"", DOUBLE) == b""


def test_format_floats_refuses_other_kinds(native):
    import pytest
    with pytest.raises(ValueError):
        native.json_format_floats(b"\0" * 8, 3)
    with pytest.raises(ValueError):
        native.json_format_floats(b"\0" * 7, DOUBLE)
