"""JSON number arrays parsed on the device (gpu::DeviceParseNumberArrays,
json_number_array_kernel; gpu::ParseNumbersOnDevice behind json2pb).
Everything is compared byte for byte with the host twin
native.json_parse_numbers, which
brpc_amd/csrc/tests/decimal_to_double_unittest.cc pins to strtod and
tests/test_json_float_parse.py to Python's float()."""
import math
import random
import struct
from fractions import Fraction

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

NUMBERS, FLOAT64, FLOAT32 = 0, 1, 2
INT64, UINT64, DOUBLE, NEEDS_EXACT = 0, 1, 2, 3
BLOCK = 256       # elements per workgroup
LDS_SPAN = 16384  # gpu/json_kernels.hip kIntSpan
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


def _mixed(n, seed=0):
    """Elements of 1 to 25 characters side by side, every class among them."""
    pattern = ["1", "-1.2345678901234567e-0006", "0.5", "-0", "1e300", "18446744073709551615", "2.5E+0", "-0.0",
               "123456.0", "9223372036854775807", "4.9e-324", "0.1234567890123456789", "-7", "1e22", "3.4028235e38",
               "-9223372036854775808", "1.7976931348623157e308", "6", "1e-400", "0.000001"]
    rng = random.Random(seed)
    out = [pattern[i % len(pattern)] for i in range(n)]
    for i in range(0, n, 7):
        out[i] = repr(rng.gauss(0.0, 1.0))
    assert max(len(t) for t in pattern) == 25 and min(len(t) for t in pattern) == 1
    return out


def _join(elems, pad=0):
    return (",".join(" " * pad + e for e in elems)).encode()


def _seps(text):
    """Separator offsets of bare text: -1 (before the first byte), the commas, the end."""
    a = np.frombuffer(text, dtype=np.uint8)
    return np.concatenate([[-1], np.nonzero(a == 0x2C)[0], [len(text)]]).astype(np.int64)


def _twin_as(native, text, mode):
    """What the device must write in `mode`, from the host twin."""
    payload, classes = native.json_parse_numbers(text)
    p = np.frombuffer(payload, dtype=np.uint64)
    c = np.frombuffer(classes, dtype=np.uint8)
    if mode == NUMBERS:
        return p, c
    d = np.where(c == DOUBLE, p.view(np.float64), np.where(c == UINT64, p.astype(np.float64), p.view(np.int64).astype(np.float64)))
    if mode == FLOAT64:
        return d.view(np.uint64), c
    with np.errstate(all="ignore"):
        return d.astype(np.float32).view(np.uint32), c


def _run(native, dev, jobs, redo_cap=8):
    """jobs: [(text bytes, mode)] in one launch -> [(err, first_bad, n_redo, out, classes, redo)] as numpy."""
    keep, args = [], [[] for _ in range(8)]
    for text, mode in jobs:
        seps = _seps(text)
        n = len(seps) - 1
        t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
        s = torch.from_numpy(seps.astype(np.uint32).view(np.int32)).to(dev)
        out = torch.full((n,), 0x5A5A5A5A if mode == FLOAT32 else 0x5A5A5A5A5A5A5A5A,
                         dtype=torch.int32 if mode == FLOAT32 else torch.int64, device=dev)
        cls = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        redo = torch.full((max(redo_cap, 1),), -1, dtype=torch.int32, device=dev)
        keep.append((t, s, out, cls, redo))
        for lst, v in zip(args, [t.data_ptr(), s.data_ptr(), n, mode, out.data_ptr(),
                                 cls.data_ptr() if mode == NUMBERS else 0, redo.data_ptr() if redo_cap else 0, redo_cap]):
            lst.append(v)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_json_parse_numbers(*args, 0)
    out = []
    for (err, bad, n_redo), (t, s, o, cls, redo) in zip(res, keep):
        o = o.cpu().numpy()
        out.append((err, bad, n_redo, o.view(np.uint32) if o.dtype == np.int32 else o.view(np.uint64), cls.cpu().numpy(),
                    redo.cpu().numpy().view(np.uint32)))
    return out


@pytest.mark.parametrize("mode", [NUMBERS, FLOAT64, FLOAT32])
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1])
def test_counts_and_mixed_lengths(native, dev, mode, n):
    text = _join(_mixed(n, seed=n))
    want, want_cls = _twin_as(native, text, mode)
    (err, bad, n_redo, out, cls, _), = _run(native, dev, [(text, mode)])
    assert (err, bad, n_redo) == (0, NONE, 0)
    assert out.tobytes() == want.tobytes()
    if mode == NUMBERS:
        assert cls.tobytes() == want_cls.tobytes()
    else:
        assert bool((cls == 0xEE).all())  # typed modes write no classes


def test_span_beyond_the_lds_window_next_to_a_staged_one(native, dev):
    """The first workgroup's 256 elements carry about 80 spaces each (over
    20 KiB: read from memory directly), the second workgroup's are bare (LDS)."""
    elems = _mixed(2 * BLOCK, seed=3)
    text = _join(elems[:BLOCK], pad=80) + b"," + _join(elems[BLOCK:])
    assert len(_join(elems[:BLOCK], pad=80)) > LDS_SPAN > len(_join(elems[BLOCK:]))
    for mode in (NUMBERS, FLOAT64, FLOAT32):
        want, want_cls = _twin_as(native, text, mode)
        (err, bad, n_redo, out, cls, _), = _run(native, dev, [(text, mode)])
        assert (err, bad, n_redo) == (0, NONE, 0)
        assert out.tobytes() == want.tobytes()
        if mode == NUMBERS:
            assert cls.tobytes() == want_cls.tobytes()
    # whitespace of every kind on both sides
    text = b" 1.5\t,\n-2 ,\r\n 3e2 \t\t"
    (err, _, _, out, cls, _), = _run(native, dev, [(text, NUMBERS)])
    assert err == 0 and list(cls) == [DOUBLE, INT64, DOUBLE]
    assert out.tobytes() == _twin_as(native, text, NUMBERS)[0].tobytes()


def test_mixed_classes_and_negative_zero(native, dev):
    text = b"1,-0,-0.0,9223372036854775807,9223372036854775808,18446744073709551615,18446744073709551616,-9223372036854775808,-9223372036854775809,0.5,1e400,-1e-400"
    want, want_cls = _twin_as(native, text, NUMBERS)
    assert list(want_cls) == [INT64, INT64, DOUBLE, INT64, UINT64, UINT64, DOUBLE, INT64, DOUBLE, DOUBLE, DOUBLE, DOUBLE]
    (n_res, f64_res, f32_res) = _run(native, dev, [(text, NUMBERS), (text, FLOAT64), (text, FLOAT32)])
    assert n_res[:3] == (0, NONE, 0) and f64_res[:3] == (0, NONE, 0) and f32_res[:3] == (0, NONE, 0)
    assert n_res[3].tobytes() == want.tobytes() and n_res[4].tobytes() == want_cls.tobytes()
    assert n_res[3][1] == 0 and n_res[3][2] == 1 << 63  # -0 the integer, -0.0 the double
    f64 = f64_res[3].view(np.float64)
    assert f64_res[3].tobytes() == _twin_as(native, text, FLOAT64)[0].tobytes()
    assert f64_res[3][1] == 0 and f64_res[3][2] == 1 << 63  # "-0" is +0.0, as json2pb makes it
    assert f64[4] == 2.0 ** 63 and f64[5] == 2.0 ** 64 and f64[7] == -2.0 ** 63 and math.isinf(f64[10])
    assert f32_res[3].tobytes() == _twin_as(native, text, FLOAT32)[0].tobytes()


def _round_trip_values(width):
    rng = np.random.default_rng(width)
    if width == 64:
        bits = rng.integers(0, 2 ** 64, 4096, dtype=np.uint64)
        pows = (np.arange(1, 2047, dtype=np.uint64) << np.uint64(52))  # the 2046 powers of two
        sub = np.array([1, 2, 3, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 51), (1 << 51) - 1], dtype=np.uint64)
        a = np.concatenate([bits, pows, sub, sub | np.uint64(1 << 63)]).view(np.float64)
    else:
        bits = rng.integers(0, 2 ** 32, 4096, dtype=np.uint32)
        pows = (np.arange(1, 255, dtype=np.uint32) << np.uint32(23))
        sub = np.concatenate([np.array([1, 2, 3, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 1 << 22], dtype=np.uint32),
                              np.uint32(1) << np.arange(23, dtype=np.uint32)])  # every subnormal power of two
        a = np.concatenate([bits, pows, sub, sub | np.uint32(1 << 31)]).view(np.float32)
    return a[np.isfinite(a)]


@pytest.mark.parametrize("width", [32, 64])
def test_round_trip_with_the_printer(native, dev, width):
    from brpc_amd import ops
    a = _round_trip_values(width)
    assert len(a) > 4000
    t = torch.from_numpy(a.copy()).to(dev)
    text = ops.json_print_floats(t)
    back = ops.json_parse_floats(text, dtype=t.dtype)
    assert back.dtype == t.dtype and back.shape == t.shape
    assert back.cpu().numpy().tobytes() == a.tobytes()
    # a float's text read as doubles, then narrowed: numpy's astype
    if width == 32:
        as_double = ops.json_parse_floats(text, dtype=torch.float64).cpu().numpy()
        assert as_double.astype(np.float32).tobytes() == a.tobytes()
    bracketed = torch.cat([torch.tensor([0x5B], dtype=torch.uint8, device=dev), text,
                           torch.tensor([0x5D], dtype=torch.uint8, device=dev)])
    assert ops.json_parse_floats(bracketed, dtype=t.dtype).cpu().numpy().tobytes() == a.tobytes()
    assert ops.json_parse_floats(torch.empty(0, dtype=torch.uint8, device=dev)).numel() == 0


def test_float32_mode_is_the_narrowed_double(native, dev):
    rng = random.Random(32)
    elems = []
    for _ in range(2000):
        d = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if d == d and abs(d) != float("inf"):
            # in and around the float range, float subnormals and halves among them
            elems.append("%.17g" % math.ldexp(math.frexp(d)[0], rng.randrange(-160, 135)))
    elems += ["3.4028235677973366e38", "3.4028235677973362e38", "7.006492321624085e-46", "7.006492321624086e-46",
              "1.1754943508222875e-38", "1.1754942807573643e-38", "1e39", "-1e39", "1e-46", "16777217", "16777219"]
    text = _join(elems)
    (_, f64_res, f32_res) = _run(native, dev, [(text, NUMBERS), (text, FLOAT64), (text, FLOAT32)])
    assert f64_res[:3] == (0, NONE, 0) and f32_res[:3] == (0, NONE, 0)
    with np.errstate(all="ignore"):
        want = f64_res[3].view(np.float64).astype(np.float32)
    assert f32_res[3].tobytes() == want.tobytes()
    assert f64_res[3].tobytes() == np.array([float(e) for e in elems]).tobytes()


def _three_undecided(native):
    """Three 30-digit numbers the host twin reports as needing exact
    arithmetic: the 19-digit truncation and its successor straddle the point
    halfway between two doubles. Searched, not listed."""
    found = []
    rng = random.Random(30)
    while len(found) < 3:
        # a double, the exact halfway point above it, 30 of its digits
        d = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(62) | (1 << 61)))[0]
        if not (1e-300 < d < 1e300):
            continue
        mid = (Fraction(d) + Fraction(math.nextafter(d, math.inf))) / 2
        e10 = math.floor(math.log10(d))
        digits = str(int(mid * Fraction(10) ** (29 - e10)))
        if len(digits) != 30:
            continue
        t = "%s.%se%d" % (digits[0], digits[1:], e10)
        _, classes = native.json_parse_numbers(t.encode(), False)
        if classes[0] == NEEDS_EXACT:
            found.append(t)
    return found


def test_redo_list(native, dev):
    undecided = _three_undecided(native)
    assert len(undecided) == 3 and all(len(t.split("e")[0]) == 31 for t in undecided)
    elems = _mixed(BLOCK + 40, seed=9)
    where = [5, BLOCK - 1, BLOCK + 17]
    for i, t in zip(where, undecided):
        elems[i] = t
    text = _join(elems)
    _, classes = native.json_parse_numbers(text, False)
    assert [i for i, c in enumerate(classes) if c == NEEDS_EXACT] == where
    want, want_cls = _twin_as(native, text, NUMBERS)
    (err, bad, n_redo, out, cls, redo), = _run(native, dev, [(text, NUMBERS)])
    assert (err, bad, n_redo) == (0, NONE, 3)
    assert sorted(redo[:3].tolist()) == where
    keep = np.ones(len(elems), dtype=bool)
    keep[where] = False
    assert out[keep].tobytes() == want[keep].tobytes() and cls[keep].tobytes() == want_cls[keep].tobytes()
    assert bool((out[where] == 0x5A5A5A5A5A5A5A5A).all()) and bool((cls[where] == 0xEE).all())  # nothing written
    # through the host entry point the three are repaired: the exact values
    payload, got_cls, redone = native.gpu.json_parse_numbers(text, 0)
    assert redone == 3
    assert payload == want.tobytes() and got_cls == want_cls.tobytes()
    for i in where:
        assert payload[8 * i:8 * i + 8] == struct.pack("<d", float(elems[i]))
    # a list too short: err 3, the count still 3
    (err, bad, n_redo, _, _, redo), = _run(native, dev, [(text, NUMBERS)], redo_cap=2)
    assert (err, bad, n_redo) == (3, NONE, 3)
    assert set(redo[:2].tolist()) <= set(where)
    (err, _, n_redo, _, _, _), = _run(native, dev, [(text, FLOAT64)], redo_cap=0)
    assert (err, n_redo) == (3, 3)
    # an element longer than a lane reads lands on the list
    longer = "0." + "3" * native.json_max_device_number_chars()
    text = _join(["1.5", longer, "2"])
    (err, bad, n_redo, out, cls, redo), = _run(native, dev, [(text, NUMBERS)])
    assert (err, bad, n_redo) == (0, NONE, 1) and redo[0] == 1
    payload, got_cls, redone = native.gpu.json_parse_numbers(text, 0)
    assert redone == 1 and payload[8:16] == struct.pack("<d", float(longer)) and list(got_cls) == [DOUBLE, DOUBLE, INT64]
    # the op repairs them too
    from brpc_amd import ops
    t = torch.from_numpy(np.frombuffer(_join(elems), dtype=np.uint8).copy()).to(dev)
    got = ops.json_parse_floats(t).cpu().numpy()
    assert got.tobytes() == _twin_as(native, _join(elems), FLOAT64)[0].tobytes()


@pytest.mark.parametrize("at", [0, BLOCK - 1, BLOCK, 2 * BLOCK + 9])
def test_malformed_element(native, dev, at):
    from brpc_amd import ops
    elems = _mixed(2 * BLOCK + 10, seed=at)
    assert at < len(elems) and 2 * BLOCK + 9 == len(elems) - 1
    elems[at] = "1."
    text = _join(elems)
    (err, bad, _, _, _, _), = _run(native, dev, [(text, NUMBERS)])
    assert (err, bad) == (1, at)
    with pytest.raises(ValueError):
        native.gpu.json_parse_numbers(text, 0)
    with pytest.raises(ValueError, match="element %d " % at):
        ops.json_parse_floats(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev))
    if at + 300 < len(elems):  # a second one further on: the lower index is reported
        elems[at + 300] = '"NaN"'
        (err, bad, _, _, _, _), = _run(native, dev, [(_join(elems), FLOAT32)])
        assert (err, bad) == (1, at)


def test_refused_before_any_launch(native, dev):
    text = torch.from_numpy(np.frombuffer(b"1.5,2.5", dtype=np.uint8).copy()).to(dev)
    seps = torch.tensor([-1, 3, 7], dtype=torch.int32, device=dev)
    out = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
    cls = torch.full((8,), 0xEE, dtype=torch.uint8, device=dev)

    def code(mode, out_ptr, cls_ptr=0, text_ptr=None, count=2):
        (err, bad, n_redo), = native.gpu.device_json_parse_numbers(
            [text.data_ptr() if text_ptr is None else text_ptr], [seps.data_ptr()], [count], [mode], [out_ptr],
            [cls_ptr], [0], [0], 0)
        assert (bad, n_redo) == (NONE, 0)
        return err

    assert code(FLOAT64, 0) == 2                                  # null out
    assert code(3, out.data_ptr(), cls.data_ptr()) == 2           # bad mode
    assert code(FLOAT64, out.data_ptr() + 4) == 2                 # misaligned for a double
    assert code(FLOAT32, out.data_ptr() + 2) == 2                 # misaligned for a float
    assert code(NUMBERS, out.data_ptr()) == 2                     # numbers without classes
    assert code(FLOAT64, out.data_ptr(), text_ptr=0) == 2         # null text
    assert code(FLOAT64, out.data_ptr(), count=(1 << 32) - 1) == 2
    torch.cuda.synchronize(dev)
    assert bool((out == 0xEE).all()) and bool((cls == 0xEE).all())
    assert code(FLOAT64, out.data_ptr()) == 0
    assert bytes(out[:16].cpu().numpy()) == struct.pack("<2d", 1.5, 2.5)
    assert code(FLOAT64, out.data_ptr(), count=0) == 0            # empty: nothing to parse


def test_json2pb_float_arrays_end_to_end(native, dev):
    """With the GPU JSON path on and the float threshold low, the fs and ds
    arrays of a body are parsed by the device after the integer offload
    declined them, to the same message as with the GPU path off; an array
    with a quoted "NaN" and a flag of 0 stay on the host."""
    rng = np.random.default_rng(5000)
    fs = rng.standard_normal(5000).astype(np.float32)
    ds = rng.standard_normal(5000)
    ds[17], ds[18] = 5e-324, -1.7976931348623157e308
    f_text, d_text = native.json_format_floats(fs.tobytes(), 8).decode(), native.json_format_floats(ds.tobytes(), 9).decode()
    body = ('{"name":"e","fs":[%s],"ds":[%s]}' % (f_text, d_text)).encode()
    with_nan = ('{"name":"e","fs":[1.5,2.5],"ds":[%s,"NaN"]}' % d_text).encode()
    want = native.json_to_pb_to_json("mrpc.test.FloatArrays", body)
    want_nan = native.json_to_pb_to_json("mrpc.test.FloatArrays", with_nan)
    assert want == body.decode()
    before = native.get_flag("gpu_json2pb_float_min_elems")
    native.set_flag("gpu_json2pb_float_min_elems", "8")
    native.gpu.enable_json_index(0, 1024)
    keys = ("number_arrays", "number_elems", "number_array_fallbacks", "number_redo_elems", "int_arrays",
            "int_array_fallbacks")
    try:
        j0 = native.gpu.json_stats()
        assert native.json_to_pb_to_json("mrpc.test.FloatArrays", body) == want
        j1 = native.gpu.json_stats()
        assert j1["indexed_bodies"] - j0["indexed_bodies"] == 1, (j0, j1)
        assert j1["number_arrays"] - j0["number_arrays"] == 2, (j0, j1)
        assert j1["number_elems"] - j0["number_elems"] == 10000, (j0, j1)
        assert j1["int_array_fallbacks"] - j0["int_array_fallbacks"] == 2, (j0, j1)  # still tried first
        assert j1["number_array_fallbacks"] == j0["number_array_fallbacks"]
        # a quoted string breaks the run of plain elements: the host parses
        # that array and no counter moves for it (fs is below both thresholds)
        assert native.json_to_pb_to_json("mrpc.test.FloatArrays", with_nan) == want_nan
        j2 = native.gpu.json_stats()
        assert j2["indexed_bodies"] - j1["indexed_bodies"] == 1
        assert all(j2[k] == j1[k] for k in keys), (j1, j2)
        # the flag is read at every call: 0 hands every array back to the host
        native.set_flag("gpu_json2pb_float_min_elems", "0")
        assert native.json_to_pb_to_json("mrpc.test.FloatArrays", body) == want
        j3 = native.gpu.json_stats()
        assert all(j3[k] == j2[k] for k in keys if k.startswith("number_")), (j2, j3)
    finally:
        native.gpu.disable_json_index()
        native.set_flag("gpu_json2pb_float_min_elems", str(before))
