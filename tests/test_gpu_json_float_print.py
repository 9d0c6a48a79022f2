"""Float / double arrays printed as JSON text on the device
(gpu::DevicePrintFloatArrays, json_float_size_kernel / json_float_place_kernel;
gpu::PrintFloatsOnDevice behind pb2json). Everything is compared byte for
byte with the host printer native.json_format_floats, which
brpc_amd/csrc/tests/shortest_double_unittest.cc pins to the element-wise
oracle."""
import math
import os

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT, DOUBLE = 8, 9
CHUNK = 256  # gpu/kernels.h kJsonFloatChunkElems
KINDS = {FLOAT: np.float32, DOUBLE: np.float64}


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


def _mixed(n, kind, seed=0):
    """Text lengths from 3 to 25 bytes side by side: a wrong prefix sum shows
    up as shifted text."""
    tiny = 1e-40 if kind == FLOAT else 5e-324  # subnormal in either width
    big = 1e30 if kind == FLOAT else 1e300
    pattern = [1.0, 0.1234567890123456789, big, -0.0, tiny, -1.2345678901234567e-6, 2.5, -tiny * 3, 123456.0, 1e22]
    rng = np.random.default_rng(seed)
    a = np.array([pattern[i % len(pattern)] for i in range(n)], dtype=np.float64)
    a[::7] *= rng.standard_normal(len(a[::7]))
    return a.astype(KINDS[kind])


def _host(native, a):
    kind = FLOAT if a.dtype == np.float32 else DOUBLE
    return native.json_format_floats(a.tobytes(), kind)


def _print(ops, a, dev):
    return bytes(ops.json_print_floats(torch.from_numpy(a).to(dev)).cpu().numpy())


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1])
def test_counts_and_mixed_lengths(native, dev, kind, n):
    from brpc_amd import ops
    a = _mixed(n, kind, seed=n)
    assert _print(ops, a, dev) == _host(native, a)


def test_power_of_two_exceptions(native, dev):
    """The doubles on which the oracle's rule (smallest p whose correctly
    rounded p-digit decimal converts back) prints more digits than the
    shortest decimal that converts back (Python's repr): found here through
    the oracle, all in one array."""
    from brpc_amd import ops
    pows = [math.ldexp(1.0, e) for e in range(-1022, 1024)]
    assert len(pows) == 2046

    def digits(text):  # significant digits of a decimal
        return len(text.lstrip("-").split("e")[0].replace(".", "").strip("0")) or 1

    odd = [d for d in pows if digits(native.json_shortest_double(d).decode()) > digits(repr(d))]
    assert len(odd) == 46, len(odd)
    assert math.ldexp(1.0, -1017) in odd
    a = np.array(odd, dtype=np.float64)
    got = _print(ops, a, dev)
    assert got == b",".join(native.json_shortest_double(d) for d in odd)
    assert b"7.1202363472230444e-307" in got.split(b",")
    # and every power of two, the other 2000 included
    a = np.array(pows, dtype=np.float64)
    assert _print(ops, a, dev) == _host(native, a)


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
def test_non_finite_first_and_last(native, dev, kind):
    """The last element of a full chunk is the array's last: no trailing
    comma after a quoted string."""
    from brpc_amd import ops
    for n in (2 * CHUNK, 2):
        a = _mixed(n, kind)
        a[n // 2] = np.inf
        a[0] = np.nan
        a[-1] = -np.inf
        got = _print(ops, a, dev)
        assert got == _host(native, a)
        assert got.startswith(b'"NaN",') and got.endswith(b',"-Infinity"')


def _launch(native, dev, tensors, caps=None, dsts=None):
    outs = [torch.full((native.gpu.json_float_worst_case(max(t.numel(), 1)) + 64,), 0xEE, dtype=torch.uint8, device=dev)
            for t in tensors]
    kinds = [FLOAT if t.dtype == torch.float32 else DOUBLE for t in tensors]
    caps = caps or [o.numel() for o in outs]
    torch.cuda.synchronize(dev)
    res = native.gpu.device_json_print_floats([t.data_ptr() for t in tensors], [t.numel() for t in tensors], kinds,
                                              dsts or [o.data_ptr() for o in outs], caps, 0)
    return res, outs


def test_two_jobs_of_different_kinds_and_an_empty_one(native, dev):
    f = _mixed(3 * CHUNK + 17, FLOAT, seed=1)
    d = _mixed(CHUNK + 5, DOUBLE, seed=2)
    tf, td = torch.from_numpy(f).to(dev), torch.from_numpy(d).to(dev)
    empty = torch.empty(0, dtype=torch.float64, device=dev)
    res, outs = _launch(native, dev, [tf, empty, td])
    want_f, want_d = _host(native, f), _host(native, d)
    assert [tuple(r) for r in res] == [(len(want_f), 0), (0, 0), (len(want_d), 0)]
    assert bytes(outs[0][:len(want_f)].cpu().numpy()) == want_f
    assert bytes(outs[2][:len(want_d)].cpu().numpy()) == want_d
    assert int(outs[0][len(want_f)]) == 0xEE and int(outs[2][len(want_d)]) == 0xEE  # nothing past the text
    assert bool((outs[1] == 0xEE).all())


def test_count_zero_gives_an_empty_result(native, dev):
    from brpc_amd import ops
    for dt in (torch.float32, torch.float64):
        out = ops.json_print_floats(torch.empty(0, dtype=dt, device=dev))
        assert out.numel() == 0 and out.dtype == torch.uint8
    assert native.gpu.json_print_floats(b"", 0, DOUBLE, 0) == b""


def test_cap_one_byte_short(native, dev):
    a = _mixed(2 * CHUNK + 3, DOUBLE, seed=3)
    want = _host(native, a)
    t = torch.from_numpy(a).to(dev)
    res, outs = _launch(native, dev, [t], caps=[len(want) - 1])
    assert tuple(res[0]) == (len(want), 3)
    assert bool((outs[0] == 0xEE).all())  # dst untouched
    res, outs = _launch(native, dev, [t], caps=[len(want)])
    assert tuple(res[0]) == (len(want), 0)
    assert bytes(outs[0][:len(want)].cpu().numpy()) == want


def test_refused_before_any_launch(native, dev):
    a = torch.from_numpy(_mixed(CHUNK, DOUBLE)).to(dev)
    as_bytes = a.view(torch.uint8)
    out = torch.full((8192,), 0xEE, dtype=torch.uint8, device=dev)
    cases = [
        (as_bytes[4:].data_ptr(), 8, DOUBLE, out.data_ptr()),   # misaligned for a double
        (as_bytes[2:].data_ptr(), 8, FLOAT, out.data_ptr()),    # misaligned for a float
        (0, 8, DOUBLE, out.data_ptr()),                         # null src
        (a.data_ptr(), 8, DOUBLE, 0),                           # null dst
        (a.data_ptr(), 8, 3, out.data_ptr()),                   # not a float kind
        (a.data_ptr(), (1 << 32) // 26 + 1, DOUBLE, out.data_ptr()),  # worst case above 2^32 - 1
    ]
    for src, count, kind, dst in cases:
        res = native.gpu.device_json_print_floats([src], [count], [kind], [dst], [out.numel()], 0)
        assert tuple(res[0]) == (0, 2), (src, count, kind, dst, res)
    torch.cuda.synchronize(dev)
    assert bool((out == 0xEE).all())


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
def test_view_at_an_aligned_offset(native, dev, kind):
    from brpc_amd import ops
    a = _mixed(2 * CHUNK + 40, kind, seed=4)
    t = torch.from_numpy(a).to(dev)
    for off in (1, 3, 37):  # element offsets: aligned for the element, not for 16-byte loads
        view = t[off:off + CHUNK + 9]
        assert view.data_ptr() == t.data_ptr() + off * t.element_size()
        assert bytes(ops.json_print_floats(view).cpu().numpy()) == _host(native, a[off:off + CHUNK + 9])


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
def test_host_values_through_the_device(native, dev, kind):
    a = _mixed(5 * CHUNK + 11, kind, seed=5)
    assert native.gpu.json_print_floats(a.tobytes(), len(a), kind, 0) == _host(native, a)


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _float_arrays_wire(fs, ds):
    """mrpc.test.FloatArrays (brpc_amd/proto/json_arrays.proto)."""
    wire = b"\x0a\x01e"  # name = "e"
    if len(fs):
        wire += b"\x12" + _varint(4 * len(fs)) + fs.astype("<f4").tobytes()
    if len(ds):
        wire += b"\x1a" + _varint(8 * len(ds)) + ds.astype("<f8").tobytes()
    return wire


def _to_json(native, wire, pretty=False):
    ok, err, out = native.json_proto_from_wire(os.path.join(ROOT, "brpc_amd", "proto"), "json_arrays.proto",
                                               "mrpc.test.FloatArrays", wire, False, pretty)
    assert ok, err
    return out


def test_pb2json_float_fields_end_to_end(native, dev):
    """With the GPU JSON path on and the float threshold low, a message's
    float and double fields are printed by the device, to the same bytes as
    with the offload disabled; pretty output and short arrays stay on the
    host and leave the counters alone."""
    fs, ds = _mixed(3000, FLOAT, seed=6), _mixed(2000, DOUBLE, seed=7)
    fs[5], ds[1999] = np.inf, np.nan
    wire = _float_arrays_wire(fs, ds)
    small = _float_arrays_wire(fs[:100], ds[:99])
    want, want_small, want_pretty = _to_json(native, wire), _to_json(native, small), _to_json(native, wire, True)
    assert want == '{"name":"e","fs":[' + _host(native, fs).decode() + '],"ds":[' + _host(native, ds).decode() + "]}"
    before = native.get_flag("gpu_pb2json_float_min_elems")
    native.set_flag("gpu_pb2json_float_min_elems", "1000")
    native.gpu.enable_json_index(0, 65536)
    try:
        j0 = native.gpu.json_stats()
        assert _to_json(native, wire) == want
        j1 = native.gpu.json_stats()
        assert j1["pb2json_float_arrays"] - j0["pb2json_float_arrays"] == 2, (j0, j1)
        assert j1["pb2json_float_elems"] - j0["pb2json_float_elems"] == 5000, (j0, j1)
        assert j1["pb2json_failures"] == j0["pb2json_failures"]
        assert _to_json(native, wire, True) == want_pretty
        assert _to_json(native, small) == want_small
        j2 = native.gpu.json_stats()
        assert j2["pb2json_float_arrays"] == j1["pb2json_float_arrays"]
        assert j2["pb2json_float_elems"] == j1["pb2json_float_elems"]
        # the flag is read at every call: 0 hands every array back to the host printer
        native.set_flag("gpu_pb2json_float_min_elems", "0")
        assert _to_json(native, wire) == want
        assert native.gpu.json_stats()["pb2json_float_arrays"] == j1["pb2json_float_arrays"]
    finally:
        native.gpu.disable_json_index()
        native.set_flag("gpu_pb2json_float_min_elems", str(before))
