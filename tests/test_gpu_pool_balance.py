"""Pool balance of the offload entry points in brpc_amd/csrc/gpu: every call
holds its pooled pinned / HBM blocks through the owners of gpu/scoped.h, so
after a warm-up call 50 more calls leave the HBM pool with the live blocks
and bytes it had and take no new pinned region, on the success paths and on
the paths that decline (an error code or ValueError) alike. The calls run on
the calling thread with the same shapes: the per-thread caches and the slab
regions have their steady size after the warm-up."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

FLOAT, DOUBLE = 8, 9
CALLS = 50


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


def _balanced(native, call, calls=CALLS):
    call()  # warm-up
    before = native.gpu.hbm_pool_stats(0)
    for _ in range(calls):
        call()
    after = native.gpu.hbm_pool_stats(0)
    assert after["live_blocks"] == before["live_blocks"], (before, after)
    assert after["live_bytes"] == before["live_bytes"], (before, after)
    assert after["pinned_bytes"] <= before["pinned_bytes"], (before, after)


def _floats(n):
    return [repr(0.37 * i - 40.0) for i in range(n)]


@pytest.mark.parametrize("kind", [FLOAT, DOUBLE])
def test_json_print_floats(native, dev, kind):
    a = (np.arange(257) * 0.37 - 40.0).astype(np.float32 if kind == FLOAT else np.float64)  # two 256-element chunks
    want = native.json_format_floats(a.tobytes(), kind)

    def call():
        assert native.gpu.json_print_floats(a.tobytes(), len(a), kind, 0) == want

    _balanced(native, call)


def test_json_parse_numbers(native, dev):
    text = ("[" + ",".join(_floats(257)) + "]").encode()  # two 256-element blocks
    want = native.json_parse_numbers(text)

    def call():
        payload, classes, redone = native.gpu.json_parse_numbers(text, 0)
        assert (payload, classes) == tuple(want) and redone == 0

    _balanced(native, call)


def test_json_parse_numbers_declined(native, dev):
    elems = _floats(257)
    elems[200] = "1."
    text = ("[" + ",".join(elems) + "]").encode()

    def call():
        with pytest.raises(ValueError):
            native.gpu.json_parse_numbers(text, 0)

    _balanced(native, call)


@pytest.mark.parametrize("direct", [True, False])
def test_json_index_bytes(native, dev, direct):
    from brpc_amd.ops.json import json_index_host
    body = b"[" + b",".join(b'{"id":%d,"tag":"t%d","ok":true}' % (i, i % 7) for i in range(700)) + b"]"
    assert 20 * 1024 <= len(body) < 32 * 1024  # two 16 KiB tiles
    want = json_index_host(body)[0]

    def call():
        assert native.gpu.json_index_bytes(body, 0) == want

    native.set_flag("json_index_direct_host", "true" if direct else "false")
    try:
        _balanced(native, call)
    finally:
        native.set_flag("json_index_direct_host", "true")


def test_device_json_print_floats_error_codes(native, dev):
    a = np.arange(257, dtype=np.float64) * 0.37 - 40.0
    want = native.json_format_floats(a.tobytes(), DOUBLE)
    t = torch.from_numpy(a).to(dev)
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)  # torch fills/copies run on its own stream

    def call():
        # a cap one byte short (3) beside a kind that is refused before any launch (2)
        res = native.gpu.device_json_print_floats([t.data_ptr(), t.data_ptr()], [len(a), len(a)], [DOUBLE, 7],
                                                  [out.data_ptr(), out.data_ptr()], [len(want) - 1, out.numel()], 0)
        assert [tuple(r) for r in res] == [(len(want), 3), (0, 2)], res

    _balanced(native, call)


def test_crc32c_sync(native, dev):
    t = torch.arange(4096, dtype=torch.int32, device=dev).to(torch.uint8)
    torch.cuda.synchronize(dev)
    want = native.crc32c(bytes(t.cpu().numpy().tobytes()))

    def call():
        assert native.gpu.crc32c_sync(t.data_ptr(), t.numel(), 0) == want

    _balanced(native, call)


def test_device_decode_packed_truncated_run(native, dev):
    wire = bytearray()
    for v in range(1000):
        v *= 977
        while v >= 0x80:
            wire.append((v & 0x7F) | 0x80)
            v >>= 7
        wire.append(v)
    wire[-1] |= 0x80  # ends inside a varint
    src = torch.frombuffer(wire, dtype=torch.uint8).to(dev)
    dst = torch.zeros(8 * 1000, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def call():
        [(_, code)] = native.gpu.device_decode_packed([src.data_ptr()], [len(wire)], [4], [dst.data_ptr()], 0)
        assert code == 1

    _balanced(native, call)


def test_gpu_snappy_offload_round_trip(native, dev):
    """The set-up of test_gpu_snappy.py::test_gpu_snappy_offload_is_standard_snappy, one body."""
    data = b"abcdefgh" * 8192
    native.gpu.enable_snappy(0, 1024, packed_only=False)
    try:
        def call():
            c = native.compress(1, data)
            assert native.snappy_uncompress(c) == data
            assert native.decompress(1, c) == data

        _balanced(native, call, calls=5)
    finally:
        native.gpu.disable_snappy()


def test_press_echo_through_the_gpu_handler(native, dev):
    """The handler leg of test_gpu_resident.py over the default copy engine:
    the same press again, once the first one's server and client are gone,
    leaves the pool where the first one left it."""
    import gc
    from brpc_amd.models import start_echo_server

    def call():
        srv = start_echo_server("127.0.0.1:0", gpu_device=0)
        try:
            p = native.Press({"server": srv.address, "concurrency": 8, "attachment_size": 65536, "gpu_device": 0,
                              "check_echo": True, "gpu_process": True})
            p.run_requests(200)
            st = p.stats()
            assert st["success"] == 200 and st["error"] == 0, st
            del p
            gc.collect()
        finally:
            srv.stop()

    _balanced(native, call, calls=1)
