"""Device-built attachments on the RPC path (Press option device_build_ids):
every call's attachment is serialized ON THE DEVICE from a body and int64 ids
that live in HBM (gpu::BuildDeviceMessage), lent to the server, echoed, and
compared byte for byte with what the host serializer makes of the same
EchoRequest; the reply's packed ids are located by its device field table and
decoded on the device."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("compress", [0, 1])
def test_device_built_attachments_echo(dev, compress):
    from brpc_amd import native
    from brpc_amd.models import start_echo_server
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        c0 = native.gpu.device_codec_stats()
        p = native.Press({"server": s.address, "concurrency": 16, "attachment_size": 16384,
                          "attachment_body": "text", "device_attachment": True, "device_build_ids": 4000,
                          "device_scan": True, "device_compress": compress, "gpu_device": 0, "check_echo": True})
        p.run_requests(500)
        st = p.stats()
        # every reply was byte-equal to the host serializer's output
        assert st["success"] == 500 and st["error"] == 0, st
        c1 = native.gpu.device_codec_stats()
        assert c1["built_messages"] - c0["built_messages"] == 500, (c0, c1)
        assert c1["build_errors"] == c0["build_errors"]
        # device replies had field 8 decoded on the device; the connection's
        # first window travels over TCP while the hello is in flight, and
        # those replies are host-accessible and checked on the host
        assert c1["packed_runs"] - c0["packed_runs"] >= 450, (c0, c1)
        assert c1["packed_errors"] == c0["packed_errors"]
    finally:
        s.stop()
