"""A Batch composed on the device travels as a device attachment: the block
gpu::BuildDeviceMessage makes of the scalar field and the block
gpu::BuildDeviceRows makes of the ragged rows are appended to one Buf
(protobuf concatenation is merge), lent to the echo server, and arrive
byte-equal to the host serialization of the same batch."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_rows_wire as W  # noqa: E402


def test_composed_batch_echoes_byte_equal():
    from brpc_amd import native
    from brpc_amd.models import start_echo_server
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda", 0)
    sizes = [5, 0, 2100, 1, 0, 300]
    arr = W.values(W.FIXED32, sum(sizes), 21)
    ends = np.cumsum(sizes).astype(np.int32)
    model = np.frombuffer(b"model-7", dtype=np.uint8)
    vals_t = torch.from_numpy(arr.copy()).to(dev)
    ends_t = torch.from_numpy(ends.copy()).to(dev)
    model_t = torch.from_numpy(model.copy()).to(dev)
    torch.cuda.synchronize()
    want = b"\x0a" + W.varint(model.size) + model.tobytes() + W.reference(4, 2, W.FIXED32, arr, ends)
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        ch = native.Channel(s.address)
        c0 = native.gpu.device_codec_stats()
        got = ch.echo_device_rows([(1, W.BYTES, model_t.data_ptr(), model.size)],
                                  (4, 2, W.FIXED32, vals_t.data_ptr(), arr.size, ends_t.data_ptr(), ends.size), 0)
        c1 = native.gpu.device_codec_stats()
    finally:
        s.stop()
    assert got == want
    assert c1["built_row_jobs"] - c0["built_row_jobs"] == 1 and c1["built_messages"] - c0["built_messages"] == 1
