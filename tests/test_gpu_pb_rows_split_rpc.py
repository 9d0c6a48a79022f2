"""A Batch composed on the device travels as a device attachment, is echoed,
and is split where it arrives (gpu::DeviceSplitRows on the echoed device
block): the model string in front of the rows is skipped and counted, the
values and row ends come back as they were sent, and no byte of the message
is copied to the host."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_rows_wire as W  # noqa: E402


def test_composed_batch_is_split_where_it_arrives():
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
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        ch = native.Channel(s.address)
        c0 = native.gpu.device_codec_stats()
        values, row_ends, others = ch.echo_device_rows_split(
            [(1, W.BYTES, model_t.data_ptr(), model.size)],
            (4, 2, W.FIXED32, vals_t.data_ptr(), arr.size, ends_t.data_ptr(), ends.size), 0)
        c1 = native.gpu.device_codec_stats()
    finally:
        s.stop()
    assert values == arr.tobytes()
    assert row_ends == ends.tolist()
    assert others == 1
    assert c1["split_row_jobs"] - c0["split_row_jobs"] == 1 and c1["split_rows"] - c0["split_rows"] == len(sizes)
