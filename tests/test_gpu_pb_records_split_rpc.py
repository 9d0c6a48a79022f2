"""A Batch of records composed on the device travels as a device attachment,
is echoed, and is split where it arrives (gpu::DeviceSplitRecords on the
echoed device block): the model string in front of the records is skipped and
counted, every column comes back as the twin gives it for the same bytes, and
no byte of the message is copied to the host."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_records_split_ref as S  # noqa: E402
import pb_records_wire as RW  # noqa: E402
import pb_rows_wire as W  # noqa: E402


def test_composed_records_are_split_where_they_arrive():
    from brpc_amd import native
    from brpc_amd.models import start_echo_server
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda", 0)
    rows = 300
    columns = S.make_columns(S.EXAMPLE, rows, 23, 7)
    cols = S.split_columns(columns)
    model = np.frombuffer(b"model-7", dtype=np.uint8)
    wire = S.bytes_field(1, model.tobytes()) + RW.reference(4, columns, rows)
    want = native.pb_split_records(4, cols, wire)
    assert want[0] == 0 and want[1] == rows and want[2] == 1
    keep, table = [], []
    for c in columns:
        vals = torch.from_numpy(c["arr"].copy()).to(dev)
        ends = None if c["ends"] is None else torch.from_numpy(c["ends"].astype(np.int32)).to(dev)
        keep.append((vals, ends))
        table.append((c["inner"], c["kind"], vals.data_ptr(), c["arr"].size, 0 if ends is None else ends.data_ptr()))
    model_t = torch.from_numpy(model.copy()).to(dev)
    torch.cuda.synchronize()
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        ch = native.Channel(s.address)
        c0 = native.gpu.device_codec_stats()
        got, others = ch.echo_device_records_split([(1, W.BYTES, model_t.data_ptr(), model.size)], 4, table, rows, cols, 0)
        c1 = native.gpu.device_codec_stats()
    finally:
        s.stop()
    assert others == 1
    assert [(v, e, a) for v, e, a in got] == [(c[2], c[3], c[1]) for c in want[4]]
    assert [(v, e) for v, e, _ in got] == S.expected(columns)
    assert c1["split_record_jobs"] - c0["split_record_jobs"] == 1 and c1["split_records"] - c0["split_records"] == rows
