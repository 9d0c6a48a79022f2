"""A Batch whose repeated element has several fields, composed on the device,
travels as a device attachment: the block gpu::BuildDeviceMessage makes of
the scalar `model` field and the block gpu::BuildDeviceRecords makes of the
columns are appended to one Buf (protobuf concatenation is merge), lent to
the echo server, and arrive byte-equal to the references of the two parts;
the host parser reads the batch back through its .proto."""
import json

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_records_wire as R  # noqa: E402
import pb_rows_wire as W  # noqa: E402


def test_composed_batch_of_records_echoes_byte_equal(tmp_path):
    from brpc_amd import native
    from brpc_amd.models import start_echo_server
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    rows = 300
    id_sizes = rng.integers(0, 30, rows)
    w_sizes = rng.integers(0, 12, rows) * (rng.integers(0, 2, rows))
    blob_sizes = rng.integers(0, 20, rows)
    cols = [R.column(1, 3, W.values(3, int(id_sizes.sum()), 32), np.cumsum(id_sizes)),
            R.column(2, W.FIXED32, W.values(W.FIXED32, int(w_sizes.sum()), 33), np.cumsum(w_sizes)),
            R.column(3, 0, W.values(0, rows, 34)),
            R.column(4, W.BYTES, W.values(W.BYTES, int(blob_sizes.sum()), 35), np.cumsum(blob_sizes))]
    model = np.frombuffer(b"model-7", dtype=np.uint8)
    keep, table = [], []
    for c in cols:
        vals_t = torch.from_numpy(c["arr"].copy()).to(dev)
        ends_t = None if c["ends"] is None else torch.from_numpy(c["ends"].view(np.int32).copy()).to(dev)
        keep += [vals_t, ends_t]
        table.append((c["inner"], c["kind"], vals_t.data_ptr() if c["arr"].size else 0, c["arr"].size,
                      0 if ends_t is None else ends_t.data_ptr()))
    model_t = torch.from_numpy(model.copy()).to(dev)
    torch.cuda.synchronize()
    want = b"\x0a" + W.varint(model.size) + model.tobytes() + R.reference(4, cols, rows)
    s = start_echo_server("127.0.0.1:0", gpu_device=0)
    try:
        ch = native.Channel(s.address)
        c0 = native.gpu.device_codec_stats()
        got = ch.echo_device_records([(1, W.BYTES, model_t.data_ptr(), model.size)], 4, table, rows, 0)
        c1 = native.gpu.device_codec_stats()
    finally:
        s.stop()
    assert got == want
    assert c1["built_record_jobs"] - c0["built_record_jobs"] == 1 and c1["built_records"] - c0["built_records"] == rows
    assert c1["built_messages"] - c0["built_messages"] == 1
    (tmp_path / "batch.proto").write_text(R.proto_text(4, cols, model_field=1))
    ok, err, back = native.json_proto_from_wire(str(tmp_path), "batch.proto", "Batch", got, bytes_to_base64=True)
    assert ok, err
    doc = json.loads(back)
    assert doc["model"] == "model-7" and len(doc["examples"]) == rows
    # the host serializer makes the same bytes of the same batch, and they print as the same JSON
    _, wire, host_back = native.json_proto_roundtrip(str(tmp_path), "batch.proto", "Batch",
                                                     R.batch_json(cols, rows, model="model-7"), base64_to_bytes=True)
    assert wire == got
    assert doc == json.loads(host_back)
