"""pb::SerializeRows (native.pb_serialize_rows), the host twin of the device
row builder: its bytes equal what the project's own host serializer makes of
the same batch given as JSON against a .proto written at run time, and what
this directory's numpy serializer (pb_rows_wire.reference) writes from the
wire rules."""
import pytest

np = pytest.importorskip("numpy")

import pb_rows_wire as W  # noqa: E402


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _twin(native, number, inner, kind, arr, ends):
    err, first_bad, wire = native.pb_serialize_rows(number, inner, kind, arr.tobytes(), [int(e) for e in ends])
    assert err == 0 and first_bad == 0xFFFFFFFF
    return wire


def test_the_batch_of_the_issue(native, tmp_path):
    """{"rows":[{"v":[1.5,2.25]},{},{"v":[0.125]}]} as repeated Row rows = 4
    with repeated float v = 2 [packed]."""
    arr = np.array([1.5, 2.25, 0.125], dtype=np.float32)
    ends = [2, 2, 3]
    (tmp_path / "b.proto").write_text(W.proto_text(W.FIXED32, 4, 2))
    _, wire, back = native.json_proto_roundtrip(str(tmp_path), "b.proto", "Batch",
                                                b'{"rows":[{"v":[1.5,2.25]},{},{"v":[0.125]}]}')
    assert wire.hex() == "220a12080000c03f00001040" "2200" "22061204" "0000003e"
    assert _twin(native, 4, 2, W.FIXED32, arr, ends) == wire


@pytest.mark.parametrize("kind,inner", [(k, 2) for k in sorted(W.KINDS)] + [(W.BYTES, 0)])
def test_every_kind_equals_the_host_serializer(native, tmp_path, kind, inner):
    rng = np.random.default_rng(kind * 7 + inner)
    sizes = [0, 0, 1, 5, 0, 129, 0, 3, 700, 1, 0]
    arr = W.values(kind, sum(sizes), 40 + kind)
    ends = np.cumsum(sizes)
    number = int(rng.choice([1, 15, 16, 2047, 2048, 2**29 - 1]))
    wire, _, _ = W.host_wire(native, tmp_path, kind, number, inner, arr, ends)
    got = _twin(native, number, inner, kind, arr, ends)
    assert got == wire
    assert got == W.reference(number, inner, kind, arr, ends)


def test_header_lengths_step_in_separate_rows(native):
    """Payloads of 125..129 and 16381..16385 bytes: the inner length grows a
    row earlier than the outer one at both varint steps."""
    sizes = [125, 126, 127, 128, 129, 16381, 16382, 16383, 16384, 16385]
    arr = W.values(W.BYTES, sum(sizes), 3)
    ends = np.cumsum(sizes)
    for inner in (0, 1, 16):
        assert _twin(native, 2047, inner, W.BYTES, arr, ends) == W.reference(2047, inner, W.BYTES, arr, ends)


def test_bad_tables_and_refusals(native):
    arr = np.arange(10, dtype=np.int32)
    assert native.pb_serialize_rows(1, 2, 0, arr.tobytes(), [3, 2, 10])[:2] == (1, 1)
    assert native.pb_serialize_rows(1, 2, 0, arr.tobytes(), [3, 9])[:2] == (1, 1)
    assert native.pb_serialize_rows(1, 2, 0, arr.tobytes(), [3, 11])[:2] == (1, 1)
    for number, inner, kind, ends in [(0, 2, 0, [10]), (2**29, 2, 0, [10]), (1, 2**29, 0, [10]), (1, 0, 0, [10]),
                                      (1, 2, 0, [])]:
        err, _, wire = native.pb_serialize_rows(number, inner, kind, arr.tobytes(), ends)
        assert err == 2 and wire == b""
    with pytest.raises(ValueError):
        native.pb_serialize_rows(1, 2, 10, arr.tobytes(), [10])
