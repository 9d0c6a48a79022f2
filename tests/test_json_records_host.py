"""json::FormatRecordObjects (native.json_format_record_objects), the host twin
of the device record printer: its bytes equal what json_records_ref.reference
composes from the printers other tests pin (json_format_number_rows,
json_escape, base64_encode), Python's json module reads the text back as the
columns, and the project's own json2pb reads it as the message the record
builder's twin serializes from the same columns."""
import json

import pytest

np = pytest.importorskip("numpy")

import json_records_ref as J  # noqa: E402

NONE = J.NONE


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _twin(native, columns, rows, brackets=True):
    err, first_bad, bad_column, text = native.json_format_record_objects(J.twin_columns(columns), rows, brackets)
    assert (err, first_bad, bad_column) == (0, NONE, NONE)
    return text


def test_one_batch_by_hand(native):
    cols = [J.column("label", J.INT32, [3, -7]),
            J.column("ids", J.INT64, [1, 2], [2, 2]),
            J.column("scores", J.FLOAT, [0.5, 0.25, np.nan], [2, 3]),
            J.column("text", J.BYTES, np.frombuffer(b'a"b\n', dtype=np.uint8), [0, 4], J.STRING),
            J.column("blob", J.BYTES, np.frombuffer(b"ab", dtype=np.uint8), [2, 2], J.BASE64)]
    want = (b'[{"label":3,"ids":[1,2],"scores":[0.5,0.25],"text":"","blob":"YWI="},'
            b'{"label":-7,"ids":[],"scores":["NaN"],"text":"a\\"b\\n","blob":""}]')
    assert _twin(native, cols, 2) == want
    assert _twin(native, cols, 2, False) == want[1:-1]
    assert J.reference(native, cols, 2) == want


@pytest.mark.parametrize("seed", range(40))
def test_random_columns_equal_the_reference_and_load_back(native, seed):
    rng = np.random.default_rng(3000 + seed)
    rows = int(rng.integers(0, 60)) if seed else 0
    cols = J.random_columns(rng, rows, 1 + seed % 8, seed)
    for brackets in (True, False):
        text = _twin(native, cols, rows, brackets)
        assert text == J.reference(native, cols, rows, brackets)
    text = _twin(native, cols, rows)
    assert json.loads(text.decode("latin-1")) == J.structure(cols, rows)
    # host only: no pointer is read (a nonzero row_ends means a ragged column)
    cap = native.gpu.json_records_worst_case(
        [(c["key"], c["kind"], c["text"], 8 if c["arr"].size else 0, c["arr"].size, 0 if c["ends"] is None else 4)
         for c in cols], rows, True)
    assert len(text) <= cap < 1 << 32


def test_float32_cells_are_exact_values(native):
    a = J.values(J.FLOAT, 500, 9, nonfinite=False)
    text = _twin(native, [J.column("w", J.FLOAT, a), J.column("v", J.FLOAT, a, np.arange(1, 501))], 500)
    back = json.loads(text)
    assert [rec["w"] for rec in back] == [float(np.float32(x)) for x in a]
    assert [rec["v"] for rec in back] == [[float(np.float32(x))] for x in a]


@pytest.mark.parametrize("seed", range(30))
def test_bad_tables(native, seed):
    rng = np.random.default_rng(4000 + seed)
    rows = int(rng.integers(1, 40))
    cols = J.random_columns(rng, rows, 2 + seed % 7, seed)
    ragged = [c for c in cols if c["ends"] is not None]
    if not ragged:
        cols[0] = J.column(cols[0]["key"], J.INT64, np.arange(rows), np.arange(1, rows + 1))
        ragged = [cols[0]]
    for col in ragged[:1 + seed % 2]:  # one column, or two at once
        r = (0, rows - 1, int(rng.integers(0, rows)))[seed % 3]
        how = int(rng.integers(0, 3))
        if how == 0:
            col["ends"][r] = col["arr"].size + 1 + int(rng.integers(0, 3))
        elif how == 1 and r and col["ends"][r - 1]:
            col["ends"][r] = col["ends"][r - 1] - 1
        else:
            col["ends"][rows - 1] += 1
    bad = J.first_bad(cols, rows)
    assert bad is not None
    err, first_bad, bad_column, text = native.json_format_record_objects(J.twin_columns(cols), rows, True)
    assert (err, first_bad, bad_column, text) == (1, bad[0], bad[1], b"")


def test_keys(native):
    col = lambda key: J.column(key, J.INT32, [1])  # noqa: E731
    assert _twin(native, [col(b'q"\\\x01\x80\xff')], 1) == b'[{"q\\"\\\\\\u0001\x80\xff":1}]'
    assert len(_twin(native, [col(b"k" * 255)], 1)) == 255 + 8
    assert len(_twin(native, [col(b"k" * 249 + b"\x02")], 1)) == 255 + 8
    for key in (b"k" * 256, b"k" * 250 + b"\x02", b'"' * 128):
        assert native.json_format_record_objects(J.twin_columns([col(key)]), 1, True)[0] == 2
    assert native.json_format_record_objects(J.twin_columns([col(b"a"), col(b"b"), col(b"a")]), 1, True)[0] == 2


def test_refusals(native):
    ok = J.twin_columns([J.column("a", J.INT64, [1, 2], [1, 2])])[0]
    fmt = native.json_format_record_objects
    assert fmt([ok], 2, True)[0] == 0
    assert fmt([], 0, True)[0] == 2
    assert fmt([(b"k%d" % i,) + ok[1:] for i in range(9)], 2, True)[0] == 2
    assert fmt([(b"k%d" % i,) + ok[1:] for i in range(8)], 2, True)[0] == 0
    assert fmt([(ok[0], 10, 0) + ok[3:]], 2, True)[0] == 2           # a kind there is not
    assert fmt([(ok[0], 3, J.STRING) + ok[3:]], 2, True)[0] == 2     # a text form on a number kind
    assert fmt([(ok[0], 7, J.NUMBER) + ok[3:]], 2, True)[0] == 2     # bytes without a text form
    assert fmt([(ok[0], 7, 3) + ok[3:]], 2, True)[0] == 2            # a text form there is not
    assert fmt([(ok[0], 7, J.STRING, b"ab", None)], 2, True)[0] == 2  # bytes without row ends
    assert fmt([(ok[0], 3, 0, ok[3], None)], 3, True)[0] == 2         # a scalar column of another length


PROTO = """syntax = "proto2";
message Example {
  repeated int64 input_ids = 1 [packed = true];
  repeated float weights = 2 [packed = true];
  optional int32 label = 3;
  optional bytes blob = 4;
}
message Batch { repeated Example examples = 4; }
"""


def test_json2pb_reads_the_text_as_the_message_the_record_builder_writes(native, tmp_path):
    """Finite values only (json2pb takes no quoted NaN for a float). Rows of no
    element are in: the text says "input_ids":[] where the wire omits the
    field, and pb2json prints neither."""
    (tmp_path / "b.proto").write_text(PROTO)
    rng = np.random.default_rng(77)
    rows = 37
    id_ends = np.cumsum(rng.integers(0, 6, rows))
    w_ends = np.cumsum(rng.integers(0, 4, rows))
    blob_ends = np.cumsum(rng.integers(0, 9, rows))
    ids = J.values(J.INT64, int(id_ends[-1]), 1)
    weights = J.values(J.FLOAT, int(w_ends[-1]), 2, nonfinite=False)
    labels = J.values(J.INT32, rows, 3)
    blob = J.values(J.BYTES, int(blob_ends[-1]), 4)
    cols = [J.column("input_ids", J.INT64, ids, id_ends), J.column("weights", J.FLOAT, weights, w_ends),
            J.column("label", J.INT32, labels), J.column("blob", J.BYTES, blob, blob_ends, J.BASE64)]
    text = _twin(native, cols, rows)
    ok, err, from_json = native.json_proto_parse(str(tmp_path), "b.proto", "Batch", b'{"examples":' + text + b"}", True)
    assert ok, err
    ends = lambda e: [int(x) for x in e]  # noqa: E731
    werr, _, _, wire = native.pb_serialize_records(
        4, [(1, J.INT64, ids.tobytes(), ends(id_ends)), (2, J.FLOAT, weights.tobytes(), ends(w_ends)),
            (3, J.INT32, labels.tobytes(), None), (4, J.BYTES, blob.tobytes(), ends(blob_ends))], rows)
    assert werr == 0
    ok, err, from_wire = native.json_proto_from_wire(str(tmp_path), "b.proto", "Batch", wire, bytes_to_base64=True)
    assert ok, err
    assert from_json == from_wire
    assert len(json.loads(from_wire)["examples"]) == rows
