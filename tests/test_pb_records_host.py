"""pb::SerializeRecords (native.pb_serialize_records), the host twin of the
device record builder: its bytes equal what this directory's numpy serializer
(pb_records_wire.reference) writes from the wire rules, what the project's own
host serializer makes of the same batch given as JSON against a .proto written
at run time, and, for a job of one column, what pb::SerializeRows writes."""
import json

import pytest

np = pytest.importorskip("numpy")

import pb_records_wire as R  # noqa: E402
import pb_rows_wire as W  # noqa: E402

NUMBERS = (1, 15, 16, 2047, 2048, 2**29 - 1)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _twin(native, number, columns, rows):
    err, first_bad, bad_column, wire = native.pb_serialize_records(number, R.twin_columns(columns), rows)
    assert (err, first_bad, bad_column) == (0, NONE, NONE)
    return wire


def _random_columns(rng, rows, ncols, first_kind, distinct=False):
    cols = []
    for c in range(ncols):
        kind = (first_kind + c) % 10
        inner = c + 1 if distinct else int(rng.choice(NUMBERS))
        if kind != W.BYTES and rng.integers(0, 3) == 0:
            cols.append(R.column(inner, kind, W.values(kind, rows, int(rng.integers(0, 1 << 30)))))
            continue
        sizes = rng.integers(0, 40, rows) * (rng.integers(0, 3, rows) > 0)
        if rng.integers(0, 6) == 0:
            sizes[:] = 0
        arr = W.values(kind, int(sizes.sum()), int(rng.integers(0, 1 << 30)))
        cols.append(R.column(inner, kind, arr, np.cumsum(sizes)))
    return cols


def test_the_batch_of_the_issue(native, tmp_path):
    """Two examples: ids [1, 300] / weights [1.5] / label 7 / blob "ab", then
    no ids, no weights, label 0 (written: explicit presence) and an empty
    blob (written)."""
    cols = [R.column(1, 3, np.array([1, 300], dtype=np.int64), [2, 2]),
            R.column(2, W.FIXED32, np.array([1.5], dtype=np.float32), [1, 1]),
            R.column(3, 0, np.array([7, 0], dtype=np.int32)),
            R.column(4, W.BYTES, np.frombuffer(b"ab", dtype=np.uint8), [2, 2])]
    got = _twin(native, 4, cols, 2)
    assert got.hex() == "2211" "0a0301ac02" "12040000c03f" "1807" "22026162" "2204" "1800" "2200"
    assert got == R.reference(4, cols, 2)
    wire, back, _ = R.host_wire(native, tmp_path, 4, cols, 2)
    assert got == wire
    assert json.loads(back)["examples"][0]["f1"] in ([1, 300], ["1", "300"])


@pytest.mark.parametrize("seed", range(20))
def test_random_columns_equal_the_numpy_reference(native, seed):
    """Columns of every kind and shape (packed, bytes, scalar; empty rows,
    a column without any element), one to eight of them, repeated inner
    numbers included."""
    rng = np.random.default_rng(1000 + seed)
    rows = int(rng.integers(1, 60))
    cols = _random_columns(rng, rows, 1 + seed % 8, seed)
    number = int(rng.choice(NUMBERS))
    got = _twin(native, number, cols, rows)
    assert got == R.reference(number, cols, rows)
    # host only: no pointer is read (a nonzero row_ends means a ragged column)
    cap = native.gpu.device_records_worst_case(
        number, [(c["inner"], c["kind"], 0, c["arr"].size, 0 if c["ends"] is None else 4) for c in cols], rows)
    assert cap >= len(got)


@pytest.mark.parametrize("seed", range(10))
def test_equals_the_host_serializer_and_parses_back(native, tmp_path, seed):
    """Columns in ascending field number, so the host serializer's output is
    canonical: the same bytes, and the twin's bytes parse back to the JSON
    the serializer's own bytes print as."""
    rng = np.random.default_rng(2000 + seed)
    rows = int(rng.integers(1, 30))
    cols = _random_columns(rng, rows, 1 + (seed * 3) % 8, seed, distinct=True)
    got = _twin(native, 4, cols, rows)
    wire, back, proto = R.host_wire(native, tmp_path, 4, cols, rows)
    assert got == wire
    ok, err, text = native.json_proto_from_wire(str(tmp_path), proto, "Batch", got, bytes_to_base64=True)
    assert ok, err
    assert json.loads(text) == json.loads(back)
    assert len(json.loads(text).get("examples", [])) == rows


@pytest.mark.parametrize("kind", sorted(W.KINDS))
def test_one_column_equals_the_row_twin(native, kind):
    sizes = [0, 0, 1, 5, 0, 129, 0, 3, 700, 1, 0]
    arr = W.values(kind, sum(sizes), 40 + kind)
    ends = np.cumsum(sizes)
    err, _, rows_wire = native.pb_serialize_rows(2047, 16, kind, arr.tobytes(), [int(e) for e in ends])
    assert err == 0
    got = _twin(native, 2047, [R.column(16, kind, arr, ends)], len(sizes))
    assert got == rows_wire
    assert got == W.reference(2047, 16, kind, arr, ends)


def test_length_varints_grow_at_127_and_16383(native):
    """Sub-message sizes of 127, 128, 16383 and 16384 bytes, made of a bytes
    field (tag, length, payload) and a scalar bool (two bytes)."""
    want_sizes = [127, 128, 16383, 16384]
    blobs = [123, 124, 16378, 16379]  # + tag + a length of 1 or 2 bytes + the bool's two bytes
    cols = [R.column(1, W.BYTES, W.values(W.BYTES, sum(blobs), 5), np.cumsum(blobs)),
            R.column(2, 6, np.ones(4, dtype=np.uint8))]
    assert [len(s) for s in R.reference_records(9, cols, 4)] == want_sizes
    assert _twin(native, 9, cols, 4) == R.reference(9, cols, 4)


def test_bad_tables_name_the_lowest_row_then_the_lowest_column(native):
    arr = np.arange(10, dtype=np.int32).tobytes()
    fine, down1, down2, short = [3, 5, 10], [3, 2, 10], [3, 5, 4], [3, 5, 9]

    def code(tables):
        return native.pb_serialize_records(1, [(c + 1, 0, arr, t) for c, t in enumerate(tables)], 3)

    assert code([fine, down2, down1, down1]) == (1, 1, 2, b"")
    assert code([fine, down2, short, short]) == (1, 2, 1, b"")
    assert code([fine, fine, short, down1]) == (1, 1, 3, b"")
    assert code([fine, fine, [3, 5, 11]]) == (1, 2, 2, b"")
    assert code([fine, fine, fine])[0] == 0


def test_refusals(native):
    arr = np.arange(10, dtype=np.int32).tobytes()
    good = (1, 0, arr, [3, 10])
    scalar = (2, 0, arr[:8], None)
    assert native.pb_serialize_records(1, [good, scalar], 2)[0] == 0
    assert native.pb_serialize_records(1, [(c + 1, 0, arr, [3, 10]) for c in range(8)], 2)[0] == 0
    refused = [
        (0, [good], 2), (2**29, [good], 2),                      # the repeated field's number
        (1, [(0, 0, arr, [3, 10])], 2), (1, [(2**29, 0, arr, [3, 10])], 2),  # inner
        (1, [(1, 10, arr, [3, 10])], 2),                         # kind
        (1, [(1, W.BYTES, arr[:2], None)], 2),                   # bytes have no scalar form
        (1, [], 2), (1, [(c + 1, 0, arr, [3, 10]) for c in range(9)], 2),  # 0 and 9 columns
        (1, [good, (2, 0, arr, None)], 2),                       # a scalar column of 10 elements, 2 records
        (1, [(1, 0, b"", [])], 0),                               # no record
    ]
    for number, cols, rows in refused:
        assert native.pb_serialize_records(number, cols, rows) == (2, NONE, NONE, b"")
    with pytest.raises(ValueError):
        native.pb_serialize_records(1, [(1, 0, arr, [3, 5, 10])], 2)  # a table of another length
    with pytest.raises(ValueError):
        native.pb_serialize_records(1, [(1, 0, arr[:7], [3, 10])], 2)  # half an element
