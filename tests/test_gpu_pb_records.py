"""Device record builder (gpu/device_codec.h DeviceBuildRecords and the
kernels behind LaunchPbRecordsBuild): several columns in HBM become the
occurrences of one repeated sub-message with several fields in HBM. Every
case compares the device's bytes with the host twin
(native.pb_serialize_records) and with pb_records_wire.reference (a numpy
serializer written from the wire rules); every destination sits in a field of
sentinel bytes. The host checks and the twin run without a GPU in
brpc_amd/csrc/tests/pb_records_unittest.cc and tests/test_pb_records_host.py."""
import json

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_records_wire as R  # noqa: E402
import pb_rows_wire as W  # noqa: E402

SENTINEL = 0xA5
GUARD = 64
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _upload(arr, dev):
    """The array's memory in HBM at its natural alignment but not at 16 bytes
    (torch's own allocations are 256-byte aligned)."""
    eb = arr.dtype.itemsize
    raw = np.frombuffer(arr.tobytes(), dtype=np.uint8)
    t = torch.zeros(eb + raw.size, dtype=torch.uint8, device=dev)
    if raw.size:
        t[eb:] = torch.from_numpy(raw.copy()).to(dev)
    assert (t.data_ptr() + eb) % 16 != 0 and (t.data_ptr() + eb) % eb == 0
    return t, t.data_ptr() + eb


def _device_columns(columns, dev, keep):
    table = []
    for c in columns:
        src_t, src = _upload(c["arr"], dev)
        keep.append(src_t)
        ends_ptr = 0
        if c["ends"] is not None:
            ends_t = torch.from_numpy(c["ends"].view(np.int32).copy()).to(dev)
            keep.append(ends_t)
            ends_ptr = ends_t.data_ptr()
        count = c.get("count", c["arr"].size)
        table.append((c["inner"], c["kind"], src if count else 0, count, ends_ptr))
    return table


def _run(native, dev, jobs):
    """jobs: dicts with number, columns (pb_records_wire.column, optionally
    with a count override), rows and optionally cap and phase (dst's 16-byte
    alignment). All jobs go into ONE call. Returns [(len, err, first_bad,
    bad_column, message bytes)] after checking the sentinels: everything
    around the message, and all of dst when err is 1, 2 or 3."""
    keep, table, bufs = [], [], []
    for j in jobs:
        cols = _device_columns(j["columns"], dev, keep)
        worst = native.gpu.device_records_worst_case(j["number"], cols, j["rows"])
        cap = j.get("cap", worst)
        phase = j.get("phase", 0)
        buf = torch.full((GUARD + 32 + max(cap, worst, 1) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        skip = (-buf.data_ptr() - GUARD) % 16 + phase  # dst = 16-byte boundary + phase
        dst = buf.data_ptr() + GUARD + skip
        assert dst % 16 == phase % 16
        bufs.append((buf, GUARD + skip, cap))
        table.append((j["number"], cols, j["rows"], dst, cap))
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    res = native.gpu.device_build_records(table, 0)
    out = []
    for (n, err, first_bad, bad_column), (buf, at, cap) in zip(res, bufs):
        host = buf.cpu().numpy()
        written = n if err in (0, 4) else 0
        assert written <= cap
        assert (host[:at] == SENTINEL).all(), "bytes in front of dst changed"
        assert (host[at + written:] == SENTINEL).all(), "bytes beyond the message changed (err %d)" % err
        out.append((n, err, first_bad, bad_column, host[at:at + written].tobytes()))
    return out


def _want(native, number, columns, rows):
    """The reference's bytes, which the host twin must write too."""
    want = R.reference(number, columns, rows)
    err, _, _, twin = native.pb_serialize_records(number, R.twin_columns(columns), rows)
    assert err == 0 and twin == want
    return want


def _check(native, dev, number, columns, rows, **more):
    (n, err, first_bad, bad_column, got), = _run(native, dev, [dict(number=number, columns=columns, rows=rows, **more)])
    want = _want(native, number, columns, rows)
    assert (err, first_bad, bad_column) == (0, NONE, NONE)
    assert n == len(want)
    assert got == want
    return got


def _sizes(rng, rows, count):
    """`rows` row lengths that sum to count, about a third of them 0."""
    w = rng.random(rows) * (rng.integers(0, 3, rows) > 0)
    w[rng.integers(0, rows)] += 1e-3
    return rng.multinomial(count, w / w.sum())


def _five(rng, rows, counts, seed):
    """int64 ids (packed varints), float32 weights (packed), a blob (bytes), an
    int32 label and a double score (scalars)."""
    ids, weights, blob = counts
    return [R.column(1, 3, W.values(3, ids, seed), np.cumsum(_sizes(rng, rows, ids))),
            R.column(2, W.FIXED32, W.values(W.FIXED32, weights, seed + 1), np.cumsum(_sizes(rng, rows, weights))),
            R.column(3, 0, W.values(0, rows, seed + 2)),
            R.column(4, W.BYTES, W.values(W.BYTES, blob, seed + 3), np.cumsum(_sizes(rng, rows, blob))),
            R.column(5, W.FIXED64, W.values(W.FIXED64, rows, seed + 4))]


# per-column counts at the chunk edges (2048 elements) and two chunks and one
# element, over row counts at the row-block edge (256 rows)
@pytest.mark.parametrize("rows,counts", [(255, (2047, 2048, 2049)), (256, (2048, 2049, 4097)),
                                         (257, (2049, 4097, 2047)), (257, (4097, 2047, 2048))])
def test_five_columns_at_chunk_and_row_block_edges(native, dev, tmp_path, rows, counts):
    rng = np.random.default_rng(rows * 7 + counts[0])
    cols = _five(rng, rows, counts, 300 + counts[0])
    got = _check(native, dev, 4, cols, rows)
    # columns in ascending field number: the host serializer writes the same
    wire, _, _ = R.host_wire(native, tmp_path, 4, cols, rows)
    assert got == wire


@pytest.mark.parametrize("kind", [0, 3, 5, W.BYTES, W.FIXED32])
def test_rows_that_start_at_a_group_edge(native, dev, kind):
    """Rows that start at elements 63, 64, 65, 127, 128, 129 of a column: the
    bytes before them are a group prefix plus 63, 0 or 1 element sizes."""
    sizes = [63, 1, 1, 62, 1, 1, 64, 63, 65, 0, 129]
    cols = [R.column(1, kind, W.values(kind, sum(sizes), 50 + kind), np.cumsum(sizes)),
            R.column(2, 2, W.values(2, len(sizes), 60 + kind)),
            R.column(3, 4, W.values(4, 2 * 64, 70 + kind).view(np.uint64), np.cumsum([64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64]))]
    _check(native, dev, 16, cols, len(sizes))


@pytest.mark.parametrize("rows", [16, 17])
def test_sixteen_and_seventeen_rows_meet_one_chunk(native, dev, rows):
    """A chunk that meets 16 rows leaves segment by segment, one that meets
    17 element by element; so do the scalar columns' chunks of 16 and 17
    elements."""
    rng = np.random.default_rng(rows)
    sizes = 1 + rng.multinomial(1900 - rows, np.ones(rows) / rows)  # no empty row: all of them meet the chunk
    cols = []
    for c, kind in enumerate((3, W.FIXED32, W.BYTES, 0, 6, W.FIXED64)):
        cols.append(R.column(c + 1, kind, W.values(kind, int(sizes.sum()), 80 + c), np.cumsum(sizes)))
    for c, kind in enumerate((0, 5, 6, W.FIXED32, W.FIXED64)):
        cols.append(R.column(c + 7, kind, W.values(kind, rows, 90 + c)))
    _check(native, dev, 4, cols[:6], rows)
    _check(native, dev, 4, cols[6:], rows)
    _check(native, dev, 4, cols[4:8] + cols[:4], rows)


def test_length_varints_grow_at_127_and_16383(native, dev):
    """Sub-message sizes of 127, 128, 16383 and 16384 bytes (a bytes field and
    a scalar bool), in both orders and between records of other sizes."""
    want_sizes = [127, 128, 1, 16383, 16384, 128, 127]
    blobs = [123, 124, 0, 16378, 16379, 124, 123]  # + tag + a length of 1 or 2 bytes + the bool's two bytes
    cols = [R.column(1, W.BYTES, W.values(W.BYTES, sum(blobs), 5), np.cumsum(blobs)),
            R.column(2, 6, np.ones(len(blobs), dtype=np.uint8))]
    want_sizes[2] = 4  # the empty blob is written: tag 0x00
    assert [len(s) for s in R.reference_records(9, cols, len(blobs))] == want_sizes
    _check(native, dev, 9, cols, len(blobs))
    # the same sizes out of packed varints: 125 one-byte elements + tag + length = 127
    ones = [125, 126, 0, 16380, 16381]
    cols = [R.column(1, 3, np.ones(sum(ones), dtype=np.int64), np.cumsum(ones))]
    assert [len(s) for s in R.reference_records(9, cols, len(ones))] == [127, 128, 0, 16383, 16384]
    _check(native, dev, 9, cols, len(ones))


@pytest.mark.parametrize("empty", [(0,), (3,), (6,), (0, 1, 5, 6), (0, 1, 2, 3, 4, 5, 6)])
def test_records_whose_fields_are_all_omitted(native, dev, empty):
    """Only packed columns, and records without an element in any of them:
    tag 0x00, first, in the middle, last, and all of them."""
    rows = 7
    cols = []
    for c, kind in enumerate((3, W.FIXED32, 6)):
        sizes = np.array([3 + c, 70, 1, 2, 64, 5, 9])
        sizes[list(empty)] = 0
        cols.append(R.column(c + 1, kind, W.values(kind, int(sizes.sum()), 20 + c), np.cumsum(sizes)))
    got = _check(native, dev, 4, cols, rows)
    subs = R.reference_records(4, cols, rows)
    assert [len(s) == 0 for s in subs] == [r in empty for r in range(rows)]
    if len(empty) == rows:
        assert got == b"\x22\x00" * rows


def test_a_packed_column_without_any_element(native, dev):
    rows = 300
    rng = np.random.default_rng(11)
    cols = _five(rng, rows, (0, 700, 0), 400)
    _check(native, dev, 4, cols, rows)
    _check(native, dev, 4, cols[:1], rows)  # nothing but omitted fields: no chunk at all
    _check(native, dev, 4, [cols[3]], rows)  # and nothing but empty blobs


def test_one_record(native, dev):
    rng = np.random.default_rng(12)
    _check(native, dev, 2047, _five(rng, 1, (5000, 1, 0), 500), 1)
    _check(native, dev, 1, [R.column(2**29 - 1, 0, np.array([-1], dtype=np.int32))], 1)


def test_every_dst_alignment_in_one_call(native, dev):
    """Sixteen jobs in one call, dst at every phase of a 16-byte unit; the
    sentinels in front of dst and behind len stay (checked in _run)."""
    rng = np.random.default_rng(13)
    jobs = []
    for phase in range(16):
        rows = 20 + phase
        jobs.append(dict(number=4, columns=_five(rng, rows, (300 + phase, 2100, 900 - phase), 600 + phase), rows=rows,
                         phase=phase))
    for j, (n, err, first_bad, bad_column, got) in zip(jobs, _run(native, dev, jobs)):
        want = _want(native, j["number"], j["columns"], j["rows"])
        assert (err, first_bad, bad_column) == (0, NONE, NONE)
        assert n == len(want) and got == want


def test_eight_columns_are_built_and_nine_refused(native, dev):
    rows = 40
    rng = np.random.default_rng(14)
    cols = []
    for c in range(9):
        kind = (3, W.FIXED32, W.BYTES, 0, 5, 6, W.FIXED64, 1, 2)[c]
        if c % 3 == 0:
            cols.append(R.column(c + 1, kind, W.values(kind, rows, 700 + c)))
        else:
            cols.append(R.column(c + 1, kind, W.values(kind, 500, 700 + c), np.cumsum(_sizes(rng, rows, 500))))
    _check(native, dev, 4, cols[:8], rows)
    (n, err, _, _, got), = _run(native, dev, [dict(number=4, columns=cols, rows=rows, cap=1 << 16)])
    assert (n, err, got) == (0, 2, b"")
    assert native.gpu.device_records_worst_case(4, [(c + 1, 0, 0, rows, 0) for c in range(9)], rows) == 0


def test_good_refused_short_and_malformed_jobs_in_one_call(native, dev):
    rng = np.random.default_rng(15)
    rows = 300
    good = dict(number=4, columns=_five(rng, rows, (2500, 900, 1200), 800), rows=rows)
    refused = dict(number=0, columns=_five(rng, 5, (10, 10, 10), 810), rows=5, cap=4096)
    short_cols = _five(rng, rows, (900, 2500, 100), 820)
    need = len(R.reference(4, short_cols, rows))
    short = dict(number=4, columns=short_cols, rows=rows, cap=need - 1)
    five = _five(rng, rows, (1200, 1300, 1400), 830)
    bad_cols = [five[0], five[1], five[3], five[2], five[4]]  # tables in columns 0, 1 and 2
    ends = bad_cols[2]["ends"].copy()
    assert ends[199] >= 1
    ends[200] = ends[199] - 1  # row 200 of column 2 ends before it starts; row 201 is fine again
    bad_cols[2] = dict(bad_cols[2], ends=ends)
    bad = dict(number=4, columns=bad_cols, rows=rows)
    other = dict(number=5, columns=_five(rng, 17, (100, 0, 50), 840), rows=17, phase=3)
    stats0 = native.gpu.device_codec_stats()

    res = _run(native, dev, [good, refused, short, bad, other])
    want = _want(native, 4, good["columns"], rows)
    assert res[0] == (len(want), 0, NONE, NONE, want)
    assert res[1] == (0, 2, NONE, NONE, b"")
    assert res[2] == (need, 3, NONE, NONE, b"")  # dst still the sentinel fill (checked in _run)
    assert res[3][1:] == (1, 200, 2, b"")
    other_want = _want(native, 5, other["columns"], 17)
    assert res[4] == (len(other_want), 0, NONE, NONE, other_want)
    # the twin names the same offender
    assert native.pb_serialize_records(4, R.twin_columns(bad_cols), rows)[:3] == (1, 200, 2)
    stats1 = native.gpu.device_codec_stats()
    assert stats1["built_record_jobs"] - stats0["built_record_jobs"] == 2
    assert stats1["built_records"] - stats0["built_records"] == rows + 17
    assert stats1["built_record_bytes"] - stats0["built_record_bytes"] == len(want) + len(other_want)
    assert stats1["build_errors"] - stats0["build_errors"] == 3

    # then a lower row in column 1 is bad as well; and, in a job of its own,
    # a last entry beyond the column's count
    ends1 = bad_cols[1]["ends"].copy()
    assert ends1[7] >= 1
    ends1[8] = ends1[7] - 1
    both = list(bad_cols)
    both[1] = dict(bad_cols[1], ends=ends1)
    assert native.pb_serialize_records(4, R.twin_columns(both), rows)[:3] == (1, 8, 1)
    tail_cols = list(good["columns"])
    tail = tail_cols[0]["ends"].copy()
    tail[-1] += 1
    tail_cols[0] = dict(tail_cols[0], ends=tail)
    res = _run(native, dev, [dict(number=4, columns=both, rows=rows), good,
                             dict(number=4, columns=tail_cols, rows=rows)])
    assert res[0][1:] == (1, 8, 1, b"")
    assert res[1] == (len(want), 0, NONE, NONE, want)
    assert res[2][1:] == (1, rows - 1, 0, b"")


@pytest.mark.parametrize("kind", sorted(W.KINDS))
def test_one_column_equals_the_row_builder(native, dev, kind):
    # both sides run the same kernels (a rows job is a one-column record job);
    # the independent check of the rows is the host twin in test_gpu_pb_rows.py
    sizes = [0, 3, 0, 0, 2045, 1, 2, 700, 0, 64, 63, 65, 0]
    arr = W.values(kind, sum(sizes), 200 + kind)
    ends = np.cumsum(sizes).astype(np.uint32)
    got = _check(native, dev, 2047, [R.column(16, kind, arr, ends)], len(sizes))
    src_t, src = _upload(arr, dev)
    ends_t = torch.from_numpy(ends.view(np.int32).copy()).to(dev)
    cap = native.gpu.device_rows_worst_case(2047, 16, kind, arr.size, len(sizes))
    out = torch.full((cap,), SENTINEL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    (n, err, _), = native.gpu.device_build_rows(
        [(2047, 16, kind, src, arr.size, ends_t.data_ptr(), len(sizes), out.data_ptr(), cap)], 0)
    assert err == 0
    assert out[:n].cpu().numpy().tobytes() == got


def test_the_splitter_returns_each_records_sub_message(native, dev):
    """The built message through device_split_rows(number, inner 0, kind
    bytes): every record comes back as its sub-message's bytes. (With the
    records' own inner numbers the splitter answers 6: several fields.)"""
    from brpc_amd.ops import pb as P
    rng = np.random.default_rng(16)
    rows = 300
    cols = _five(rng, rows, (2100, 800, 1500), 900)
    got = _check(native, dev, 4, cols, rows)
    msg = torch.from_numpy(np.frombuffer(got, dtype=np.uint8).copy()).to(dev)
    values, row_ends = P.pb_split_rows(msg, 4, "bytes")
    subs = R.reference_records(4, cols, rows)
    assert values.cpu().numpy().tobytes() == b"".join(subs)
    assert row_ends.cpu().numpy().tolist() == np.cumsum([len(s) for s in subs]).tolist()
    with pytest.raises(ValueError, match="host parser"):
        P.pb_split_rows(msg, 4, "int64", inner=1)


def test_pb_build_records_from_the_json_parsers_outputs(native, dev, tmp_path):
    """ops.pb.pb_build_records fed with what json_parse_int_rows,
    json_parse_float_rows(ragged=True) and json_unescape_string_rows return,
    unchanged; the dynamic parser reads the batch back."""
    from brpc_amd import ops
    rng = np.random.default_rng(17)
    rows = 120
    ids = [[int(x) for x in rng.integers(-2**40, 2**40, int(n))] for n in rng.integers(1, 40, rows)]
    weights = [[float(x) / 8 for x in rng.integers(-2**20, 2**20, int(n))] for n in rng.integers(1, 30, rows)]
    blobs = ["blob %d é \"%s\"" % (r, "x" * int(rng.integers(0, 50))) for r in range(rows)]
    blobs[5] = ""
    labels = rng.integers(-5, 5, rows).astype(np.int32)

    def text(doc):
        return torch.from_numpy(np.frombuffer(json.dumps(doc).encode(), dtype=np.uint8).copy()).to(dev)

    id_values, id_ends = ops.json_parse_int_rows(text(ids), ragged=True)
    w_values, w_ends = ops.json_parse_float_rows(text(weights), dtype=torch.float32, ragged=True)
    b_values, b_ends = ops.json_unescape_string_rows(text(blobs))
    label_t = torch.from_numpy(labels).to(dev)
    msg = ops.pb_build_records(4, [(1, id_values, id_ends, "int64"), (2, w_values, w_ends, "float32"),
                                   (3, label_t, None, "int32"), (4, b_values, b_ends, "bytes")])
    got = msg.cpu().numpy().tobytes()
    raw = [b.encode() for b in blobs]
    cols = [R.column(1, 3, np.array(sum(ids, []), dtype=np.int64), np.cumsum([len(r) for r in ids])),
            R.column(2, W.FIXED32, np.array(sum(weights, []), dtype=np.float32), np.cumsum([len(r) for r in weights])),
            R.column(3, 0, labels),
            R.column(4, W.BYTES, np.frombuffer(b"".join(raw), dtype=np.uint8), np.cumsum([len(b) for b in raw]))]
    assert got == _want(native, 4, cols, rows)
    (tmp_path / "b.proto").write_text(R.proto_text(4, cols))
    ok, err, back = native.json_proto_from_wire(str(tmp_path), "b.proto", "Batch", got, bytes_to_base64=True)
    assert ok, err
    examples = json.loads(back)["examples"]
    assert len(examples) == rows
    assert [int(x) for x in examples[7]["f1"]] == ids[7]
    assert examples[7]["f2"] == weights[7]
    assert [e["f3"] for e in examples] == labels.tolist()

    # equal rows from a 2-D tensor, a scalar column from a 1-D one, and the error text of a bad table
    grid = torch.arange(12, dtype=torch.int32, device=dev).reshape(4, 3)
    msg = ops.pb_build_records(2, [(1, grid, None, "sint32"), (2, grid[:, 0].contiguous(), None, "int32")])
    cols = [R.column(1, 2, np.arange(12, dtype=np.int32), [3, 6, 9, 12]),
            R.column(2, 0, np.arange(0, 12, 3, dtype=np.int32))]
    assert msg.cpu().numpy().tobytes() == R.reference(2, cols, 4)
    down = torch.tensor([3, 2, 12, 12], dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match=r"row 1, column 1"):
        ops.pb_build_records(2, [(2, grid[:, 0].contiguous(), None, "int32"), (1, grid, down, "sint32")])
    with pytest.raises(ValueError, match="holds 3 records"):
        ops.pb_build_records(2, [(1, grid, None, "sint32"), (2, grid[0].contiguous(), None, "int32")])
