"""Records printed as JSON objects on the device
(gpu::DevicePrintRecordObjects; the json_records_* kernels). Every byte of a
sentinel-filled buffer, in front of the text and behind it too, is compared
with the host twin native.json_format_record_objects, which
tests/test_json_records_host.py pins to a composition of the pinned cell
printers and brpc_amd/csrc/tests/json_records_unittest.cc to a naive printer.
Every pointer handed over is valid for the sizes given with it."""
import json

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import json_records_ref as J  # noqa: E402

NONE = J.NONE
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def C(native):
    return native.gpu.json_records_chunk_elems()


@pytest.fixture(scope="module")
def B(native):
    return native.gpu.json_records_block_rows()


def _to_dev(a, dev):
    """The memory image of a numpy array in device memory (uint32 / uint64
    travel as bytes: not every torch has those dtypes)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


class Job:
    """One job of a call: sources and tables in device memory and a
    sentinel-filled destination whose text starts at `phase` (mod 16)."""

    def __init__(self, native, dev, cols, rows, brackets=True, phase=0, cap=None):
        self.cols, self.rows, self.brackets = cols, rows, brackets
        self.keep, self.table = [], []
        for c in cols:
            src = _to_dev(c["arr"], dev) if c["arr"].size else None
            ends = _to_dev(c["ends"], dev) if c["ends"] is not None and c["ends"].size else None
            self.keep += [src, ends]
            # a table of no rows is still a ragged column: never read, any aligned address stands for it
            ends_ptr = 0 if c["ends"] is None else (ends.data_ptr() if ends is not None else 4)
            self.table.append((c["key"], c["kind"], c["text"], src.data_ptr() if src is not None else 0,
                               int(c["arr"].size), ends_ptr))
        self.twin = native.json_format_record_objects(J.twin_columns(cols), rows, brackets)
        self.worst = native.gpu.json_records_worst_case(self.table, rows, brackets)
        self.cap = self.worst if cap is None else cap
        self.buf = torch.full((16 + phase + self.cap + 48,), SENTINEL, dtype=torch.uint8, device=dev)
        self.off = (phase - self.buf.data_ptr()) % 16

    def row(self):
        return (self.table, self.rows, self.brackets, self.buf.data_ptr() + self.off, self.cap)

    def check(self, result):
        """The device's result against the twin's, and every byte of the buffer."""
        length, err, first_bad, bad_column = result
        t_err, t_bad, t_col, t_text = self.twin
        got = bytes(self.buf.cpu().numpy())
        if t_err == 0 and len(t_text) > self.cap:
            assert (length, err, first_bad, bad_column) == (len(t_text), 3, NONE, NONE)
            t_text = b""
        else:
            assert (err, first_bad, bad_column) == (t_err, t_bad, t_col)
            assert length == len(t_text)  # 0 unless printed
            if err == 0:
                assert len(t_text) <= self.worst
        assert got[self.off:self.off + len(t_text)] == t_text
        assert got[:self.off] == bytes([SENTINEL]) * self.off  # nothing before the text
        rest = got[self.off + len(t_text):]
        assert rest == bytes([SENTINEL]) * len(rest)  # and nothing behind it


def _run(native, jobs):
    torch.cuda.synchronize()
    results = native.gpu.device_json_print_records([j.row() for j in jobs], 0)
    assert len(results) == len(jobs)
    for j, r in zip(jobs, results):
        j.check(r)
    return results


def _ok(native, jobs):
    for r in _run(native, jobs):
        assert r[1] == 0
    return jobs


def _bytes_col(key, sizes, seed, text):
    ends = np.cumsum(sizes)
    return J.column(key, J.BYTES, J.values(J.BYTES, int(ends[-1]), seed), ends, text)


@pytest.mark.parametrize("which", range(6))
def test_one_column_of_each_kind_scalar_and_ragged(native, dev, B, which):
    """rows in {1, 2, B - 1, B, B + 1, 2B + 1}: a job per kind and shape, all in one call."""
    rows = [1, 2, B - 1, B, B + 1, 2 * B + 1][which]
    jobs = []
    for kind in J.NUMBER_KINDS:
        jobs.append(Job(native, dev, [J.column("s", kind, J.values(kind, rows, rows))], rows, phase=kind))
        ends = J.ragged(rows, rows + kind)
        jobs.append(Job(native, dev, [J.column("r", kind, J.values(kind, int(ends[-1]), rows + 1), ends)], rows,
                        brackets=kind % 2 == 0))
    ends = J.ragged(rows, rows + 77, longest=9)
    for text in (J.STRING, J.BASE64):
        jobs.append(Job(native, dev, [J.column("b", J.BYTES, J.values(J.BYTES, int(ends[-1]), text), ends, text)], rows))
    _ok(native, jobs)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_one_element_rows_across_a_chunk_edge(native, dev, C, delta):
    n = C + delta
    ones = np.arange(1, n + 1)
    _ok(native, [Job(native, dev, [J.column("v", J.INT64, J.values(J.INT64, n, 5), ones)], n),
                 Job(native, dev, [J.column("f", J.DOUBLE, J.values(J.DOUBLE, n, 6), ones)], n),
                 Job(native, dev, [J.column("s", J.BYTES, J.values(J.BYTES, n, 7), ones, J.STRING)], n),
                 Job(native, dev, [J.column("b", J.BYTES, J.values(J.BYTES, n, 8), ones, J.BASE64)], n)])


def test_one_row_of_three_chunks_and_one(native, dev, C):
    n = 3 * C + 1
    _ok(native, [Job(native, dev, [J.column("v", kind, J.values(kind, n, 9), [n])], 1)
                 for kind in (J.SINT32, J.UINT64, J.FLOAT, J.BOOL)] +
                [Job(native, dev, [J.column("t", J.BYTES, J.values(J.BYTES, n, 10), [n], text)], 1)
                 for text in (J.STRING, J.BASE64)])


def test_empty_rows_straddle_a_chunk_edge_and_a_block_edge(native, dev, C, B):
    """B - 2 rows that hold a whole number of chunks, B + 5 empty rows (over
    the block edge at row B, between the last element of one chunk and the
    first of the next), three rows of two."""
    head = [1] * (B - 3)
    head.append(C - (B - 3) % C)
    assert sum(head) % C == 0
    sizes = head + [0] * (B + 5) + [2, 2, 2]
    rows, ends = len(sizes), np.cumsum(sizes)
    n = int(ends[-1])
    _ok(native, [Job(native, dev, [J.column("ids", J.INT32, J.values(J.INT32, n, 11), ends),
                                   J.column("text", J.BYTES, J.values(J.BYTES, n, 12), ends, J.STRING),
                                   J.column("blob", J.BYTES, J.values(J.BYTES, n, 13), ends, J.BASE64),
                                   J.column("label", J.BOOL, J.values(J.BOOL, rows, 14))], rows)])


def test_empty_first_and_last_rows_and_a_column_without_elements(native, dev):
    sizes = [0, 3, 0, 0, 5, 1, 0]
    ends = np.cumsum(sizes)
    none = np.zeros(len(sizes), dtype=np.uint32)
    jobs = [Job(native, dev, [J.column("a", J.INT64, J.values(J.INT64, 9, 1), ends),
                              J.column("w", J.FLOAT, np.zeros(0), none),
                              J.column("s", J.BYTES, np.zeros(0), none, J.STRING),
                              J.column("b", J.BYTES, J.values(J.BYTES, 9, 2), ends, J.BASE64)], len(sizes)),
            Job(native, dev, [J.column("only", J.UINT32, np.zeros(0), none)], len(sizes)),
            Job(native, dev, [J.column("only", J.BYTES, np.zeros(0), none, J.BASE64)], len(sizes), brackets=False)]
    _ok(native, jobs)
    assert jobs[1].twin[3] == b"[" + b",".join([b'{"only":[]}'] * 7) + b"]"


@pytest.mark.parametrize("seed", range(6))
def test_eight_columns_of_mixed_kinds(native, dev, B, seed):
    rng = np.random.default_rng(seed)
    rows = int(rng.integers(1, 2 * B))
    _ok(native, [Job(native, dev, J.random_columns(rng, rows, 8, seed), rows, brackets=seed % 2 == 0, phase=seed)])


def test_keys(native, dev):
    vals = J.values(J.INT32, 5, 1)
    cols = [J.column(b'q"\\\x01\x80\xff', J.INT32, vals), J.column(b"k" * 255, J.INT32, vals),
            J.column(b"j" * 249 + b"\x02", J.INT32, vals, np.arange(1, 6)), J.column(b"", J.INT32, vals)]
    job, = _ok(native, [Job(native, dev, cols, 5)])
    assert job.twin[3].startswith(b'[{"q\\"\\\\\\u0001\x80\xff":-2147483648,"kkk')


def test_nonfinite_floats_and_integer_extremes(native, dev):
    f32 = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, 3.4028235e38, 1e22, 0.1], dtype=np.float32)
    f64 = np.array([np.nan, np.inf, -np.inf, -0.0, 5e-324, 1.7976931348623157e308, 1e21, 1e-7], dtype=np.float64)
    cols = [J.column("f", J.FLOAT, f32), J.column("d", J.DOUBLE, f64), J.column("fr", J.FLOAT, f32, [3, 8] + [8] * 6),
            J.column("dr", J.DOUBLE, f64, [0] * 7 + [8])]
    for kind in (J.INT32, J.UINT32, J.SINT32, J.INT64, J.UINT64, J.SINT64):
        info = np.iinfo(J.DTYPES[kind])
        cols.append(J.column("i%d" % kind, kind, np.array([info.min, info.max] * 4, dtype=J.DTYPES[kind])))
    jobs = _ok(native, [Job(native, dev, cols[:8], 8), Job(native, dev, cols[8:], 8)])
    assert b'"f":"NaN"' in jobs[0].twin[3] and b'"fr":["NaN","Infinity","-Infinity"]' in jobs[0].twin[3]
    assert b"18446744073709551615" in jobs[1].twin[3] and b"-9223372036854775808" in jobs[1].twin[3]


def test_string_rows_across_a_chunk_edge(native, dev, C):
    """Quotes, control bytes and bytes >= 0x80 on both sides of the edge: one
    row over it, one that ends at it, one that starts at it."""
    sizes = [C - 3, 7, C - 4, 5, C, 1]
    col = _bytes_col("text", sizes, 21, J.STRING)
    edge = col["arr"]
    edge[C - 2:C + 2] = np.frombuffer(b'"\x01\x80\\', dtype=np.uint8)
    edge[2 * C - 1], edge[2 * C] = 0x1f, ord('"')
    _ok(native, [Job(native, dev, [col], len(sizes), phase=3)])


def test_base64_row_lengths(native, dev, C):
    sizes = list(range(8)) + [C - 1, C, C + 1, 0, 3 * C + 2]
    _ok(native, [Job(native, dev, [_bytes_col("blob", sizes, 22, J.BASE64)], len(sizes), phase=5)])


@pytest.mark.parametrize("phase", [0, 1, 7, 15])
@pytest.mark.parametrize("brackets", [True, False])
def test_dst_phases_and_brackets(native, dev, phase, brackets):
    rng = np.random.default_rng(phase)
    cols = J.random_columns(rng, 40, 5, 3)
    job, = _ok(native, [Job(native, dev, cols, 40, brackets=brackets, phase=phase)])
    assert (job.buf.data_ptr() + job.off) % 16 == phase
    assert job.twin[3][:1] == (b"[" if brackets else b"{")


def test_no_rows(native, dev):
    none = np.zeros(0, dtype=np.uint32)
    cols = [J.column("a", J.INT64, np.zeros(0), none), J.column("s", J.INT32, np.zeros(0))]
    before = native.gpu.json_stats()["record_print_jobs"]
    jobs = [Job(native, dev, cols, 0, brackets=True, phase=1), Job(native, dev, cols, 0, brackets=False),
            Job(native, dev, cols, 0, brackets=True, cap=1), Job(native, dev, cols, 0, brackets=True, cap=0)]
    res = _run(native, jobs)
    assert [r[:2] for r in res] == [(2, 0), (0, 0), (2, 3), (2, 3)]
    assert jobs[0].twin[3] == b"[]" and jobs[1].twin[3] == b""
    assert native.gpu.json_stats()["record_print_jobs"] == before  # nothing was launched for them


def test_short_caps(native, dev):
    rng = np.random.default_rng(5)
    cols = J.random_columns(rng, 70, 6, 2)
    full, = _ok(native, [Job(native, dev, cols, 70)])
    need = len(full.twin[3])
    res = _run(native, [Job(native, dev, cols, 70, cap=need - 1, phase=2), Job(native, dev, cols, 70, cap=0),
                        Job(native, dev, cols, 70, cap=need, phase=9)])
    assert [r[:2] for r in res] == [(need, 3), (need, 3), (need, 0)]


def _hurt(col, r, how, rows):
    if how == "above":
        col["ends"][r] = col["arr"].size + 2
    elif how == "below":
        col["ends"][r] = col["ends"][r - 1] - 1
    else:
        col["ends"][rows - 1] += 1


@pytest.mark.parametrize("case", ["row0_col0", "middle_col0", "last_col0", "row0_later", "middle_later", "last_later",
                                  "two_columns", "two_columns_same_row", "short_cap"])
def test_bad_tables(native, dev, B, case):
    """first_bad, bad_column and the untouched buffer equal the twin's."""
    rows = 2 * B + 9
    mid = B + 3

    def cols():
        ends = np.arange(1, rows + 1) * 2
        return [J.column("a", J.INT64, J.values(J.INT64, 2 * rows, 1), ends.copy()),
                J.column("l", J.INT32, J.values(J.INT32, rows, 2)),
                J.column("s", J.BYTES, J.values(J.BYTES, 2 * rows, 3), ends.copy(), J.STRING),
                J.column("b", J.BYTES, J.values(J.BYTES, 2 * rows, 4), ends.copy(), J.BASE64)]
    cs, cap, want = cols(), None, None
    if case == "row0_col0":
        _hurt(cs[0], 0, "above", rows)
        want = (0, 0)
    elif case == "middle_col0":
        _hurt(cs[0], mid, "below", rows)
        want = (mid, 0)
    elif case == "last_col0":
        _hurt(cs[0], rows - 1, "last", rows)
        want = (rows - 1, 0)
    elif case == "row0_later":
        _hurt(cs[3], 0, "above", rows)
        want = (0, 3)
    elif case == "middle_later":
        _hurt(cs[2], mid, "above", rows)
        want = (mid, 2)
    elif case == "last_later":
        _hurt(cs[3], rows - 1, "last", rows)
        want = (rows - 1, 3)
    elif case == "two_columns":
        _hurt(cs[0], mid + 1, "below", rows)
        _hurt(cs[2], mid, "below", rows)
        want = (mid, 2)
    elif case == "two_columns_same_row":
        _hurt(cs[3], mid, "above", rows)
        _hurt(cs[2], mid, "below", rows)
        want = (mid, 2)
    else:  # a bad table and a cap that is too short: the table wins
        _hurt(cs[2], 7, "above", rows)
        cap, want = 5, (7, 2)
    assert J.first_bad(cs, rows) == want
    (length, err, first_bad, bad_column), = _run(native, [Job(native, dev, cs, rows, cap=cap)])
    assert (length, err, first_bad, bad_column) == (0, 1) + want


def test_refusals_launch_nothing(native, dev):
    """Each refusal of code 2: the result, an untouched buffer, and the
    counters of printed jobs stand still."""
    vals = _to_dev(np.arange(8, dtype=np.int64), dev)
    ends = _to_dev(np.array([4, 8], dtype=np.uint32), dev)
    buf = torch.full((256,), SENTINEL, dtype=torch.uint8, device=dev)
    good = (b"k", J.INT64, J.NUMBER, vals.data_ptr(), 8, ends.data_ptr())
    scalar = (b"s", J.INT64, J.NUMBER, vals.data_ptr(), 2, 0)

    def job(cols, rows=2, dst=buf.data_ptr(), cap=256):
        return (cols, rows, True, dst, cap)
    table = [
        job([good[:3] + (0,) + good[4:]]),                          # a null source with elements
        job([good], dst=0),                                         # a null dst with a cap
        job([good[:3] + (vals.data_ptr() + 4,) + good[4:]]),        # an int64 at 4 (mod 8)
        job([good[:5] + (ends.data_ptr() + 2,)]),                   # a table at 2 (mod 4)
        job([(b"k", 10, J.NUMBER) + good[3:]]),                     # a kind there is not
        job([(b"k", J.BYTES, 3) + good[3:]]),                       # a text form there is not
        job([(b"k", J.BYTES, J.STRING) + scalar[3:]]),              # bytes without row ends
        job([(b"k", J.INT64, J.BASE64) + good[3:]]),                # a text form on a number kind
        job([]),                                                    # no column
        job([(b"k%d" % i,) + good[1:] for i in range(9)]),          # nine columns
        job([scalar[:4] + (3, 0)]),                                 # a scalar column whose count is not rows
        job([(b"k" * 256,) + good[1:]]),                            # a key above 255 bytes
        job([(b"\x01" * 43,) + good[1:]]),                          # a key above 255 bytes once escaped
        job([good, scalar, good]),                                  # two equal keys
        job([good], dst=vals.data_ptr() + 8, cap=16),               # dst inside a source
        job([good], dst=ends.data_ptr() + 4, cap=4),                # dst inside a table
        job([good[:4] + (1 << 28,) + good[5:]]),                    # a worst case above 2^32 - 1
    ]
    before = native.gpu.json_stats()
    torch.cuda.synchronize()
    res = native.gpu.device_json_print_records(table, 0)
    assert res == [(0, 2, NONE, NONE)] * len(table)
    after = native.gpu.json_stats()
    assert (after["record_print_jobs"], after["record_print_rows"]) == \
        (before["record_print_jobs"], before["record_print_rows"])
    assert bytes(buf.cpu().numpy()) == bytes([SENTINEL]) * 256
    assert bytes(vals.cpu().numpy().tobytes()) == np.arange(8, dtype=np.int64).tobytes()
    # the same call prints the good job between refused ones
    res = native.gpu.device_json_print_records([table[0], job([good, scalar]), table[1]], 0)
    assert [r[1] for r in res] == [2, 0, 2]
    want = native.json_format_record_objects(
        [(b"k", J.INT64, 0, np.arange(8, dtype=np.int64).tobytes(), [4, 8]),
         (b"s", J.INT64, 0, np.arange(2, dtype=np.int64).tobytes(), None)], 2, True)[3]
    assert bytes(buf.cpu().numpy())[:res[1][0]] == want
    after = native.gpu.json_stats()
    assert after["record_print_jobs"] == before["record_print_jobs"] + 1
    assert after["record_print_rows"] == before["record_print_rows"] + 2


def test_six_jobs_with_mixed_verdicts_in_one_call(native, dev, C, B):
    rng = np.random.default_rng(8)
    a = J.random_columns(rng, B + 7, 4, 1)
    b = J.random_columns(rng, 3, 8, 5)
    bad = [J.column("x", J.INT64, J.values(J.INT64, 2 * C, 1), np.arange(1, C + 1) * 2),
           J.column("y", J.BYTES, J.values(J.BYTES, 2 * C, 2), np.arange(1, C + 1) * 2, J.STRING)]
    bad[1]["ends"][C // 2] = 0
    short = J.random_columns(rng, 50, 3, 7)
    none = [J.column("n", J.FLOAT, np.zeros(0), np.zeros(0, dtype=np.uint32))]
    jobs = [Job(native, dev, a, B + 7, phase=1), Job(native, dev, bad, C, phase=2), Job(native, dev, b, 3, False, 3),
            Job(native, dev, short, 50, cap=17, phase=4), Job(native, dev, none, 0, phase=5),
            Job(native, dev, a[::-1], B + 7, phase=6)]
    res = _run(native, jobs)
    assert [r[1] for r in res] == [0, 1, 0, 3, 0, 0]
    assert res[1][2:] == (C // 2, 1)


def _text(t):
    return bytes(t.cpu().numpy())


def test_ops_build_split_print_load(native, dev):
    """pb_build_records -> pb_split_records -> json_print_records ->
    json.loads gives the original columns."""
    from brpc_amd import ops
    rows = 300
    id_ends = J.ragged(rows, 1, longest=6)
    w_ends = J.ragged(rows, 2, longest=3)
    blob_ends = J.ragged(rows, 3, longest=9)
    ids = J.values(J.INT64, int(id_ends[-1]), 1)
    weights = J.values(J.FLOAT, int(w_ends[-1]), 2, nonfinite=False)
    labels = J.values(J.INT32, rows, 3)
    blob = J.values(J.BYTES, int(blob_ends[-1]), 4)
    t = lambda a: torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    e = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)  # noqa: E731
    msg = ops.pb_build_records(4, [(1, t(ids), e(id_ends), "int64"), (2, t(weights), e(w_ends), "float32"),
                                   (3, t(labels), None, "int32"), (4, t(blob), e(blob_ends), "bytes")])
    split = ops.pb_split_records(msg, 4, [(1, "int64", False), (2, "float32", False), (3, "int32", True),
                                          (4, "bytes", False)], max_rows=rows)
    names = [("input_ids", "int64"), ("weights", "float32"), ("label", "int32"), ("blob", "base64")]
    text = _text(ops.json_print_records([(k, v, ends, kind) for (k, kind), (v, ends) in zip(names, split)]))
    cols = [J.column("input_ids", J.INT64, ids, id_ends), J.column("weights", J.FLOAT, weights, w_ends),
            J.column("label", J.INT32, labels), J.column("blob", J.BYTES, blob, blob_ends, J.BASE64)]
    assert text == native.json_format_record_objects(J.twin_columns(cols), rows, True)[3]
    assert json.loads(text) == J.structure(cols, rows)
    # the same blob as a string, an int64 table, no brackets
    text = _text(ops.json_print_records([("t", split[3][0], split[3][1].to(torch.int64), "string")], brackets=False))
    scol = [J.column("t", J.BYTES, blob, blob_ends, J.STRING)]
    assert text == native.json_format_record_objects(J.twin_columns(scol), rows, False)[3]
    assert json.loads("[" + text.decode("latin-1") + "]") == J.structure(scol, rows)


def test_ops_tensors_of_one_and_two_dimensions(native, dev):
    from brpc_amd import ops
    square = torch.arange(12, dtype=torch.float32, device=dev).reshape(4, 3) / 4
    label = torch.tensor([1, 0, 1, 1], dtype=torch.bool, device=dev)
    ids = torch.tensor([-1, 2, -3, 4], dtype=torch.int64, device=dev)
    text = _text(ops.json_print_records([("scores", square, None, "float32"), ("ok", label, None, "bool"),
                                         (b"id", ids, None, "sint64")]))
    assert json.loads(text) == [{"scores": [float(x) for x in square[r].cpu()], "ok": bool(label[r]), "id": int(ids[r])}
                                for r in range(4)]
    assert text.startswith(b'[{"scores":[0.0,0.25,0.5],"ok":true,"id":-1},')
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    assert _text(ops.json_print_records([("a", empty, None, "int64")])) == b"[]"
    assert _text(ops.json_print_records([("a", empty, None, "int64")], brackets=False)) == b""
    with pytest.raises(ValueError, match=r"column 1: row_ends\[1\]"):
        ops.json_print_records([("a", ids, None, "int64"),
                                ("b", ids, torch.tensor([2, 1, 4, 4], device=dev), "int64")])
    with pytest.raises(ValueError, match="holds 3 records"):
        ops.json_print_records([("a", ids, None, "int64"), ("b", ids[:3], None, "int64")])
    with pytest.raises(ValueError, match="unknown kind"):
        ops.json_print_records([("a", ids, None, "fixed64")])
    with pytest.raises(ValueError, match="needs row_ends"):
        ops.json_print_records([("a", ids.to(torch.uint8), None, "string")])
    with pytest.raises(TypeError):
        ops.json_print_records([("a", ids, None, "int32")])
    with pytest.raises(ValueError, match="refused"):
        ops.json_print_records([("a", ids, None, "int64"), ("a", ids, None, "int64")])
