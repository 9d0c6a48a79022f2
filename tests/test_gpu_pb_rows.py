"""Device row builder (gpu/device_codec.h DeviceBuildRows and the kernels
behind LaunchPbRecordsBuild, which it runs as a record job of one column,
headerless for inner 0): a flat array in HBM plus a table of row ends
becomes the occurrences of one repeated field in HBM. Every case compares the
device's bytes with pb_rows_wire.reference (a numpy serializer written from
the wire rules), one case per kind also with the project's host serializer;
every destination sits in a field of sentinel bytes. The host checks and the
host twin run without a GPU in brpc_amd/csrc/tests/pb_rows_unittest.cc and
tests/test_pb_rows_host.py."""
import json

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_rows_wire as W  # noqa: E402

SENTINEL = 0xA5
GUARD = 64
ALL = [(k, 2) for k in sorted(W.KINDS)] + [(W.BYTES, 0)]
NUMBERS = (1, 15, 16, 2047, 2048, 2**29 - 1)


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


def _run(native, dev, jobs):
    """jobs: dicts with number, inner, kind, arr, ends and optionally cap (an
    int, or a function of the reference's length), phase (dst's 16-byte
    alignment), count / rows overrides. All jobs go into ONE call. Returns
    [(len, err, first_bad, message bytes)] after checking the sentinels:
    everything around the message, and all of dst when err is 1, 2 or 3."""
    keep, table, bufs = [], [], []
    for j in jobs:
        arr, ends = j["arr"], np.asarray(j["ends"], dtype=np.uint32)
        count = j.get("count", arr.size)
        rows = j.get("rows", ends.size)
        src_t, src = _upload(arr, dev)
        ends_t = torch.from_numpy(ends.view(np.int32).copy()).to(dev) if ends.size else \
            torch.zeros(1, dtype=torch.int32, device=dev)
        worst = native.gpu.device_rows_worst_case(j["number"], j["inner"], j["kind"], count, rows)
        cap = j.get("cap", worst)
        if callable(cap):
            cap = cap(len(W.reference(j["number"], j["inner"], j["kind"], arr, ends)))
        phase = j.get("phase", 0)
        buf = torch.full((GUARD + 32 + max(cap, worst, 1) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        skip = (-buf.data_ptr() - GUARD) % 16 + phase  # dst = 16-byte boundary + phase
        dst = buf.data_ptr() + GUARD + skip
        assert dst % 16 == phase % 16
        keep.append((src_t, ends_t))
        bufs.append((buf, GUARD + skip, cap))
        table.append((j["number"], j["inner"], j["kind"], src if count else 0, count, ends_t.data_ptr(), rows, dst,
                      cap))
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    res = native.gpu.device_build_rows(table, 0)
    out = []
    for (n, err, first_bad), (buf, at, cap) in zip(res, bufs):
        host = buf.cpu().numpy()
        written = n if err in (0, 4) else 0
        assert written <= cap
        assert (host[:at] == SENTINEL).all(), "bytes in front of dst changed"
        assert (host[at + written:] == SENTINEL).all(), "bytes beyond the message changed (err %d)" % err
        out.append((n, err, first_bad, host[at:at + written].tobytes()))
    return out


def _check(native, dev, number, inner, kind, arr, ends, **more):
    job = dict(number=number, inner=inner, kind=kind, arr=arr, ends=ends, **more)
    (n, err, first_bad, got), = _run(native, dev, [job])
    want = W.reference(number, inner, kind, arr, ends)
    assert err == 0 and first_bad == 0xFFFFFFFF
    assert n == len(want)
    assert got == want
    return got


# rows ending at elements 2047, 2048 and 2049, empty rows at the start, at
# the end and 300 of them exactly at element 2048, one row over three chunks
# (5000 elements), then 4100 one-element rows: more rows than a chunk has
# elements
BOUNDARY_ENDS = np.concatenate([[0, 0, 0, 2047, 2048], np.full(300, 2048), [2049, 7049],
                                7049 + 1 + np.arange(4100), np.full(3, 7049 + 4100)]).astype(np.uint32)


@pytest.mark.parametrize("kind,inner", ALL)
def test_chunk_boundaries_and_empty_rows(native, dev, kind, inner):
    arr = W.values(kind, int(BOUNDARY_ENDS[-1]), 100 + kind)
    got = _check(native, dev, 4, inner, kind, arr, BOUNDARY_ENDS)
    # the host twin writes the same bytes
    err, _, twin = native.pb_serialize_rows(4, inner, kind, arr.tobytes(), [int(e) for e in BOUNDARY_ENDS])
    assert err == 0 and twin == got


@pytest.mark.parametrize("kind,inner", [(1, 2), (W.FIXED32, 2), (W.BYTES, 0), (W.BYTES, 3)])
def test_rows_around_a_row_block_and_elements_around_a_chunk(native, dev, kind, inner):
    """255, 256 and 257 rows (a row block is 256) over 2047, 2048 and 2049
    elements (a chunk is 2048), the first and the last row empty: the smallest
    shapes that cross a row block and a chunk, each against the host twin."""
    rng = np.random.default_rng(40 + kind + inner)
    for rows in (255, 256, 257):
        for count in (2047, 2048, 2049):
            arr = W.values(kind, count, 400 + kind)
            ends = np.concatenate([[0], np.sort(rng.integers(0, count + 1, rows - 3)), [count, count]]).astype(np.uint32)
            assert ends.size == rows and ends[0] == 0 and ends[-2] == ends[-1] == count
            got = _check(native, dev, 4, inner, kind, arr, ends)
            err, _, twin = native.pb_serialize_rows(4, inner, kind, arr.tobytes(), [int(e) for e in ends])
            assert err == 0 and twin == got, (rows, count)


@pytest.mark.parametrize("kind,inner", ALL)
def test_matches_the_host_serializer_and_parses_back(native, dev, tmp_path, kind, inner):
    """Against the wire bytes of the project's own host serializer (the batch
    given as JSON, the type parsed from a .proto at run time); floats are
    multiples of 1/8, exact as text. The host parser accepts the device's
    bytes and prints the same JSON."""
    sizes = [0, 3, 0, 0, 2045, 1, 2, 700, 0, 64, 63, 65, 0]
    arr = W.values(kind, sum(sizes), 200 + kind)
    ends = np.cumsum(sizes)
    wire, back, proto = W.host_wire(native, tmp_path, kind, 4, inner, arr, ends)
    got = _check(native, dev, 4, inner, kind, arr, ends)
    assert got == wire
    ok, err, text = native.json_proto_from_wire(str(tmp_path), proto, "Batch", got, bytes_to_base64=True)
    assert ok, err
    assert json.loads(text) == json.loads(back)


@pytest.mark.parametrize("kind,inner", [(W.FIXED32, 2), (1, 2), (W.BYTES, 0), (W.BYTES, 3)])
def test_one_empty_row_alone(native, dev, kind, inner):
    arr = np.zeros(0, dtype=W.KINDS[kind][0])
    got = _check(native, dev, 4, inner, kind, arr, [0])
    assert got == {(W.FIXED32, 2): b"\x22\x00", (1, 2): b"\x22\x00", (W.BYTES, 0): b"\x22\x00",
                   (W.BYTES, 3): b"\x22\x02\x1a\x00"}[(kind, inner)]


@pytest.mark.parametrize("kind", [W.BYTES, 1, 6])
def test_varint_length_of_the_row_size(native, dev, kind):
    """Payloads of 125..129 and 16381..16385 bytes (one-byte elements): the
    1 -> 2 and 2 -> 3 byte steps of the inner and of the outer length fall
    into separate rows, the inner one a row earlier."""
    sizes = [125, 126, 127, 128, 129, 16381, 16382, 16383, 16384, 16385]
    if kind == 1:
        arr = np.random.default_rng(5).integers(0, 128, sum(sizes)).astype(np.uint32)
    else:
        arr = W.values(kind, sum(sizes), 5)
    ends = np.cumsum(sizes)
    for inner in ((0, 1, 2047) if kind == W.BYTES else (1, 2047)):
        _check(native, dev, 16, inner, kind, arr, ends)


def test_field_numbers_in_one_call(native, dev):
    """number and inner of 1, 15, 16, 2047, 2048 and 2^29-1 (tags of 1, 2, 3
    and 5 bytes), all 36 pairs as jobs of one call."""
    arr = W.values(2, 300, 9)
    ends = [0, 1, 1, 120, 299, 300]
    jobs = [dict(number=a, inner=b, kind=2, arr=arr, ends=ends) for a in NUMBERS for b in NUMBERS]
    for j, (n, err, _, got) in zip(jobs, _run(native, dev, jobs)):
        want = W.reference(j["number"], j["inner"], 2, arr, ends)
        assert err == 0 and n == len(want) and got == want, (j["number"], j["inner"])


@pytest.mark.parametrize("kind,inner", [(1, 2), (5, 2), (W.FIXED32, 2), (W.FIXED64, 2), (W.BYTES, 0)])
def test_every_destination_alignment(native, dev, kind, inner):
    """dst at each of the 16 byte alignments. A row of 2100 elements fills
    the first chunk (it leaves as one aligned segment), three long rows share
    the next (segments at other phases), 400 one-element rows follow (a chunk
    of many rows, stored element by element)."""
    sizes = [2100, 500, 37, 1000] + [1] * 400 + [0, 9]
    arr = W.values(kind, sum(sizes), 300 + kind)
    ends = np.cumsum(sizes)
    want = W.reference(7, inner, kind, arr, ends)
    jobs = [dict(number=7, inner=inner, kind=kind, arr=arr, ends=ends, phase=p) for p in range(16)]
    for p, (n, err, _, got) in enumerate(_run(native, dev, jobs)):
        assert err == 0 and got == want, "phase %d" % p


def test_a_refused_and_a_short_job_leave_the_others_alone(native, dev):
    a = W.values(3, 5000, 1)
    b = W.values(W.FIXED64, 3000, 2)
    c = W.values(W.BYTES, 2600, 3)
    a_ends, b_ends, c_ends = [10, 10, 2500, 5000], np.arange(1, 3001), [0, 2049, 2049, 2600]
    jobs = [dict(number=3, inner=1, kind=3, arr=a, ends=a_ends),
            dict(number=0, inner=1, kind=3, arr=a, ends=a_ends),                      # refused: number 0
            dict(number=3, inner=1, kind=3, arr=a, ends=a_ends, cap=lambda n: n - 1),  # a byte short
            dict(number=3, inner=0, kind=3, arr=a, ends=a_ends),                      # refused: no wrapper, not bytes
            dict(number=9, inner=4, kind=W.FIXED64, arr=b, ends=b_ends, cap=lambda n: n),  # cap == len
            dict(number=5, inner=0, kind=W.BYTES, arr=c, ends=c_ends),                # no wrapper: repeated bytes
            dict(number=3, inner=1, kind=3, arr=a, ends=[10, 9, 2500, 5000])]         # row_ends decreases at row 1
    c0 = native.gpu.device_codec_stats()
    res = _run(native, dev, jobs)
    c1 = native.gpu.device_codec_stats()
    want_a = W.reference(3, 1, 3, a, a_ends)
    want_b = W.reference(9, 4, W.FIXED64, b, b_ends)
    want_c = W.reference(5, 0, W.BYTES, c, c_ends)
    assert [r[1] for r in res] == [0, 2, 3, 2, 0, 0, 1]
    assert res[0][3] == want_a and res[4][3] == want_b and res[5][3] == want_c
    assert res[2][0] == len(want_a)  # the size it needs
    assert res[6][2] == 1            # the row; _run saw its dst untouched, as the short job's
    assert [r[2] for r in res[:6]] == [0xFFFFFFFF] * 6
    assert c1["built_row_jobs"] - c0["built_row_jobs"] == 3
    assert c1["built_rows"] - c0["built_rows"] == 4 + 3000 + 4
    assert c1["built_row_bytes"] - c0["built_row_bytes"] == len(want_a) + len(want_b) + len(want_c)
    assert c1["build_errors"] - c0["build_errors"] == 4
    for k in ("built_record_jobs", "built_records", "built_record_bytes"):
        assert c1[k] == c0[k]


def test_a_rows_job_counts_as_rows_only(native, dev):
    arr = W.values(2, 300, 9)
    ends = [0, 1, 1, 120, 299, 300]
    c0 = native.gpu.device_codec_stats()
    got = _check(native, dev, 4, 2, 2, arr, ends)
    c1 = native.gpu.device_codec_stats()
    assert "built_record_jobs" in c0 and "build_errors" in c0
    # the record counters, the error counter and every other one stay
    moved = {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]}
    assert moved == {"built_row_jobs": 1, "built_rows": len(ends), "built_row_bytes": len(got)}


@pytest.mark.parametrize("kind", [1, W.FIXED32])
def test_malformed_row_ends_are_found_on_the_device(native, dev, kind):
    arr = W.values(kind, 6000, 4)
    ends = np.arange(100, 6001, 100, dtype=np.uint32)  # 60 rows of 100
    down = ends.copy()
    down[30] = down[29] - 1  # row 30 starts at element 3000, in the second chunk
    down[45] = 0             # not the first
    (n, err, first_bad, _), = _run(native, dev, [dict(number=1, inner=2, kind=kind, arr=arr, ends=down)])
    assert (err, first_bad) == (1, 30)
    short = ends.copy()
    short[-1] = 5999
    (n, err, first_bad, _), = _run(native, dev, [dict(number=1, inner=2, kind=kind, arr=arr, ends=short)])
    assert (err, first_bad) == (1, 59)
    beyond = ends.copy()
    beyond[-1] = 6001
    (n, err, first_bad, _), = _run(native, dev, [dict(number=1, inner=2, kind=kind, arr=arr, ends=beyond)])
    assert (err, first_bad) == (1, 59)


def test_refusals_reach_no_kernel(native, dev):
    arr = W.values(1, 64, 8)
    src_t, src = _upload(arr, dev)
    ends_t = torch.tensor([64], dtype=torch.int32, device=dev)
    dst = torch.zeros(1024, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    good = (1, 2, 1, src, 64, ends_t.data_ptr(), 1, dst.data_ptr(), 1024)

    def with_(**kw):
        names = ["number", "inner", "kind", "src", "count", "row_ends", "rows", "dst", "cap"]
        return tuple(kw.get(k, v) for k, v in zip(names, good))
    bad = [with_(number=0), with_(number=2**29), with_(inner=2**29), with_(kind=10), with_(inner=0),
           with_(src=0), with_(src=src + 1), with_(row_ends=0), with_(row_ends=ends_t.data_ptr() + 2),
           with_(rows=0), with_(dst=0), with_(count=2**32), with_(count=2**31, rows=1)]
    res = native.gpu.device_build_rows(bad + [good], 0)
    assert [r[1] for r in res] == [2] * len(bad) + [0]
    assert (dst[:res[-1][0]].cpu().numpy().tobytes() == W.reference(1, 2, 1, arr, [64]))


def test_json_text_to_rows_end_to_end(native, dev, tmp_path):
    """Nested float text in HBM -> json_parse_float_rows(ragged=True) ->
    pb_build_rows: the host wire bytes of the same batch."""
    from brpc_amd.ops import json_parse_float_rows, pb_build_rows
    sizes = [3, 1, 700, 2, 65]  # the number text has no empty rows
    arr = W.values(W.FIXED32, sum(sizes), 11)
    ends = np.cumsum(sizes)
    rows = [[float(x) for x in arr[e - s:e]] for s, e in zip(sizes, ends)]
    text = torch.from_numpy(np.frombuffer(json.dumps(rows).encode(), dtype=np.uint8).copy()).to(dev)
    vals, row_ends = json_parse_float_rows(text, torch.float32, ragged=True)
    got = pb_build_rows(4, vals, row_ends, "float32", inner=2)
    wire, _, _ = W.host_wire(native, tmp_path, W.FIXED32, 4, 2, arr, ends)
    assert got.cpu().numpy().tobytes() == wire


def test_equal_rows_from_a_2d_tensor(native, dev):
    from brpc_amd.ops import pb_build_rows
    arr = W.values(5, 37 * 129, 12)
    t = torch.from_numpy(arr.reshape(37, 129).copy()).to(dev)
    ends = torch.arange(129, 37 * 129 + 1, 129, dtype=torch.int32, device=dev)
    a = pb_build_rows(6, t, None, "sint64", inner=1)
    b = pb_build_rows(6, t.view(-1), ends, "sint64", inner=1)
    assert torch.equal(a, b)
    assert a.cpu().numpy().tobytes() == W.reference(6, 1, 5, arr, ends.cpu().numpy())
    blobs = pb_build_rows(5, t.view(torch.uint8).view(37, -1), None, "bytes")
    assert blobs.cpu().numpy().tobytes() == W.reference(5, 0, W.BYTES, np.frombuffer(arr.tobytes(), dtype=np.uint8),
                                                        np.arange(1, 38) * 129 * 8)
    with pytest.raises(ValueError, match="row 1"):
        pb_build_rows(6, t.view(-1), torch.tensor([5, 4, 37 * 129], dtype=torch.int32, device=dev), "sint64", inner=1)
