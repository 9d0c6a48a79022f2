"""Device record splitter (gpu/device_codec.h DeviceSplitRecords and the
kernels behind LaunchPbRecordsSplit): a message in HBM whose field `number`
repeats once per record becomes every column's flat array, row ends and
scalars in HBM. Every result is compared with the host twin
(native.pb_split_records) and with this directory's pure-python splitter
(pb_records_split_ref.split); every output sits in a field of sentinel bytes,
checked around the result and over all of it when the code is 1, 2, 5 or 6.
The message starts at a byte that is no multiple of 16. The twin and the rules
run without a GPU in tests/test_pb_records_split_host.py and
brpc_amd/csrc/tests/pb_records_split_unittest.cc."""
import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_records_split_ref as S  # noqa: E402
import pb_rows_wire as W  # noqa: E402

SENTINEL = 0xA5
GUARD = 64
# kind -> (kind name of ops.pb, the dtype pb_split_records returns)
NAMES = {0: ("int32", torch.int32), 1: ("uint32", torch.int32), 2: ("sint32", torch.int32), 3: ("int64", torch.int64),
         4: ("uint64", torch.int64), 5: ("sint64", torch.int64), 6: ("bool", torch.bool), W.BYTES: ("bytes", torch.uint8),
         W.FIXED32: ("float32", torch.float32), W.FIXED64: ("float64", torch.float64)}


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


def _place(data, dev, phase):
    """data in HBM at a 16-byte boundary + phase."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    t = torch.zeros(32 + raw.size, dtype=torch.uint8, device=dev)
    at = (-t.data_ptr()) % 16 + phase
    if raw.size:
        t[at:at + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return t, t.data_ptr() + at


def _sentinels(nbytes, dev):
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    at = GUARD + (-buf.data_ptr() - GUARD) % 16
    return buf, at


def _run(native, dev, jobs, ref=True):
    """jobs: dicts with number, cols [(inner, kind, scalar)], msg and
    optionally row_cap, caps (default: the twin's worst case), phase (the
    message's alignment, default 5). All jobs go into ONE call. Checks every
    job against the twin (and the python splitter) and the sentinels; returns
    the twin's tuples."""
    table, keep, wants = [], [], []
    for j in jobs:
        msg, cols = bytes(j["msg"]), j["cols"]
        row_cap = j.get("row_cap", len(msg) // 2)
        caps = j.get("caps") or [row_cap if scalar else len(msg) // (S.EB[kind] if kind >= 8 else 1)
                                 for _, kind, scalar in cols]
        got = native.pb_split_records(j["number"], cols, msg, row_cap, caps)
        want = (got[0], got[1], got[2], got[3], [tuple(c) for c in got[4]])
        if ref:
            assert want == S.split(j["number"], cols, msg, row_cap, caps)
        msg_t, msg_p = _place(msg, dev, j.get("phase", 5))
        outs, columns = [], []
        for (inner, kind, scalar), cap in zip(cols, caps):
            vals, vat = _sentinels(cap * S.EB[kind], dev)
            ends, eat = _sentinels(0 if scalar else row_cap * 4, dev)
            outs.append((vals, vat, ends, eat))
            columns.append((inner, kind, scalar, vals.data_ptr() + vat, cap, 0 if scalar else ends.data_ptr() + eat))
        keep.append((msg_t, outs))
        wants.append(want)
        table.append((j["number"], columns, msg_p if msg else 0, len(msg), row_cap))
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    res = native.gpu.device_split_records(table, 0)
    for i, ((rows, others, err, first_bad, counts), want, (_, outs)) in enumerate(zip(res, wants, keep)):
        assert (err, rows, others, first_bad) == want[:4], "job %d" % i
        assert [tuple(c) for c in counts] == [c[:2] for c in want[4]], "job %d: counts and absent" % i
        for c, ((vals, vat, ends, eat), (_, kind, scalar)) in enumerate(zip(outs, jobs[i]["cols"])):
            count, _, values, row_ends = want[4][c]
            hv, he = vals.cpu().numpy(), ends.cpu().numpy()
            nv, ne = (count * S.EB[kind], 0 if scalar else rows * 4) if err == 0 else (0, 0)
            where = "job %d column %d" % (i, c)
            assert (hv[:vat] == SENTINEL).all() and (hv[vat + nv:] == SENTINEL).all(), where + ": bytes around values"
            assert (he[:eat] == SENTINEL).all() and (he[eat + ne:] == SENTINEL).all(), where + ": bytes around row_ends"
            if err == 0:
                assert hv[vat:vat + nv].tobytes() == values, where + ": values"
                if not scalar:
                    assert he[eat:eat + ne].view(np.uint32).tolist() == row_ends, where + ": row_ends"
    return wants


def _as_expected(job, want):
    err, rows, others, first_bad, cols = want
    assert err == job.get("code", 0), job.get("what")
    if "first_bad" in job:
        assert first_bad == job["first_bad"], job.get("what")
    if err in (0, 5) and "rows" in job:
        assert rows == job["rows"]
    if err == 0:
        assert others == job.get("others", 0)
        if "values" in job:
            assert [(c[2], c[3]) for c in cols] == job["values"]
        assert [c[1] for c in cols] == job.get("absent", [0] * len(cols))
    if "counts" in job:
        assert [c[0] for c in cols] == job["counts"]


def _check(native, dev, jobs):
    wants = _run(native, dev, jobs)
    for job, want in zip(jobs, wants):
        _as_expected(job, want)
    return wants


def _tensor(col, dev):
    arr = col["arr"]
    signed = {"uint32": "int32", "uint64": "int64"}.get(arr.dtype.name, arr.dtype.name)
    return torch.from_numpy(arr.view(signed).copy()).to(dev)


@pytest.mark.parametrize("ncols", [1, 2, 4, 8])
def test_builder_round_trip(native, dev, ncols):
    """Every kind as a ragged and as a scalar column: DeviceBuildRecords'
    bytes (about three chunks, so records, field headers and payloads straddle
    chunk ends) split into the columns they were built from."""
    from brpc_amd.ops import pb_build_records
    jobs = []
    for i, (specs, rows, per_row) in enumerate(S.round_trip_sets()):
        if len(specs) != ncols:
            continue
        columns = S.make_columns(specs, rows, 300 + i, per_row)
        built = pb_build_records(4, [(c["inner"], _tensor(c, dev), None if c["ends"] is None else
                                      torch.from_numpy(c["ends"].astype(np.int32)).to(dev), NAMES[c["kind"]][0])
                                     for c in columns])
        jobs.append(S.case(columns, rows, msg=built.cpu().numpy().tobytes()))
    assert jobs and all(8192 < len(j["msg"]) < 5 * 4096 for j in jobs)
    _check(native, dev, jobs)


def test_every_byte_of_a_record_on_a_chunk_end(native, dev):
    jobs = S.seam_cases()
    assert len(jobs) == 41 and len(jobs[0]["msg"]) > 2 * 4096
    _check(native, dev, jobs)


def test_record_counts_around_a_block_of_records(native, dev):
    jobs = S.record_count_cases()
    assert [w[1] for w in _check(native, dev, jobs)] == [255, 256, 257, 513]


def test_element_counts_around_an_output_chunk(native, dev):
    jobs = S.element_count_cases()
    for want, count in zip(_check(native, dev, jobs), (2047, 2048, 2049)):
        assert [c[0] for c in want[4]] == [count] * 3


def test_one_record_longer_than_eight_chunks(native, dev):
    job = S.long_record_case()
    assert len(job["msg"]) > 10 * 4096
    _check(native, dev, [job])


@pytest.mark.parametrize("skip", [1, 3, 64])
def test_every_span_of_the_serial_hops(native, dev, skip):
    """-device_split_skip 1 (no skip table), 3 and 64 (one hop spans the whole
    message); the default of 8 runs everywhere else. A malformed field in the
    last chunk is found behind every kind of hop."""
    jobs = S.skip_cases()
    jobs += [dict(number=4, cols=j["cols"], msg=j["msg"] + b"\x0b", code=1, first_bad=len(j["msg"])) for j in jobs]
    native.set_flag("device_split_skip", str(skip))
    try:
        _check(native, dev, jobs)
    finally:
        native.set_flag("device_split_skip", "8")


def test_record_shapes(native, dev):
    """Fields reversed, a packed / a bytes / a scalar column absent, empty
    records, foreign top-level fields between the records."""
    jobs = S.shape_cases()
    wants = _check(native, dev, jobs)
    assert [c[1] for c in wants[3][4]] == [0, 0, 20, 0]  # the scalar column absent from every other record
    assert wants[-1][2] == 41                            # others


def test_payload_that_looks_like_wire(native, dev):
    _check(native, dev, [S.wire_like_case()])


def test_malformed_and_unsupported_messages(native, dev):
    jobs = S.code_cases()
    wants = _check(native, dev, jobs)
    assert {w[0] for w in wants} == {1, 6}


def test_capacities(native, dev):
    """Each column's cap short by one; row_cap short by one, which zeroes
    every count; codes 1 and 6 win over 5."""
    jobs = S.capacity_cases()
    wants = _check(native, dev, jobs)
    assert [w[0] for w in wants] == [0, 5, 5, 5, 5, 5, 1]


def test_refusals_reach_no_kernel(native, dev):
    msg = S.good_example()
    msg_t, msg_p = _place(msg, dev, 5)
    vals = [torch.zeros(1024, dtype=torch.int64, device=dev) for _ in range(9)]
    ends = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(9)]
    big = torch.zeros(9 << 20, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def table(number, cols, msg=msg_p, n=len(msg), row_cap=64, values=None, row_ends=None):
        return (number, [(inner, kind, scalar, vals[c].data_ptr() if values is None else values, 128,
                          0 if scalar else (ends[c].data_ptr() if row_ends is None else row_ends))
                         for c, (inner, kind, scalar) in enumerate(cols)], msg, n, row_cap)
    good = S.EXAMPLE_COLS
    bad = [table(number, cols) for number, cols in S.refused_cases()]
    bad += [table(4, good, msg=0), table(4, good, values=0), table(4, good, values=vals[0].data_ptr() + 2),
            table(4, good, row_ends=0), table(4, good, row_ends=ends[0].data_ptr() + 2),
            table(4, good, msg=12345, n=native.gpu.device_split_max_bytes() + 1),
            # min(row_cap, n / 2) * 8 columns * 8 bytes is above 256 MiB
            table(4, [(i + 1, 0, True) for i in range(8)], msg=big.data_ptr(), n=big.numel(), row_cap=big.numel())]
    c0 = native.gpu.device_codec_stats()
    res = native.gpu.device_split_records(bad, 0)
    c1 = native.gpu.device_codec_stats()
    assert [r[2] for r in res] == [2] * len(bad)
    assert c1["split_record_jobs"] == c0["split_record_jobs"] and c1["split_records"] == c0["split_records"]
    (rows, others, err, _, counts), = native.gpu.device_split_records([table(4, good)], 0)
    assert (rows, others, err) == (6, 0, 0) and counts[2] == (6, 0)
    assert native.gpu.device_split_records([table(4, good, msg=0, n=0)], 0) == [
        (0, 0, 0, 2**64 - 1, [(0, 0)] * 4)]
    c2 = native.gpu.device_codec_stats()
    assert c2["split_record_jobs"] - c1["split_record_jobs"] == 2 and c2["split_records"] - c1["split_records"] == 6


def test_one_call_mixes_good_empty_refused_and_failing_jobs(native, dev):
    columns, msg = S.seam_message()
    cols = S.split_columns(columns)
    other = S.element_count_cases()[0]
    jobs = [S.case(columns, 48, msg=msg), dict(number=4, cols=cols, msg=b""), dict(number=0, cols=cols, msg=msg, code=2),
            dict(number=4, cols=cols, msg=msg + b"\x0b", code=1, first_bad=len(msg)), other,
            dict(number=4, cols=cols, msg=msg, row_cap=47, code=5, rows=48, counts=[0] * 4)]
    c0 = native.gpu.device_codec_stats()
    wants = _check(native, dev, jobs)
    c1 = native.gpu.device_codec_stats()
    assert [w[0] for w in wants] == [0, 0, 2, 1, 0, 5]
    assert c1["split_record_jobs"] - c0["split_record_jobs"] == 3
    assert c1["split_records"] - c0["split_records"] == 48 + other["rows"]
    assert c1["split_row_jobs"] == c0["split_row_jobs"]


def test_the_row_splitter_still_answers_6_for_records(native, dev):
    from brpc_amd.ops import pb_split_rows
    _, msg = S.seam_message()
    t = torch.from_numpy(np.frombuffer(msg, dtype=np.uint8).copy()).to(dev)
    with pytest.raises(ValueError, match="use the host parser"):
        pb_split_rows(t, 4, "int64", inner=1)


def test_torch_op(native, dev):
    """pb_split_records(pb_build_records(...)) returns the columns, and
    pb_build_records of that returns the bytes."""
    from brpc_amd.ops import pb_build_records, pb_split_records
    specs = [(3, False), (W.FIXED32, False), (0, True), (W.BYTES, False), (6, False), (W.FIXED64, True), (5, True)]
    rows = 300
    columns = S.make_columns(specs, rows, 17, 9)
    build = [(c["inner"], _tensor(c, dev), None if c["ends"] is None else
              torch.from_numpy(c["ends"].astype(np.int32)).to(dev), NAMES[c["kind"]][0]) for c in columns]
    built = pb_build_records(4, build)
    names = [(c["inner"], NAMES[c["kind"]][0], c["ends"] is None) for c in columns]
    got = pb_split_records(built, 4, names)
    for (values, row_ends), c, (want_values, want_ends) in zip(got, columns, S.expected(columns)):
        assert values.dtype == NAMES[c["kind"]][1]
        assert values.cpu().numpy().tobytes() == want_values
        assert (row_ends is None) == (want_ends is None)
        if row_ends is not None:
            assert row_ends.dtype == torch.int32 and row_ends.tolist() == want_ends
    again = pb_build_records(4, [(inner, values, row_ends, name) for (values, row_ends), (inner, name, _) in
                                 zip(got, names)])
    assert torch.equal(again, built)
    with pytest.raises(ValueError, match=r"300 records, elements per column"):
        pb_split_records(built, 4, names, max_rows=299)
    with pytest.raises(ValueError, match="use the host parser"):
        pb_split_records(built, 4, names[:-1])
    with pytest.raises(ValueError, match="refused"):
        pb_split_records(built, 4, names + [names[0]])
    with pytest.raises(ValueError, match="malformed wire \\(offset %d\\)" % built.numel()):
        pb_split_records(torch.cat([built, torch.tensor([0x0b], dtype=torch.uint8, device=dev)]), 4, names)
