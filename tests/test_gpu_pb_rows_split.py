"""Device row splitter (gpu/device_codec.h DeviceSplitRows and the kernels
behind LaunchPbRowsSplit): a message in HBM whose field `number` repeats once
per row becomes the flat array and the row ends in HBM. Every result is
compared with the host twin (native.pb_split_rows) and with this directory's
pure-python splitter (pb_rows_split_ref.split); values and row_ends sit in a
field of sentinel bytes, checked around the output and over all of it when
the code is 1, 2, 5 or 6. The message starts at a byte that is no multiple of
16 unless a case says otherwise. The twin and the wire rules run without a
GPU in tests/test_pb_rows_split_host.py and
brpc_amd/csrc/tests/pb_rows_split_unittest.cc."""
import json

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import pb_rows_split_ref as R  # noqa: E402
import pb_rows_wire as W  # noqa: E402

SENTINEL = 0xA5
GUARD = 64
EB = {0: 4, 1: 4, 2: 4, 3: 8, 4: 8, 5: 8, 6: 1, W.BYTES: 1, W.FIXED32: 4, W.FIXED64: 8}
# kind -> (kind name of ops.pb, the dtype pb_split_rows returns)
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


def _sentinels(nbytes, dev, align):
    buf = torch.full((GUARD + 16 + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    at = GUARD + (-buf.data_ptr() - GUARD) % 16
    assert (buf.data_ptr() + at) % align == 0
    return buf, at


def _run(native, dev, jobs, ref=True):
    """jobs: dicts with number, inner, kind, msg and optionally cap, row_cap
    (default: the twin's worst case), phase (the message's alignment, default
    5). All jobs go into ONE call. Checks every job against the twin (and the
    python splitter) and the sentinels; returns the twin's tuples."""
    table, keep, wants = [], [], []
    for j in jobs:
        kind, msg = j["kind"], bytes(j["msg"])
        eb = EB[kind]
        cap = j.get("cap", len(msg) // (1 if kind <= W.BYTES else eb))
        row_cap = j.get("row_cap", len(msg) // 2)
        want = tuple(native.pb_split_rows(j["number"], j["inner"], kind, msg, cap, row_cap))
        if ref:
            assert want == R.split(j["number"], j["inner"], kind, msg, cap, row_cap)
        msg_t, msg_p = _place(msg, dev, j.get("phase", 5))
        vals, vat = _sentinels(cap * eb, dev, 16)
        ends, eat = _sentinels(row_cap * 4, dev, 16)
        keep.append((msg_t, vals, vat, ends, eat))
        wants.append(want)
        table.append((j["number"], j["inner"], kind, msg_p if msg else 0, len(msg), vals.data_ptr() + vat, cap,
                      ends.data_ptr() + eat, row_cap))
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    res = native.gpu.device_split_rows(table, 0)
    for i, ((count, rows, others, err, first_bad), want, (_, vals, vat, ends, eat)) in enumerate(zip(res, wants, keep)):
        eb = EB[jobs[i]["kind"]]
        assert (err, count, rows, others, first_bad) == want[:5], "job %d" % i
        hv, he = vals.cpu().numpy(), ends.cpu().numpy()
        nv, ne = (count * eb, rows * 4) if err == 0 else (0, 0)
        assert (hv[:vat] == SENTINEL).all() and (hv[vat + nv:] == SENTINEL).all(), "job %d: bytes around values" % i
        assert (he[:eat] == SENTINEL).all() and (he[eat + ne:] == SENTINEL).all(), "job %d: bytes around row_ends" % i
        if err == 0:
            assert hv[vat:vat + nv].tobytes() == want[5], "job %d: values" % i
            assert he[eat:eat + ne].view(np.uint32).tolist() == want[6], "job %d: row_ends" % i
    return wants


def _job(kind, inner, msg, number=4, **more):
    return dict(number=number, inner=inner, kind=kind, msg=msg, **more)


@pytest.mark.parametrize("kind,inner", R.ALL)
def test_chunk_seams(native, dev, kind, inner):
    msg, arr = R.boundary_message(kind, inner)
    (want,) = _run(native, dev, [_job(kind, inner, msg)])
    assert want[:3] == (0, arr.size, R.BOUNDARY_ENDS.size)
    assert want[5] == ((arr != 0).astype(np.uint8) if kind == 6 else arr).tobytes()


@pytest.mark.parametrize("skip", [1, 3, 64])
def test_every_span_of_the_serial_hops(native, dev, skip):
    """-device_split_skip 1 (the chase hops chunk by chunk, no skip table), 3
    (landings that are no multiple of anything) and 64 (one hop spans the
    whole message); the default of 8 runs everywhere else. A malformed field
    in the last chunk is found behind every kind of hop."""
    msgs = [(k, i, R.boundary_message(k, i)[0]) for k, i in ((1, 2), (W.FIXED64, 2), (W.BYTES, 0))]
    jobs = [_job(k, i, m) for k, i, m in msgs] + [_job(k, i, m + b"\x0b") for k, i, m in msgs]
    native.set_flag("device_split_skip", str(skip))
    try:
        wants = _run(native, dev, jobs)
    finally:
        native.set_flag("device_split_skip", "8")
    assert [w[0] for w in wants] == [0, 0, 0, 1, 1, 1]
    assert [w[4] for w in wants[3:]] == [len(m) for _, _, m in msgs]


@pytest.mark.parametrize("kind,inner", [(1, 2), (W.FIXED32, 2), (W.BYTES, 0)])
def test_every_byte_of_a_row_on_a_chunk_end(native, dev, kind, inner):
    """A foreign bytes field of every length 0..40 in front, 41 jobs of one
    call: every byte of a tag, a length, a sub-header and a payload's end
    falls on a chunk end once."""
    msg, arr = R.boundary_message(kind, inner)
    jobs = [_job(kind, inner, R.bytes_field(9, b"\x22" * length) + msg) for length in range(41)]
    for want in _run(native, dev, jobs):
        assert (want[0], want[1], want[3]) == (0, arr.size, 1)


def test_payload_that_looks_like_wire(native, dev):
    for want in _run(native, dev, [_job(kind, inner, msg) for kind, inner, msg in R.wire_like_cases()]):
        assert want[0] == 0


def test_field_numbers_in_one_call(native, dev):
    jobs = [_job(2, b, R.small_message(2, b, number=a)[0], number=a) for a in R.NUMBERS for b in R.NUMBERS]
    for want in _run(native, dev, jobs):
        assert want[:3] == (0, 203, 6)


def test_foreign_fields_are_counted(native, dev):
    cases = R.foreign_cases()
    for want, case in zip(_run(native, dev, [_job(k, i, m) for k, i, m, _ in cases]), cases):
        assert want[0] == 0 and want[2] == 4 and want[3] == case[3]


def test_noncanonical_varints_are_accepted(native, dev):
    for want in _run(native, dev, [_job(k, i, m) for k, i, m in R.noncanonical_cases()]):
        assert want[:4] == (0, 6, 3, 1)


def test_malformed_messages(native, dev):
    cases = R.malformed_cases()
    for want, case in zip(_run(native, dev, [_job(k, i, m) for k, i, m in cases]), cases):
        assert want[0] == 1 and want[4] < len(case[2])
    codes = [w[0] for w in _run(native, dev, [_job(k, i, m) for k, i, m in R.cut_cases()])]
    assert set(codes) == {0, 1} and codes.count(1) >= 18


def test_unsupported_shapes(native, dev):
    cases = R.unsupported_cases()
    for want, case in zip(_run(native, dev, [_job(k, i, m) for k, i, m, _ in cases]), cases):
        assert want[0] == case[3]


@pytest.mark.parametrize("kind,inner", [(1, 2), (W.FIXED64, 2), (W.BYTES, 3)])
def test_capacities(native, dev, kind, inner):
    msg, arr = R.boundary_message(kind, inner)
    rows = R.BOUNDARY_ENDS.size
    wants = _run(native, dev, [_job(kind, inner, msg, cap=arr.size, row_cap=rows),
                               _job(kind, inner, msg, cap=arr.size - 1, row_cap=rows),
                               _job(kind, inner, msg, cap=arr.size, row_cap=rows - 1)])
    assert [w[0] for w in wants] == [0, 5, 5]
    assert all(w[1:3] == (arr.size, rows) for w in wants)


@pytest.mark.parametrize("kind,inner", [(5, 2), (W.FIXED64, 2), (W.BYTES, 0)])
def test_every_message_alignment(native, dev, kind, inner):
    msg, arr = R.boundary_message(kind, inner)
    for want in _run(native, dev, [_job(kind, inner, msg, phase=p) for p in range(16)]):
        assert want[:2] == (0, arr.size)


def test_refusals_reach_no_kernel(native, dev):
    msg, arr = R.small_message(1, 2)
    msg_t, msg_p = _place(msg, dev, 5)
    vals = torch.zeros(1024, dtype=torch.int32, device=dev)
    ends = torch.zeros(64, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    good = (4, 2, 1, msg_p, len(msg), vals.data_ptr(), 1024, ends.data_ptr(), 64)

    def with_(**kw):
        names = ["number", "inner", "kind", "msg", "n", "values", "cap", "row_ends", "row_cap"]
        return tuple(kw.get(k, v) for k, v in zip(names, good))
    bad = [with_(number=0), with_(number=2**29), with_(inner=2**29), with_(kind=10), with_(inner=0), with_(msg=0),
           with_(values=0), with_(values=vals.data_ptr() + 2), with_(row_ends=0), with_(row_ends=ends.data_ptr() + 2),
           with_(msg=12345, n=native.gpu.device_split_max_bytes() + 1)]
    c0 = native.gpu.device_codec_stats()
    res = native.gpu.device_split_rows(bad, 0)
    c1 = native.gpu.device_codec_stats()
    assert [r[3] for r in res] == [2] * len(bad)
    assert c1["split_row_jobs"] == c0["split_row_jobs"] and c1["split_rows"] == c0["split_rows"]
    (count, rows, others, err, _), = native.gpu.device_split_rows([good], 0)
    assert (count, rows, others, err) == (arr.size, 6, 0, 0)
    assert native.gpu.device_split_rows([with_(n=0, msg=0)], 0) == [(0, 0, 0, 0, 2**64 - 1)]


def test_a_refused_and_a_malformed_job_leave_the_others_alone(native, dev):
    a, a_arr = R.boundary_message(3, 1)
    b, b_arr = R.boundary_message(W.FIXED64, 2)
    c, c_arr = R.small_message(W.BYTES, 0)
    jobs = [_job(3, 1, a), _job(3, 1, a, number=0), _job(3, 1, a + b"\x0b"), _job(W.FIXED64, 2, b), _job(W.BYTES, 0, c)]
    c0 = native.gpu.device_codec_stats()
    wants = _run(native, dev, jobs)
    c1 = native.gpu.device_codec_stats()
    assert [w[0] for w in wants] == [0, 2, 1, 0, 0]
    assert wants[2][4] == len(a)
    assert c1["split_row_jobs"] - c0["split_row_jobs"] == 3
    assert c1["split_rows"] - c0["split_rows"] == 2 * R.BOUNDARY_ENDS.size + 6


@pytest.mark.parametrize("kind,inner", R.ALL)
def test_round_trip_with_the_builder_and_the_host_serializer(native, dev, tmp_path, kind, inner):
    """device_build_rows -> device_split_rows gives the inputs back (bools as
    0 / 1), and the host serializer's bytes split to the same arrays."""
    from brpc_amd.ops import pb_build_rows, pb_split_rows
    sizes = [0, 3, 0, 0, 2045, 1, 2, 700, 0, 64, 63, 65, 0]
    arr = W.values(kind, sum(sizes), 200 + kind)
    ends = np.cumsum(sizes).astype(np.int32)
    name, dtype = NAMES[kind]
    signed = {"uint32": "int32", "uint64": "int64"}.get(arr.dtype.name, arr.dtype.name)
    vals_t = torch.from_numpy(arr.view(signed).copy()).to(dev)
    ends_t = torch.from_numpy(ends.copy()).to(dev)
    built = pb_build_rows(4, vals_t, ends_t, name, inner=inner or None)
    values, row_ends = pb_split_rows(built, 4, name, inner=inner or None)
    back = (arr != 0).astype(np.uint8) if kind == 6 else arr
    assert values.dtype == dtype and row_ends.dtype == torch.int32
    assert values.cpu().numpy().tobytes() == back.tobytes()
    assert row_ends.cpu().numpy().tolist() == ends.tolist()
    assert torch.equal(pb_build_rows(4, values, row_ends, name, inner=inner or None), built)
    wire, _, _ = W.host_wire(native, tmp_path, kind, 4, inner, arr, ends)
    (want,) = _run(native, dev, [_job(kind, inner, wire)])
    assert want[0] == 0 and want[5] == back.tobytes() and want[6] == ends.tolist()


def test_json_text_to_rows_and_back(native, dev):
    from brpc_amd.ops import json_parse_float_rows, pb_build_rows, pb_split_rows
    sizes = [3, 1, 700, 2, 65]
    arr = W.values(W.FIXED32, sum(sizes), 11)
    ends = np.cumsum(sizes)
    rows = [[float(x) for x in arr[e - s:e]] for s, e in zip(sizes, ends)]
    text = torch.from_numpy(np.frombuffer(json.dumps(rows).encode(), dtype=np.uint8).copy()).to(dev)
    vals, row_ends = json_parse_float_rows(text, torch.float32, ragged=True)
    values, back_ends = pb_split_rows(pb_build_rows(4, vals, row_ends, "float32", inner=2), 4, "float32", inner=2)
    assert torch.equal(values, vals) and back_ends.tolist() == ends.tolist()
    with pytest.raises(ValueError, match="use the host parser"):
        pb_split_rows(torch.tensor([0x22, 0x02, 0x10, 0x07], dtype=torch.uint8, device=dev), 4, "float32", inner=2)
    with pytest.raises(ValueError, match="offset 2"):
        pb_split_rows(torch.tensor([0x22, 0x00, 0x23], dtype=torch.uint8, device=dev), 4, "float32", inner=2)


@pytest.mark.parametrize("kind,per", [(1, 1), (W.FIXED32, 1024)])
def test_one_long_chase(native, dev, kind, per):
    """1 MiB of one-element uint32 rows (every chunk has an entry and ~800
    rows) and 1 MiB of 1024-float rows (most chunks are jumped over); against
    the twin."""
    if kind == 1:
        arr = np.random.default_rng(3).integers(0, 128, 2**20 // 5).astype(np.uint32)
        image = np.empty((arr.size, 5), dtype=np.uint8)  # tag, 3, inner tag, 1, the value
        image[:, :4] = [0x22, 3, 0x12, 1]
        image[:, 4] = arr
        msg = image.tobytes()
    else:
        arr = W.values(kind, 2**18, 3)
        msg = W.reference(4, 2, kind, arr, np.arange(per, arr.size + 1, per))
    ends = np.arange(per, arr.size + 1, per)
    assert 2**20 - 8192 <= len(msg) <= 2**20 + 8192
    (want,) = _run(native, dev, [_job(kind, 2, msg)], ref=False)
    assert want[:3] == (0, arr.size, ends.size) and want[5] == arr.tobytes()
