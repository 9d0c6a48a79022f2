"""Device message builder (gpu/device_codec.h DeviceBuildMessages and the
kernels behind LaunchPbMsgEncode): arrays in HBM become one serialized
protobuf message in HBM. Every message is compared byte for byte with this
file's own numpy serializer; the builder's own host checks run without a GPU
in brpc_amd/csrc/tests/device_message_unittest.cc."""
import threading

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

BYTES = 7
# kind -> (numpy dtype of the source array, wire value of each element)
_PB_KINDS = {
    0: ("int32", lambda a: a.astype("int64").view("uint64")),        # int32: sign-extended, 10 bytes if < 0
    1: ("uint32", lambda a: a.astype("uint64")),
    2: ("int32", lambda a: ((a.astype("int64") << 1) ^ (a.astype("int64") >> 63)).view("uint64") & 0xFFFFFFFF),
    3: ("int64", lambda a: a.view("uint64")),
    4: ("uint64", lambda a: a),
    5: ("int64", lambda a: ((a << 1) ^ (a >> 63)).view("uint64")),
    6: ("uint8", lambda a: (a != 0).astype("uint64")),               # any nonzero byte is true
}


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _varints(wire):
    """Vectorized protobuf varint encoding of a uint64 array."""
    wire = wire.astype(np.uint64)
    nbytes = np.ones(wire.shape, dtype=np.int64)
    for k in range(1, 10):
        nbytes += (wire >> np.uint64(7 * k)) > 0
    start = np.cumsum(nbytes) - nbytes
    out = np.zeros(int(nbytes.sum()), dtype=np.uint8)
    for k in range(10):
        m = nbytes > k
        byte = ((wire[m] >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8)
        byte |= np.where(nbytes[m] > k + 1, 0x80, 0).astype(np.uint8)
        out[start[m] + k] = byte
    return out.tobytes()


def _values(kind, n, seed):
    """Every varint length 1..10 next to each other: small values, full-width
    ones, negative int32 (10 bytes), both signs under zigzag; bools are any
    byte."""
    rng = np.random.default_rng(seed)
    if kind == 6:
        v = rng.integers(0, 256, n).astype(np.uint8)
        v[::2] = 0
        return v
    if kind in (0, 2):
        v = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        v[::3] = rng.integers(-100, 100, len(v[::3]))
        return v
    if kind == 1:
        return rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 32, n).astype(np.uint32)
    if kind in (3, 5):
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) >> rng.integers(0, 63, n)
    return rng.integers(0, 2**64 - 1, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)


def _payload(kind, arr):
    return arr.tobytes() if kind == BYTES else _varints(_PB_KINDS[kind][1](arr))


def _reference(fields):
    """fields: [(number, kind, numpy array)] -> (message bytes, [(off, len)])
    as the host serializer writes them: packed fields of no element are
    omitted, bytes fields never."""
    out, pos = bytearray(), []
    for number, kind, arr in fields:
        if kind != BYTES and arr.size == 0:
            pos.append((0, 0))
            continue
        p = _payload(kind, arr)
        out += _varint((number << 3) | 2) + _varint(len(p))
        pos.append((len(out), len(p)))
        out += p
    return bytes(out), pos


def _upload(arr, dev):
    """The array's memory in HBM (as uint8: torch has no ops on the unsigned
    wide types, and the builder takes raw pointers)."""
    raw = np.frombuffer(arr.tobytes(), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(dev) if raw.size else torch.empty(0, dtype=torch.uint8, device=dev)


def _rows(fields, tensors):
    rows = []
    for (number, kind, arr), t in zip(fields, tensors):
        count = arr.nbytes if kind == BYTES else arr.size
        rows.append((number, kind, t.data_ptr() if count else 0, count))
    return rows


def _build(native, dev, fields, slack=0):
    """Builds `fields` into a fresh buffer of the worst-case size; returns
    (message bytes, err, positions)."""
    tensors = [_upload(arr, dev) for _, _, arr in fields]
    rows = _rows(fields, tensors)
    cap = native.gpu.device_message_worst_case(rows) + slack
    dst = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    n, err, pos = native.gpu.device_build_message(rows, dst.data_ptr(), cap, 0)
    return dst[:n].cpu().numpy().tobytes() if err == 0 else b"", err, [tuple(p) for p in pos]


COUNTS = (1, 255, 256, 257, 2047, 2048, 2049, 100003)


@pytest.mark.parametrize("kind", sorted(_PB_KINDS))
def test_packed_fields_of_every_kind_match_the_reference(dev, kind):
    """One message of eight packed fields: one element, around the 256
    elements of a round, around the 2048 of a chunk, and ~49 chunks."""
    from brpc_amd import native
    dtype = _PB_KINDS[kind][0]
    fields = [(i + 1, kind, _values(kind, n, seed=kind * 100 + i).astype(dtype)) for i, n in enumerate(COUNTS)]
    want, want_pos = _reference(fields)
    c0 = native.gpu.device_codec_stats()
    got, err, pos = _build(native, dev, fields)
    assert err == 0
    assert len(got) == len(want)
    assert got == want
    assert pos == want_pos
    c1 = native.gpu.device_codec_stats()
    assert c1["built_messages"] - c0["built_messages"] == 1
    assert c1["built_fields"] - c0["built_fields"] == len(COUNTS)
    assert c1["built_bytes"] - c0["built_bytes"] == len(want)


def test_headers_of_every_length(dev):
    """Length varints growing at 127/128 and 16383/16384 bytes, tags of 1 to
    5 bytes, the empty fields, and bytes fields around the 16-byte store."""
    from brpc_amd import native
    rng = np.random.default_rng(5)
    numbers = (1, 15, 16, 2047, 2048, 2**29 - 1)
    sizes = (127, 128, 16383, 16384)
    fields = []
    for i in range(12):  # every field number with two of the sizes, every size at least twice
        fields.append((numbers[i % 6], 6, _values(6, sizes[(i + i // 6) % 4], seed=40 + i)))
    fields.append((3, 3, np.zeros(0, dtype=np.int64)))    # packed, no element: omitted
    fields.append((4, BYTES, np.zeros(0, dtype=np.uint8)))  # bytes, empty: tag + 0x00
    for n in (1, 15, 16, 17, 100003):
        fields.append((5, BYTES, rng.integers(0, 256, n).astype(np.uint8)))
    # tensors as bytes fields: the wire form of packed fixed32 / fixed64 / float
    fields.append((6, BYTES, rng.integers(-2**31, 2**31, 1001, dtype=np.int64).astype(np.int32)))
    fields.append((7, BYTES, rng.integers(-2**63, 2**63 - 1, 1001, dtype=np.int64)))
    fields.append((9, BYTES, rng.standard_normal(1001).astype(np.float32)))
    want, want_pos = _reference(fields)
    got, err, pos = _build(native, dev, fields)
    assert err == 0
    assert got == want
    assert pos == want_pos
    assert want_pos[12] == (0, 0)
    at = want_pos[13][0]
    assert want_pos[13][1] == 0 and want[at - 2:at] == b"\x22\x00"
    # the two empty fields alone
    got, err, pos = _build(native, dev, [fields[13]])
    assert (got, err, pos) == (b"\x22\x00", 0, [(2, 0)])
    got, err, pos = _build(native, dev, [fields[12]], slack=16)
    assert (got, err, pos) == (b"", 0, [(0, 0)])


def test_any_destination_alignment_and_exact_capacity(dev):
    from brpc_amd import native
    rng = np.random.default_rng(6)
    fields = [(1, BYTES, rng.integers(0, 256, 40001).astype(np.uint8)),   # 3 bytes chunks
              (8, 3, _values(3, 5000, seed=61)),                         # 3 numeric chunks
              (9, 6, _values(6, 300, seed=62)),
              (10, 2, _values(2, 1, seed=63)),
              (11, 1, _values(1, 4100, seed=64))]
    want, want_pos = _reference(fields)
    # sources at their natural alignment only: the bytes field at an odd
    # address, the 64-bit field 8 and the 32-bit fields 4 bytes off a 16-byte
    # boundary (every other test's sources are 16-byte aligned)
    shift = (3, 8, 0, 4, 4)
    tensors = [_upload(np.frombuffer(bytes(sh) + arr.tobytes(), dtype=np.uint8), dev)
               for sh, (_, _, arr) in zip(shift, fields)]
    rows = [(number, kind, ptr + sh, count) for sh, (number, kind, ptr, count) in zip(shift, _rows(fields, tensors))]
    front = 32
    for off in (0, 1, 7, 15):
        buf = torch.full((front + off + len(want) + 64,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # torch fills/copies run on its own stream
        n, err, pos = native.gpu.device_build_message(rows, buf.data_ptr() + front + off, len(want), 0)  # cap == len
        assert (n, err) == (len(want), 0), off
        assert [tuple(p) for p in pos] == want_pos
        host = buf.cpu().numpy()
        assert host[front + off:front + off + n].tobytes() == want, off
        assert (host[:front + off] == 0xA5).all() and (host[front + off + n:] == 0xA5).all(), off
        # one byte short: refused as a whole, nothing written
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        n, err, pos = native.gpu.device_build_message(rows, buf.data_ptr() + front + off, len(want) - 1, 0)
        assert err == 3 and n == len(want), (off, n, err)
        assert (buf.cpu().numpy() == 0xA5).all(), off


def test_malformed_jobs_are_refused(dev):
    from brpc_amd import native
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    dst = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p, d = src.data_ptr(), dst.data_ptr()
    bad = [
        ([(1, 9, p, 4)], d),                # kind 9
        ([(0, 3, p, 4)], d),                # field number 0
        ([(1, 6, p, 1)] * 129, d),          # 129 fields
        ([(1, 3, p + 4, 4)], d),            # misaligned int64 source
        ([(1, 3, p, 4)], 0),                # null destination
    ]
    c0 = native.gpu.device_codec_stats()
    for rows, to in bad:
        n, err, pos = native.gpu.device_build_message(rows, to, 4096, 0)
        assert (n, err) == (0, 2), rows[:2]
    c1 = native.gpu.device_codec_stats()
    assert c1["build_errors"] - c0["build_errors"] == len(bad)
    assert c1["built_messages"] == c0["built_messages"]
    assert (dst.cpu().numpy() == 0xA5).all()


def test_built_message_round_trips_through_the_device_decoder(dev):
    """Build, scan and decode, all in HBM: the table of the built message
    locates every field, and the packed fields decode to the source arrays."""
    from brpc_amd import native
    rng = np.random.default_rng(8)
    fields = [(1, BYTES, rng.integers(0, 256, 30000).astype(np.uint8)),
              (2, 0, _values(0, 20000, seed=81)),
              (3, 5, _values(5, 7001, seed=82)),
              (4, 6, _values(6, 5000, seed=83))]
    tensors = [_upload(arr, dev) for _, _, arr in fields]
    rows = _rows(fields, tensors)
    cap = native.gpu.device_message_worst_case(rows)
    msg = torch.zeros(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    n, err, pos = native.gpu.device_build_message(rows, msg.data_ptr(), cap, 0)
    assert err == 0
    nf, table = native.gpu.device_pb_scan(msg.data_ptr(), n, 0)
    assert nf == 4
    for (number, kind, arr), (off, ln) in zip(fields, pos):
        assert native.gpu.device_payload_field(nf, table, number) == (off, ln)
    assert native.gpu.device_payload_field(nf, table, 5) is None
    host = msg[:n].cpu().numpy()
    assert host[pos[0][0]:pos[0][0] + pos[0][1]].tobytes() == fields[0][2].tobytes()
    outs = [torch.zeros(arr.nbytes, dtype=torch.uint8, device=dev) for _, _, arr in fields[1:]]
    torch.cuda.synchronize()
    res = native.gpu.device_decode_packed([msg.data_ptr() + off for off, _ in pos[1:]], [ln for _, ln in pos[1:]],
                                          [kind for _, kind, _ in fields[1:]], [o.data_ptr() for o in outs], 0)
    for (number, kind, arr), o, (count, code) in zip(fields[1:], outs, res):
        assert code == 0 and count == arr.size, (number, count, code)
        got = np.frombuffer(o.cpu().numpy().tobytes(), dtype=arr.dtype)
        assert np.array_equal(got, (arr != 0).astype(np.uint8) if kind == 6 else arr), number


@pytest.mark.parametrize("kind", sorted(_PB_KINDS))
def test_bare_runs_match_the_host_fed_encoder(dev, kind):
    """device_encode_packed (values in HBM, sizes measured on the device)
    against pb_run_encode (values on the host, sizes computed there)."""
    from brpc_amd import native
    arr = _values(kind, 3001, seed=90 + kind).astype(_PB_KINDS[kind][0])
    want = native.gpu.pb_run_encode(arr.tobytes(), arr.size, kind)
    assert want == _payload(kind, arr)
    src = _upload(arr, dev)
    dst = torch.zeros(10 * arr.size, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    [(n, err)] = native.gpu.device_encode_packed([src.data_ptr()], [arr.size], [kind], [dst.data_ptr()],
                                                 [dst.numel()], 0)
    assert err == 0 and n == len(want)
    assert dst[:n].cpu().numpy().tobytes() == want
    # the decoder keeps refusing the bytes kind, and a bare run has none
    [(_, code)] = native.gpu.device_decode_packed([dst.data_ptr()], [n], [BYTES], [src.data_ptr()], 0)
    assert code == 2
    [(n, err)] = native.gpu.device_encode_packed([src.data_ptr()], [16], [BYTES], [dst.data_ptr()], [dst.numel()], 0)
    assert (n, err) == (0, 2)


def test_concurrent_builds_share_codec_batches(dev):
    """8 threads x 20 different messages at once: every message is right
    whatever the batch it travelled in."""
    from brpc_amd import native
    nthreads, per = 8, 20
    jobs = []
    for k in range(nthreads * per):
        rng = np.random.default_rng(1000 + k)
        kind = k % 7
        fields = [(1 + k % 30, kind, _values(kind, 1 + (k * 37) % 5000, seed=k).astype(_PB_KINDS[kind][0])),
                  (40, BYTES, rng.integers(0, 256, (k * 101) % 20000).astype(np.uint8))]
        tensors = [_upload(arr, dev) for _, _, arr in fields]
        rows = _rows(fields, tensors)
        cap = native.gpu.device_message_worst_case(rows)
        dst = torch.zeros(cap, dtype=torch.uint8, device=dev)
        jobs.append((fields, tensors, rows, cap, dst))
    torch.cuda.synchronize()  # torch fills/copies run on its own stream
    results = [None] * len(jobs)

    def work(t):
        for k in range(t * per, (t + 1) * per):
            _, _, rows, cap, dst = jobs[k]
            results[k] = native.gpu.device_build_message(rows, dst.data_ptr(), cap, 0)

    b0 = native.gpu.codec_batch_stats()
    threads = [threading.Thread(target=work, args=(t,)) for t in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    b1 = native.gpu.codec_batch_stats()
    print("codec batch: %d requests in %d launches, %d message chunks" % (
        b1["requests"] - b0["requests"], b1["launches"] - b0["launches"], b1["msg_chunks"] - b0["msg_chunks"]))
    for k, (fields, _, _, _, dst) in enumerate(jobs):
        want, want_pos = _reference(fields)
        n, err, pos = results[k]
        assert (n, err) == (len(want), 0), k
        assert [tuple(p) for p in pos] == want_pos, k
        assert dst[:n].cpu().numpy().tobytes() == want, k


def test_pb_build_message_on_torch_tensors(dev):
    """ops.pb.pb_build_message: tensors in, a trimmed uint8 tensor out; a
    tensor produced by a torch kernel just before the call needs no manual
    synchronize (the op waits for the caller's stream)."""
    from brpc_amd.ops.pb import pb_build_message
    ids = torch.from_numpy(_values(3, 50000, seed=11)).to(dev)
    flags = torch.from_numpy(_values(6, 777, seed=12)).to(dev)
    emb = torch.randn(4096, device=dev)
    fresh = (torch.arange(300001, device=dev, dtype=torch.int64) * 7919 - 1234567) * ids[0].sign()  # still running
    msg, pos = pb_build_message([(1, emb, "bytes"), (2, ids, "sint64"), (3, flags, "bool"), (8, fresh, "int64"),
                                 (9, ids[:0], "int64")])
    assert msg.dtype == torch.uint8 and msg.device == emb.device
    want, want_pos = _reference([(1, BYTES, emb.cpu().numpy()), (2, 5, ids.cpu().numpy()),
                                 (3, 6, flags.cpu().numpy()), (8, 3, fresh.cpu().numpy()),
                                 (9, 3, np.zeros(0, dtype=np.int64))])
    assert msg.numel() == len(want)
    assert msg.cpu().numpy().tobytes() == want
    assert pos == want_pos
    with pytest.raises(ValueError):
        pb_build_message([(0, ids, "int64")])
    with pytest.raises(TypeError):
        pb_build_message([(1, emb, "int64")])
