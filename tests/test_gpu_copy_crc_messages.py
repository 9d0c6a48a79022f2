"""The copy/CRC engine's launched kernels against the host CRC32C.

gpu/kernels.hip copy_crc32c_kernel (byte tables), copy_crc32c_mfma_kernel
(matrix cores) and crc32c_mfma_kernel, with the host code that prepares their
launches (fill_batch, next_group, fold_chunk / flush_run / fold_segment_crc):

  * messages of several segments folded on the device, through the launch the
    copy engine issues by default (LaunchBatchedCopyCrc32cMessages) and through
    the engine itself (BatchedCopy with fold_crc);
  * the fused MFMA kernel walking 2 and 3 chunks per workgroup (launches of
    more than 2048 and more than 4096 chunks of 16 KiB);
  * crc32c_packed with more chunks than waves, more segments than the scan
    kernel has lanes, and a segment past the initial x^(8*64KiB*m) table.

The reference is the host SSE4.2 CRC over a message's concatenated bytes; the
unmarked tests pin it to a bit-at-a-time CRC32C and to known vectors. Every CRC
comparison is exact and every destination buffer is compared byte for byte,
the bytes between and around the destinations included."""
import functools
import random
import threading

import pytest

torch = pytest.importorskip("torch")

C = 16384  # chunk of the fused copy + CRC kernels (kChunkBytes)
MiB = 1 << 20
FILL = 0xEE  # every destination byte before a launch
GARBAGE = 0x5A5A5A5A


def _crc32c_bitwise(data):
    """CRC32C one bit at a time: reflected polynomial 0x82F63B78, register
    starts at ~0 and is inverted at the end."""
    crc = 0xFFFFFFFF
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


# ---------------------------------------------------------------- the reference, without a GPU
def test_host_crc_matches_bitwise_every_short_length():
    from brpc_amd.ops import crc32c_host
    data = random.Random(11).randbytes(300)
    for n in range(301):
        assert crc32c_host(data[:n]) == _crc32c_bitwise(data[:n]), n


def test_host_crc_matches_bitwise_random_lengths():
    from brpc_amd.ops import crc32c_host
    rnd = random.Random(12)
    for _ in range(20):
        n = rnd.randint(301, 70000)
        data = rnd.randbytes(n)
        assert crc32c_host(data) == _crc32c_bitwise(data), n


@pytest.mark.parametrize("data,want", [
    (b"123456789", 0xE3069283),
    (bytes(32), 0x8A9136AA),
    (b"\xff" * 32, 0x62A8AB43),
    (bytes(range(32)), 0x46DD794E),
    (bytes(range(31, -1, -1)), 0x113FDB5C),
])
def test_host_crc_known_vectors(data, want):
    from brpc_amd.ops import crc32c_host
    assert _crc32c_bitwise(data) == want
    assert crc32c_host(data) == want


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    assert native.gpu.device_arch(0) == "gfx950"
    return torch.device("cuda", 0)


def _u32(t):
    return [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]


# (a) segment lengths of each message of the shapes call
SHAPES = [
    [1],
    [0],
    [0, 0, 0],
    [0, 5, 0],
    [C],
    [C - 1, 1],
    [1, C],
    [C + 1, C - 1],
    [7, 3 * C + 5, 9],
    [100, 40000, 0, 1, 33000],
    [64] * 32,
]
FIRST_MSG = 3


class _Call:
    """The segments of a list of messages laid out for one launch: segment
    k's source at phase (3 + 5k) % 16 of a device buffer (every third one in
    pinned host memory instead), its destination 7 phases further, every
    fourth segment checksum-only (dst 0), at least 16 fill bytes before and
    after each destination."""

    def __init__(self, dev, msgs, seed=1234):
        self.lens = [n for m in msgs for n in m]
        self.msg_of = [FIRST_MSG + i for i, m in enumerate(msgs) for _ in m]
        self.nmsg = len(msgs)
        spos, dpos = [], []
        s_cur = d_cur = 16
        for k, n in enumerate(self.lens):
            spos.append(s_cur + (3 + 5 * k) % 16)
            s_cur = (spos[-1] + n + 15) // 16 * 16 + 16
            if k % 4 == 3:
                dpos.append(None)
                continue
            dpos.append(d_cur + (10 + 5 * k) % 16)
            d_cur = (dpos[-1] + n + 15) // 16 * 16 + 16
        host = torch.randint(0, 256, (s_cur,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        self.src_dev = host.to(dev)
        self.src_pin = host.clone().pin_memory()
        self.dst = torch.empty(d_cur, dtype=torch.uint8, device=dev)
        self.want_dst = torch.full((d_cur,), FILL, dtype=torch.uint8, device=dev)
        hb = host.numpy().tobytes()
        self.seg_bytes = [hb[p:p + n] for p, n in zip(spos, self.lens)]
        self.srcs, self.dsts = [], []
        for k, (sp, dp, n) in enumerate(zip(spos, dpos, self.lens)):
            assert sp % 16 == (3 + 5 * k) % 16
            self.srcs.append((self.src_pin if k % 3 == 1 else self.src_dev).data_ptr() + sp)
            self.dsts.append(0 if dp is None else self.dst.data_ptr() + dp)
            if dp is not None:
                assert dp % 16 != sp % 16
                self.want_dst[dp:dp + n] = self.src_dev[sp:sp + n]
        from brpc_amd.ops import crc32c_host
        self.seg_crcs = [crc32c_host(b) for b in self.seg_bytes]
        self.msg_crcs, k = [], 0
        for m in msgs:
            self.msg_crcs.append(crc32c_host(b"".join(self.seg_bytes[k:k + len(m)])))
            k += len(m)
        torch.cuda.synchronize()

    def segments_of(self, m):
        return [k for k, x in enumerate(self.msg_of) if x == FIRST_MSG + m]

    def reset_dst(self):
        self.dst.fill_(FILL)
        torch.cuda.synchronize()  # the copy engine runs on a stream of its own

    def check_dst(self, what=""):
        torch.cuda.synchronize()
        assert torch.equal(self.dst, self.want_dst), "destination bytes differ " + str(what)


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [True, False])
def test_messages_launch_segment_shapes(dev, mfma):
    """fill_batch's tail_poly / msg_init / first_of_msg, fold_chunk (or
    flush_run) shifting a segment's chunks by the bytes after it in its
    message, the two-atomic fold of fold_segment_crc with several chunks per
    message and its single-chunk shortcut, next_group splitting the 55
    segments into launches of 23 and 32, and out + msg_of[i]. Three launches on
    one stream with garbage in `out`: the fold scratch is left zeroed."""
    from brpc_amd import native
    from brpc_amd.ops._common import stream_handle
    call = _Call(dev, SHAPES)
    assert call.msg_crcs[2] == 0  # three empty segments
    g = torch.Generator().manual_seed(5)
    for rep in range(3):
        call.reset_dst()
        out = torch.full((FIRST_MSG + call.nmsg + 4,), GARBAGE, dtype=torch.int32, device=dev)
        if rep:
            out[FIRST_MSG:FIRST_MSG + call.nmsg] = torch.randint(0, 2**31 - 1, (call.nmsg,), dtype=torch.int32,
                                                                 generator=g).to(dev)
        native.gpu.batched_copy_crc32c_messages_launch(call.srcs, call.dsts, call.lens, call.msg_of, out.data_ptr(),
                                                       stream_handle(dev), mfma)
        torch.cuda.synchronize()
        got = _u32(out)
        assert got[FIRST_MSG:FIRST_MSG + call.nmsg] == call.msg_crcs, rep
        assert got[:FIRST_MSG] == [GARBAGE] * FIRST_MSG, rep
        assert got[FIRST_MSG + call.nmsg:] == [GARBAGE] * 4, rep
        call.check_dst(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [True, False])
def test_messages_launch_refuses_a_message_over_one_group(dev, mfma):
    """next_group returning false: 33 segments of one message launch nothing."""
    from brpc_amd import native
    from brpc_amd.ops._common import stream_handle
    call = _Call(dev, [[64] * 33])
    call.reset_dst()
    out = torch.full((FIRST_MSG + 2,), GARBAGE, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        native.gpu.batched_copy_crc32c_messages_launch(call.srcs, call.dsts, call.lens, call.msg_of, out.data_ptr(),
                                                       stream_handle(dev), mfma)
    torch.cuda.synchronize()
    assert _u32(out) == [GARBAGE] * (FIRST_MSG + 2)
    assert int((call.dst != FILL).sum()) == 0
    with pytest.raises(ValueError):  # list sizes
        native.gpu.batched_copy_crc32c_messages_launch(call.srcs, call.dsts, call.lens, call.msg_of[:-1],
                                                       out.data_ptr(), stream_handle(dev), mfma)
    with pytest.raises(ValueError):  # message numbers are consecutive: a gap would leave fill_batch's 32 slots
        native.gpu.batched_copy_crc32c_messages_launch(call.srcs[:2], call.dsts[:2], call.lens[:2], [0, 2],
                                                       out.data_ptr(), stream_handle(dev), mfma)
    torch.cuda.synchronize()
    assert _u32(out) == [GARBAGE] * (FIRST_MSG + 2)


@pytest.mark.gpu
def test_messages_wrapper(dev):
    """ops.batched_copy_crc32c_messages: one CRC per message, None = checksum only."""
    from brpc_amd.ops import batched_copy_crc32c_messages, crc32c_host
    src = torch.randint(0, 256, (3 * C + 50,), dtype=torch.uint8, device=dev)
    parts = [src[1:9], src[9:9 + C + 3], src[C + 12:], src[:0], src[5:77]]
    dsts = [torch.zeros_like(p) for p in parts]
    dsts[2] = None
    got = batched_copy_crc32c_messages(parts, dsts, [7, 7, 7, 8, 9]).tolist()
    hb = src.cpu().numpy().tobytes()
    assert got == [crc32c_host(hb[1:]), 0, crc32c_host(hb[5:77])]
    for p, d in zip(parts, dsts):
        assert d is None or torch.equal(p, d)


# ---------------------------------------------------------------- (c) the copy engine
THREAD_LENS = [0, 1, 7, 100, 4096, 16384, 16385, 65537]


def _engine_threads(dev, nthreads=6, rounds=10):
    """Submissions from several threads at once: batches that hold several
    submissions (BatchedCopy's first / first_msg offsets into the batch)."""
    from brpc_amd import native
    from brpc_amd.ops import crc32c_host
    size = 1 << 20
    host = torch.randint(0, 256, (size,), dtype=torch.uint8, generator=torch.Generator().manual_seed(77))
    src = host.to(dev)
    pin = host.clone().pin_memory()
    hb = host.numpy().tobytes()
    torch.cuda.synchronize()
    errors = []

    def worker(seed):
        r = random.Random(seed)
        cap = 40 * (65537 + 40) + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        try:
            for rnd in range(rounds):
                n = r.randint(1, 40)
                fold = r.random() < 0.5
                out.fill_(FILL)
                want = torch.full((cap,), FILL, dtype=torch.uint8, device=dev)
                srcs, dsts, lens, blobs = [], [], [], []
                pos = 16 + r.randint(0, 15)
                for i in range(n):
                    ln = r.choice(THREAD_LENS)
                    off = r.randint(0, size - ln)
                    srcs.append((pin if r.random() < 0.3 else src).data_ptr() + off)
                    if r.random() < 0.2:
                        dsts.append(0)
                    else:
                        dsts.append(out.data_ptr() + pos)
                        want[pos:pos + ln] = src[off:off + ln]
                        pos += ln + r.randint(16, 31)
                    lens.append(ln)
                    blobs.append(hb[off:off + ln])
                torch.cuda.synchronize()
                crcs = list(native.gpu.engine_copy(srcs, dsts, lens, 0, True, fold))
                ref = [crc32c_host(b"".join(blobs))] if fold else [crc32c_host(b) for b in blobs]
                if crcs != ref:
                    errors.append("crc mismatch seed=%d round=%d n=%d fold=%s lens=%s" % (seed, rnd, n, fold, lens))
                if not torch.equal(out, want):
                    errors.append("copy mismatch seed=%d round=%d n=%d lens=%s" % (seed, rnd, n, lens))
        except Exception as e:  # a thread's failure must reach the test
            errors.append("seed=%d: %r" % (seed, e))

    ths = [threading.Thread(target=worker, args=(s,)) for s in range(nthreads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return errors


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", ["true", "false"])
def test_copy_engine_folds_messages_on_the_launch_path(dev, mfma):
    """BatchedCopy with the resident worker off: each submission is a message
    of the launch (fold), or one message per segment (no fold); 40 segments
    are folded on the host with crc32c::Combine; threads merge submissions
    into one batch."""
    from brpc_amd import native
    assert native.get_flag("copy_engine_resident") == "false"
    saved = {f: native.get_flag(f) for f in ("copy_engine_crc_mfma", "copy_engine_crc_mfma_min_bytes")}
    native.set_flag("copy_engine_crc_mfma", mfma)
    native.set_flag("copy_engine_crc_mfma_min_bytes", "0")
    try:
        many = [(17 * i) % 300 for i in range(40)]
        call = _Call(dev, SHAPES + [many])
        for fold in (True, False):
            call.reset_dst()
            for m in range(call.nmsg):
                ks = call.segments_of(m)
                got = list(native.gpu.engine_copy([call.srcs[k] for k in ks], [call.dsts[k] for k in ks],
                                                  [call.lens[k] for k in ks], 0, True, fold))
                want = [call.msg_crcs[m]] if fold else [call.seg_crcs[k] for k in ks]
                assert got == want, (m, fold)
            call.check_dst(fold)
        errors = _engine_threads(dev)
        assert not errors, errors[:5]
    finally:
        for f, v in saved.items():
            native.set_flag(f, v)


# ---------------------------------------------------------------- (d) several chunks per workgroup
# Chunk count of the launch in (2048, 4096]: 2 chunks per workgroup.
WALK2 = [
    5 * C + 100, 3 * C - 7, 100, 0, C, 8 * MiB + 12345, 2 * C, C + 1, 1, 2 * C - 3, 3 * MiB + 1, 0, 4 * MiB - 5,
    6 * MiB + 77, 5 * MiB + C - 1, 7 * MiB + 1, 100003,
]
# ... in (4096, 6144]: 3 chunks per workgroup.
WALK3 = [
    4 * C + 9, C - 1, 7, 0, 3 * C, 50, 3 * C - 100, 100, 300, 2 * C + 1, 9 * MiB + 4321, 8 * MiB + 1, 10 * MiB - 9,
    0, 7 * MiB + C + 1, 6 * MiB + 3, 5 * MiB + 11, 8 * MiB + 8191, 33, 3 * MiB - 1, 4 * MiB + C + 2, 6 * MiB + 100,
]
WALK_SRC_BYTES = 12 * MiB


def _chunks(n):
    return max(1, -(-n // C))


def _walk_offsets(lens):
    """Overlapping views of one source buffer, at phase (3 + 5i) % 16."""
    offs = []
    for i, n in enumerate(lens):
        room = WALK_SRC_BYTES - n - 32
        offs.append((i * 1048583) % room // 16 * 16 + (3 + 5 * i) % 16)
    return offs


def _walk_groupings(lens, per):
    """msg_of lists: three messages by thirds, and one where a segment of
    exactly `per` chunks that starts a workgroup's range is a message alone."""
    n = len(lens)
    thirds = [0 if i < n // 3 else 1 if i < 2 * n // 3 else 2 for i in range(n)]
    starts = [0]
    for x in lens:
        starts.append(starts[-1] + _chunks(x))
    alone = [i for i, x in enumerate(lens) if _chunks(x) == per and starts[i] % per == 0]
    assert alone and 0 < alone[0] < n - 1
    j = alone[0]
    own = [0 if i < j else 1 if i == j else 2 for i in range(n)]
    return thirds, own, j


@functools.lru_cache(maxsize=None)
def _walk_reference(per):
    """Host bytes of the source buffer and the host CRC of every segment and
    of every message of both groupings: computed once per list."""
    from brpc_amd.ops import crc32c_host
    lens = {2: WALK2, 3: WALK3}[per]
    host = torch.randint(0, 256, (WALK_SRC_BYTES,), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(100 + per))
    hb = host.numpy().tobytes()
    offs = _walk_offsets(lens)
    blobs = [hb[o:o + n] for o, n in zip(offs, lens)]
    seg = [crc32c_host(b) for b in blobs]
    thirds, own, _ = _walk_groupings(lens, per)
    msgs = [[crc32c_host(b"".join(b for b, m in zip(blobs, g) if m == k)) for k in range(3)] for g in (thirds, own)]
    return host, seg, msgs[0], msgs[1]


@pytest.mark.gpu
@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("per", [2, 3])
def test_copy_crc_more_chunks_than_workgroups(dev, per, mfma):
    """copy_crc32c_mfma_kernel with `per` chunks per workgroup: the Horner
    step across the chunks of a run (c_x2n[17]), runs that begin inside a
    segment (has_first false) and end inside one (after_last > 0, beyond the
    128-entry table for the segments over 2 MiB), a flush at a segment change
    inside a workgroup's range, one-chunk and empty segments inside a range,
    fold_segment_crc adding r.n > 1 to a message's count, and its shortcut for
    a message that one workgroup holds whole. The byte-table kernel runs the
    same lists with one workgroup per chunk."""
    from brpc_amd import native
    from brpc_amd.ops._common import stream_handle
    lens = {2: WALK2, 3: WALK3}[per]
    nseg = len(lens)
    assert nseg <= 32
    counts = [_chunks(n) for n in lens]
    nchunks = sum(counts)
    assert -(-nchunks // min(nchunks, 2048)) == per
    starts = [sum(counts[:i]) for i in range(nseg)]
    # the list is what the docstring says it is
    assert any(s % per == 0 for s in starts[1:]) and any(s % per for s in starts)
    assert any(c == 1 and n > 0 and s % per == 1 for c, n, s in zip(counts, lens, starts))
    assert any(n == 0 and s % per == 1 for n, s in zip(lens, starts))
    assert any(n > 2 * MiB for n in lens) and any(n % C for n in lens)
    thirds, own, alone = _walk_groupings(lens, per)
    host, want_seg, want_thirds, want_own = _walk_reference(per)
    offs = _walk_offsets(lens)
    assert any(o % 16 for o in offs)
    src = host.to(dev)
    # about half of the 3-chunk list is only checksummed (memory); some of the other
    only_crc = [(i % 2 == 1) if per == 3 else (i % 5 == 4) for i in range(nseg)]
    dpos, d_cur = [], 16
    for i, n in enumerate(lens):
        dpos.append(d_cur + (10 + 5 * i) % 16)
        if not only_crc[i]:
            d_cur = (dpos[-1] + n + 15) // 16 * 16 + 16
    dst = torch.empty(d_cur, dtype=torch.uint8, device=dev)
    want_dst = torch.full((d_cur,), FILL, dtype=torch.uint8, device=dev)
    for i, n in enumerate(lens):
        if not only_crc[i]:
            want_dst[dpos[i]:dpos[i] + n] = src[offs[i]:offs[i] + n]
    srcs = [src.data_ptr() + o for o in offs]
    dsts = [0 if only_crc[i] else dst.data_ptr() + dpos[i] for i in range(nseg)]
    stream = stream_handle(dev)

    def run(msg_of, nout):
        dst.fill_(FILL)
        out = torch.full((nout + 2,), GARBAGE, dtype=torch.int32, device=dev)
        if msg_of is None:
            native.gpu.batched_copy_crc32c_launch(srcs, dsts, lens, out.data_ptr(), stream, mfma)
        else:
            native.gpu.batched_copy_crc32c_messages_launch(srcs, dsts, lens, msg_of, out.data_ptr(), stream, mfma)
        torch.cuda.synchronize()
        got = _u32(out)
        assert got[nout:] == [GARBAGE] * 2
        assert torch.equal(dst, want_dst), "destination bytes differ"
        return got[:nout]

    got = run(None, nseg)
    assert got == want_seg, [i for i in range(nseg) if got[i] != want_seg[i]]
    assert run(thirds, 3) == want_thirds
    assert counts[alone] == per and starts[alone] % per == 0
    assert run(own, 3) == want_own


# ---------------------------------------------------------------- crc32c_packed beyond one turn
@pytest.mark.gpu
def test_crc32c_packed_more_chunks_than_waves(dev):
    """9001 segments, 9004 chunks of 64 KiB: scan_tiles_kernel gives each of
    its 1024 lanes 9 entries, and the 8192 waves of crc32c_mfma_kernel's
    capped grid take a second turn of the `chunk += nwaves` loop."""
    from brpc_amd.ops import crc32c_host, crc32c_packed
    cycle = [0, 1, 63, 64, 65, 300, 2048, 2049]
    sizes = [cycle[i % 8] for i in range(8999)]
    sizes.insert(4500, 65537)
    sizes.insert(7000, 3 * 65536)
    assert len(sizes) == 9001
    assert sum(max(1, -(-n // 65536)) for n in sizes) > 2048 * 4
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    host = torch.randint(0, 256, (offs[-1],), dtype=torch.uint8, generator=torch.Generator().manual_seed(9001))
    got = crc32c_packed(host.to(dev), torch.tensor(offs, dtype=torch.int64, device=dev)).tolist()
    hb = host.numpy().tobytes()
    want = [crc32c_host(hb[offs[i]:offs[i + 1]]) for i in range(len(sizes))]
    assert got == want, [i for i in range(len(sizes)) if got[i] != want[i]][:10]


@pytest.mark.gpu
def test_crc32c_packed_segment_past_the_initial_shift_table(dev):
    """A segment of 64 MiB + 4097 bytes has 1025 chunks: its first chunk reads
    xc[1024], one past the 1024 entries ensure_xc starts with, so the table
    grows; a later small launch runs against the table that was kept."""
    from brpc_amd.ops import crc32c, crc32c_host, crc32c_packed
    n = 64 * MiB + 4097
    buf = torch.randint(0, 256, (100 + n,), dtype=torch.uint8, device=dev)
    offs = [0, 100, 100 + n]
    got = crc32c_packed(buf, torch.tensor(offs, dtype=torch.int64, device=dev)).tolist()
    hb = buf.cpu().numpy().tobytes()
    assert got == [crc32c_host(hb[:100]), crc32c_host(hb[100:])]
    assert crc32c(torch.tensor(list(b"123456789"), dtype=torch.uint8, device=dev)) == 0xE3069283
