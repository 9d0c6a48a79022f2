"""The device snappy compressor (gpu/snappy_kernels.hip: compress_wave and
its three kernels) on built inputs: every job is launched from a job table
this file writes itself (exact dst_cap, chosen pointer alignment, chosen
launch mates), into slots pre-filled with a sentinel between guard bytes.
Each stream is checked against the host codec, against the byte-wise decoder
of snappy_stream.py, for untouched bytes around it, for the element forms
the input was built to provoke (a form that does not show up fails the
test), and last through both device decoders."""
import pytest

torch = pytest.importorskip("torch")

import snappy_stream as S  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64  # bytes in front of and behind every destination slot
BLOCKS = S.BLOCKS


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0
    return torch.device("cuda", 0)


def _bound(n):
    from brpc_amd import native
    b = int(native.gpu.snappy_max_compressed_length(n))
    assert b == 32 + n + n // 6
    return b


def _launch(dev, datas, max_ulen, caps, src_off, dst_off):
    """One compress launch. Job i reads datas[i] at byte offset src_off of a
    16-byte boundary and writes a slot of caps[i] bytes at offset dst_off of
    one. Returns (errs, out_lens, destination bytes, slot starts, slot area
    ends): the area of job i is [start - GUARD - dst_off, end)."""
    from brpc_amd import native
    from brpc_amd.ops._common import stream_handle
    n = len(datas)
    src_at, pos = [], 0
    for d in datas:
        src_at.append(pos + src_off)
        pos = (pos + src_off + len(d) + 15) & ~15
    src_host = bytearray(max(pos, 16))
    for at, d in zip(src_at, datas):
        src_host[at:at + len(d)] = d
    starts, ends, pos = [], [], 0
    for cap in caps:
        starts.append(pos + GUARD + dst_off)
        pos = (pos + GUARD + dst_off + cap + GUARD + 15) & ~15
        ends.append(pos)
    src = torch.frombuffer(src_host, dtype=torch.uint8).to(dev)
    dst = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=dev)
    uses_scratch = max_ulen > 16384
    scratch_bytes = n * int(native.gpu.snappy_compress_scratch_per_block()) if uses_scratch else 64
    scratch = torch.full((scratch_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    jobs = []
    for i, d in enumerate(datas):
        jobs += [src.data_ptr() + src_at[i], dst.data_ptr() + starts[i], len(d), caps[i]]
    jobs_dev = torch.tensor(jobs, dtype=torch.int64).to(dev)
    meta = torch.full((2 * n,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        native.gpu.snappy_compress_launch(jobs_dev.data_ptr(), n, max_ulen, scratch.data_ptr(), meta.data_ptr(),
                                          meta.data_ptr() + 4 * n, stream_handle(dev))
    m = meta.cpu().tolist()
    if not uses_scratch:
        assert scratch.cpu().numpy().tobytes() == bytes([SENTINEL]) * 64, "an LDS-slot launch wrote the scratch"
    return m[n:], m[:n], dst.cpu().numpy().tobytes(), starts, ends


def _device_decode(dev, datas, streams, max_ulen):
    """Both device decoders rebuild every input from the device's streams."""
    from brpc_amd.ops import snappy_decompress, snappy_decompress_streams
    offs, pos = [], 0
    for c in streams:
        offs.append(pos)
        pos += len(c)
    packed = torch.frombuffer(bytearray(b"".join(streams) + b"\0"), dtype=torch.uint8).to(dev)
    sizes, raw = [len(c) for c in streams], [len(d) for d in datas]
    want = b"".join(datas)
    assert snappy_decompress(packed, offs, sizes, raw).cpu().numpy().tobytes() == want
    if max_ulen <= 8192:  # one piece per stream, up to 8 KiB: the parallel piece decoder
        out = snappy_decompress_streams(packed, offs, sizes, raw, piece_limit=max_ulen)
        assert out.cpu().numpy().tobytes() == want


def _minimal_forms(elements):
    """What holds for every element the compressor may emit: the shortest
    literal tag for the length, copies of 4..64 bytes, the 2-byte copy form
    exactly for lengths under 12 at distances under 2048, no 5-byte form."""
    for el in elements:
        if el.kind == S.LITERAL:
            assert el.tag_width == (1 if el.length <= 60 else 2 if el.length <= 256 else 3), el
        else:
            assert 4 <= el.length <= 64, el
            assert el.kind == (S.COPY1 if el.length < 12 and el.offset < 2048 else S.COPY2), el


def _compress_checked(dev, datas, max_ulen=None, caps=None, src_off=0, dst_off=0, forms=None):
    """Launches the jobs and asserts, per job and in this order: no error and
    a size within the exact bound; the host codec decodes the stream to the
    input; so does snappy_stream.decode; nothing outside the stream was
    written; the forms (forms(i, elements) plus _minimal_forms). Then the
    device decoders. Returns the streams."""
    from brpc_amd import native
    if max_ulen is None:
        max_ulen = max(len(d) for d in datas)
    if caps is None:
        caps = [_bound(len(d)) for d in datas]
    errs, lens, dst, starts, ends = _launch(dev, datas, max_ulen, caps, src_off, dst_off)
    streams = []
    for i, d in enumerate(datas):
        where = "job %d of %d bytes" % (i, len(d))
        assert errs[i] == 0 and 0 < lens[i] <= caps[i], (where, errs[i], lens[i], caps[i])
        stream = dst[starts[i]:starts[i] + lens[i]]
        assert native.snappy_uncompress(stream) == d, where
        assert S.decode(stream) == d, where
        front = starts[i] - GUARD - dst_off
        assert dst[front:starts[i]] == bytes([SENTINEL]) * (starts[i] - front), where
        assert dst[starts[i] + lens[i]:ends[i]] == bytes([SENTINEL]) * (ends[i] - starts[i] - lens[i]), where
        ulen, elements = S.walk(stream)
        assert ulen == len(d)
        _minimal_forms(elements)
        if forms:
            forms(i, elements)
        streams.append(stream)
    _device_decode(dev, datas, streams, max_ulen)
    return streams


def _copy_split(L):
    """The pieces of a copy of L bytes as snappy's encoder cuts it: 64s while
    68 or more remain, a 60 if more than 64 remain, then the rest (>= 4)."""
    out = []
    while L >= 68:
        out.append(64)
        L -= 64
    if L > 64:
        out.append(60)
        L -= 60
    return out + [L]


def _assert_planted(n, L, D, elements):
    """The planted span is made of copies at distance D cut as _copy_split
    says, and they are the block's only copies but for the helper copy in
    front of a plant deep inside its segment."""
    q, t = S.plant_site(n, L, D)
    inside = S.span_elements(elements, t, t + L)
    assert [el.kind != S.LITERAL for el in inside] == [True] * len(inside), inside
    assert [el.offset for el in inside] == [D] * len(inside), inside
    assert [el.length for el in inside] == _copy_split(L), inside
    lo, _ = S.segment(n, t // S.seg_len(n))
    others = [el for el in elements if el.kind != S.LITERAL and not t <= el.pos < t + L]
    if t - lo < 32:
        assert others == [], others
    else:
        assert sum(el.length for el in others) == t - lo - S.LEAD and others[0].pos == lo, others


@pytest.mark.parametrize("n", BLOCKS)
def test_copy_length_sweep(dev, n):
    """One copy of exactly L bytes per job: the 64 / 60 / rest split (65..67
    give 60 + 5..7, 68 gives 64 + 4), and at 8192 the 7-bit match records
    (L - 4 up to 124 at segment offsets up to 4)."""
    seg = S.seg_len(n)
    D = seg + 37
    Ls = S.sweep_lengths(n)
    assert len(Ls) == {64: 10, 128: 18}.get(seg, 19)
    datas = [S.planted_copy(n, 100 + L, L, D) for L in Ls]
    assert _copy_split(66) == [60, 6] and _copy_split(68) == [64, 4] and _copy_split(129) == [64, 60, 5]
    _compress_checked(dev, datas, forms=lambda i, els: _assert_planted(n, Ls[i], D, els))


@pytest.mark.parametrize("n", BLOCKS)
def test_copy_offset_boundary(dev, n):
    """The 2-byte copy form exactly when L < 12 and D < 2048, on both sides
    of each limit; D < L copies overlap their source; 65531 is the farthest
    a 4-byte copy can reach in a 64 KiB block."""
    cases = S.distance_cases(n)
    assert len(cases) == (28 if n == 65536 else 21)
    datas = [S.planted_copy(n, 1000 * L + D, L, D) for L, D in cases]

    def forms(i, els):
        L, D = cases[i]
        _assert_planted(n, L, D, els)
        _, t = S.plant_site(n, L, D)
        (el,) = S.span_elements(els, t, t + L)
        assert el.kind == (S.COPY1 if L < 12 and D < 2048 else S.COPY2), el

    _compress_checked(dev, datas, forms=forms)


@pytest.mark.parametrize("n", BLOCKS)
def test_periodic_blocks_overlapping_copies(dev, n):
    """Whole blocks of period 1, 2, 3, 5, 7: lane 0 emits the unit as a
    literal and the rest of its segment as copies at distance = period,
    the first of them longer than its distance."""
    periods = [1, 2, 3, 5, 7]
    datas = [S.periodic(n, 7 + p, p) for p in periods]

    def forms(i, els):
        p = periods[i]
        lo, hi = S.segment(n, 0)
        first = S.span_elements(els, lo, hi)
        assert (first[0].kind, first[0].length) == (S.LITERAL, p), first[0]
        assert [el.offset for el in first[1:]] == [p] * (len(first) - 1), first
        assert [el.length for el in first[1:]] == _copy_split(hi - p), first
        assert first[1].length > first[1].offset

    _compress_checked(dev, datas, forms=forms)


@pytest.mark.parametrize("n,width", [(3840, 1), (3904, 2), (16384, 2), (16385, 3)])
def test_literal_tag_forms(dev, n, width):
    """Incompressible blocks whose segments are 60, 61, 256 and 257 bytes:
    one literal per non-empty lane, with 1, 2, 2 and 3 tag bytes (16385
    leaves lane 63 194 bytes: 2 tag bytes)."""
    seg = S.seg_len(n)
    assert seg == {1: 60, 2: 61 if n < 4096 else 256, 3: 257}[width]

    def forms(i, els):
        assert [el.kind for el in els] == [S.LITERAL] * 64, [el.kind for el in els]
        for lane, el in enumerate(els):
            lo, hi = S.segment(n, lane)
            assert (el.pos, el.length) == (lo, hi - lo), (lane, el)
        assert [el.tag_width for el in els[:63]] == [width] * 63
        assert els[63].tag_width == (2 if n == 16385 else width)

    _compress_checked(dev, [S.incompressible(n, n)], forms=forms)


@pytest.mark.parametrize("n", BLOCKS)
def test_more_literals_than_deferred_spans(dev, n):
    """A lane with 13 literals (12 of one byte between 12 four-byte copies):
    the 9th and later ones take the in-place byte loop; every other lane has
    one literal, copied after the walk."""
    lane = 5
    lo, hi = S.segment(n, lane)

    def forms(i, els):
        inside = S.span_elements(els, lo, hi)
        assert len(inside) == 2 * S.MANY + 1
        for k in range(S.MANY):
            lit, cp = inside[2 * k], inside[2 * k + 1]
            assert (lit.kind, lit.length, lit.pos) == (S.LITERAL, 1, lo + 5 * k), lit
            assert cp.kind != S.LITERAL and (cp.length, cp.offset) == (4, lo + 5 * k + 1 - 4 * k), cp
        assert (inside[-1].kind, inside[-1].length) == (S.LITERAL, hi - lo - 5 * S.MANY), inside[-1]
        assert sum(el.kind == S.LITERAL for el in inside) >= 9
        rest = [el for el in els if not lo <= el.pos < hi]
        assert [el.kind for el in rest] == [S.LITERAL] * 63  # the deferred path: one span per lane

    _compress_checked(dev, [S.many_literals(n, 1, lane)], forms=forms)


@pytest.mark.parametrize("n", BLOCKS)
def test_constant_and_tiled_blocks_cross_segments(dev, n):
    """All zeros: every lane from 1 on opens with a copy that reaches into an
    earlier segment. One segment-sized tile repeated: every such lane is one
    match from the block's start that runs exactly to its segment's end, the
    last one to the block's end."""
    datas = [bytes(n), S.tiled(n, 5)]

    def forms(i, els):
        for lane in range(1, 64):
            lo, hi = S.segment(n, lane)
            if lo == hi:
                continue
            inside = S.span_elements(els, lo, hi)
            assert inside[0].kind != S.LITERAL and inside[0].pos == lo and inside[0].offset > 0, (lane, inside[0])
            if i == 1 or hi - lo >= 4:
                assert [el.offset for el in inside] == [lo] * len(inside), (lane, inside)
                assert [el.length for el in inside] == _copy_split(hi - lo), (lane, inside)
        if i == 1:
            lo, hi = S.segment(n, 0)
            (el,) = S.span_elements(els, lo, hi)
            assert el.kind == S.LITERAL

    _compress_checked(dev, datas, forms=forms)


@pytest.mark.parametrize("max_ulen", [1024, 16384, 65536])
@pytest.mark.parametrize("kind", ["incompressible", "equal"])
def test_every_length_to_1024_within_the_exact_bound(dev, kind, max_ulen):
    """Jobs of 1..1024 bytes in one launch of each kernel, each with dst_cap
    = 32 + n + n / 6 exactly: lengths of 64k + 1 (empty trailing lanes), not
    divisible by 4, and the short blocks whose 64 one-byte segments would
    each pay a tag."""
    if kind == "equal":
        datas = [bytes([n & 0xFF]) * n for n in range(1, 1025)]
    else:
        whole = S.incompressible(1024, 77)
        datas = [whole[:n] for n in range(1, 1025)]

    def forms(i, els):
        n = i + 1
        if kind == "incompressible":
            lanes = [S.segment(n, k) for k in range(64)]
            assert [(el.kind, el.pos, el.length) for el in els] == \
                [(S.LITERAL, lo, hi - lo) for lo, hi in lanes if hi > lo], n

    _compress_checked(dev, datas, max_ulen=max_ulen, forms=forms)


@pytest.mark.parametrize("block", [38, 64, 128, 192])
def test_public_op_with_blocks_shorter_than_512(dev, block):
    """ops.snappy_compress sizes its slots by snappy_max_compressed_length of
    the block: blocks this short used to overrun it (64 one-byte segments)."""
    from brpc_amd import native
    from brpc_amd.ops import snappy_compress, snappy_decompress
    data = S.incompressible(1000, block)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    packed, offs, sizes, raw = snappy_compress(t, block=block)
    host = packed.cpu().numpy().tobytes()
    assert b"".join(native.snappy_uncompress(host[o:o + z]) for o, z in zip(offs, sizes)) == data
    assert all(z <= _bound(r) for z, r in zip(sizes, raw))
    assert snappy_decompress(packed, offs, sizes, raw).cpu().numpy().tobytes() == data


@pytest.mark.parametrize("big", [65536, 16384, 8192])
def test_mixed_sizes_in_one_launch(dev, big):
    """Jobs of 1, 5, 64 and 4096 bytes next to two of the launch's largest."""
    sizes = [1, 5, 64, 4096, big]
    datas = [S.text(n, n) if k % 2 else S.incompressible(n, n) for k, n in enumerate(sizes)]
    datas.append(S.text(big, 3))
    _compress_checked(dev, datas)


@pytest.mark.parametrize("n", BLOCKS)
def test_unaligned_source_and_destination(dev, n):
    """src at byte 1, 7 and 15 of a 16-byte boundary (byte-wise staging), dst
    at 1 and 8 (slot-by-slot copy-out; the text block is small enough that an
    aligned dst would have taken the LDS-assembled one), dst_cap still exact."""
    datas = [S.text(n, 11), S.planted_copy(n, 12, 13, S.seg_len(n) + 37), S.text(n - 3, 13)]

    def forms(i, els):
        if i == 1:
            _assert_planted(n, 13, S.seg_len(n) + 37, els)

    aligned = _compress_checked(dev, datas, forms=forms)
    if n <= 16384:  # fits the stage in the earliest-position table: 8 KiB with the candidate array, else 16
        assert len(aligned[0]) <= (8192 if n <= 8192 else 16384)
    for src_off, dst_off in [(1, 0), (7, 0), (15, 0), (0, 1), (0, 8), (7, 1)]:
        got = _compress_checked(dev, datas, src_off=src_off, dst_off=dst_off, forms=forms)
        assert got == aligned, (src_off, dst_off)


@pytest.mark.parametrize("max_ulen", [4096, 16384, 32768])
def test_refusals_write_nothing(dev, max_ulen):
    """err 1: a job longer than its launch's in_cap (max_ulen rounded up to
    16). err 2: a stream one byte longer than dst_cap. Both report out_len 0
    and leave slot and guards as they were; their launch mates are served."""
    in_cap = (max_ulen + 15) & ~15
    good = S.text(max_ulen, 1)
    datas = [good, S.text(in_cap + 1, 2), S.incompressible(max_ulen - 5, 3)]
    caps = [_bound(len(d)) for d in datas]
    errs, lens, dst, starts, ends = _launch(dev, datas, max_ulen, caps, 0, 0)
    assert errs == [0, 1, 0] and lens[1] == 0 and lens[0] > 0 and lens[2] > 0, (errs, lens)
    front = starts[1] - GUARD
    assert dst[front:ends[1]] == bytes([SENTINEL]) * (ends[1] - front)
    needed = [lens[0], lens[2]]
    datas = [good, datas[2], good, datas[2]]
    caps = [needed[0] - 1, needed[1] - 1, needed[0], needed[1]]
    errs, lens, dst, starts, ends = _launch(dev, datas, max_ulen, caps, 0, 0)
    assert errs == [2, 2, 0, 0] and lens == [0, 0] + needed, (errs, lens)
    for i in (0, 1):
        front = starts[i] - GUARD
        assert dst[front:ends[i]] == bytes([SENTINEL]) * (ends[i] - front), i
    from brpc_amd import native
    for i in (2, 3):
        assert native.snappy_uncompress(dst[starts[i]:starts[i] + lens[i]]) == datas[i]
        assert dst[starts[i] + lens[i]:ends[i]] == bytes([SENTINEL]) * (ends[i] - starts[i] - lens[i])


@pytest.mark.parametrize("block_kb", [8, 16, 64])
def test_rpc_body_codec_at_each_kernels_block_size(block_kb):
    """The RPC body codec with the offload installed and -gpu_snappy_block_kb
    selecting each compress kernel: one 40000-byte mixed body, both ways
    against the host codec."""
    from brpc_amd import native
    old = native.get_flag("gpu_snappy_block_kb")
    native.set_flag("gpu_snappy_block_kb", str(block_kb))
    native.gpu.enable_snappy(0, 1024, packed_only=False)
    try:
        data = S.incompressible(9000, 1) + S.text(17000, 2) + bytes(5000) + S.tiled(8192, 3) + S.text(808, 4)
        assert len(data) == 40000
        before = native.gpu.snappy_stats()
        c = native.compress(1, data)
        assert native.snappy_uncompress(c) == data
        assert S.decode(c) == data
        assert native.decompress(1, c) == data
        assert native.decompress(1, native.snappy_compress(data)) == data
        after = native.gpu.snappy_stats()
        assert after["compress_calls"] == before["compress_calls"] + 1, (before, after)
        assert after["decompress_calls"] == before["decompress_calls"] + 2, (before, after)
        assert after["fallbacks"] == before["fallbacks"], (before, after)
    finally:
        native.gpu.disable_snappy()
        native.set_flag("gpu_snappy_block_kb", old)
