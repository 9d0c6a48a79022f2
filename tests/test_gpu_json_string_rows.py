"""The text of an array of JSON strings on the device
(gpu::DeviceUnescapeJsonStringRows, gpu/json_string_kernels.hip) against the
host twin (native.json_unescape_rows) and the pure-python parser of this
directory: lengths around a lane and a chunk, every src x dst alignment in one
call, quotes, backslash runs and surrogate pairs across chunk edges, chunks
wholly inside a string, predecessors that cross whole chunks of whitespace, the
densest rows, a job longer than one tile of the carry kernel, every refusal at
a chunk edge, capacities, the code-2 refusals and the ops on top."""
import random

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import json_string_rows_ref as R  # noqa: E402

GUARD = 16


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


@pytest.fixture(scope="module")
def C(native):
    c = native.gpu.json_string_chunk_bytes()
    assert c % 16 == 0 and c >= 256 * 16
    return c


def _to_dev(data, dev):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev)


def _run(native, dev, jobs):
    """jobs: [(text, src offset, dst offset, cap or None, row_cap or None)] in
    one call -> [(len, rows, depth, err, first_bad, dst bytes [0, cap), row-end
    bytes [0, 4 row_cap), guards intact)]. Every buffer is 0xEE-filled; src and
    dst start `offset` bytes past a 256-byte boundary plus GUARD."""
    keep, srcs, ns, dsts, caps, ends, row_caps = [], [], [], [], [], [], []
    for text, so, do, cap, row_cap in jobs:
        n = len(text)
        cap = native.gpu.json_string_rows_max_bytes(n) if cap is None else cap
        row_cap = native.gpu.json_string_rows_max_rows(n) if row_cap is None else row_cap
        sbuf = torch.full((GUARD + so + n + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        if n:
            sbuf[GUARD + so:GUARD + so + n] = _to_dev(text, dev)
        dbuf = torch.full((GUARD + do + cap + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        ebuf = torch.full((GUARD + 4 * row_cap + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0 and ebuf.data_ptr() % 256 == 0
        keep.append((dbuf, do, cap, ebuf, row_cap, sbuf))
        srcs.append(sbuf.data_ptr() + GUARD + so)
        ns.append(n)
        dsts.append(dbuf.data_ptr() + GUARD + do)
        caps.append(cap)
        ends.append(ebuf.data_ptr() + GUARD)
        row_caps.append(row_cap)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_json_unescape_rows(srcs, ns, dsts, caps, ends, row_caps, 0)
    out = []
    for r, (dbuf, do, cap, ebuf, row_cap, _) in zip(res, keep):
        host, ehost = dbuf.cpu().numpy(), ebuf.cpu().numpy()
        lo = GUARD + do
        guards = (bool((host[:lo] == 0xEE).all()) and bool((host[lo + cap:] == 0xEE).all()) and
                  bool((ehost[:GUARD] == 0xEE).all()) and bool((ehost[GUARD + 4 * row_cap:] == 0xEE).all()))
        out.append(tuple(r) + (host[lo:lo + cap].tobytes(), ehost[GUARD:GUARD + 4 * row_cap].tobytes(), guards))
    return out


def _check(native, texts, res, ref=False):
    """Every result against the host twin (and the python parser): code, offset,
    depth, len, rows, bytes, row ends; guards intact; outputs untouched when refused."""
    for text, (length, rows, depth, err, first_bad, data, ends, guards) in zip(texts, res):
        want = native.json_unescape_rows(text)
        tag = (len(text), text[:24], text[-24:])
        assert guards, tag
        if ref:
            py = R.parse(text)
            assert (py if isinstance(py, int) else (b"".join(py[0]), R.row_ends(py[0]), py[1])) == \
                (want[1] if want[0] is None else want), tag
        if want[0] is None:
            assert (err, first_bad, length, rows, depth) == (1, want[1], 0, 0, 0), tag
            assert data == b"\xee" * len(data) and ends == b"\xee" * len(ends), tag
        else:
            assert (err, length, rows, depth) == (0, len(want[0]), len(want[1]), want[2]), tag
            assert data[:length] == want[0], tag
            assert data[length:] == b"\xee" * (len(data) - length), tag
            assert np.frombuffer(ends[:4 * rows], dtype=np.uint32).tolist() == want[1], tag
            assert ends[4 * rows:] == b"\xee" * (len(ends) - 4 * rows), tag


def _same(native, dev, texts, ref=False, offsets=True):
    jobs = [(t, (3 * k + 1) % 16 if offsets else 0, (5 * k + 2) % 16 if offsets else 0, None, None)
            for k, t in enumerate(texts)]
    res = _run(native, dev, jobs)
    _check(native, texts, res, ref)
    return res


def _text_of(n, depth, native):
    """A valid text of exactly n bytes (n >= 2 + 2 * depth): rows of mixed content, the last one padded."""
    unit = b'"ab\\n\\u00e9c\\\\","","\\"q\\ud83d\\ude00",'
    inner = n - 2 * depth
    body = (unit * (inner // len(unit) + 1))[:inner]
    for k in range(2, 40):  # replace the cut-off tail by one plain string
        t = body[:inner - k]
        if t == b"" or t.endswith(b","):
            t += b'"' + b"x" * (k - 2) + b'"'
            t = b"[" + t + b"]" if depth else t
            if native.json_unescape_rows(t)[0] is not None:
                assert len(t) == n
                return t
    raise AssertionError("no valid cut")


def test_lengths_around_a_lane_and_a_chunk(native, dev, C):
    texts = []
    for n in [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]:
        for depth in (0, 1):
            if n >= 2 + 2 * depth:
                texts.append(_text_of(n, depth, native))
        texts.append((b' "' + b"q" * n)[:n])  # refused: never closed (n >= 2), or whitespace
        texts.append(b" " * n)
    texts += [b"[", b"]", b'"', b"[]", b'""', b"[ ]"]
    _same(native, dev, texts, ref=True)


def test_every_src_and_dst_alignment(native, dev, C):
    for sa in range(16):
        texts = [_text_of(C + 40 + da, da & 1, native) for da in range(16)]
        res = _run(native, dev, [(t, sa, da, None, None) for da, t in enumerate(texts)])
        _check(native, texts, res)


def test_quotes_at_a_chunk_edge(native, dev, C):
    texts = []
    for shift in (-1, 0, 1):
        e = C + shift
        texts.append(b'"' + b"a" * (e - 4) + b'","' + b"b" * 20 + b'"')     # ',' '"' around the edge
        texts.append(b'"' + b"a" * (e - 3) + b'","' + b"b" * 20 + b'"')     # opening quote last byte of the chunk
        texts.append(b'"' + b"a" * (e - 1) + b'","' + b"b" * 20 + b'"')     # closing quote first byte of the next
        texts.append(b'["' + b"a" * (e - 3) + b'"]')
    _same(native, dev, texts, ref=True)


def test_backslash_runs_ending_at_a_chunk_edge(native, dev, C):
    texts = []
    for run in range(1, 21):
        # `run` backslashes end at byte C - 1, a quote follows: odd runs escape it, even runs close the string
        head = b'["' + b"a" * (C - 2 - run) + b"\\" * run
        assert len(head) == C
        texts.append(head + b'","tail"]')
        texts.append(head + b'"]')
        texts.append(head + b'" ,"x"]')
    _same(native, dev, texts, ref=True)


def test_surrogate_pair_straddles_the_edge_at_every_split(native, dev, C):
    texts = []
    for start in range(C - 11, C + 1):
        texts.append(b'"' + b"a" * (start - 1) + b"\\ud83d\\ude00" + b'z","k"')
        texts.append(b'"' + b"a" * (start - 1) + b"\\ud83d\\ude0" + b'","k"')  # cut short: refused at the backslash
    res = _same(native, dev, texts, ref=True)
    assert res[0][3] == 0 and res[1][3] == 1


def test_a_chunk_wholly_inside_a_string(native, dev, C):
    inner = (b"a,b [c] ,\t]\n[ " * (2 * C // 14 + 40))
    assert len(inner) > 2 * C + 100
    texts = [b'["x","' + inner + b'","y"]', b'"' + inner + b'"', b'["x","' + inner + b'\\n","y" x]']
    res = _same(native, dev, texts, ref=True)
    assert [r[3] for r in res] == [0, 0, 1]


def test_whitespace_runs_carry_the_predecessor_across_chunks(native, dev, C):
    w = b" \n\t\r" * (3 * C // 4)
    good = [w + b'["a","b"]', b'["a"' + w + b',"b"]', b'["a",' + w + b'"b"]', b'["a","b"' + w + b"]", b'["a","b"]' + w,
            w + b'"a"' + w + b"," + w + b'"b"' + w, b"[" + w + b"]", w]
    bad = [w + b'"a"' + w + b'"b"', b'["a"' + w + b"x]", b'["a",' + w + b",]", b"[" + w + b",", b'["a"]' + w + b"]",
           b'"a",' + w, b'["a"' + w, w + b"]", b'"a"' + w + b"]", b'["a",' + w + b"]"]
    res = _same(native, dev, good + bad, ref=True)
    assert all(r[3] == 0 for r in res[:len(good)]) and all(r[3] == 1 for r in res[len(good):])


def test_rows(native, dev, C):
    k = (2 * C + 5 - 2) // 3  # "","",...,"" is 3 k + 2 bytes; spaces in front fill the rest
    dense = b" " * (2 * C + 5 - 3 * k - 2) + b'"",' * k + b'""'
    assert len(dense) == 2 * C + 5 and k + 1 == (2 * C + 6) // 3
    texts = [dense, b"[" + dense + b"]"]
    rng = random.Random(5)
    for size in (1, 32, 1024):
        rows = [bytes(rng.choice(b'ab"\\\n\x00\xc3\xa9 ,[]') for _ in range(size)) for _ in range(3 * C // (size + 3) + 2)]
        ends = R.row_ends(rows)
        text = native.json_escape(b"".join(rows), row_ends=np.array(ends, dtype=np.uint32).tobytes())
        assert native.json_unescape_rows(text) == (b"".join(rows), ends, 0)
        texts += [text, b" [" + text + b"] "]
    res = _same(native, dev, texts, ref=True)
    assert res[0][1] == (2 * C + 6) // 3 and all(r[3] == 0 for r in res)


def test_a_job_longer_than_one_carry_tile(native, dev, C):
    # 260 chunks: the carry kernel composes a second tile of 256, entered inside a string after an odd run
    unit = b'"k\\\\\\"v\\u00e9, [x]\\n",'
    body = bytearray((unit * (260 * C // len(unit) + 1))[:260 * C - 40])
    k = 256 * C  # a backslash run that crosses the tile's edge, inside a string
    body[k - 40:k + 40] = b"m" * 20 + b"\\" * 41 + b"n" * 19
    body = bytes(body)
    text = None
    for cut in range(len(unit) + 2):
        t = body[:len(body) - cut]
        for tail in (b'"', b'""', b'x"', b""):
            if native.json_unescape_rows(t + tail)[0] is not None:
                text = t + tail
                break
        if text:
            break
    assert text is not None and len(text) > 259 * C
    want = native.json_unescape_rows(text)
    assert want[0] is not None and len(want[1]) > 1000
    res = _same(native, dev, [text, b"[" + text + b"]", text[:257 * C + 5]], offsets=False)
    assert res[0][3] == 0 and res[1][3] == 0


REFUSALS = [  # (head, tail): the offender is the first byte of tail, or the end of head when tail is empty
    (b'["a"', b'"b"]'), (b'["a",', b",]"), (b'["a"', b'x,"b"]'), (b'["a",', b'["b"]]'), (b'["a",', b'1,"b"]'),
    (b'["a",', b'null]'), (b'["a",', b'{"k":"v"}]'), (b'["a"]', b']'), (b'["a"]', b',"b"'), (b'["a"]', b'"b"'),
    (b'"a"', b']'), (b'"a",', b']'), (b'["a","b', b'\\q"]'), (b'["a","b', b'\\u12G4"]'), (b'["a","b', b'\\ud83dx"]'),
    (b'["a","b', b'\\ude00"]'), (b'["a","b', b""), (b'["a",', b""), (b'["a"', b""), (b'"a","b', b"\\"),
    (b'"a"', b'\\"'), (b'"a"', b'[')]


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_every_refusal_at_a_chunk_edge(native, dev, C, shift):
    texts, wants = [], []
    for head, tail in REFUSALS:
        for pad in (b" ", b"s"):  # the offender after whitespace outside, or after bytes inside the first string
            at = C + shift
            fill = at - len(head)
            if pad == b" ":
                text = b" " * fill + head + tail
            else:
                cut = head.index(b'"') + 1
                text = head[:cut] + b"s" * fill + head[cut:] + tail
            texts.append(text)
            wants.append(at)
    res = _same(native, dev, texts, ref=True)
    assert [(r[3], r[4]) for r in res] == [(1, w) for w in wants]


def test_capacities(native, dev, C):
    text = _text_of(2 * C + 100, 1, native)
    data, ends, _ = native.json_unescape_rows(text)
    n, rows = len(data), len(ends)
    jobs = [(text, 1, 2, n, rows), (text, 3, 5, n - 1, rows), (text, 0, 7, n, rows - 1), (text, 2, 0, n - 1, rows - 1),
            (text, 2, 9, 0, 0), (b"[ ]", 0, 0, 0, 0)]
    res = _run(native, dev, jobs)
    assert all(r[7] for r in res)
    assert res[0][:5] == (n, rows, 1, 0, 0) and res[0][5] == data
    assert np.frombuffer(res[0][6], dtype=np.uint32).tolist() == ends
    for r in res[1:5]:  # code 3 names both needs and writes nothing
        assert r[:5] == (n, rows, 1, 3, 0)
        assert r[5] == b"\xee" * len(r[5]) and r[6] == b"\xee" * len(r[6])
    assert res[5][:5] == (0, 0, 1, 0, 0)


def test_refusals_before_any_launch(native, dev, C):
    text = b'["abc","d"]'
    n = len(text)
    buf = torch.full((1024,), 0xEE, dtype=torch.uint8, device=dev)
    buf[256:256 + n] = _to_dev(text, dev)
    torch.cuda.synchronize(dev)
    base = buf.data_ptr()
    src, dst, ends = base + 256, base + 512, base + 768
    big = 1 << 32
    jobs = [
        (0, n, dst, 16, ends, 4),            # a null src
        (src, n, 0, 16, ends, 4),            # a null dst with a capacity
        (src, n, dst, 16, 0, 4),             # a null row_ends with a capacity
        (src, big - 1, dst, 16, ends, 4),    # n above 2^32 - 2
        (src, n, dst, 16, ends + 2, 4),      # row_ends not 4-byte aligned
        (src, n, src + 4, 16, ends, 4),      # dst overlaps src
        (src, n, dst, 16, src + 4, 4),       # row_ends overlaps src
        (src, n, dst, 16, dst + 4, 4),       # row_ends overlaps dst
        (0, 0, 0, 0, 0, 0),                  # n == 0: code 0, nothing written
        (src, n, dst, 16, ends, 4),          # a live job beside them
    ]
    res = native.gpu.device_json_unescape_rows(*[list(col) for col in zip(*jobs)], 0)
    assert [r[3] for r in res] == [2] * 8 + [0, 0]
    assert res[8] == (0, 0, 0, 0, 0) and res[9] == (4, 2, 1, 0, 0)
    host = buf.cpu().numpy()
    assert host[512:516].tobytes() == b"abcd" and np.frombuffer(host[768:776].tobytes(), dtype=np.uint32).tolist() == [3, 4]
    keep = np.ones(1024, dtype=bool)
    keep[256:256 + n] = keep[512:516] = keep[768:776] = False
    assert (host[keep] == 0xEE).all()
    # only refused jobs: nothing is launched, nothing written
    buf2 = torch.full((1024,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    b2 = buf2.data_ptr()
    assert [r[3] for r in native.gpu.device_json_unescape_rows([b2, 0], [8, 0], [b2 + 4, 0], [8, 0], [b2 + 512, 0], [2, 0],
                                                               0)] == [2, 0]
    assert (buf2.cpu().numpy() == 0xEE).all()


@pytest.mark.parametrize("seed", range(2))
def test_seeded_differential_set(native, dev, C, seed):
    texts = R.differential_texts(2024 + seed, 384, long_row=3 * C - 200)
    assert max(len(t) for t in texts) > 2 * C
    for at in range(0, len(texts), 64):
        _same(native, dev, texts[at:at + 64], ref=True)


def test_ops_round_trip_with_the_escaper(native, dev, C):
    from brpc_amd.ops.json import json_escape_string, json_unescape_string_rows
    rng = random.Random(11)
    pool = bytes(range(0x20)) + b'"\\' * 4 + bytes(range(256))
    for sizes in ([0, 1, 0, 40, C + 3, 2, 0], [5] * 300, []):
        rows = [bytes(rng.choice(pool) for _ in range(s)) for s in sizes]
        ends = R.row_ends(rows)
        data = _to_dev(b"".join(rows), dev)
        ends_t = torch.tensor(ends, dtype=torch.int32, device=dev)
        text = json_escape_string(data, ends_t)
        got, got_ends = json_unescape_string_rows(text)
        assert got.dtype == torch.uint8 and got_ends.dtype == torch.int32 and got.device == data.device
        assert got.cpu().numpy().tobytes() == b"".join(rows) and got_ends.cpu().tolist() == ends
    with pytest.raises(ValueError, match="takes 6 bytes in 2 rows"):
        json_unescape_string_rows(_to_dev(b'["abc","def"]', dev), max_bytes=5)
    with pytest.raises(ValueError, match="takes 6 bytes in 2 rows"):
        json_unescape_string_rows(_to_dev(b'["abc","def"]', dev), max_rows=1)


def test_ops_feed_the_row_builder(native, dev):
    from brpc_amd.ops import pb
    from brpc_amd.ops.json import json_unescape_string_rows
    rows = [b"alpha", b"", b'be"ta', b"\xc3\xa9\n" * 50]
    text = b"[" + b",".join(native.json_escape(r) for r in rows) + b"]"
    data, ends = json_unescape_string_rows(_to_dev(text, dev))
    msg = pb.pb_build_rows(4, data, ends, "bytes")
    back, back_ends = pb.pb_split_rows(msg, 4, "bytes")[:2]
    assert back.cpu().numpy().tobytes() == b"".join(rows)
    assert back_ends.cpu().tolist() == R.row_ends(rows)


def test_ops_code_1_falls_back_to_the_reader(native, dev):
    from brpc_amd.ops.json import json_unescape_string_rows
    lone = b'["a","\\ud83d","b"]'
    assert native.json_unescape_rows(lone) == (None, 6)
    want = native.json_reader_string_array(lone)
    assert want is not None and len(want) == 3
    data, ends = json_unescape_string_rows(_to_dev(lone, dev))
    assert data.cpu().numpy().tobytes() == b"".join(want) and ends.cpu().tolist() == R.row_ends(want)
    with pytest.raises(ValueError, match=r"offset 5\b"):
        json_unescape_string_rows(_to_dev(b'["a" "b"]', dev))
