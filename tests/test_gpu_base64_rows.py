"""Base64 rows on the device (gpu::DeviceBase64EncodeRows /
DeviceBase64DecodeRows, gpu/base64_kernels.hip) against the host twins
(native.base64_encode_rows / base64_decode_rows) and the pure-python reference
of this directory: lengths around a group, a lane and a chunk, every src x dst
alignment in one call, row boundaries and tokens on either side of a chunk
edge, both place paths of the encoder, chunks wholly inside a row or a string,
predecessors that cross whole chunks of whitespace, the densest rows, a job
longer than one tile of the carry kernel, every refusal at a chunk edge,
capacities, bad tables, the code-2 refusals and the ops on top."""
import base64
import random

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

import base64_rows_ref as R  # noqa: E402

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
def CE(native):
    c = native.gpu.base64_rows_encode_chunk_bytes()
    assert c % 12 == 0 and c >= 256 * 12
    return c


@pytest.fixture(scope="module")
def CD(native):
    c = native.gpu.base64_rows_decode_chunk_bytes()
    assert c % 16 == 0 and c >= 256 * 16
    return c


def _to_dev(data, dev):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev)


def _filled(nbytes, dev):
    t = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 256 == 0
    return t


def _payload(n, seed=0):
    return np.random.default_rng(n * 31 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------ encode

def _encode(native, dev, jobs, brackets):
    """jobs: [(data, ends, src offset, dst offset, cap or None)] in one call ->
    [(len, err, first_bad, dst bytes [0, cap), guards intact)]. Every buffer is
    0xEE-filled; src and dst start `offset` bytes past a 256-byte boundary plus
    GUARD."""
    keep, srcs, ns, tabs, rows, dsts, caps = [], [], [], [], [], [], []
    for data, ends, so, do, cap in jobs:
        n = len(data)
        cap = native.gpu.base64_rows_worst_case(n, len(ends), brackets) if cap is None else cap
        sbuf = _filled(GUARD + so + n + GUARD, dev)
        if n:
            sbuf[GUARD + so:GUARD + so + n] = _to_dev(data, dev)
        tbuf = torch.from_numpy(np.asarray(list(ends) + [0], dtype=np.uint32).view(np.int32).copy()).to(dev)
        dbuf = _filled(GUARD + do + cap + GUARD, dev)
        keep.append((dbuf, do, cap, sbuf, tbuf))
        srcs.append(sbuf.data_ptr() + GUARD + so)
        ns.append(n)
        tabs.append(tbuf.data_ptr() if len(ends) else 0)
        rows.append(len(ends))
        dsts.append(dbuf.data_ptr() + GUARD + do)
        caps.append(cap)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_base64_encode_rows(srcs, ns, tabs, rows, brackets, dsts, caps, 0)
    out = []
    for r, (dbuf, do, cap, _, _) in zip(res, keep):
        host = dbuf.cpu().numpy()
        lo = GUARD + do
        guards = bool((host[:lo] == 0xEE).all()) and bool((host[lo + cap:] == 0xEE).all())
        out.append(tuple(r) + (host[lo:lo + cap].tobytes(), guards))
    return out


def _ends_image(ends):
    return np.asarray(ends, dtype=np.uint32).tobytes()


def _encode_same(native, dev, tables, brackets, ref=False, offsets=True):
    """tables: [(data, ends)], all valid: the device text equals the twin's (and the reference's)."""
    jobs = [(d, e, (3 * k + 1) % 16 if offsets else 0, (5 * k + 2) % 16 if offsets else 0, None)
            for k, (d, e) in enumerate(tables)]
    res = _encode(native, dev, jobs, brackets)
    for (data, ends), (length, err, first_bad, text, guards) in zip(tables, res):
        tag = (len(data), len(ends), ends[:6], brackets)
        want = native.base64_encode_rows(data, _ends_image(ends), brackets)
        if ref:
            assert want == R.print_rows(R.split(data, ends), brackets), tag
        assert guards, tag
        assert (err, length) == (0, len(want)), tag
        assert text[:length] == want, tag
        assert text[length:] == b"\xee" * (len(text) - length), tag
    return res


def _layouts(n):
    """Row tables over n bytes: one row, rows of 1, 2, 3 and 7 bytes, one long row among empty ones."""
    out = [[n]]
    for k in (1, 2, 3, 7):
        out.append(list(range(k, n, k)) + [n])
    out.append([0, 0, n, n, n])
    return out


def test_encode_lengths_around_a_group_a_lane_and_a_chunk(native, dev, CE):
    for brackets in (False, True):
        tables = []
        for n in [0, 1, 2, 3, 4, 11, 12, 13, 47, 48, 49, CE - 1, CE, CE + 1, 3 * CE + 7]:
            tables += [(_payload(n), ends) for ends in _layouts(n)]
        _encode_same(native, dev, tables, brackets, ref=True)


def test_encode_no_rows(native, dev):
    (length, err, _, text, guards), = _encode(native, dev, [(b"", [], 0, 3, 8)], True)
    assert (length, err, text[:2], guards) == (2, 0, b"[]", True) and text[2:] == b"\xee" * 6
    (length, err, _, text, guards), = _encode(native, dev, [(b"", [], 0, 3, 8)], False)
    assert (length, err, guards) == (0, 0, True) and text == b"\xee" * 8


def test_encode_every_alignment_in_one_call(native, dev):
    data = _payload(200)
    ends = [0, 1, 3, 6, 50, 50, 127, 200]
    jobs = [(data, ends, k // 16, k % 16, None) for k in range(256)]
    for brackets in (False, True):
        want = native.base64_encode_rows(data, _ends_image(ends), brackets)
        for length, err, _, text, guards in _encode(native, dev, jobs, brackets):
            assert guards and (err, length) == (0, len(want)) and text[:length] == want


def test_encode_chunk_edges(native, dev, CE):
    seg = native.gpu.base64_rows_segment_rows()
    tables = []
    n = 2 * CE + 40
    data = _payload(n, 1)
    # a row boundary at each of the three group phases on either side of a chunk edge, for each phase of the row's start
    for s in (0, 1, 2, 3):
        for e in range(CE - 3, CE + 4):
            tables.append((data, ([s] if s else []) + [e, n]))
            tables.append((data, ([s] if s else []) + [e, e, e + 1, n]))
    # a chunk wholly inside one row
    tables.append((_payload(2 * CE + 5 + 16, 2), [7, 7 + 2 * CE + 5, 2 * CE + 5 + 16]))
    # exactly as many rows as the segment path takes, one more, and many more
    for rows_per_chunk in (seg - 1, seg, seg + 1, seg + 2, 31, 100):
        k = CE // rows_per_chunk
        tables.append((data, list(range(k, n, k)) + [n]))
        tables.append((data, list(range(k - 1, n, k - 1)) + [n]))
    # a chunk of one-byte rows
    tables.append((_payload(CE + 50, 3), list(range(1, CE + 51))))
    # 5000 empty rows in a run at a chunk edge, and around it
    for at in (CE - 1, CE, CE + 1):
        tables.append((_payload(CE + 100, 4), [at] * 5001 + [CE + 100]))
        tables.append((_payload(CE + 100, 4), [5, at - 2] + [at] * 5001 + [at + 1, at + 1, at + 2, at + 3] + [CE + 100]))
    for brackets in (False, True):
        _encode_same(native, dev, tables, brackets, ref=True)


def test_encode_capacities(native, dev, CE):
    data = _payload(CE + 77, 5)
    ends = [0, 5, CE - 1, CE + 2, CE + 77]
    for brackets in (False, True):
        want = native.base64_encode_rows(data, _ends_image(ends), brackets)
        exact, below = _encode(native, dev, [(data, ends, 1, 2, len(want)), (data, ends, 2, 1, len(want) - 1)], brackets)
        assert exact[:2] == (len(want), 0) and exact[3] == want and exact[4]
        assert below[:2] == (len(want), 3) and below[3] == b"\xee" * (len(want) - 1) and below[4]
    # rows of one byte attain the worst case
    rows = 1000
    want = native.base64_encode_rows(b"x" * rows, _ends_image(range(1, rows + 1)), True)
    assert len(want) == native.gpu.base64_rows_worst_case(rows, rows, True)
    (length, err, _, text, guards), = _encode(native, dev, [(b"x" * rows, list(range(1, rows + 1)), 0, 0, None)], True)
    assert (length, err, guards) == (len(want), 0, True) and text == want


def test_encode_bad_tables(native, dev, CE):
    n = CE + 300
    data = _payload(n, 6)
    good = list(range(100, n, 100)) + [n]
    last = len(good) - 1
    cases = []

    def bad(ends, first_bad):
        cases.append((ends, first_bad))

    bad([n + 1] + good[1:], 0)                          # row 0 ends beyond the data
    bad([0xFFFFFFFF] + good[1:], 0)
    bad([good[1] + 1] + good[1:], 1)                    # a decrease at the first row that can show one
    bad(good[:15] + [good[14] - 1] + good[16:], 15)     # in the middle
    bad(good[:last] + [good[last - 1] - 1], last)       # at the last row
    bad(good[:last] + [n - 1], last)                    # a last end that is not n
    bad(good[:last] + [n + 1], last)
    bad(good[:7] + [good[6] - 1] + good[8:20] + [3] + good[21:], 7)  # two: the lowest wins
    bad(good[:last - 1] + [good[last - 1] + 50, n - 1], last)
    res = _encode(native, dev, [(data, e, 1, 2, None) for e, _ in cases], True)
    for (ends, want), (length, err, first_bad, text, guards) in zip(cases, res):
        assert (err, first_bad, length) == (1, want, 0), (ends[:3], want)
        assert guards and text == b"\xee" * len(text)


# ------------------------------------------------------------------ decode

def _decode(native, dev, jobs):
    """jobs: [(text, src offset, dst offset, cap or None, row_cap or None)] in
    one call -> [(len, rows, depth, err, first_bad, dst bytes [0, cap), row-end
    bytes [0, 4 row_cap), guards intact)]."""
    keep, srcs, ns, dsts, caps, ends, row_caps = [], [], [], [], [], [], []
    for text, so, do, cap, row_cap in jobs:
        n = len(text)
        cap = native.gpu.base64_rows_max_bytes(n) if cap is None else cap
        row_cap = native.gpu.base64_rows_max_rows(n) if row_cap is None else row_cap
        sbuf = _filled(GUARD + so + n + GUARD, dev)
        if n:
            sbuf[GUARD + so:GUARD + so + n] = _to_dev(text, dev)
        dbuf = _filled(GUARD + do + cap + GUARD, dev)
        ebuf = _filled(GUARD + 4 * row_cap + GUARD, dev)
        keep.append((dbuf, do, cap, ebuf, row_cap, sbuf))
        srcs.append(sbuf.data_ptr() + GUARD + so)
        ns.append(n)
        dsts.append(dbuf.data_ptr() + GUARD + do)
        caps.append(cap)
        ends.append(ebuf.data_ptr() + GUARD)
        row_caps.append(row_cap)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_base64_decode_rows(srcs, ns, dsts, caps, ends, row_caps, 0)
    out = []
    for r, (dbuf, do, cap, ebuf, row_cap, _) in zip(res, keep):
        host, ehost = dbuf.cpu().numpy(), ebuf.cpu().numpy()
        lo = GUARD + do
        guards = (bool((host[:lo] == 0xEE).all()) and bool((host[lo + cap:] == 0xEE).all()) and
                  bool((ehost[:GUARD] == 0xEE).all()) and bool((ehost[GUARD + 4 * row_cap:] == 0xEE).all()))
        out.append(tuple(r) + (host[lo:lo + cap].tobytes(), ehost[GUARD:GUARD + 4 * row_cap].tobytes(), guards))
    return out


def _decode_check(native, texts, res, ref=False):
    """Every result against the host twin (and the python parser): code, offset,
    depth, len, rows, bytes, row ends; guards intact; outputs untouched when refused."""
    for text, (length, rows, depth, err, first_bad, data, ends, guards) in zip(texts, res):
        want = native.base64_decode_rows(text)
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


def _decode_same(native, dev, texts, ref=False, offsets=True):
    jobs = [(t, (3 * k + 1) % 16 if offsets else 0, (5 * k + 2) % 16 if offsets else 0, None, None)
            for k, t in enumerate(texts)]
    res = _decode(native, dev, jobs)
    _decode_check(native, texts, res, ref)
    return res


UNIT = b'"QUJD","","3q2+7w==","QQ",\n"QUI=", "QUJDRA"\t,'


def _string_of(m):
    """A string of m + 2 bytes, or m + 1 and a blank where a lone symbol would trail."""
    if m % 4 == 1:
        return b'"' + b"Q" * (m - 1) + b'" '
    return b'"' + (b"QUJDRUZH" * (m // 8 + 1))[:m] + b'"'


def _text_of(n, depth, units=True):
    """A valid text of exactly n bytes: whole units of mixed rows, then one string that fills the rest."""
    inner = n - 2 * depth
    if inner < 2:
        assert depth == 0 or inner >= 0
        return b"[" * depth + b" " * inner + b"]" * depth
    k = (inner - 2) // len(UNIT) if units else 0
    t = UNIT * k + _string_of(inner - 2 - len(UNIT) * k)
    t = b"[" + t + b"]" if depth else t
    assert len(t) == n
    return t


def test_decode_lengths_around_a_lane_and_a_chunk(native, dev, CD):
    texts = []
    for n in [0, 1, 2, 3, 4, 11, 12, 13, 47, 48, 49, CD - 1, CD, CD + 1, 3 * CD + 7]:
        for depth in (0, 1):
            if n >= 2 * depth:
                texts.append(_text_of(n, depth))
                texts.append(_text_of(n, depth, units=False))
    res = _decode_same(native, dev, texts, ref=True)
    assert all(r[3] == 0 for r in res)


def test_decode_every_alignment_in_one_call(native, dev):
    text = _text_of(300, 1)
    jobs = [(text, k // 16, k % 16, None, None) for k in range(256)]
    res = _decode(native, dev, jobs)
    _decode_check(native, [text] * 256, res)
    assert all(r[3] == 0 for r in res)


def _with_tail_at(tail, k, p, depth=1):
    """A valid text in which byte k of `tail` (strings and commas, ending the text) stands at offset p."""
    start = p - k
    row = b'"QUJDQUJD",'
    inner = start - depth
    count = inner // len(row)
    t = b"[" * depth + row * count + b" " * (inner - count * len(row)) + tail + b"]" * depth
    assert t[p] == tail[k]
    return t


def test_decode_chunk_edges(native, dev, CD):
    texts = []
    # an opening quote, a closing quote, each '=', a comma and every body phase as the last and the first byte of a chunk
    tail = b'"QQ==","QUI=" ,"QUJD","QUJDRUY","Q0RFRkdI"'
    for k in range(len(tail)):
        for p in (CD - 1, CD):
            texts.append(_with_tail_at(tail, k, p))
            texts.append(_with_tail_at(tail, k, p + CD, depth=0))
    # a long string crossing an edge at each of the four body phases, and chunks wholly inside a string
    for k in range(8):
        texts.append(_with_tail_at(b'"' + b"QUJDRUZH" * 40 + b'"', 0, CD - 1 - k))
        texts.append(_with_tail_at(b'"' + b"QUJDRUZH" * (CD // 4) + b'QQ==","QQ"', 0, CD - 1 - k))
    texts.append(b'"' + b"QUJD" * (3 * CD // 4) + b'"')
    # whole chunks of whitespace between tokens: the predecessor is carried over
    ws = b" " * (2 * CD + 5)
    texts.append(b'["QQ==",' + ws + b'"QUJD"' + ws + b"," + ws + b'"QUI="' + b"\n" * (CD + 3) + b"]")
    texts.append(ws + b"[" + ws + b"]" + ws)
    texts.append(ws)
    texts.append(ws + b'"QQ=="' + ws)
    # the densest rows
    texts.append((b'"",' * (CD + 1))[:-1])
    texts.append(b"[" + (b'"",' * (CD + 1))[:-1] + b"]")
    res = _decode_same(native, dev, texts, ref=True)
    assert all(r[3] == 0 for r in res)


def test_decode_job_longer_than_one_carry_tile(native, dev, CD):
    n = 258 * CD + 11
    text = _text_of(n, 1)
    open_string = text[:n - 3]  # ends inside its last string
    res = _decode_same(native, dev, [text, open_string], offsets=False)
    assert res[0][3] == 0 and res[1][3:5] == (1, n - 3)


SNIPPETS = [b'"Q"', b'"="', b'"Q="', b'"QQ="', b'"QQ=Q"', b'"QQ==="', b'"QUI=="', b'"QUJD="', b'"QUJDR"', b'"QU\\/D"',
            b'"QU JD"', b'"QU\nJD"', b'"QU-_"', b'"QUJD" "QQ"', b'x', b'12', b',', b'[', b'{"a":"QQ=="}', b'"QQ==",]']


def test_decode_refusals_at_chunk_edges(native, dev, CD):
    texts = []
    for snip in SNIPPETS:
        for start in range(CD - 7, CD + 2):
            for depth in (0, 1):
                row = b'"QUJDQUJD",'
                inner = start - depth
                count = inner // len(row)
                texts.append(b"[" * depth + row * count + b" " * (inner - count * len(row)) + snip + b',"QUJD"' +
                             b"]" * depth)
    res = _decode_same(native, dev, texts, ref=True)
    assert all(r[3] == 1 for r in res)
    bad_at = {r[4] for r in res}
    assert {CD - 1, CD, CD + 1} <= bad_at


def test_decode_refusals_listed(native, dev, CD):
    ws = b" " * (2 * CD)
    good = _text_of(CD - 100, 0)
    texts = [
        b'"QU\\/D"', b'["QU-_"]', b'"QU\nJD"', b'"QUJD', b'[["QQ=="]]', b"[1,2]", b'"QQ==",', b'["QQ==",]', b'"QQ=="]',
        b'["QQ=="', b'"QQ=="' + ws + b'"QUJD"', b'["QQ=="]' + ws + b"x", b'"QQ=="' + ws + b"]", b"[" + ws + b",",
        # two faults in one text: the lower one wins, also when they sit in different chunks
        good + b',"Q"' + ws + b',"QQ="', good + b',"QQ="' + ws + b',"Q"', b'"="' + ws + ws + b"x",
        b"[" + good + ws + b'"QUJD"' + ws + b"x]",
        # a text that ends inside a string, chunks later
        b'["QUJD","' + b"QUJD" * CD,
    ]
    res = _decode_same(native, dev, texts, ref=True)
    assert all(r[3] == 1 for r in res)


def test_decode_capacities(native, dev, CD):
    text = _text_of(2 * CD + 50, 1)
    data, ends, _ = native.base64_decode_rows(text)
    nb, nr = len(data), len(ends)
    jobs = [(text, 1, 2, nb, nr), (text, 2, 1, nb - 1, nr), (text, 3, 3, nb, nr - 1), (text, 0, 5, 0, 0)]
    res = _decode(native, dev, jobs)
    _decode_check(native, [text], res[:1])
    for length, rows, depth, err, first_bad, out, eout, guards in res[1:]:
        assert (err, length, rows) == (3, nb, nr) and guards
        assert out == b"\xee" * len(out) and eout == b"\xee" * len(eout)
    # the bounds, on texts that attain them
    for n in (2, 3, 4, 5, 6, 7, 8, 9, CD, CD + 1, CD + 2, CD + 4):
        m = n - 2 if (n - 2) % 4 != 1 else n - 3
        t = b'"' + b"Q" * m + b'"' + b" " * (n - 2 - m)
        (length, rows, _, err, _, _, _, guards), = _decode(native, dev, [(t, 0, 0, None, None)])
        assert (err, length, rows, guards) == (0, native.gpu.base64_rows_max_bytes(n), 1, True)
    dense = (b'"",' * 700)[:-1]
    (length, rows, _, err, _, _, _, guards), = _decode(native, dev, [(dense, 0, 0, None, None)])
    assert (err, length, rows, guards) == (0, 0, native.gpu.base64_rows_max_rows(len(dense)), True) and rows == 700


def test_code_2(native, dev):
    buf = _filled(4096, dev)
    p = buf.data_ptr()
    enc = native.gpu.device_base64_encode_rows
    dec = native.gpu.device_base64_decode_rows

    def e(src, n, tab, rows, dst, cap):
        (length, err, _), = enc([src], [n], [tab], [rows], True, [dst], [cap], 0)
        return err

    assert e(0, 8, p + 1024, 1, p + 2048, 100) == 2            # no src
    assert e(p, 8, p + 1024, 1, 0, 100) == 2                   # no dst
    assert e(p, 8, 0, 1, p + 2048, 100) == 2                   # rows without row_ends
    assert e(p, 8, p + 1024, 0, p + 2048, 100) == 2            # bytes without rows
    assert e(p, 8, p + 1026, 1, p + 2048, 100) == 2            # a misaligned row_ends
    assert e(p, (1 << 32) - 1, p + 1024, 1, p + 2048, 100) == 2  # n above 2^32 - 2
    assert e(p, 3 << 30, p + 1024, 1, p + (4 << 30), 1 << 33) == 2  # an output above 2^32 - 1
    assert e(p, 64, p + 1024, 1, p + 32, 200) == 2             # src and dst overlap
    assert e(p, 64, p + 1024, 4, p + 1000, 200) == 2           # row_ends and dst overlap
    assert e(0, 0, 0, 0, 0, 100) == 2                          # "[]" needs a dst

    def d(src, n, dst, cap, ends, row_cap):
        (length, rows, depth, err, _), = dec([src], [n], [dst], [cap], [ends], [row_cap], 0)
        return err

    assert d(0, 8, p + 1024, 100, p + 2048, 10) == 2           # no src
    assert d(p, (1 << 32) - 1, p + (5 << 30), 100, p + (6 << 30), 10) == 2
    assert d(p, 8, 0, 100, p + 2048, 10) == 2                  # no dst for a capacity
    assert d(p, 8, p + 1024, 100, 0, 10) == 2                  # no row_ends for a capacity
    assert d(p, 8, p + 1024, 100, p + 2050, 10) == 2           # a misaligned row_ends
    assert d(p, 64, p + 32, 100, p + 2048, 10) == 2            # src and dst overlap
    assert d(p, 64, p + 1024, 100, p + 32, 10) == 2            # src and row_ends overlap
    assert d(p, 64, p + 1024, 100, p + 1028, 10) == 2          # dst and row_ends overlap
    assert d(0, 0, 0, 0, 0, 0) == 0                            # nothing to do
    assert bool((buf == 0xEE).all())


def test_many_jobs_of_mixed_verdicts(native, dev, CE, CD):
    good = _text_of(CD + 300, 1)
    data, ends, _ = native.base64_decode_rows(good)
    jobs = [(good, 1, 1, None, None), (b'"Q"', 0, 0, None, None), (good, 2, 3, len(data) - 1, None), (b"", 0, 0, None, None),
            (_text_of(3 * CD, 0), 5, 7, None, None), (good[:-1], 0, 0, None, None), (b" \n", 0, 0, None, None)]
    res = _decode(native, dev, jobs)
    assert [r[3] for r in res] == [0, 1, 3, 0, 0, 1, 0]
    _decode_check(native, [good, b'"Q"'], res[:2])
    _decode_check(native, [j[0] for j in jobs[3:]], res[3:])
    assert res[2][5] == b"\xee" * len(res[2][5]) and res[2][7]

    payload = _payload(CE + 200, 9)
    table = [3, 3, CE - 1, CE + 200]
    want = native.base64_encode_rows(payload, _ends_image(table), True)
    ejobs = [(payload, table, 1, 2, None), (payload, [5, 4, CE + 200], 0, 0, None), (payload, table, 3, 1, len(want) - 1),
             (b"", [], 0, 0, None), (b"", [0, 0], 0, 1, None), (_payload(7), [7], 2, 2, None)]
    eres = _encode(native, dev, ejobs, True)
    assert [(r[1], r[2]) for r in eres] == [(0, 0), (1, 1), (3, 0), (0, 0), (0, 0), (0, 0)]
    assert eres[0][3][:eres[0][0]] == want and eres[3][3][:2] == b"[]" and eres[4][3][:7] == b'["",""]'
    assert eres[5][3][:eres[5][0]] == R.print_rows([_payload(7)])
    assert all(r[4] for r in eres)
    assert eres[1][3] == b"\xee" * len(eres[1][3]) and eres[2][3] == b"\xee" * len(eres[2][3])


# --------------------------------------------------------------------- ops

def test_ops_round_trip(native, dev, CE):
    from brpc_amd import ops
    rng = random.Random(5)
    rows = [bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 1, 2, 3, 50, CE // 3, CE + 9]))) for _ in range(40)]
    data = _to_dev(b"".join(rows), dev)
    for dtype in (torch.int32, torch.int64):
        ends = torch.tensor(R.row_ends(rows), dtype=dtype, device=dev)
        for brackets in (True, False):
            text = ops.base64_encode_rows(data, ends, brackets=brackets)
            assert bytes(text.cpu().numpy()) == R.print_rows(rows, brackets)
            back, back_ends = ops.base64_decode_rows(text)
            assert back_ends.dtype == torch.int32 and torch.equal(back, data)
            assert back_ends.tolist() == R.row_ends(rows)
    # a 2-D tensor means equal rows
    grid = _to_dev(_payload(60), dev).view(12, 5)
    text = ops.base64_encode_rows(grid)
    assert bytes(text.cpu().numpy()) == R.print_rows([bytes(r) for r in grid.cpu().numpy()])
    # no rows
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    assert bytes(ops.base64_encode_rows(empty, none).cpu().numpy()) == b"[]"
    assert ops.base64_encode_rows(empty, none, brackets=False).numel() == 0
    b, e = ops.base64_decode_rows(_to_dev(b"[ ]", dev))
    assert b.numel() == 0 and e.numel() == 0
    with pytest.raises(ValueError, match="row 1"):
        ops.base64_encode_rows(data[:10], torch.tensor([5, 4, 10], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="too small"):
        ops.base64_decode_rows(text, max_rows=3)


def test_ops_pb_link(native, dev):
    from brpc_amd import ops
    rows = [b"", b"A", b"\x00\xff" * 70, b"tensor-bytes", b""]
    data = _to_dev(b"".join(rows), dev)
    ends = torch.tensor(R.row_ends(rows), dtype=torch.int32, device=dev)
    message = ops.pb_build_rows(4, data, ends, "bytes")
    values, row_ends = ops.pb_split_rows(message, 4, "bytes")[:2]
    text = ops.base64_encode_rows(values, row_ends)
    assert bytes(text.cpu().numpy()) == R.print_rows(rows)
    back, back_ends = ops.base64_decode_rows(text)
    again = ops.pb_build_rows(4, back, back_ends, "bytes")
    assert torch.equal(again, message)


def test_ops_host_fallback(native, dev):
    from brpc_amd import ops
    rows = [b"hello world, this is a row", b"", b"xy"]
    body = base64.b64encode(rows[0])
    for line_break in (b"\n", b"\\n"):  # raw, and as an escape
        text = b'["' + body[:8] + line_break + body[8:] + b'", "", "eHk"]'
        assert native.base64_decode_rows(text) == (None, 10)
        host = [native.base64_decode(s) for s in native.json_reader_string_array(text)]
        assert host == rows
        got, got_ends = ops.base64_decode_rows(_to_dev(text, dev))
        assert bytes(got.cpu().numpy()) == b"".join(host) and got_ends.tolist() == R.row_ends(host)
    with pytest.raises(ValueError, match="offset 3"):
        ops.base64_decode_rows(_to_dev(b'["Q"]', dev))
