"""JSON string bodies on the device (gpu::DeviceEscapeJsonStrings /
DeviceUnescapeJsonStrings / DeviceValidateUtf8, gpu/json_string_kernels.hip)
against the host twins and, for well-formed cases, Python's json module and
UTF-8 decoder: every length around a lane (16 bytes) and a chunk, every src x
dst alignment in one call, escapes and backslash runs across chunk edges, the
verdicts with their offsets, rows, refusals."""
import json
import struct

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

GUARD = 16


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def C(native):
    c = native.gpu.json_string_chunk_bytes()
    assert c % 16 == 0 and c >= 256 * 16
    return c


def _data(n):
    return (bytes(range(256)) * (n // 256 + 1))[:n]


def _lengths(C):
    return [0, 1, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]


def _to_dev(data, dev):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev)


def _run(native, dev, kind, jobs, quote=True):
    """kind: "escape" / "unescape". jobs: [(src bytes, src offset, dst offset,
    cap or None, row_ends list or None)] in one call -> [(len, err, first_bad,
    dst bytes [0, cap), guards intact)]. Every buffer is 0xEE-filled; src and
    dst start `offset` bytes past a 256-byte boundary plus GUARD."""
    keep, srcs, ns, dsts, caps, ends, rows = [], [], [], [], [], [], []
    with_rows = any(j[4] is not None for j in jobs)
    for src, so, do, cap, row_ends in jobs:
        n = len(src)
        if cap is None:
            if kind == "unescape":
                cap = n
            else:
                cap = native.gpu.json_escape_worst_case(n, len(row_ends) if row_ends is not None else 0)
        sbuf = torch.full((GUARD + so + n + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        if n:
            sbuf[GUARD + so:GUARD + so + n] = _to_dev(src, dev)
        dbuf = torch.full((GUARD + do + cap + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0
        keep.append((dbuf, do, cap, sbuf))
        srcs.append(sbuf.data_ptr() + GUARD + so)
        ns.append(n)
        dsts.append(dbuf.data_ptr() + GUARD + do)
        caps.append(cap)
        if with_rows:
            if row_ends is None:
                ends.append(0)
                rows.append(0)
            else:
                e = torch.tensor(row_ends, dtype=torch.int64).to(torch.int32).to(dev)
                keep[-1] += (e,)
                ends.append(e.data_ptr())
                rows.append(len(row_ends))
    torch.cuda.synchronize(dev)
    if kind == "escape":
        res = native.gpu.device_json_escape(srcs, ns, dsts, caps, ends, rows, quote, 0)
    else:
        res = native.gpu.device_json_unescape(srcs, ns, dsts, caps, 0)
    out = []
    for r, k in zip(res, keep):
        dbuf, do, cap = k[0], k[1], k[2]
        host = dbuf.cpu().numpy()
        lo = GUARD + do
        guards = bool((host[:lo] == 0xEE).all()) and bool((host[lo + cap:] == 0xEE).all())
        out.append((r[0], r[1], r[2], host[lo:lo + cap].tobytes(), guards))
    return out


def _validate(native, dev, texts, offset=0):
    keep, srcs, ns = [], [], []
    for k, t in enumerate(texts):
        so = (offset + k) % 16 if offset else 0
        buf = torch.full((GUARD + so + len(t) + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        if t:
            buf[GUARD + so:GUARD + so + len(t)] = _to_dev(t, dev)
        keep.append(buf)
        srcs.append(buf.data_ptr() + GUARD + so)
        ns.append(len(t))
    torch.cuda.synchronize(dev)
    return native.gpu.device_utf8_validate(srcs, ns, 0)


def _py_start(t):
    try:
        t.decode()
        return None
    except UnicodeDecodeError as e:
        return e.start


def _check_unescape(native, bodies, res):
    """Every result against the host twin: verdict, offset, bytes; dst untouched when refused."""
    for body, (length, err, first_bad, data, guards) in zip(bodies, res):
        want, bad = native.json_unescape(body)
        tag = (len(body), body[:24], body[-24:])
        assert guards, tag
        if want is None:
            assert (err, first_bad) == (1, bad), tag
            assert data == b"\xee" * len(data), tag
        else:
            assert (length, err) == (len(want), 0), tag
            assert data[:length] == want, tag
            assert data[length:] == b"\xee" * (len(data) - length), tag


def _valid_body(pattern, n, native):
    """n bytes of `pattern` repeated, its cut-off last escape replaced by x's."""
    body = (pattern * (n // len(pattern) + 1))[:n]
    for k in range(0, 13):
        t = body[:n - k] + b"x" * k
        if native.json_unescape(t)[0] is not None:
            return t
    raise AssertionError("no valid cut")


# ------------------------------------------------------------------ lengths

def test_escape_lengths(native, dev, C):
    jobs = [(_data(n), 0, 0, None, None) for n in _lengths(C)]
    for q in (True, False):
        for n, (length, err, _, text, guards) in zip(_lengths(C), _run(native, dev, "escape", jobs, quote=q)):
            want = native.json_escape(_data(n), quote=q)
            assert (length, err) == (len(want), 0), (n, q)
            assert text[:length] == want, (n, q)
            assert text[length:] == b"\xee" * (len(text) - length) and guards, (n, q)


def test_unescape_lengths(native, dev, C):
    bodies = []
    for n in _lengths(C):
        bodies.append(_data(n))  # a quote at 0x22 at the latest
        bodies.append(native.json_escape(_data(2 * n), quote=False)[:n])  # may cut its last escape
        bodies.append(_valid_body(b'ab\\n\\u00e9c\\\\\\ud83d\\ude00 \\"', n, native))
    res = _run(native, dev, "unescape", [(b, 0, 0, None, None) for b in bodies])
    _check_unescape(native, bodies, res)
    assert {r[1] for r in res} == {0, 1}


def test_validate_lengths(native, dev, C):
    unit = "aé€\U0001f600".encode()
    texts = []
    for n in _lengths(C):
        t = (unit * (n // len(unit) + 1))[:n]
        while _py_start(t) is not None:  # a character cut at the end: ASCII instead
            cut = _py_start(t)
            t = t[:cut] + b"a" * (n - cut)
        assert len(t) == n
        texts.append(t)
    assert _validate(native, dev, texts) == [(0, 0)] * len(texts)
    assert _validate(native, dev, texts, offset=1) == [(0, 0)] * len(texts)


# --------------------------------------------------------------- alignments

@pytest.mark.parametrize("extra", [100, "C+5"])
def test_every_alignment_in_one_call(native, dev, C, extra):
    n = 100 if extra == 100 else C + 5
    offsets = [(so, do) for so in range(16) for do in range(16)]
    specials = b'"\\\n\x01'
    datas = []
    for so, do in offsets:
        d = bytearray((97 + (i * 7 + so * 31 + do) % 26) for i in range(n))
        for i in range((so + do) % 29, n, 29 + do):  # an escape every 29 bytes or so; none at all in a few
            if (so, do) not in ((0, 0), (3, 5), (15, 15)):
                d[i] = specials[(i + so) % 4]
        datas.append(bytes(d))
    res = _run(native, dev, "escape", [(d, so, do, None, None) for d, (so, do) in zip(datas, offsets)], quote=False)
    texts = []
    for d, (so, do), (length, err, _, text, guards) in zip(datas, offsets, res):
        want = native.json_escape(d, quote=False)
        assert (length, err) == (len(want), 0), (so, do)
        assert text[:length] == want, (so, do)
        assert guards, (so, do)  # the 16 bytes before and after dst are untouched
        texts.append(want)
    res = _run(native, dev, "unescape", [(t, so, do, None, None) for t, (so, do) in zip(texts, offsets)])
    for d, (so, do), (length, err, _, data, guards) in zip(datas, offsets, res):
        assert (length, err) == (n, 0), (so, do)
        assert data[:length] == d, (so, do)
        assert guards, (so, do)


def test_greatest_expansion(native, dev, C):
    n = C + 1
    plain = bytes(97 + i % 26 for i in range(n))
    jobs = [(b"\x01" * n, 1, 3, None, None), (plain, 2, 5, None, None), (b'"' * n, 0, 7, None, None)]
    (l1, e1, _, t1, g1), (l2, e2, _, t2, g2), (l3, e3, _, t3, g3) = _run(native, dev, "escape", jobs)
    assert (l1, e1) == (6 * n + 2, 0) and t1 == b'"' + b"\\u0001" * n + b'"' and g1
    assert (l2, e2) == (n + 2, 0) and t2[:l2] == b'"' + plain + b'"' and g2
    assert (l3, e3) == (2 * n + 2, 0) and t3[:l3] == b'"' + b'\\"' * n + b'"' and g3


# --------------------------------------------------------------- chunk edges

def test_escapes_across_a_chunk_edge(native, dev, C):
    bodies, wants = [], []
    for esc in ["\\n", "\\u00e9", "\\u20ac", "\\ud83d\\ude00"]:
        for k in range(1, len(esc) + 1):
            body = "a" * (C - k) + esc + "b" * 20
            bodies.append(body.encode())
            wants.append(json.loads('"' + body + '"').encode())
    res = _run(native, dev, "unescape", [(b, k % 16, (3 * k) % 16, None, None) for k, b in enumerate(bodies)])
    _check_unescape(native, bodies, res)
    for want, (length, err, _, data, _) in zip(wants, res):
        assert err == 0 and data[:length] == want


def test_backslash_runs_across_chunk_edges(native, dev, C):
    bodies, wants = [], []
    for run in range(1, 7):
        for end in (C - 1, C, C + 1):  # the offset of the run's last backslash
            body = b"a" * (end + 1 - run) + b"\\" * run + b"nzz"
            bodies.append(body)
            wants.append(b"a" * (end + 1 - run) + b"\\" * (run // 2) + (b"\n" if run % 2 else b"n") + b"zz")
    bodies += [b"\\" * (2 * C + 1) + b'"', b"\\" * (2 * C) + b'"', b"\\" * (3 * C)]
    res = _run(native, dev, "unescape", [(b, 0, 0, None, None) for b in bodies])
    _check_unescape(native, bodies, res)
    for want, (length, err, _, data, _) in zip(wants, res):
        assert err == 0 and data[:length] == want
    odd, even, whole = res[-3:]
    assert (odd[0], odd[1]) == (C + 1, 0) and odd[3][:C + 1] == b"\\" * C + b'"'  # the carry crossed a whole chunk
    assert (even[1], even[2]) == (1, 2 * C)
    assert (whole[0], whole[1]) == (3 * C // 2, 0)


# ----------------------------------------------------------------- verdicts

CODE1 = [(b'"', 0), (b"\\", 0), (b"\\x41", 0), (b"\\u12", 0), (b"\\u", 0), (b"\\u12g4 more", 0), (b"\\ud83d", 0),
         (b"\\ud83dabcdefgh", 0), (b"\\ud83d\\n", 0), (b"\\ud83d\\u0041", 0), (b"\\ud83d\\ude0", 0), (b"\\ude00", 0),
         (b"\\ud83d\\ude00\\ude00", 12), (b"\\\\ud83d\\ude00", 7), (b"\\ud83d\\ud83d\\ude00", 0)]


def test_every_refused_form_with_its_offset(native, dev, C):
    bodies, offsets = [], []
    for lead in (0, 5, C - 3, C, 2 * C + 17):
        for tail, at in CODE1:
            # the form ends the text, or fine text follows it
            bodies.append(b"p" * lead + tail + (b"" if lead % 2 else b" and fine text after it \\n"))
            offsets.append(lead + at)
    res = _run(native, dev, "unescape", [(b, k % 16, (5 * k) % 16, None, None) for k, b in enumerate(bodies)])
    _check_unescape(native, bodies, res)
    assert [(r[1], r[2]) for r in res] == [(1, o) for o in offsets]


def test_lowest_bad_spot_wins(native, dev, C):
    good = b"abcdef\\nghijklmn" * (4 * C // 16)  # an escape in every lane, letters at 0..5 and 8..15

    def spoil(*offsets):
        t = bytearray(good)
        for o in offsets:
            assert o % 16 not in (6, 7)
            t[o] = ord('"')
        return bytes(t)

    lo, hi = C + 5, 3 * C - 1
    lane0, lane255 = 2 * C, 2 * C + 16 * 255 + 15
    bodies = [spoil(lo, hi), spoil(hi), spoil(lane0, lane255), spoil(lane255), good]
    res = _run(native, dev, "unescape", [(b, 0, 0, None, None) for b in bodies])
    _check_unescape(native, bodies, res)
    assert [(r[1], r[2]) for r in res] == [(1, lo), (1, hi), (1, lane0), (1, lane255), (0, 0)]
    assert res[4][3][:res[4][0]] == native.json_unescape(good)[0]  # the good job next to them is whole


# -------------------------------------------------------------------- UTF-8

ILL_FORMED = [b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",
              b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\x80", b"\xbf",
              b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xe2\x82\x41", b"\xf0\x9f\x98\x41", b"\xe2\x82\xac\x80",
              b"\xf0\x9f\x98\x41\x80", b"\xe2\x82\x41\x80", b"\xc3\xa9\xa9"]


def test_utf8_ill_formed_classes_report_python_s_start(native, dev, C):
    texts = []
    for lead in (b"", b"abc", "€".encode() * 7, b"a" * (C - 2), b"a" * C, "é".encode() * C):
        for bad in ILL_FORMED:
            texts += [lead + bad, lead + bad + b"tail \xc3\xa9"]
    got = _validate(native, dev, texts, offset=3)
    for t, (err, first_bad) in zip(texts, got):
        assert (err, first_bad) == (1, _py_start(t)), (len(t), t[-12:])
        assert native.utf8_first_bad(t) == first_bad


def test_utf8_characters_across_a_chunk_edge(native, dev, C):
    good, cut, wants = [], [], []
    for ch in ("é", "€", "\U0001f600"):
        enc = ch.encode()
        for k in range(1, len(enc)):  # k bytes of the character before the edge
            t = b"a" * (C - k) + enc + b"z" * 9
            good.append(t)
            cut.append(t[:C])  # cut at the edge: the lead byte's offset
            wants.append(C - k)
    assert _validate(native, dev, good) == [(0, 0)] * len(good)
    assert _validate(native, dev, cut) == [(1, w) for w in wants]
    stray = [b"a" * C + b"\x80" + b"b" * 5,                       # a stray continuation as a chunk's first byte
             b"a" * (C - 2) + b"\xc3\xa9" + b"\xa9",             # ... right behind a whole character
             b"a" * (C - 3) + b"\xf0\x9f\x98" + b"A\x80",        # a cut-off lead, then a stray: the lead wins
             b"a" * (C - 2) + b"\xe2\x82" + b"A\x80",
             b"a" * (C - 3) + b"\xf0\x9f\x98\x80" + b"\x80"]     # a whole character across the edge, then a stray
    got = _validate(native, dev, stray)
    assert got == [(1, C), (1, C), (1, C - 3), (1, C - 2), (1, C + 1)]
    assert [g[1] for g in got] == [_py_start(t) for t in stray]


def test_utf8_two_bad_spots_report_the_lower(native, dev, C):
    base = bytearray("é".encode() * (2 * C))
    lo, hi = C + 4, 3 * C + 1
    both, high = bytearray(base), bytearray(base)
    both[lo] = both[hi] = high[hi] = 0xFF
    got = _validate(native, dev, [bytes(both), bytes(high), bytes(base)])
    assert got == [(1, _py_start(bytes(both))), (1, _py_start(bytes(high))), (0, 0)]
    assert got[0][1] <= lo and got[1][1] > lo


# --------------------------------------------------------------------- rows

def _ends(rows):
    total, out = 0, []
    for r in rows:
        total += len(r)
        out.append(total)
    return out


def _rows_want(rows):
    return ",".join(json.dumps(r.decode("latin-1"), ensure_ascii=False) for r in rows).encode("latin-1")


def test_rows(native, dev, C):
    word = b'say "hi"\n\tback\\slash \x01 '
    fill = lambda n, k=0: (word * (n // len(word) + 1))[k:k + n]
    cases = [
        [fill(10)],
        [fill(C + 9)],
        [fill(7), fill(C)],
        [fill(31, r % 5) for r in range(257)],
        [b"", b"", fill(40), b"", fill(3), b"", b""],              # empty rows first, in the middle, last
        [fill(100)] + [b""] * 5000 + [fill(50)],                   # mostly punctuation, at one offset inside a chunk
        [fill(C - 1), fill(2), fill(C - 1)],                       # a boundary at C - 1 and at C + 1
        [fill(C), fill(5)],                                        # ... at C
        [fill(5), fill(2 * C + 40), fill(5)],                      # a row that spans three chunks
        [fill(9, r) for r in range(40)] + [fill(3 * C)] + [fill(1)] * 300,  # both place paths in one job
        [b"", b""],
    ]
    jobs = [(b"".join(rows), k % 16, (7 * k) % 16, None, _ends(rows)) for k, rows in enumerate(cases)]
    res = _run(native, dev, "escape", jobs)
    for rows, (length, err, _, text, guards) in zip(cases, res):
        want = _rows_want(rows)
        assert want == native.json_escape(b"".join(rows), row_ends=struct.pack("<%dI" % len(rows), *_ends(rows)))
        assert (length, err) == (len(want), 0), len(rows)
        assert text[:length] == want, len(rows)
        assert text[length:] == b"\xee" * (len(text) - length) and guards, len(rows)


def test_rows_bad_ends(native, dev, C):
    data = bytes(97 + i % 26 for i in range(C + 50))
    n = len(data)
    jobs = [(data, 0, 0, None, [10, 20, 15, n]),          # a decrease: the row that ends too low
            (data, 0, 0, None, [10, 20, n - 1]),          # does not end at n
            (data, 0, 0, None, [10, n + 5, n]),           # beyond n, then back
            (data, 0, 0, None, [10, 20, n]),
            (data, 0, 0, None, None)]
    res = _run(native, dev, "escape", jobs)
    assert [(r[1], r[2]) for r in res[:3]] == [(1, 2), (1, 2), (1, 2)]
    for r in res[:3]:
        assert r[3] == b"\xee" * len(r[3]) and r[4]
    want = b'"' + data[:10] + b'","' + data[10:20] + b'","' + data[20:] + b'"'
    assert (res[3][0], res[3][1]) == (len(want), 0) and res[3][3][:len(want)] == want
    assert (res[4][0], res[4][1]) == (n + 2, 0) and res[4][3][:n + 2] == b'"' + data + b'"'


def test_rows_of_a_split_repeated_string(native, dev):
    from brpc_amd.ops.json import json_escape_string
    from brpc_amd.ops.pb import pb_build_rows, pb_split_rows
    strings = ["plain", "", 'quoted "text"', "line\nbreak\ttab", "back\\slash", "é€\U0001f600", "\x01\x1f", "x" * 5000, ""]
    enc = [s.encode() for s in strings]
    values = _to_dev(b"".join(enc), dev)
    ends = torch.tensor(_ends(enc), dtype=torch.int32, device=dev)
    msg = pb_build_rows(4, values, ends, "bytes")
    got_values, got_ends = pb_split_rows(msg, 4, "bytes")
    text = json_escape_string(got_values, row_ends=got_ends)
    want = json.dumps(strings, ensure_ascii=False, separators=(",", ":"))[1:-1].encode()
    assert text.cpu().numpy().tobytes() == want


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_good_job_alone(native, dev, C):
    data = (b'ab"c\n' * C)[:C + 1]
    text = native.json_escape(data)
    (l1, e1, _, d1, g1), (l2, e2, _, d2, g2) = _run(native, dev, "escape",
                                                   [(data, 0, 0, len(text) - 1, None), (data, 1, 2, len(text), None)])
    assert (l1, e1) == (len(text), 3) and d1 == b"\xee" * (len(text) - 1) and g1
    assert (l2, e2) == (len(text), 0) and d2 == text and g2
    body = text[1:-1]
    (l1, e1, _, d1, g1), (l2, e2, _, d2, g2) = _run(native, dev, "unescape",
                                                   [(body, 0, 0, len(body) - 1, None), (body, 1, 2, None, None)])
    assert (l1, e1) == (len(body), 3) and d1 == b"\xee" * (len(body) - 1) and g1
    assert (l2, e2) == (len(data), 0) and d2[:l2] == data and g2
    # null src, overlapping ranges, rows without row_ends, next to a good job
    src = _to_dev(data, dev)
    both = torch.full((len(data) + len(text),), 0xEE, dtype=torch.uint8, device=dev)
    both[:len(data)] = src
    out = torch.full((len(text),), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    p = both.data_ptr()
    res = native.gpu.device_json_escape([0, p, p, src.data_ptr()], [len(data)] * 4,
                                        [out.data_ptr(), p + len(data) - 1, p, out.data_ptr()], [len(text)] * 4)
    assert [r[1] for r in res] == [2, 2, 2, 0]
    assert res[3][0] == len(text) and out.cpu().numpy().tobytes() == text
    assert both.cpu().numpy()[len(data):].tobytes() == b"\xee" * len(text)  # nothing was launched for them
    res = native.gpu.device_json_escape([src.data_ptr()], [len(data)], [out.data_ptr()], [len(text)], [0], [3])
    assert res[0][1] == 2
    ends = torch.tensor([len(data)], dtype=torch.int32, device=dev)
    res = native.gpu.device_json_escape([src.data_ptr()], [len(data)], [out.data_ptr()], [len(text)],
                                        [ends.data_ptr() + 1], [1])  # misaligned row_ends
    assert res[0][1] == 2
    tsrc = _to_dev(body, dev)
    back = torch.full((len(body),), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_json_unescape([0, tsrc.data_ptr(), tsrc.data_ptr()], [len(body)] * 3,
                                          [back.data_ptr(), tsrc.data_ptr() + 8, back.data_ptr()], [len(body)] * 3, 0)
    assert [r[1] for r in res] == [2, 2, 0]
    assert res[2][0] == len(data) and back.cpu().numpy()[:len(data)].tobytes() == data
    assert tsrc.cpu().numpy().tobytes() == body
    assert native.gpu.device_utf8_validate([0, tsrc.data_ptr()], [5, len(body)], 0) == [(2, 0), (0, 0)]
    # nothing to do is no launch and no error
    assert native.gpu.device_json_escape([0], [0], [0], [0], quote=False) == [(0, 0, 0)]
    assert native.gpu.device_json_unescape([0], [0], [0], [0], 0) == [(0, 0, 0)]
    assert native.gpu.device_utf8_validate([0], [0], 0) == [(0, 0)]
    # an empty string with its quotes is two bytes
    two = torch.full((4,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    assert native.gpu.device_json_escape([0], [0], [two.data_ptr() + 1], [2]) == [(2, 0, 0)]
    assert two.cpu().numpy().tobytes() == b'\xee""\xee'


def test_string_field_of_a_scanned_payload(native, dev):
    from brpc_amd.ops.pb import pb_build_message
    first = torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev)
    value = ('He said "no".\n\tThen: C:\\temp \x01 é€\U0001f600 ' * 30).encode()[:1000]
    field = _to_dev(value, dev)
    msg, _ = pb_build_message([(1, first, "bytes"), (2, field, "bytes")])
    torch.cuda.synchronize(dev)
    nf, table = native.gpu.device_pb_scan(msg.data_ptr(), msg.numel(), 0)
    off, ln = native.gpu.device_payload_field(nf, table, 2)
    assert ln == 1000 and (msg.data_ptr() + off) % 16 != 0
    want = native.json_escape(value)
    prefix = b'"text":'
    nbody = len(want) - 2  # the room an unescape of the body must be given
    buf = torch.full((len(prefix) + len(want) + nbody,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    text_at = buf.data_ptr() + len(prefix)
    (length, err, _), = native.gpu.device_json_escape([msg.data_ptr() + off], [ln], [text_at], [len(want)])
    assert (length, err) == (len(want), 0)
    (length, err, _), = native.gpu.device_json_unescape([text_at + 1], [nbody], [text_at + len(want)], [nbody], 0)
    assert (length, err) == (1000, 0)
    host = buf.cpu().numpy().tobytes()
    assert host[:len(prefix)] == b"\xee" * len(prefix)
    assert host[len(prefix):len(prefix) + len(want)] == want
    assert host[len(prefix) + len(want):][:1000] == value
    assert host[len(prefix) + len(want) + 1000:] == b"\xee" * (nbody - 1000)


# ---------------------------------------------------------------------- ops

def test_ops_round_trip(native, dev, C):
    from brpc_amd.ops.json import json_escape_string, json_unescape_string, utf8_validate
    g = torch.Generator().manual_seed(3)
    rand = torch.randint(0, 256, (3 * C + 11,), dtype=torch.uint8, generator=g)
    kinds = 'every kind: \\ " / \b \f \n \r \t \x00 \x1f \x7f é € \U0001f600 end'.encode()
    for raw in (rand.numpy().tobytes(), kinds, b""):
        t = _to_dev(raw, dev) if raw else torch.empty(0, dtype=torch.uint8, device=dev)
        body = json_escape_string(t, quote=False)
        assert body.cpu().numpy().tobytes() == native.json_escape(raw, quote=False)
        assert json_escape_string(t).cpu().numpy().tobytes() == native.json_escape(raw)
        assert json_unescape_string(body).cpu().numpy().tobytes() == raw
    assert json.loads(json_escape_string(_to_dev(kinds, dev)).cpu().numpy().tobytes().decode()) == kinds.decode()
    assert utf8_validate(_to_dev(kinds, dev)) is None
    assert utf8_validate(_to_dev(kinds + b"\xed\xa0\x80", dev)) == len(kinds)
    with pytest.raises(ValueError, match=r"takes \d+"):
        json_escape_string(_to_dev(kinds, dev), max_bytes=len(kinds))


def test_ops_unescape_host_route(native, dev):
    from brpc_amd.ops.json import json_unescape_string
    lone = b"a lone \\ud83d surrogate"
    assert native.json_unescape(lone) == (None, 7)
    want = native.json_reader_string(lone)
    assert want is not None
    assert json_unescape_string(_to_dev(lone, dev)).cpu().numpy().tobytes() == want
    with pytest.raises(ValueError, match=r"offset 9\b"):
        json_unescape_string(_to_dev(b"a bad esc\\q here", dev))
