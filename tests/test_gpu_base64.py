"""Base64 on the device (gpu::DeviceBase64Encode / DeviceBase64Decode,
gpu/base64_kernels.hip) against Python's stdlib: every length around a lane
(12 bytes / 16 symbols) and a chunk, every src x dst alignment in one launch,
what the decoder calls canonical and what it hands to the host."""
import base64

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")
pytestmark = pytest.mark.gpu

NONE_ODD = 0  # first_odd of a job that is not err 1


@pytest.fixture(scope="module")
def dev():
    from brpc_amd import native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert native.gpu.device_count() > 0, "native runtime sees no HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def C(native):
    c = native.gpu.base64_chunk_bytes()
    assert c % 12 == 0 and c >= 256 * 12
    return c


def _data(n):
    return (bytes(range(256)) * (n // 256 + 1))[:n]


def _lengths(C):
    return [0, 1, 2, 3, 4, 11, 12, 13, 47, 48, 49, C - 1, C, C + 1, 3 * C + 7]


GUARD = 16


def _run(native, dev, encode, jobs):
    """jobs: [(src bytes, src offset, dst offset, cap or None)] in one launch
    -> [(len, err, first_odd, dst bytes [0, cap), guards intact)]. Every buffer
    is 0xEE-filled; src and dst start `offset` bytes past a 256-byte boundary
    plus GUARD."""
    keep, srcs, ns, dsts, caps = [], [], [], [], []
    for src, so, do, cap in jobs:
        n = len(src)
        if cap is None:
            cap = (n + 2) // 3 * 4 if encode else n // 4 * 3 + (n % 4) * 3 // 4
        sbuf = torch.full((GUARD + so + n + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        if n:
            sbuf[GUARD + so:GUARD + so + n] = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
        dbuf = torch.full((GUARD + do + cap + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        assert sbuf.data_ptr() % 256 == 0 and dbuf.data_ptr() % 256 == 0
        keep.append((dbuf, do, cap))
        srcs.append(sbuf.data_ptr() + GUARD + so)
        ns.append(n)
        dsts.append(dbuf.data_ptr() + GUARD + do)
        caps.append(cap)
        keep.append(sbuf)
    torch.cuda.synchronize(dev)
    fn = native.gpu.device_base64_encode if encode else native.gpu.device_base64_decode
    res = fn(srcs, ns, dsts, caps, 0)
    out = []
    for r, (dbuf, do, cap) in zip(res, keep[::2]):
        host = dbuf.cpu().numpy()
        lo = GUARD + do
        guards = bool((host[:lo] == 0xEE).all()) and bool((host[lo + cap:] == 0xEE).all())
        out.append((r[0], r[1], r[2] if len(r) > 2 else NONE_ODD, host[lo:lo + cap].tobytes(), guards))
    return out


def test_encode_lengths(native, dev, C):
    jobs = [(_data(n), 0, 0, None) for n in _lengths(C)]
    for n, (length, err, _, text, guards) in zip(_lengths(C), _run(native, dev, True, jobs)):
        want = base64.b64encode(_data(n))
        assert (length, err) == (len(want), 0), n
        assert text == want, n
        assert guards, n
    everything = b"".join(base64.b64encode(_data(n)) for n in _lengths(C))
    assert len(set(everything)) == 65 and b"==" in everything  # all 64 symbols, both pad forms


@pytest.mark.parametrize("extra", [100, "C+5"])
def test_every_alignment_in_one_call(native, dev, C, extra):
    n = 100 if extra == 100 else C + 5
    offsets = [(so, do) for so in range(16) for do in range(16)]
    datas = [bytes((i * 7 + so * 31 + do) & 255 for i in range(n)) for so, do in offsets]
    res = _run(native, dev, True, [(d, so, do, None) for d, (so, do) in zip(datas, offsets)])
    texts = []
    for d, (so, do), (length, err, _, text, guards) in zip(datas, offsets, res):
        want = base64.b64encode(d)
        assert (length, err) == (len(want), 0), (so, do)
        assert text == want, (so, do)
        assert guards, (so, do)  # the 16 bytes before and after dst are untouched
        texts.append(text)
    # and back: every src x dst alignment of the decoder
    res = _run(native, dev, False, [(t, so, do, None) for t, (so, do) in zip(texts, offsets)])
    for d, (so, do), (length, err, _, data, guards) in zip(datas, offsets, res):
        assert (length, err) == (n, 0), (so, do)
        assert data[:length] == d, (so, do)
        assert guards, (so, do)


def test_decode_round_trip_padded_and_unpadded(native, dev, C):
    lengths = _lengths(C)
    padded = [base64.b64encode(_data(n)) for n in lengths]
    jobs = [(t, 0, 0, None) for t in padded] + [(t.rstrip(b"="), 3, 5, None) for t in padded]
    res = _run(native, dev, False, jobs)
    for k, (length, err, _, data, guards) in enumerate(res):
        n = lengths[k % len(lengths)]
        assert (length, err) == (n, 0), (k, n)  # len is right for p = 0, 1, 2
        assert data[:n] == _data(n), (k, n)
        assert guards, (k, n)
    assert {len(t) - len(t.rstrip(b"=")) for t in padded} == {0, 1, 2}


def test_decode_length_rule(native, dev, C):
    body = base64.b64encode(_data(C))  # 4 * C / 3 symbols
    texts = [b"Q", body + b"Q", body[:5], body + b"QQ=", body + b"Q==", body[:6] + b"=", b"=", b"=="]
    res = _run(native, dev, False, [(t, 0, 0, None) for t in texts])
    for t, (length, err, first_odd, _, guards) in zip(texts, res):
        assert (err, first_odd) == (1, len(t)), t[-8:]
        assert native.base64_decode(t) is None, t[-8:]  # the host refuses them too
        assert guards


def test_decode_bad_bytes_in_different_workgroups(native, dev, C):
    S = C * 4 // 3
    good = base64.b64encode(_data(4 * C))
    assert len(good) == 4 * S
    lo, hi = S + 5, 3 * S - 1

    def spoil(*offsets):
        t = bytearray(good)
        for o in offsets:
            t[o] = ord("!")
        return bytes(t)

    lane0, lane255 = 2 * S, 2 * S + 16 * 255 + 15
    texts = [spoil(lo, hi), spoil(hi), spoil(lane0, lane255), spoil(lane255), good]
    res = _run(native, dev, False, [(t, 0, 0, None) for t in texts])
    assert [(r[1], r[2]) for r in res] == [(1, lo), (1, hi), (1, lane0), (1, lane255), (0, NONE_ODD)]
    assert res[4][0] == 4 * C and res[4][3] == _data(4 * C)  # the good job next to them is whole


@pytest.mark.parametrize("odd", [b"=", b"\n", b"\r", b" "])
def test_decode_pad_and_whitespace_in_the_middle(native, dev, C, odd):
    from brpc_amd.ops.json import base64_decode
    data = _data(C + 300)
    text = base64.b64encode(data)
    at = len(text) // 2 + 1
    broken = text[:at] + odd + text[at:]
    (length, err, first_odd, _, _), = _run(native, dev, False, [(broken, 0, 0, None)])
    assert (err, first_odd) == (1, at)
    t = torch.from_numpy(np.frombuffer(broken, dtype=np.uint8).copy()).to(dev)
    if odd == b"=":
        with pytest.raises(ValueError, match=r"offset %d\b" % at):
            base64_decode(t)
    else:  # the host decoder skips it: its result comes back
        assert base64_decode(t).cpu().numpy().tobytes() == data


def test_ops_decode_raises_on_junk_naming_the_offset(dev):
    from brpc_amd.ops.json import base64_decode
    text = bytearray(base64.b64encode(_data(999)))
    text[777] = ord("*")
    t = torch.from_numpy(np.frombuffer(bytes(text), dtype=np.uint8).copy()).to(dev)
    with pytest.raises(ValueError, match=r"offset 777\b"):
        base64_decode(t)


def test_decode_non_canonical_trailing_bits_as_on_the_host(native, dev):
    texts = [b"QR==", b"QUJ=", b"QR", b"QUJ", b"QUJDQR=="]
    res = _run(native, dev, False, [(t, 0, 0, None) for t in texts])
    for t, (length, err, _, data, _) in zip(texts, res):
        want = native.base64_decode(t)
        assert want is not None
        assert (length, err) == (len(want), 0), t
        assert data[:length] == want, t
    assert res[0][3][:1] == b"A"


def test_refusals_leave_the_good_job_alone(native, dev, C):
    data = _data(C + 1)
    text = base64.b64encode(data)
    # cap one too small, each direction
    (l1, e1, _, d1, g1), (l2, e2, _, d2, g2) = _run(native, dev, True,
                                                   [(data, 0, 0, len(text) - 1), (data, 1, 2, None)])
    assert (l1, e1) == (len(text), 3) and d1 == b"\xee" * (len(text) - 1) and g1
    assert (l2, e2) == (len(text), 0) and d2 == text and g2
    need = len(text) // 4 * 3  # before the padding is known
    (l1, e1, _, d1, g1), (l2, e2, _, d2, g2) = _run(native, dev, False,
                                                   [(text, 0, 0, need - 1), (text, 1, 2, None)])
    assert (l1, e1) == (need, 3) and d1 == b"\xee" * (need - 1) and g1
    assert (l2, e2) == (len(data), 0) and d2[:l2] == data and g2
    # null src, overlapping ranges, next to a good job
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    both = torch.full((len(data) + len(text),), 0xEE, dtype=torch.uint8, device=dev)
    both[:len(data)] = src
    out = torch.full((len(text),), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    p = both.data_ptr()
    res = native.gpu.device_base64_encode([0, p, p, src.data_ptr()], [len(data)] * 4,
                                          [out.data_ptr(), p + len(data) - 1, p, out.data_ptr()], [len(text)] * 4, 0)
    assert [r[1] for r in res] == [2, 2, 2, 0]
    assert res[3][0] == len(text) and out.cpu().numpy().tobytes() == text
    assert both.cpu().numpy()[len(data):].tobytes() == b"\xee" * len(text)  # nothing was launched for them
    tsrc = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    back = torch.full((need,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    res = native.gpu.device_base64_decode([0, tsrc.data_ptr(), tsrc.data_ptr()], [len(text)] * 3,
                                          [back.data_ptr(), tsrc.data_ptr() + 8, back.data_ptr()], [need] * 3, 0)
    assert [r[1] for r in res] == [2, 2, 0]
    assert res[2][0] == len(data) and back.cpu().numpy()[:len(data)].tobytes() == data
    assert tsrc.cpu().numpy().tobytes() == text
    # nothing to do is no launch and no error
    assert native.gpu.device_base64_encode([0], [0], [0], [0], 0) == [(0, 0)]
    assert native.gpu.device_base64_decode([0], [0], [0], [0], 0) == [(0, 0, 0)]


def test_bytes_field_of_a_scanned_payload(native, dev):
    from brpc_amd.ops.pb import pb_build_message
    first = torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev)
    field = torch.from_numpy(np.frombuffer(_data(1000)[::-1], dtype=np.uint8).copy()).to(dev)
    msg, _ = pb_build_message([(1, first, "bytes"), (2, field, "bytes")])
    torch.cuda.synchronize(dev)
    nf, table = native.gpu.device_pb_scan(msg.data_ptr(), msg.numel(), 0)
    off, ln = native.gpu.device_payload_field(nf, table, 2)
    assert ln == 1000 and (msg.data_ptr() + off) % 16 != 0  # after tag, length, 3 bytes, tag, length
    want = base64.b64encode(field.cpu().numpy().tobytes())
    # the text right behind a "key":" prefix, the bytes decoded back next to it
    prefix = b'"raw":"'
    cap = len(want) // 4 * 3  # what the text could hold before its padding is known
    buf = torch.full((len(prefix) + len(want) + cap,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    text_at = buf.data_ptr() + len(prefix)
    (length, err), = native.gpu.device_base64_encode([msg.data_ptr() + off], [ln], [text_at], [len(want)], 0)
    assert (length, err) == (len(want), 0)
    (length, err, _), = native.gpu.device_base64_decode([text_at], [len(want)], [text_at + len(want)], [cap], 0)
    assert (length, err) == (1000, 0)
    host = buf.cpu().numpy().tobytes()
    assert host[len(prefix):len(prefix) + len(want)] == want
    assert host[len(prefix) + len(want):][:1000] == field.cpu().numpy().tobytes()
    assert host[len(prefix) + len(want) + 1000:] == b"\xee" * (cap - 1000)
    assert host[:len(prefix)] == b"\xee" * len(prefix)


def test_ops_round_trip_of_a_float_tensor(dev):
    from brpc_amd.ops.json import base64_decode, base64_encode
    t = torch.randn(1025, device=dev, dtype=torch.float32) * 1000
    text = base64_encode(t)
    assert text.dtype == torch.uint8 and text.device == t.device
    assert text.cpu().numpy().tobytes() == base64.b64encode(t.cpu().numpy().tobytes())
    back = base64_decode(text)
    assert back.dtype == torch.uint8
    assert torch.equal(back.view(torch.int32), t.view(torch.int32))  # bit for bit
    assert torch.equal(back.view(torch.float32), t)
    assert base64_encode(t[:0]).numel() == 0 and base64_decode(text[:0]).numel() == 0
