"""snappy_stream.py (the walker, the byte-wise decoder and the input builders
of the device compressor's tests) against the host codec: the decoder agrees
with native.snappy_uncompress on the host encoder's stream of every built
input and on hand-written streams of every element form, the walker refuses
malformed streams, and the builders build what they say."""
import pytest

import snappy_stream as S


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _pinned(native, data):
    """walk and decode against the host codec on the host encoder's stream."""
    c = native.snappy_compress(data)
    assert native.snappy_uncompress(c) == data
    ulen, elements = S.walk(c)
    assert ulen == len(data) == sum(el.length for el in elements)
    assert S.decode(c) == data
    return elements


@pytest.mark.parametrize("n", S.BLOCKS)
def test_built_inputs_through_the_host_codec(native, n):
    seg = S.seg_len(n)
    assert seg == (n + 63) // 64
    D = seg + 37
    for L in S.sweep_lengths(n):
        data = S.planted_copy(n, 100 + L, L, D)
        assert data == S.planted_copy(n, 100 + L, L, D) and len(data) == n
        q, t = S.plant_site(n, L, D)
        assert t - q == D and data[q:q + L] == data[t:t + L] and data[q + L] != data[t + L]
        assert t // seg == (t + L - 1) // seg and t - S.segment(n, t // seg)[0] < 32
        _pinned(native, data)
    for L, D in S.distance_cases(n):
        data = S.planted_copy(n, 1000 * L + D, L, D)
        q, t = S.plant_site(n, L, D)
        assert t - q == D and data[q:q + L] == data[t:t + L] and (t + L == n or data[q + L] != data[t + L])
        assert t // seg == (t + L - 1) // seg
        _pinned(native, data)
    for p in (1, 2, 3, 5, 7):
        data = S.periodic(n, 7 + p, p)
        assert len(data) == n and data[p:] == data[:-p] and len(set(data[:p])) == p
        _pinned(native, data)
    tile = S.tiled(n, 5)
    assert len(tile) == n and tile[seg:] == tile[:-seg]
    _pinned(native, tile)
    many = S.many_literals(n, 1, 5)
    lo, hi = S.segment(n, 5)
    for i in range(S.MANY):
        assert many[lo + 5 * i + 1:lo + 5 * i + 5] == many[4 * i:4 * i + 4]
        assert many[lo + 5 * i + 5] != many[4 * i + 4]
    _pinned(native, many)
    _pinned(native, bytes(n))
    for k, data in enumerate((S.text(n, 11), S.text(n - 3, 13), S.incompressible(n, n))):
        assert len(data) == n - 3 * (k == 1)
        _pinned(native, data)


def test_short_and_mixed_inputs_through_the_host_codec(native):
    whole = S.incompressible(1024, 77)
    for n in range(1, 1025):
        _pinned(native, whole[:n])
        _pinned(native, bytes([n & 0xFF]) * n)
    for big in (65536, 16384, 8192):
        for k, n in enumerate((1, 5, 64, 4096, big)):
            _pinned(native, S.text(n, n) if k % 2 else S.incompressible(n, n))
        _pinned(native, S.text(big, 3))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1024, 3840, 3904, 16385])
def test_incompressible_repeats_no_four_bytes(native, n):
    data = S.incompressible(n, n)
    assert len(data) == n and data == S.incompressible(n, n)
    grams = [data[i:i + 4] for i in range(n - 3)]
    assert len(set(grams)) == len(grams)
    elements = _pinned(native, data)
    assert [el.kind for el in elements] == [S.LITERAL]
    assert elements[0].tag_width == 1 + (n > 60) + (n > 256)


def _literal(tag_bytes, n):
    body = bytes((7 * i + 1) & 0xFF for i in range(n))
    return tag_bytes + body, body


HAND = {
    # name: (elements after the preamble, output, expected (kind, length, offset, tag_width) per element)
    "literal_1": (_literal(b"\x00", 1), [(S.LITERAL, 1, 0, 1)]),
    "literal_60": (_literal(bytes([59 << 2]), 60), [(S.LITERAL, 60, 0, 1)]),
    "literal_61": (_literal(bytes([60 << 2, 60]), 61), [(S.LITERAL, 61, 0, 2)]),
    "literal_256": (_literal(bytes([60 << 2, 255]), 256), [(S.LITERAL, 256, 0, 2)]),
    "literal_257": (_literal(bytes([61 << 2, 0, 1]), 257), [(S.LITERAL, 257, 0, 3)]),
    "literal_3_length_bytes": (_literal(bytes([62 << 2, 0x2B, 0x02, 0x00]), 0x22C), [(S.LITERAL, 0x22C, 0, 4)]),
    "literal_4_length_bytes": (_literal(bytes([63 << 2, 0x04, 0x00, 0x01, 0x00]), 0x10005), [(S.LITERAL, 0x10005, 0, 5)]),
    "copy1": ((b"\x0cabcd" + bytes([(0 << 5) | (0 << 2) | 1, 4]), b"abcdabcd"),
              [(S.LITERAL, 4, 0, 1), (S.COPY1, 4, 4, 2)]),
    "copy1_far_long": ((_literal(bytes([61 << 2, 0xFF, 0x07]), 2048)[0] + bytes([(7 << 5) | (7 << 2) | 1, 0xFF]),
                        _literal(b"", 2048)[1] + _literal(b"", 2048)[1][1:12]),
                       [(S.LITERAL, 2048, 0, 3), (S.COPY1, 11, 2047, 2)]),
    "copy2": ((b"\x0cabcd" + bytes([(63 << 2) | 2, 4, 0]), b"abcd" * 17),
              [(S.LITERAL, 4, 0, 1), (S.COPY2, 64, 4, 3)]),
    "copy4": ((b"\x0cabcd" + bytes([(5 << 2) | 3, 3, 0, 0, 0]), b"abcdbcdbcd"),
              [(S.LITERAL, 4, 0, 1), (S.COPY4, 6, 3, 5)]),
    "copy_of_one_byte_run": ((b"\x00z" + bytes([(9 << 2) | 2, 1, 0]), b"z" * 11),
                             [(S.LITERAL, 1, 0, 1), (S.COPY2, 10, 1, 3)]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_streams(native, name):
    (body, want), forms = HAND[name]
    stream = S.varint(len(want)) + body
    assert native.snappy_uncompress(stream) == want
    ulen, elements = S.walk(stream)
    assert ulen == len(want)
    assert [(el.kind, el.length, el.offset, el.tag_width) for el in elements] == forms
    assert [el.pos for el in elements] == [sum(f[1] for f in forms[:i]) for i in range(len(forms))]
    assert S.decode(stream) == want


@pytest.mark.parametrize("stream", [
    b"",                                  # no preamble
    b"\x80\x80\x80\x80\x80\x01",          # preamble longer than 5 bytes
    b"\x05\x0cabcd",                      # produces 4 of 5
    b"\x03\x0cabcd",                      # produces 4 of 3
    b"\x04\x0cabc",                       # literal runs past the stream
    b"\x40\xf0\x3f",                      # literal length byte, no bytes
    b"\x08\x0cabcd\x01",                  # copy without its offset byte
    b"\x08\x0cabcd\x01\x00",              # offset 0
    b"\x08\x0cabcd\x01\x05",              # offset before the output
    b"\x04\x01\x01",                      # a copy first
    b"\x08\x0cabcd\x0e\x04",              # copy-2 without its second offset byte
], ids=lambda s: s.hex() or "empty")
def test_walk_refuses_malformed_streams(native, stream):
    with pytest.raises(ValueError):
        S.walk(stream)
    with pytest.raises(ValueError):
        S.decode(stream)
    with pytest.raises(Exception):
        native.snappy_uncompress(stream)
