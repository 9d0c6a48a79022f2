"""json::EncodeBase64Rows / DecodeBase64Rows (native.base64_encode_rows,
native.base64_decode_rows), the host twins of the device's base64 rows entries,
against the pure-python reference of this directory: every short text, random
valid and mutated long texts, random row tables, the round trip and the link to
the row serializer. (The C++ suite Base64Rows covers the local rule and the
bounds, and runs under ASan and UBSan as a program of its own: see
brpc_amd/csrc/tests/base64_rows_unittest.cc.)"""
import itertools
import random

import numpy as np

import base64_rows_ref as R
from brpc_amd import native


def _ends_bytes(ends):
    return np.asarray(ends, dtype=np.uint32).tobytes()


def _same(text):
    want = R.parse(text)
    got = native.base64_decode_rows(text)
    if isinstance(want, int):
        assert got == (None, want), (text, got, want)
    else:
        rows, depth = want
        assert got == (b"".join(rows), R.row_ends(rows), depth), (text, got, want)


def test_twin_against_reference_on_every_short_text():
    alphabet = b'Az+="\\,[] '
    for n in range(0, 7):
        for t in itertools.product(alphabet, repeat=n):
            _same(bytes(t))


def _random_rows(rng, max_rows=12, max_len=40):
    return [bytes(rng.getrandbits(8) for _ in range(0 if rng.random() < 0.25 else rng.randrange(max_len)))
            for _ in range(rng.randrange(max_rows))]


def _random_text(rng):
    rows = _random_rows(rng)
    ws = lambda: rng.choice([b"", b"", b" ", b"\n", b" \t\r\n"])  # noqa: E731
    parts = []
    for r in rows:
        body = R.base64.b64encode(r)
        if rng.random() < 0.3:
            body = body.rstrip(b"=")  # unpadded is canonical too
        parts.append(ws() + b'"' + body + b'"' + ws())
    text = b",".join(parts)
    if rng.random() < 0.5:
        text = ws() + b"[" + (text if rows else ws()) + b"]" + ws()
    return text


def test_twin_against_reference_on_long_texts():
    rng = random.Random(64)
    junk = b'Az09+/=-_"\\,[] \n{}1'
    for it in range(20000):
        text = bytearray(_random_text(rng))
        if it % 2 and text:
            for _ in range(rng.randrange(1, 3)):
                at = rng.randrange(len(text))
                how = rng.randrange(3)
                if how == 0:
                    text[at] = rng.choice(junk)
                elif how == 1:
                    del text[at]
                else:
                    text.insert(at, rng.choice(junk))
        _same(bytes(text))


def test_encode_against_reference():
    rng = random.Random(65)
    for _ in range(3000):
        rows = _random_rows(rng)
        data = b"".join(rows)
        for brackets in (False, True):
            got = native.base64_encode_rows(data, _ends_bytes(R.row_ends(rows)), brackets)
            assert got == R.print_rows(rows, brackets), rows
    assert native.base64_encode_rows(b"", b"", True) == b"[]"
    assert native.base64_encode_rows(b"", b"", False) == b""
    assert native.base64_encode_rows(b"", _ends_bytes([0, 0, 0]), False) == b'"","",""'


def test_round_trip():
    rng = random.Random(66)
    for _ in range(3000):
        rows = _random_rows(rng)
        data, ends = b"".join(rows), R.row_ends(rows)
        brackets = rng.random() < 0.5
        text = native.base64_encode_rows(data, _ends_bytes(ends), brackets)
        assert native.base64_decode_rows(text) == (data, ends, 1 if brackets else 0)


def test_decoded_rows_feed_the_row_serializer():
    rng = random.Random(67)
    for _ in range(300):
        rows = _random_rows(rng) or [b""]  # the serializer takes no empty batch
        data, ends = b"".join(rows), R.row_ends(rows)
        got_bytes, got_ends, _ = native.base64_decode_rows(R.print_rows(rows))
        want = native.pb_serialize_rows(4, 0, 7, data, ends)
        assert want[0] == 0
        assert native.pb_serialize_rows(4, 0, 7, got_bytes, got_ends) == want
        # and the wire is the field once per row
        wire = b"".join(b"\x22" + bytes([len(r)]) + r for r in rows)
        assert want[2] == wire
