"""The host base64 coder (base/util.cc over base/base64.h, the code the device
kernels run) against Python's stdlib, an oracle that shares nothing with it.
(The word-wise loops also run under AddressSanitizer and UBSan in a program of
their own, brpc_amd/csrc/tests/standalone/base64_sanitize_main.cc.)"""
import base64
import random

import pytest

from brpc_amd import native


@pytest.mark.parametrize("n", range(101))
def test_encode_every_short_length(n):
    data = bytes((i * 89 + n) & 255 for i in range(n))
    assert native.base64_encode(data) == base64.b64encode(data)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16])
def test_encode_all_byte_values(k):
    data = bytes(range(256)) * k
    text = native.base64_encode(data)
    assert text == base64.b64encode(data)
    assert set(text) >= set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")


def test_encode_random_data_up_to_1_mib():
    rng = random.Random(5)
    for n in [rng.randrange(1 << 20) for _ in range(12)] + [(1 << 20) - 1, 1 << 20]:
        data = rng.randbytes(n)
        assert native.base64_encode(data) == base64.b64encode(data), n


def test_decode_inverts_encode_padded_and_unpadded():
    rng = random.Random(6)
    for n in list(range(70)) + [4095, 4096, 4097, 100000]:
        data = rng.randbytes(n)
        text = base64.b64encode(data)
        assert native.base64_decode(text) == data
        assert base64.b64decode(text, validate=True) == data
        assert native.base64_decode(text.rstrip(b"=")) == data  # unpadded is accepted


def test_decode_named_cases():
    assert native.base64_decode(b"QR==") == b"A"  # trailing bits that are not zero are dropped
    assert native.base64_decode(b"QQ") == b"A"
    assert native.base64_decode(b"Q") is None  # a lone symbol carries no byte
    assert native.base64_decode(b"=") is None
    assert native.base64_decode(b"====") is None  # more than two pads
    assert native.base64_decode(b"QQ=Q") is None  # data after a pad
    assert native.base64_decode(b"QUJD\n") == b"ABC"
    assert native.base64_decode(b"QU JD") == b"ABC"
    assert native.base64_decode(b"QUJD\r\nREVG") == b"ABCDEF"
    assert native.base64_decode(b"QUJD!EVG") is None
    assert native.base64_decode(b"") == b""


def test_decode_skips_line_breaks_anywhere():
    data = bytes(range(256)) * 3
    text = base64.encodebytes(data)  # a '\n' every 76 symbols
    assert b"\n" in text
    assert native.base64_decode(text) == data
