"""The host twins of the device string entries (json::EscapeStringBody /
EscapeStringRows / UnescapeStringBody / Utf8FirstBad over base/json_string.h,
the code the device kernels run) against Python's json module and its UTF-8
decoder, oracles that share nothing with them. (The word-wise loops also run
under AddressSanitizer and UBSan in a program of their own,
brpc_amd/csrc/tests/standalone/json_string_sanitize_main.cc.)"""
import json
import random
import struct

import pytest

from brpc_amd import native

# every code point of U+0000..U+007F, and characters of 2, 3 and 4 bytes
ALPHABET = [chr(c) for c in range(0x80)] + ["é", "߿", "ࠀ", "€", "￿", "\U00010000",
                                            "\U0001f600", "\U0010ffff"]
POOL = bytes.fromhex("00417f808f909fa0bfc0c1c2dfe0e1eceeedeff0f1f3f4f5ff")


def _dumps(s):
    return json.dumps(s, ensure_ascii=False).encode()


def test_escape_every_ascii_code_point_alone():
    for ch in ALPHABET:
        assert native.json_escape(ch.encode()) == _dumps(ch), hex(ord(ch))
    assert native.json_escape(b"") == b'""'
    assert native.json_escape(b"", quote=False) == b""
    assert native.json_escape(b"/\x7f") == b'"/\x7f"'  # neither is escaped


@pytest.mark.parametrize("seed", range(4))
def test_escape_random_strings(seed):
    rng = random.Random(seed)
    for _ in range(2000):
        s = "".join(rng.choice(ALPHABET) for _ in range(rng.randrange(40)))
        want = _dumps(s)
        assert native.json_escape(s.encode()) == want
        assert native.json_escape(s.encode(), quote=False) == want[1:-1]


def test_escape_long_plain_runs_around_a_word():
    for n in range(40):
        for at in range(n):
            s = "a" * at + '"' + "b" * (n - at - 1)
            assert native.json_escape(s.encode()) == _dumps(s)


def _ends(rows):
    total, out = 0, []
    for r in rows:
        total += len(r)
        out.append(total)
    return struct.pack("<%dI" % len(out), *out)


@pytest.mark.parametrize("seed", range(3))
def test_escape_rows(seed):
    rng = random.Random(100 + seed)
    for _ in range(500):
        rows = ["".join(rng.choice(ALPHABET) for _ in range(rng.choice([0, 0, 1, 3, 9, 30])))
                for _ in range(rng.randrange(1, 9))]
        enc = [r.encode() for r in rows]
        want = ",".join(json.dumps(r, ensure_ascii=False) for r in rows).encode()
        assert native.json_escape(b"".join(enc), row_ends=_ends(enc)) == want


def test_escape_rows_refuses_bad_ends():
    with pytest.raises(ValueError):
        native.json_escape(b"abcd", row_ends=struct.pack("<3I", 3, 2, 4))
    with pytest.raises(ValueError):
        native.json_escape(b"abcd", row_ends=struct.pack("<2I", 1, 3))


ESCAPES = ['\\"', "\\\\", "\\/", "\\b", "\\f", "\\n", "\\r", "\\t", "\\u0041", "\\u00e9", "\\u00E9", "\\u20ac",
           "\\u0000", "\\uffff", "\\ud83d\\ude00", "\\uD83D\\uDE00", "\\udbff\\udfff", "\\ud800\\udc00"]
RAW = ["a", "z", " ", "/", "\x01", "\n", "\t", "é", "€", "\U0001f600", "u", "0", "f", "uD83D"]


@pytest.mark.parametrize("seed", range(4))
def test_unescape_well_formed_bodies(seed):
    rng = random.Random(200 + seed)
    for _ in range(2000):
        body = "".join(rng.choice(ESCAPES if rng.random() < 0.5 else RAW) for _ in range(rng.randrange(24)))
        want = json.loads('"' + body + '"', strict=False)
        got, first_bad = native.json_unescape(body.encode())
        assert got is not None, (body, first_bad)
        assert got == want.encode("utf-8", "surrogatepass"), body
        assert native.json_reader_string(body.encode()) == got  # and the reader agrees


def test_unescape_inverts_escape_on_any_bytes():
    rng = random.Random(5)
    for _ in range(2000):
        data = bytes(rng.choice(b'"\\\n\r\t\b\f\x00\x1fa\x7f\x80\xff/u') for _ in range(rng.randrange(50)))
        assert native.json_unescape(native.json_escape(data, quote=False)) == (data, 0)


@pytest.mark.parametrize("body,first_bad", [
    (b'ab"cd', 2), (b"abcdefgh\\", 8), (b"ab\\x41", 2), (b"ab\\u12", 2), (b"\\u12g4 and more", 0),
    (b"\\ud83d", 0), (b"x\\ud83dabcdef", 1), (b"\\ud83d\\u0041", 0), (b"\\ude00", 0), (b"0123456789\\udc00", 10),
    (b"\\ud83d\\ude00\\ude00", 12), (b"\\\\ud83d\\ude00", 7),
])
def test_unescape_leaves_the_loose_forms_to_the_reader(body, first_bad):
    assert native.json_unescape(body) == (None, first_bad)


def test_utf8_first_bad_classes():
    for bad in [b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",
                b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff", b"\x80",
                b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xe2\x82\x41", b"\xf0\x9f\x98\x41"]:
        for lead in [b"", b"a", b"abcdefgh", "€".encode() * 3]:
            with pytest.raises(UnicodeDecodeError) as e:
                (lead + bad + b"tail").decode()
            assert native.utf8_first_bad(lead + bad + b"tail") == e.value.start, (lead, bad)
    good = "aé€\U0001f600\U0010ffff퟿".encode()
    assert native.utf8_first_bad(good) == len(good)
    assert native.utf8_first_bad(b"") == 0


@pytest.mark.parametrize("seed", range(4))
def test_utf8_first_bad_random_strings_over_the_boundary_bytes(seed):
    rng = random.Random(300 + seed)
    for _ in range(20000):
        data = bytes(rng.choice(POOL) for _ in range(rng.randrange(1, 14)))
        try:
            data.decode()
            want = len(data)
        except UnicodeDecodeError as e:
            want = e.start
        assert native.utf8_first_bad(data) == want, data.hex()
