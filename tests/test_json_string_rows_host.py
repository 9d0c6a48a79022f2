"""json::UnescapeStringRows (native.json_unescape_rows), the host twin of the
device's rows unescaper, against this directory's pure-python parser
(json_string_rows_ref.parse) and, for accepted bracketed texts that decode as
UTF-8, against Python's json module; and as the inverse of
json::EscapeStringRows. (The twin also runs under AddressSanitizer and UBSan in
a program of its own,
brpc_amd/csrc/tests/standalone/json_string_rows_sanitize_main.cc.)"""
import json
import random
import struct

import pytest

import json_string_rows_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def native():
    from brpc_amd import native
    return native


def _same(native, text):
    """The twin's verdict on text against the reference's; returns True when accepted."""
    want = R.parse(text)
    got = native.json_unescape_rows(text)
    if isinstance(want, int):
        assert got == (None, want), text
        return False
    rows, depth = want
    assert got == (b"".join(rows), R.row_ends(rows), depth), text
    return True


ACCEPTED = [
    (b"", [], 0), (b" \t\n\r", [], 0), (b"[]", [], 1), (b" [ \n] ", [], 1),
    (b'""', [b""], 0), (b'[""]', [b""], 1), (b'"a"', [b"a"], 0), (b' "a" , "b"\t', [b"a", b"b"], 0),
    (b'["a","b"]', [b"a", b"b"], 1), (b'[ "a" ,\n"" , "c,[]\\"" ] ', [b"a", b"", b'c,[]"'], 1),
    (b'"","",""', [b"", b"", b""], 0), (b'"\\ud83d\\ude00\\u00e9"', ["\U0001f600é".encode()], 0),
    (b'["\x01\xff raw"]', [b"\x01\xff raw"], 1), (b'"\\\\","\\\\\\""', [b"\\", b'\\"'], 0),
]


@pytest.mark.parametrize("text,rows,depth", ACCEPTED)
def test_accepted_shapes(native, text, rows, depth):
    assert R.parse(text) == (rows, depth)
    assert native.json_unescape_rows(text) == (b"".join(rows), R.row_ends(rows), depth)


REFUSED = [
    (b'"abc', 4), (b'"', 1), (b'"a",', 4), (b'"a", ', 5), (b"[", 1), (b'["a"', 4), (b'["a" ', 5), (b'["a",', 5),
    (b'[["a"]]', 1), (b"[1]", 1), (b"null", 0), (b'{"a":"b"}', 0), (b'["a" "b"]', 5), (b'"a" "b"', 4), (b'"a"]', 3),
    (b"]", 0), (b",", 0), (b'[,"a"]', 1), (b'["a",]', 5), (b'["a",,"b"]', 5), (b'[]"a"', 2), (b"[] ]", 3), (b"[][", 2),
    (b'"a"x', 3), (b'x"a"', 0), (b'["a"],', 5), (b'"a\\q"', 2), (b'["\\u12"]', 2), (b'"\\ud83d"', 1),
    (b'"\\ude00"', 1), (b'"\\ud83d","\\ude00"', 1), (b'"abc\\', 4), (b'\\"a"', 0), (b'"a"\\', 3),
]


@pytest.mark.parametrize("text,first_bad", REFUSED)
def test_refusals_and_their_offsets(native, text, first_bad):
    assert R.parse(text) == first_bad
    assert native.json_unescape_rows(text) == (None, first_bad)


def test_reader_route(native):
    assert native.json_reader_string_array(b'["a","b"]') == [b"a", b"b"]
    assert native.json_reader_string_array(b' "a" , "b" ') == [b"a", b"b"]
    assert native.json_reader_string_array(b"") == []
    assert native.json_reader_string_array(b'["a",1]') is None
    assert native.json_reader_string_array(b'["a" "b"]') is None
    lone = native.json_reader_string_array(b'["\\ud83d"]')  # the twin declines it, the reader does not
    assert native.json_unescape_rows(b'["\\ud83d"]') == (None, 2) and lone is not None and len(lone) == 1


def test_seeded_differential_set_is_not_vacuous(native):
    texts = R.differential_texts(2024, 6000)
    accepted = sum(1 for t in texts if not isinstance(R.parse(t), int))
    assert 4 * accepted >= len(texts) and 4 * (len(texts) - accepted) >= len(texts), accepted
    assert sum(1 for t in texts if _same(native, t)) == accepted


@pytest.mark.parametrize("seed", range(3))
def test_differential_with_long_rows(native, seed):
    for t in R.differential_texts(seed, 300, long_row=9000):
        _same(native, t)


def test_against_python_json(native):
    checked = 0
    for t in R.differential_texts(7, 4000):
        got = native.json_unescape_rows(t)
        if got[0] is None or got[2] != 1:
            continue
        try:
            want = json.loads(t.decode("utf-8"), strict=False)
        except UnicodeDecodeError:
            continue
        rows = [r.encode("utf-8") for r in want]
        assert got == (b"".join(rows), R.row_ends(rows), 1), t
        checked += 1
    assert checked > 500


@pytest.mark.parametrize("seed", range(2))
def test_inverse_of_escape_rows(native, seed):
    rng = random.Random(300 + seed)
    for _ in range(1500):
        rows = [bytes(rng.randrange(256) for _ in range(rng.choice((0, 0, 1, 5, 40)))) for _ in range(rng.randrange(8))]
        ends = R.row_ends(rows)
        text = native.json_escape(b"".join(rows), row_ends=struct.pack("<%dI" % len(ends), *ends))
        assert native.json_unescape_rows(text) == (b"".join(rows), ends, 0)
        assert native.json_unescape_rows(b"[" + text + b"]") == (b"".join(rows), ends, 1)
