"""A pure-python sequential parser of the text of an array of JSON strings, the
grammar of brpc_amd/csrc/base/json_string_rows.h, sharing no code with it:
the oracle of json::UnescapeStringRows and of the device kernels, and the
generator of the seeded differential texts both test files run.

  depth 0   ws | ws S ws (',' ws S ws)*
  depth 1   ws '[' ws ']' ws | ws '[' ws S ws (',' ws S ws)* ']' ws

parse(text) -> (rows, depth) with rows a list of bytes, or the offset at which
a parser reading from the left cannot go on (a bad escape: its backslash; a
text that ends too soon: len(text))."""
import random

WS = b" \t\n\r"
HEX = b"0123456789abcdefABCDEF"
SIMPLE = {ord('"'): b'"', ord("\\"): b"\\", ord("/"): b"/", ord("b"): b"\b", ord("f"): b"\f", ord("n"): b"\n",
          ord("r"): b"\r", ord("t"): b"\t"}


def _hex4(text, p):
    """The code unit of the four hex digits at p, None when they are not all there."""
    h = text[p:p + 4]
    if len(h) < 4 or any(c not in HEX for c in h):
        return None
    return int(h.decode(), 16)


def _escape(text, p):
    """The escape whose backslash is text[p] -> (bytes, span), None when bad."""
    n = len(text)
    if p + 1 >= n:
        return None
    letter = text[p + 1]
    if letter in SIMPLE:
        return SIMPLE[letter], 2
    if letter != ord("u"):
        return None
    cu = _hex4(text, p + 2)
    if cu is None:
        return None
    if cu < 0xD800 or cu >= 0xE000:
        return chr(cu).encode("utf-8"), 6
    if cu >= 0xDC00:  # a low surrogate that no high one introduced
        return None
    if text[p + 6:p + 8] != b"\\u":
        return None
    lo = _hex4(text, p + 8)
    if lo is None or lo < 0xDC00 or lo >= 0xE000:
        return None
    return chr(0x10000 + ((cu - 0xD800) << 10) + (lo - 0xDC00)).encode("utf-8"), 12


def parse(text):
    text = bytes(text)
    n = len(text)
    p = 0
    rows = []

    def skip(p):
        while p < n and text[p] in WS:
            p += 1
        return p

    def string(p):
        """p at the opening quote -> (bytes, offset after the closing quote) or the bad offset."""
        p += 1
        out = bytearray()
        while True:
            if p >= n:
                return n
            c = text[p]
            if c == ord('"'):
                return bytes(out), p + 1
            if c == ord("\\"):
                got = _escape(text, p)
                if got is None:
                    return p
                out += got[0]
                p += got[1]
            else:
                out.append(c)
                p += 1

    p = skip(p)
    depth = 0
    if p < n and text[p] == ord("["):
        depth = 1
        p = skip(p + 1)
        if p < n and text[p] == ord("]"):
            p = skip(p + 1)
            return ([], 1) if p == n else p
    elif p == n:
        return [], 0
    while True:
        if p >= n:
            return n
        if text[p] != ord('"'):
            return p
        got = string(p)
        if isinstance(got, int):
            return got
        rows.append(got[0])
        p = skip(got[1])
        if p < n and text[p] == ord(","):
            p = skip(p + 1)
            continue
        break
    if depth == 1:
        if p >= n:
            return n
        if text[p] != ord("]"):
            return p
        p = skip(p + 1)
    return (rows, depth) if p == n else p


def row_ends(rows):
    total, out = 0, []
    for r in rows:
        total += len(r)
        out.append(total)
    return out


# ---- the seeded differential texts

MUTATION_BYTES = b'"\\,[] \n\tud83Dc0x{'
_PIECES = [b"a", b"xyz", b" ", b",", b"[", b"]", b"\\\\", b'\\"', b"\\n", b"\\t", b"\\/", b"\\u0041", b"\\u00e9",
           b"\\u20AC", b"\\ud83d\\ude00", b"\\uD83D\\uDE00", b"\x01", b"\x7f", b"\xc3\xa9", b"\xff", b"{", b"0"]


def _ws(rng):
    return bytes(rng.choice(WS) for _ in range(rng.choice((0, 0, 0, 1, 2))))


def valid_text(rng, max_rows=6, max_pieces=6, long_row=0):
    """A text of the grammar; long_row > 0 makes one row about that many bytes."""
    depth = rng.randrange(2)
    nrows = rng.randrange(max_rows + 1)
    long_at = rng.randrange(nrows) if nrows and long_row else -1
    strings = []
    for r in range(nrows):
        pieces = [rng.choice(_PIECES) for _ in range(rng.randrange(max_pieces + 1))]
        if r == long_at:
            while sum(len(x) for x in pieces) < long_row:
                pieces.append(rng.choice(_PIECES) * rng.randrange(1, 40))
        strings.append(b'"' + b"".join(pieces) + b'"')
    body = (_ws(rng) + b"," + _ws(rng)).join(strings) if strings else b""
    if depth:
        return _ws(rng) + b"[" + _ws(rng) + body + _ws(rng) + b"]" + _ws(rng)
    return _ws(rng) + body + _ws(rng)


def mutate(rng, text):
    """At most one mutation: none, a byte substituted, inserted or deleted, or a truncation."""
    kind = rng.randrange(8)
    if kind < 3 or not text:  # as it is
        return text
    at = rng.randrange(len(text))
    b = bytes([rng.choice(MUTATION_BYTES)])
    if kind == 3 or kind == 4:
        return text[:at] + b + text[at + 1:]
    if kind == 5:
        return text[:at] + b + text[at:]
    if kind == 6:
        return text[:at] + text[at + 1:]
    return text[:at]


def differential_texts(seed, count, long_row=0):
    rng = random.Random(seed)
    return [mutate(rng, valid_text(rng, long_row=long_row if k % 4 == 0 else 0)) for k in range(count)]
