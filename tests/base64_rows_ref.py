"""A pure-python reference for the text of a JSON array of base64 strings
(brpc_amd/csrc/base/base64_rows.h): a sequential parser that returns the rows
and the depth or the offset at which it sticks, and a printer over the stdlib
``base64``. No line of it is shared with the native code."""
import base64

WS = b" \t\n\r"
SYMBOLS = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")


def _body(text, p):
    """The string whose opening quote is text[p - 1]: (row bytes, offset behind
    the closing quote), or the offset at which the parser sticks (an int)."""
    n = len(text)
    start = p
    while p < n and text[p] in SYMBOLS:
        p += 1
    m = p - start
    pads = 0
    while p < n and text[p] == 0x3D:  # '='
        if (m + pads) % 4 < 2 or pads == 2:
            return p
        pads += 1
        p += 1
    if p >= n:
        return n
    if text[p] != 0x22:  # anything but the closing quote
        return p
    if m % 4 == 1 or (pads and (m + pads) % 4 != 0):
        return p
    symbols = text[start:start + m]
    row = base64.b64decode(symbols + b"A" * (-m % 4)) if m else b""
    return row[:m // 4 * 3 + (m % 4) * 3 // 4], p + 1


def parse(text):
    """(rows, depth) or the offset at which a left-to-right parser sticks."""
    text = bytes(text)
    n = len(text)
    p = 0
    rows, depth = [], 0

    def skip(p):
        while p < n and text[p] in WS:
            p += 1
        return p

    p = skip(p)
    if p == n:
        return rows, 0
    if text[p] == 0x5B:  # '['
        depth = 1
        p = skip(p + 1)
        if p == n:
            return n
        if text[p] == 0x5D:
            p = skip(p + 1)
            return (rows, 1) if p == n else p
    while True:
        if p == n:
            return n
        if text[p] != 0x22:
            return p
        got = _body(text, p + 1)
        if isinstance(got, int):
            return got
        row, p = got
        rows.append(row)
        p = skip(p)
        if p == n:
            return (rows, 0) if depth == 0 else n
        if text[p] == 0x2C:  # ','
            p = skip(p + 1)
            continue
        if text[p] == 0x5D and depth == 1:
            p = skip(p + 1)
            return (rows, 1) if p == n else p
        return p


def row_ends(rows):
    ends, total = [], 0
    for r in rows:
        total += len(r)
        ends.append(total)
    return ends


def print_rows(rows, brackets=True):
    body = b",".join(b'"' + base64.b64encode(bytes(r)) + b'"' for r in rows)
    return b"[" + body + b"]" if brackets else body


def split(data, ends):
    out, at = [], 0
    for e in ends:
        out.append(bytes(data[at:e]))
        at = e
    return out
