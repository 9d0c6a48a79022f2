"""Shared by the snappy compressor tests (not a test module): a walker and a
byte-wise decoder of raw snappy streams written from the format description
alone, and deterministic builders of blocks that steer the device compressor
(gpu/snappy_kernels.hip, compress_wave) into each of its element forms.

What the builders rely on: the compressor cuts a block into 64 lane segments
of seg = max(ceil(n / 64), 8) bytes; a lane never matches past its segment
end; a position's far candidate is the EARLIEST position of the block whose
4 bytes hash (snappy's multiplicative hash, top 11 or 12 bits) to the same
bucket; and a lane steps one byte at a time only within 32 bytes of its last
element. So a builder fills the block with bytes in which no 4 bytes occur
twice (nothing matches by accident), plants a pattern, repeats it a few
bytes into a later segment, and changes filler bytes until the pattern's
hash bucket holds no earlier position."""
import collections
import random
from array import array

LITERAL, COPY1, COPY2, COPY4 = "literal", "copy1", "copy2", "copy4"
Element = collections.namedtuple("Element", "kind length offset tag_width pos at")
# kind, bytes produced, copy distance (0 for a literal), bytes of tag incl.
# length / offset bytes, output position, index of the tag in the stream


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def walk(stream):
    """(ulen, [Element...]) of a raw snappy stream; ValueError if malformed."""
    stream = bytes(stream)
    n, ip, ulen, shift = len(stream), 0, 0, 0
    while True:
        if ip >= n or shift >= 35:
            raise ValueError("bad length preamble")
        c = stream[ip]
        ip += 1
        ulen |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            break
    if ulen >= 1 << 32:
        raise ValueError("length preamble above 32 bits")
    elements, pos = [], 0
    while ip < n:
        at, tag = ip, stream[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            length = (tag >> 2) + 1
            if length > 60:
                nb = length - 60
                if ip + nb > n:
                    raise ValueError("truncated literal length at %d" % at)
                length = int.from_bytes(stream[ip:ip + nb], "little") + 1
                ip += nb
            if length > n - ip:
                raise ValueError("literal at %d runs past the stream" % at)
            el = Element(LITERAL, length, 0, ip - at, pos, at)
            ip += length
        else:
            if kind == 1:
                need, length = 1, ((tag >> 2) & 7) + 4
            else:
                need, length = (2 if kind == 2 else 4), (tag >> 2) + 1
            if ip + need > n:
                raise ValueError("truncated copy at %d" % at)
            offset = int.from_bytes(stream[ip:ip + need], "little")
            if kind == 1:
                offset |= (tag >> 5) << 8
            ip += need
            if offset == 0 or offset > pos:
                raise ValueError("copy at %d reaches before the output (offset %d at %d)" % (at, offset, pos))
            el = Element((COPY1, COPY2, COPY4)[kind - 1], length, offset, 1 + need, pos, at)
        pos += el.length
        if pos > ulen:
            raise ValueError("element at %d runs past the declared length" % at)
        elements.append(el)
    if pos != ulen:
        raise ValueError("stream produces %d bytes, declares %d" % (pos, ulen))
    return ulen, elements


def decode(stream):
    """The uncompressed bytes, one byte at a time from the walked elements."""
    stream = bytes(stream)
    ulen, elements = walk(stream)
    out = bytearray()
    for el in elements:
        if el.kind == LITERAL:
            first = el.at + el.tag_width
            for k in range(el.length):
                out.append(stream[first + k])
        else:
            for _ in range(el.length):
                out.append(out[-el.offset])
    assert len(out) == ulen
    return bytes(out)


def span_elements(elements, lo, hi):
    """The elements whose output lies inside [lo, hi); ValueError unless they
    tile it exactly (an element straddles an end)."""
    inside = [el for el in elements if el.pos < hi and el.pos + el.length > lo]
    if not inside or inside[0].pos != lo or inside[-1].pos + inside[-1].length != hi:
        raise ValueError("no element boundary at %d or %d" % (lo, hi))
    return inside


# ----------------------------------------------------------------- builders

# block lengths per compress kernel: candidate array in LDS (segments of 64
# and 128 bytes); output slots in LDS; slots in global scratch (segments of
# 257 bytes with a short last lane, and of 1024)
BLOCKS = [4096, 8192, 8193, 12288, 16384, 16385, 65536]
SWEEP = [4, 5, 11, 12, 13, 59, 60, 61, 63, 64, 65, 66, 67, 68, 69, 124, 127, 128, 129]
DISTANCES = [1, 2, 3, 7, 2047, 2048, 2049, 32767, 32768, 65531]


def sweep_lengths(n):
    """The copy lengths of SWEEP that fit a segment of an n-byte block."""
    return [L for L in SWEEP if L <= seg_len(n)]


def distance_cases(n):
    """(L, D) of DISTANCES x {4, 11, 12} that fit an n-byte block."""
    return [(L, D) for D in DISTANCES for L in (4, 11, 12) if D + L < n]


def seg_len(n):
    """Bytes per lane segment of an n-byte block."""
    return max((n + 63) // 64, 8)


def segment(n, lane):
    seg = seg_len(n)
    lo = min(n, seg * lane)
    return lo, min(n, lo + seg)


def _grams(buf):
    """The little-endian 4-byte value at every position 0 .. len - 4."""
    b, n = bytes(buf), len(buf)
    out = [0] * max(n - 3, 0)
    for k in range(4):
        cnt = (n - k) // 4
        a = array("I", b[k:k + 4 * cnt])
        assert a.itemsize == 4
        if a and int.from_bytes(b[k:k + 4], "little") != a[0]:
            a.byteswap()
        out[k::4] = a.tolist()
    return out


def _bucket(gram):
    return ((gram * 0x1E35A7BD) & 0xFFFFFFFF) >> 21  # 11 bits; the 12-bit bucket refines it


def _settle(buf, fixed, sources, rnd):
    """Changes bytes of `buf` outside the `fixed` ranges until (a) every 4
    bytes that include a free byte occur once in the block and (b) no position
    before a source q (in `sources`) shares q's hash bucket."""
    n = len(buf)
    free = bytearray(b"\x01" * n)
    for lo, hi in fixed:
        free[lo:hi] = bytes(hi - lo)

    def redraw(x):
        for k in (3, 2, 1, 0):
            if x + k < n and free[x + k]:
                buf[x + k] = rnd.getrandbits(8)
                return
        raise ValueError("4 fixed bytes at %d collide; try another seed" % x)

    for _ in range(64):
        g = _grams(buf)
        dirty = False
        seen = {}
        for x, v in enumerate(g):
            if v in seen:
                y = seen[v]
                if free[x] or free[x + 1] or free[x + 2] or free[x + 3]:
                    redraw(x)
                    dirty = True
                elif free[y] or free[y + 1] or free[y + 2] or free[y + 3]:
                    redraw(y)
                    dirty = True
            else:
                seen[v] = x
        for q in sources:
            want = _bucket(g[q])
            for x in range(q):
                if _bucket(g[x]) == want:
                    redraw(x)
                    dirty = True
        if not dirty:
            return buf
    raise ValueError("block did not settle; try another seed")


def incompressible(n, seed):
    """n bytes in which no 4 bytes occur twice: no lane finds a match."""
    rnd = random.Random(seed)
    return bytes(_settle(bytearray(rnd.randbytes(n)), [], [], rnd))


LEAD = 9  # filler bytes of the target segment in front of a planted copy


def plant_site(n, L, D):
    """(q, t): where planted_copy(n, ., L, D) puts the pattern and its copy.
    t is LEAD bytes (fewer where L leaves no room) into the first segment
    from which t - D >= 0; where only the block's last bytes are that far
    from its start, t = D (see planted_copy)."""
    for lane in range(1, 64):
        lo, hi = segment(n, lane)
        if hi - lo < L:
            continue
        lead = min(LEAD, hi - lo - L)
        if lo + lead >= D:
            return lo + lead - D, lo + lead
    lo, hi = segment(n, (n - 1) // seg_len(n))
    if D < lo or D + L > hi:
        raise ValueError("a copy of %d at distance %d does not fit a %d-byte block" % (L, D, n))
    return 0, D


def planted_copy(n, seed, L, D):
    """An n-byte block whose only repeat is one of exactly L bytes at distance
    D: pattern at q, copy at t = q + D, with (q, t) = plant_site(n, L, D). For
    D < L the pattern is a run of period D, so the copy overlaps its source.
    The byte behind the copy differs from the one behind the pattern. Where t
    lies 32 or more bytes into its segment, the bytes before it (all but
    LEAD) repeat a stretch of segment 1, so the lane reaches t stepping by 1."""
    rnd = random.Random(seed)
    q, t = plant_site(n, L, D)
    buf = bytearray(rnd.randbytes(n))
    fixed, sources = [], [q]
    if D < L:
        unit = bytes(rnd.sample(range(256), D))
        run = (unit * (L // D + 2))[:D + L]
        buf[q:q + D + L] = run
        fixed.append((q, q + D + L))
    else:
        pat = bytes(rnd.sample(range(256), L)) if L <= 256 else rnd.randbytes(L)
        buf[q:q + L] = pat
        buf[t:t + L] = pat
        fixed += [(q, q + L + 1), (t, t + L)]
    if t + L < n:
        buf[t + L] = (buf[q + L] + 1 + rnd.randrange(255)) & 0xFF
        fixed.append((t + L, t + L + 1))
    lo, _ = segment(n, t // seg_len(n))
    if t - lo >= 32:
        h, hq = t - lo - LEAD, seg_len(n) + 70
        assert hq + h <= lo and (q + L <= hq or q >= hq + h)
        buf[lo:lo + h] = buf[hq:hq + h]
        buf[lo + h] = (buf[hq + h] + 1) & 0xFF
        fixed += [(hq, hq + h + 1), (lo, lo + h + 1)]
        sources.append(hq)
    return bytes(_settle(buf, fixed, sources, rnd))


def periodic(n, seed, period):
    """A whole block of one repeated unit of `period` distinct bytes."""
    unit = bytes(random.Random(seed).sample(range(256), period))
    return (unit * (n // period + 1))[:n]


def tiled(n, seed):
    """One incompressible tile of seg_len(n) bytes repeated over the block:
    every lane's segment equals lane 0's."""
    seg = seg_len(n)
    return (incompressible(seg, seed) * 64)[:n]


MANY = 12  # patterns of many_literals


def many_literals(n, seed, lane=5):
    """Twelve 4-byte patterns at the block's start; segment `lane` opens with
    twelve (fresh byte, pattern) pairs: 12 one-byte literals between 12
    copies, then the rest of the segment as a 13th literal."""
    rnd = random.Random(seed)
    buf = bytearray(rnd.randbytes(n))
    lo, hi = segment(n, lane)
    assert hi - lo >= 5 * MANY + 4 and lo >= 5 * MANY
    fixed = [(0, 4 * MANY + 1), (lo, lo + 5 * MANY + 1)]
    for i in range(MANY):
        buf[lo + 5 * i + 1:lo + 5 * i + 5] = buf[4 * i:4 * i + 4]
    for i in range(1, MANY + 1):  # the byte behind copy i - 1 differs from the one behind its pattern
        while buf[lo + 5 * i] == buf[4 * i]:
            buf[lo + 5 * i] = rnd.getrandbits(8)
    return bytes(_settle(buf, fixed, [4 * i for i in range(MANY)], rnd))


def text(n, seed):
    """Compressible: words from a small vocabulary."""
    rnd = random.Random(seed)
    words = [b"rpc", b"channel", b"server", b"mi355x", b"xgmi", b"fiber", b"snappy", b"  ", b"\n", b"0123456789"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
    return bytes(out[:n])
