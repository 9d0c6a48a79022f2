// The rules of a JSON string body (the text between the quotes) and of
// well-formed UTF-8, in integer arithmetic only, with no table in memory,
// compiled for the host (g++) and for the device (hipcc): one set of rules
// behind json::EscapeStringBody / UnescapeStringBody / Utf8FirstBad
// (json/json.h) and the device kernels (gpu/json_string_kernels.hip). The
// reference escapes and unescapes on the host through rapidjson's Writer and
// Reader.
//
//  escape    what json::EscapeString writes between its quotes: a byte is
//            copied unless it is a quote, a backslash or below 0x20; those
//            become \" and \\, \n \r \t \b \f, and \u00xx (lower-case hex) for
//            the other control bytes. 0x7f, '/' and bytes of 0x80 and above are copied.
//  unescape  a backslash that is not itself escaped starts an escape:
//            \" \\ \/ \b \f \n \r \t give one byte, \uXXXX (hex of either
//            case) the UTF-8 of the code unit, a high surrogate followed at
//            once by a low-surrogate escape the 4 bytes of the pair. All other
//            bytes are copied. Everything json::Reader treats more loosely, or
//            refuses, is "not decided here" (code 1 at the offset of the
//            offending backslash or quote): an unescaped '"', a backslash as
//            the last byte, an unknown letter, fewer than four hex digits, a
//            high surrogate without its partner, a low one without a high one.
//  UTF-8     well-formed as Unicode defines it (Table 3-7): no overlong forms,
//            no surrogates, nothing above U+10FFFF, no truncated tail.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRPC_JSTR_FN __host__ __device__ inline
#else
#define MRPC_JSTR_FN inline
#endif

namespace mrpc {
namespace json_string {

// ---------------------------------------------------------------- escape

// Bytes the escaped form of c takes: 1, 2 or 6.
MRPC_JSTR_FN uint32_t EscapedSize(uint8_t c) {
    if (c >= 0x20) return c == '"' || c == '\\' ? 2u : 1u;
    return c == '\n' || c == '\r' || c == '\t' || c == '\b' || c == '\f' ? 2u : 6u;
}

// 0x80 in every byte of w that equals c (bytes of any value, exact).
MRPC_JSTR_FN uint64_t EqMask8(uint64_t w, uint8_t c) {
    const uint64_t low7 = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t x = w ^ (0x0101010101010101ull * c);
    return ~(((x & low7) + low7) | x | low7);  // 0x80 where the byte of x is zero
}
// 0x80 in every byte of w that is below 0x20 (exact).
MRPC_JSTR_FN uint64_t Lt20Mask8(uint64_t w) {
    const uint64_t low7 = 0x7F7F7F7F7F7F7F7Full;
    // below 0x20: the top bit clear and (low 7 bits + 0x60) does not carry into it
    return ~(((w & low7) + 0x6060606060606060ull) | w | low7);
}
// Number of 0x80 marks in m.
MRPC_JSTR_FN uint32_t Marks8(uint64_t m) { return (uint32_t)(((m >> 7) * 0x0101010101010101ull) >> 56); }

// Whether no byte of the word needs an escape.
MRPC_JSTR_FN bool PlainWord8(uint64_t w) { return (Lt20Mask8(w) | EqMask8(w, '"') | EqMask8(w, '\\')) == 0; }

// Summed escaped size of the 8 bytes of w: 8 + one more for every byte with a
// two-byte escape + five more for every other control byte.
MRPC_JSTR_FN uint32_t EscapedSize8(uint64_t w) {
    const uint64_t ctl = Lt20Mask8(w);
    const uint64_t two = EqMask8(w, '"') | EqMask8(w, '\\') | EqMask8(w, '\n') | EqMask8(w, '\r') | EqMask8(w, '\t') |
                         EqMask8(w, '\b') | EqMask8(w, '\f');
    return 8u + Marks8(two) + 5u * Marks8(ctl & ~two);
}
// The same of the 4 bytes of w.
MRPC_JSTR_FN uint32_t EscapedSize4(uint32_t w) {
    // four bytes of 0x30 ('0') in the upper half: plain, one byte each
    return EscapedSize8((uint64_t)w | 0x3030303000000000ull) - 4u;
}

MRPC_JSTR_FN char HexLower(uint32_t v) { return (char)(v < 10 ? '0' + v : 'a' + (v - 10)); }

// Writes the escaped form of c at out (room for EscapedSize(c)); returns its size.
MRPC_JSTR_FN uint32_t EscapeByte(uint8_t c, char* out) {
    if (c >= 0x20) {
        if (c == '"' || c == '\\') {
            out[0] = '\\';
            out[1] = (char)c;
            return 2;
        }
        out[0] = (char)c;
        return 1;
    }
    char letter = 0;
    if (c == '\n') letter = 'n';
    if (c == '\r') letter = 'r';
    if (c == '\t') letter = 't';
    if (c == '\b') letter = 'b';
    if (c == '\f') letter = 'f';
    out[0] = '\\';
    if (letter) {
        out[1] = letter;
        return 2;
    }
    out[1] = 'u';
    out[2] = '0';
    out[3] = '0';
    out[4] = HexLower(c >> 4);
    out[5] = HexLower(c & 15);
    return 6;
}

// -------------------------------------------------------------- unescape

// Value of a hex digit of either case, -1 for any other byte.
MRPC_JSTR_FN int HexValue(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    const uint8_t l = c | 0x20;
    if (l >= 'a' && l <= 'f') return l - 'a' + 10;
    return -1;
}
// The code unit of four hex digits, -1 when one of them is no hex digit.
MRPC_JSTR_FN int Hex4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) {
    const int h3 = HexValue(a), h2 = HexValue(b), h1 = HexValue(c), h0 = HexValue(d);
    if ((h3 | h2 | h1 | h0) < 0) return -1;  // any -1 sets the sign bit of the union
    return h3 << 12 | h2 << 8 | h1 << 4 | h0;
}
// The byte of a one-letter escape, -1 for 'u' and for every unknown letter.
MRPC_JSTR_FN int SimpleEscape(uint8_t letter) {
    switch (letter) {
    case '"': return '"';
    case '\\': return '\\';
    case '/': return '/';
    case 'b': return '\b';
    case 'f': return '\f';
    case 'n': return '\n';
    case 'r': return '\r';
    case 't': return '\t';
    default: return -1;
    }
}
// UTF-8 of cp (below 0x110000) at out; returns 1..4.
MRPC_JSTR_FN uint32_t PutUtf8(uint32_t cp, char* out) {
    if (cp < 0x80) {
        out[0] = (char)cp;
        return 1;
    }
    if (cp < 0x800) {
        out[0] = (char)(0xC0 | (cp >> 6));
        out[1] = (char)(0x80 | (cp & 0x3F));
        return 2;
    }
    if (cp < 0x10000) {
        out[0] = (char)(0xE0 | (cp >> 12));
        out[1] = (char)(0x80 | ((cp >> 6) & 0x3F));
        out[2] = (char)(0x80 | (cp & 0x3F));
        return 3;
    }
    out[0] = (char)(0xF0 | (cp >> 18));
    out[1] = (char)(0x80 | ((cp >> 12) & 0x3F));
    out[2] = (char)(0x80 | ((cp >> 6) & 0x3F));
    out[3] = (char)(0x80 | (cp & 0x3F));
    return 4;
}

constexpr int kEscapeBad = -1;
// An escape seen from its (unescaped) backslash. `at(k)` gives the byte k
// places from the backslash, k in [-6, 11], and is called only for places
// inside the body: `before` bytes lie in front of the backslash (the rule looks
// at six of them) and `avail` from it to the end, itself included (the rule
// looks at twelve). `high_before` tells whether the byte at -6 is an unescaped
// backslash; it is asked only when the bytes from -6 on read \uD8xx..\uDBxx.
// Returns the bytes the escape gives (0 for the low half of a pair, which its
// high half has written) and puts them at out (room for 4), or kEscapeBad.
// *span gets the bytes the escape takes in the text (2 or 6), for a walker
// that goes from escape to escape.
template <typename At, typename HighBefore>
MRPC_JSTR_FN int DecodeEscape(At at, uint64_t before, uint64_t avail, HighBefore high_before, char* out,
                              uint32_t* span) {
    if (avail < 2) return kEscapeBad;
    const uint8_t letter = at(1);
    *span = 2;
    const int simple = SimpleEscape(letter);
    if (simple >= 0) {
        out[0] = (char)simple;
        return 1;
    }
    if (letter != 'u' || avail < 6) return kEscapeBad;
    const int cu = Hex4(at(2), at(3), at(4), at(5));
    if (cu < 0) return kEscapeBad;
    *span = 6;
    if (cu < 0xD800 || cu >= 0xE000) return (int)PutUtf8((uint32_t)cu, out);
    if (cu < 0xDC00) {  // a high surrogate: the low one must follow at once
        if (avail < 12 || at(6) != '\\' || at(7) != 'u') return kEscapeBad;
        const int lo = Hex4(at(8), at(9), at(10), at(11));
        if (lo < 0xDC00 || lo >= 0xE000) return kEscapeBad;
        return (int)PutUtf8(0x10000u + (((uint32_t)cu - 0xD800u) << 10) + ((uint32_t)lo - 0xDC00u), out);
    }
    // a low surrogate: nothing, when the high half stands right before it
    if (before < 6 || at(-6) != '\\' || at(-5) != 'u') return kEscapeBad;
    const int hi = Hex4(at(-4), at(-3), at(-2), at(-1));
    if (hi < 0xD800 || hi >= 0xDC00 || !high_before()) return kEscapeBad;
    return 0;
}

// ----------------------------------------------------------------- UTF-8

MRPC_JSTR_FN bool Utf8IsCont(uint8_t c) { return (c & 0xC0) == 0x80; }
// Length a lead byte announces: 1..4, 0 for a byte that starts no sequence
// (a continuation byte, C0, C1, F5..FF).
MRPC_JSTR_FN uint32_t Utf8NominalLen(uint8_t c) {
    if (c < 0x80) return 1;
    if (c < 0xC2) return 0;
    if (c < 0xE0) return 2;
    if (c < 0xF0) return 3;
    if (c < 0xF5) return 4;
    return 0;
}
// Length of the well-formed sequence that starts with b0 (b1..b3 follow it;
// `avail` bytes exist from b0 on, those beyond may hold anything), 0 when none
// starts there.
MRPC_JSTR_FN uint32_t Utf8SequenceLen(uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3, uint64_t avail) {
    const uint32_t len = Utf8NominalLen(b0);
    if (len <= 1) return len;
    if (avail < len) return 0;
    uint8_t lo = 0x80, hi = 0xBF;  // the second byte's range carries the special cases
    if (b0 == 0xE0) lo = 0xA0;
    if (b0 == 0xED) hi = 0x9F;
    if (b0 == 0xF0) lo = 0x90;
    if (b0 == 0xF4) hi = 0x8F;
    if (b1 < lo || b1 > hi) return 0;
    if (len >= 3 && !Utf8IsCont(b2)) return 0;
    if (len == 4 && !Utf8IsCont(b3)) return 0;
    return len;
}
// A continuation byte seen from the (up to three) bytes before it, p1 the
// nearest; `before` of them exist. True when a lead byte close enough in front
// of it announces a sequence that reaches it; whether that sequence is
// well-formed is the lead byte's matter. False: a stray continuation, where no
// sequence starts.
MRPC_JSTR_FN bool Utf8ContCovered(uint8_t p1, uint8_t p2, uint8_t p3, uint64_t before) {
    if (before >= 1 && !Utf8IsCont(p1)) return Utf8NominalLen(p1) > 1;
    if (before >= 2 && !Utf8IsCont(p2)) return Utf8NominalLen(p2) > 2;
    if (before >= 3 && !Utf8IsCont(p3)) return Utf8NominalLen(p3) > 3;
    return false;
}

}  // namespace json_string
}  // namespace mrpc
