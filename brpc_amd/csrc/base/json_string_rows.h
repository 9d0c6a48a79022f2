// The shape of a JSON array of strings, compiled for the host (g++) and for
// the device (hipcc): one set of rules behind json::UnescapeStringRows
// (json/json.h) and gpu::DeviceUnescapeJsonStringRows
// (gpu/json_string_kernels.hip), so both give one verdict on every text.
//
// Whitespace is number_text::IsSpace. A string S is '"' body '"'; the body
// obeys base/json_string.h: a backslash that is not itself escaped starts an
// escape (DecodeEscape, with offsets of the whole text), every other byte is
// copied, raw control bytes and bytes of 0x80 and above included, and a quote
// that no escape covers ends the string. The accepted texts are
//   depth 0   ws | ws S ws (',' ws S ws)*             what EscapeStringRows writes
//   depth 1   ws '[' ws ']' ws | ws '[' ws S ws (',' ws S ws)* ']' ws
// and the depth is 1 exactly when the first byte that is no whitespace is '['.
// The result is the decoded bytes of all strings, one after the other, and
// row_ends[r], the decoded bytes in strings 0..r: the pair DeviceBuildRows,
// DeviceSplitRows and the escaper's rows form use.
//
// Everything else is "not decided here" (json::Reader decides), at the offset
// where a parser that reads from left to right cannot go on: a bad escape at
// its backslash, a byte outside a string that is neither whitespace nor a
// token that may stand there at that byte, a text that ends too soon at n.
//
// The rule is local. The tokens are '[', an opening quote, a closing quote,
// ',', ']' and the end of the text; the predecessor of a token is the byte
// before it that lies outside the strings and is no whitespace (a closing
// quote counts as outside), kStart when there is none. Follows() says which
// predecessors a token accepts, EndsWell() which the end accepts; a ']' also
// needs depth 1. While a prefix of the text obeys these rules the sequential
// parser accepts that prefix, and it sticks at the first token that breaks
// them, so
//   the lowest offset at which a local rule fails  =  the offset at which the
//   sequential parser sticks,
// which is what lets the device judge every token on its own, in parallel,
// and take the minimum.
#pragma once

#include <cstdint>

#include "base/json_string.h"
#include "base/number_text.h"

namespace mrpc {
namespace json_string_rows {

// A token's kind; kStart..kCloseBracket are also what a predecessor can be.
enum Kind : uint32_t {
    kStart = 0,
    kOpenBracket = 1,
    kCloseQuote = 2,
    kComma = 3,
    kCloseBracket = 4,
    kOpenQuote = 5,  // never a predecessor of a byte outside: what follows lies inside
};

// Whether token `tok` may follow predecessor `pred`. Nothing follows a ']'.
MRPC_JSTR_FN bool Follows(uint32_t pred, uint32_t tok) {
    switch (tok) {
    case kOpenBracket: return pred == kStart;
    case kOpenQuote: return pred == kStart || pred == kOpenBracket || pred == kComma;
    case kCloseQuote: return true;  // its opening quote was judged
    case kComma: return pred == kCloseQuote;
    case kCloseBracket: return pred == kOpenBracket || pred == kCloseQuote;  // and depth 1: the caller's check
    default: return false;
    }
}
// Whether the text may end after `pred` (outside a string).
MRPC_JSTR_FN bool EndsWell(uint32_t pred, uint32_t depth) {
    return pred == kStart || (pred == kCloseQuote && depth == 0) || (pred == kCloseBracket && depth == 1);
}
// The kind of a byte outside a string, 0 when it is no token there.
MRPC_JSTR_FN uint32_t OutsideKind(uint8_t c) {
    return c == '[' ? kOpenBracket : c == ',' ? kComma : c == ']' ? kCloseBracket : c == '"' ? kOpenQuote : 0u;
}

// No text of n bytes decodes to more bytes (two of them are quotes) or holds
// more strings ("","",... is the densest).
constexpr uint64_t JsonStringRowsMaxBytes(uint64_t n) { return n < 2 ? 0 : n - 2; }
constexpr uint64_t JsonStringRowsMaxRows(uint64_t n) { return (n + 1) / 3; }

// The sequential walk. at(k) is read for k in [0, n). on_copy(from, len) takes
// a run of the text as it is, on_bytes(p, len) what an escape gives, on_row()
// ends a string. Returns 0 (then *depth is set) or 1
// (then *first_bad is).
template <typename At, typename OnCopy, typename OnBytes, typename OnRow>
MRPC_JSTR_FN int WalkStringRows(const At& at, uint64_t n, OnCopy on_copy, OnBytes on_bytes, OnRow on_row, uint32_t* depth,
                                uint64_t* first_bad) {
    uint32_t pred = kStart, d = 0;
    uint64_t p = 0;
    while (p < n) {
        const uint8_t c = at(p);
        if (number_text::IsSpace((char)c)) {
            ++p;
            continue;
        }
        const uint32_t tok = OutsideKind(c);
        if (tok == 0 || !Follows(pred, tok) || (tok == kCloseBracket && d == 0)) {
            *first_bad = p;
            return 1;
        }
        if (tok == kOpenBracket) d = 1;
        pred = tok;
        ++p;
        if (tok != kOpenQuote) continue;
        uint64_t last_escape = ~0ull;  // where the escape before this one began
        for (;;) {
            if (p >= n) {
                *first_bad = n;
                return 1;
            }
            const uint64_t run = p;
            while (p < n && at(p) != '"' && at(p) != '\\') ++p;
            if (p != run) {
                on_copy(run, p - run);
                continue;
            }
            if (at(p) == '"') break;
            char got[4];
            uint32_t span = 0;
            const int k = json_string::DecodeEscape([&](int o) { return at((uint64_t)((int64_t)p + o)); }, p, n - p,
                                                    [&] { return last_escape == p - 6; }, got, &span);
            if (k < 0) {
                *first_bad = p;
                return 1;
            }
            on_bytes(got, (uint32_t)k);
            last_escape = p;
            p += span;
        }
        on_row();
        pred = kCloseQuote;
        ++p;
    }
    if (!EndsWell(pred, d)) {
        *first_bad = n;
        return 1;
    }
    *depth = d;
    return 0;
}

}  // namespace json_string_rows
}  // namespace mrpc
