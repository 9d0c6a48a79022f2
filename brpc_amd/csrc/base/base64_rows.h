// A JSON array of base64 strings, the form http+json gives a `repeated bytes`
// field or a bytes column of records, compiled for the host (g++) and for the
// device (hipcc): one set of rules behind json::EncodeBase64Rows /
// DecodeBase64Rows (json/json.h) and gpu::DeviceBase64EncodeRows /
// DeviceBase64DecodeRows (gpu/base64_kernels.hip), so both give one verdict on
// every text. The arithmetic is base/base64.h, the grammar outside the strings
// base/json_string_rows.h (Follows, EndsWell, OutsideKind, whitespace).
//
// Encode. Row r is bytes[row_ends[r-1], row_ends[r]) with row_ends[-1] = 0
// (equal neighbours: an empty row) and prints as '"' + its '='-padded base64 +
// '"'; rows are joined by ',' and, with brackets, wrapped in '[' ']'. No
// whitespace. No rows print as nothing, or as "[]".
//
// Decode. Outside the strings the accepted texts are those of
// json_string_rows: S(,S)* at depth 0, '[' .. ']' at depth 1, JSON whitespace
// wherever JSON allows it; empty text, whitespace and "[ ]" are no rows. The
// body of a string is canonical base64 as the flat device decoder defines it:
// m alphabet symbols followed by 0, 1 or 2 '=', m % 4 != 1, padded to a
// multiple of four or not padded at all; trailing bits that are not zero are
// dropped. Everything else (a backslash, even in "\/"; whitespace inside a
// string; URL-safe symbols) is "not decided here" (json::Reader and
// base64_decode are laxer), at the offset where a parser that reads from left
// to right cannot go on.
//
// The rule inside a string is local, like the rule outside. A body byte c at
// body offset j (counted from the byte after the opening quote) with the byte
// `prev` before it is bad when
//   c is a symbol and prev == '='
//   c == '=' and j % 4 < 2
//   c is the closing quote and (prev is a symbol and j % 4 == 1, or
//                               prev == '=' and j % 4 != 0)
//   c is anything else
// and a text that ends inside a string is bad at n. The lowest offset that
// breaks a local rule is the offset at which the sequential walk sticks
// (base64_rows_unittest.cc checks this over every short text), which is what
// lets the device judge every byte on its own and take the minimum.
//
// A body decodes in groups of four symbols counted from its opening quote: a
// group with s symbols before its first byte that is no symbol gives 3 bytes
// when s == 4, else s * 3 / 4.
#pragma once

#include <cstdint>

#include "base/base64.h"
#include "base/json_string_rows.h"

namespace mrpc {
namespace base64_rows {

// The text of `rows` rows that hold n bytes in all is never longer: the
// symbols are at most those of n bytes with two bytes of slack per row, then
// two quotes per row and the commas between them.
constexpr uint64_t Base64RowsWorstCaseBytes(uint64_t n, uint64_t rows, bool brackets) {
    return rows == 0 ? (brackets ? 2u : 0u) : (n + 2 * rows) / 3 * 4 + 3 * rows - 1 + (brackets ? 2u : 0u);
}
// The text of one row of len bytes, quotes included.
MRPC_B64_FN uint64_t Base64RowTextBytes(uint64_t len) { return base64::Base64EncodedBytes(len) + 2; }

// No text of n bytes decodes to more bytes (two of them are quotes) or holds
// more strings ("","",... is the densest).
constexpr uint64_t Base64RowsMaxBytes(uint64_t n) { return n < 2 ? 0 : (n - 2) / 4 * 3 + ((n - 2) % 4) * 3 / 4; }
constexpr uint64_t Base64RowsMaxRows(uint64_t n) { return (n + 1) / 3; }

MRPC_B64_FN bool IsSymbol(uint8_t c) { return base64::Value(c) >= 0; }

// The local rule: whether body byte c at body offset j, after byte prev (the
// opening quote when j == 0), breaks it.
MRPC_B64_FN bool BodyByteBad(uint8_t c, uint8_t prev, uint64_t j) {
    if (IsSymbol(c)) return prev == '=';
    if (c == '=') return j % 4 < 2;
    if (c == '"') return (IsSymbol(prev) && j % 4 == 1) || (prev == '=' && j % 4 != 0);
    return true;
}
// Decoded bytes of a group that starts with s symbols (0..4) before its first non-symbol.
MRPC_B64_FN uint32_t GroupBytes(uint32_t s) { return s >= 4 ? 3u : s * 3 / 4; }

// The sequential walk. at(k) is read for k in [0, n). on_bytes(p, len) takes
// the 1..3 bytes a group gives, on_row() ends a string. Returns 0 (then *depth
// is set) or 1 (then *first_bad is).
template <typename At, typename OnBytes, typename OnRow>
MRPC_B64_FN int WalkBase64Rows(const At& at, uint64_t n, OnBytes on_bytes, OnRow on_row, uint32_t* depth,
                               uint64_t* first_bad) {
    namespace jr = json_string_rows;
    uint32_t pred = jr::kStart, d = 0;
    uint64_t p = 0;
    while (p < n) {
        const uint8_t c = at(p);
        if (number_text::IsSpace((char)c)) {
            ++p;
            continue;
        }
        const uint32_t tok = jr::OutsideKind(c);
        if (tok == 0 || !jr::Follows(pred, tok) || (tok == jr::kCloseBracket && d == 0)) {
            *first_bad = p;
            return 1;
        }
        if (tok == jr::kOpenBracket) d = 1;
        pred = tok;
        ++p;
        if (tok != jr::kOpenQuote) continue;
        // the body: whole groups, then what is left of the last one
        uint32_t s = 0, word = 0;  // symbols of the open group, first in the low byte
        while (p < n && IsSymbol(at(p))) {
            word |= (uint32_t)at(p) << (8 * s);
            ++p;
            if (++s == 4) {
                bool ok;
                const uint32_t le = base64::Bytes3LE(base64::Decode4(word, &ok));
                const char b[3] = {(char)le, (char)(le >> 8), (char)(le >> 16)};
                on_bytes(b, 3u);
                s = 0, word = 0;
            }
        }
        uint32_t pads = 0;
        while (p < n && at(p) == '=' && pads < 2 && s + pads >= 2 && s + pads < 4) ++p, ++pads;
        if (p >= n) {
            *first_bad = n;
            return 1;
        }
        // here stands no symbol, and an '=' only where none may stand
        if (at(p) != '"' || s == 1 || (pads != 0 && s + pads != 4)) {
            *first_bad = p;
            return 1;
        }
        if (s >= 2) {
            bool ok;
            const uint32_t fill = s == 2 ? 0x41410000u : 0x41000000u;  // 'A': zero bits
            const uint32_t le = base64::Bytes3LE(base64::Decode4(word | fill, &ok));
            const char b[2] = {(char)le, (char)(le >> 8)};
            on_bytes(b, GroupBytes(s));
        }
        on_row();
        pred = jr::kCloseQuote;
        ++p;
    }
    if (!jr::EndsWell(pred, d)) {
        *first_bad = n;
        return 1;
    }
    *depth = d;
    return 0;
}

}  // namespace base64_rows
}  // namespace mrpc
