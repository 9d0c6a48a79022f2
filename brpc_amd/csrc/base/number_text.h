// The shape of JSON number text without a separator table, compiled for the
// host (g++) and for the device (hipcc): one scanner behind
// json::ParseNumberText and the device parser gpu::DeviceParseNumberText
// (gpu/json_kernels.hip), so both give one verdict on every text.
//
// The text is cut into pieces at its commas: piece i is the text between
// comma i - 1 (or the start) and comma i (or the end). A piece that fits is
//   ws ('[' ws){lead} number ws (']' ws){trail}
// and the text is one of
//   depth 0   v,v,...,v             every piece (0, 0)
//   depth 1   [v,v,...,v]           the first piece leads 1, the last trails 1
//   depth 2   [[v,..],[v,..],..]    the first leads 2, the last trails 2, and
//                                   at every comma between: a ']' before it
//                                   exactly when a '[' follows it
// The depth is the first piece's lead. Rules a piece can check alone (with a
// look at what stands before its comma) are JudgePiece's; the ones that need
// the depth are CombineNumberText's, which the host twin and the device's
// publish step both run. Positions are 32-bit: text below 2^32 - 1 bytes.
#pragma once

#include <cstdint>

#include "base/decimal_to_double.h"

namespace mrpc {
namespace number_text {

constexpr uint32_t kNone = 0xFFFFFFFFu;

MRPC_DD_FN bool IsSpace(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
// Whether c ends a number's text: a comma, a bracket or whitespace. One
// shift of a 128-bit set instead of seven compares: a device lane tests
// every byte of its element with it, and branches cost it more than shifts.
MRPC_DD_FN bool EndsNumber(char c) {
    constexpr uint64_t kLow = 1ull << ' ' | 1ull << '\t' | 1ull << '\n' | 1ull << '\r' | 1ull << ',';
    constexpr uint64_t kHigh = 1ull << ('[' - 64) | 1ull << (']' - 64);
    const uint32_t u = (unsigned char)c;
    return (((u & 64) ? kHigh : kLow) >> (u & 63) & (u < 128 ? 1u : 0u)) != 0;
}

struct Piece {
    uint32_t nb, ne;  // the number's text [nb, ne), trimmed
    uint32_t end;     // the comma that ends the piece, or n
    uint8_t lead, trail;
    bool fits;  // the shape above; false: nothing else is meaningful
};

// The piece that starts at b (the byte after its comma, or 0); at(k) is read
// for b <= k < n only.
template <typename At>
MRPC_DD_FN void ScanPiece(const At& at, uint32_t b, uint32_t n, Piece* out) {
    out->fits = false;
    out->lead = out->trail = 0;
    uint32_t p = b;
    for (;;) {
        while (p < n && IsSpace(at(p))) ++p;
        if (p >= n || at(p) != '[') break;
        if (++out->lead > 2) return;
        ++p;
    }
    out->nb = p;
    while (p < n && !EndsNumber(at(p))) ++p;
    out->ne = p;
    for (;;) {
        while (p < n && IsSpace(at(p))) ++p;
        if (p >= n || at(p) != ']') break;
        if (++out->trail > 2) return;
        ++p;
    }
    if (p < n && at(p) != ',') return;
    out->end = p;
    out->fits = true;
}

// Whether a ']' stands before the comma at `comma` (whitespace between them
// skipped); at(k) is read for k < comma only.
template <typename At>
MRPC_DD_FN bool ClosesBefore(const At& at, uint32_t comma) {
    uint32_t k = comma;
    while (k > 0 && IsSpace(at(k - 1))) --k;
    return k > 0 && at(k - 1) == ']';
}

enum PieceVerdict : uint32_t {
    kPieceBad = 1,     // does not fit at any depth
    kPieceNested = 2,  // fits at depth 2 only (a row boundary)
    kPieceBlank = 4,   // the whole text is empty, or "[ ]": no element at all
};

// What piece `index` says alone. closes_before: ClosesBefore at its comma
// (false for piece 0). The number itself is the caller's to convert.
MRPC_DD_FN uint32_t JudgePiece(const Piece& s, uint32_t index, uint32_t n, bool closes_before) {
    if (!s.fits) return kPieceBad;
    const bool last = s.end == n;
    if (s.nb == s.ne) {
        if (index == 0 && last && s.lead == s.trail && s.lead <= 1) return kPieceBlank;
        return kPieceBad;
    }
    if (index > 0 && s.lead != (closes_before ? 1u : 0u)) return kPieceBad;
    if (!last && s.trail > 1) return kPieceBad;
    return (index > 0 && s.lead == 1) || (!last && s.trail == 1) ? kPieceNested : 0u;
}

// What the pieces leave per text for the rules that need the depth.
struct TextState {
    uint32_t bad;         // lowest index of a kPieceBad piece or of a malformed number, kNone
    uint32_t nested_min;  // lowest index of a kPieceNested piece, kNone
    uint32_t lead0;       // the first piece's lead (0 unless it fits)
    uint32_t trail_last;  // the last piece's trail (0 unless it fits)
    uint32_t blank;       // 1: kPieceBlank
};

struct TextVerdict {
    uint32_t depth, count, rows, first_bad;
};

// commas / closes: the ',' and ']' bytes of the whole text. nested_ok: the
// caller takes depth 2 (it has somewhere to put row ends).
MRPC_DD_FN TextVerdict CombineNumberText(const TextState& st, uint32_t commas, uint32_t closes, bool nested_ok) {
    TextVerdict v;
    v.depth = st.lead0;
    v.count = st.blank ? 0 : commas + 1;
    v.rows = v.depth == 2 && closes > 0 ? closes - 1 : 0;
    uint32_t bad = st.bad;
    if (v.depth == 2 && !nested_ok) bad = 0;
    if (v.depth < 2 && st.nested_min < bad) bad = st.nested_min;
    if (st.trail_last != v.depth && commas < bad) bad = commas;  // the last piece's index
    v.first_bad = bad;
    return v;
}

}  // namespace number_text
}  // namespace mrpc
