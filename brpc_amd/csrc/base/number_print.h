// Number arrays and nested number rows as JSON text, compiled for the host
// (g++) and for the device (hipcc): one set of rules behind
// json::FormatNumberRows and the device printer gpu::DevicePrintNumbers
// (gpu/json_number_print_kernels.hip), so both write the same bytes and give
// the same verdict on every table of row ends. The inverse of
// base/number_text.h: every text written here is accepted there at depth
// 0 / 1 / 2 (the quoted "NaN" / "Infinity" of non-finite floats excepted,
// which that scanner refuses).
//
// The input is `count` elements of one kind and, for the nested form, `rows`
// row ends: row_ends[r] = the elements in rows 0..r. Rows are not empty. With
// T(i) the text bytes of the elements before element i, element i starts at
//   bare       v,v,...,v            T(i) + i
//   bracketed  [v,v,...,v]          1 + T(i) + i
//   nested     [[v,..],[v,..],..]   2 + T(i) + i + 2r     (i in row r)
// and the text takes T(count) plus
//   bare       count - 1            (nothing at all for count 0)
//   bracketed  count + 1            (2, "[]", for count 0)
//   nested     count + 2 * rows + 1
// bytes. So what stands in front of element i is nothing / "[" / "[[" for
// i = 0, "],[" where i starts a row and "," elsewhere; what follows the last
// element is nothing / "]" / "]]". No whitespace anywhere.
#pragma once

#include <cstdint>

#include "base/shortest_double.h"

namespace mrpc {
namespace number_print {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// gpu::PbRunKind 0..6 and json2pb's float kinds
enum Kind : uint32_t {
    kInt32 = 0,
    kUint32 = 1,
    kSint32 = 2,  // the number itself, not its zigzag wire form
    kInt64 = 3,
    kUint64 = 4,
    kSint64 = 5,
    kBool = 6,  // one source byte per element: nonzero is true
    kFloat32 = 8,
    kFloat64 = 9,
};
enum Form : uint32_t { kBare = 0, kBracketed = 1, kNested = 2 };

MRPC_SD_FN bool KindValid(uint32_t kind) { return kind <= kBool || kind == kFloat32 || kind == kFloat64; }
MRPC_SD_FN bool KindIsFloat(uint32_t kind) { return kind == kFloat32 || kind == kFloat64; }
// Bytes of one source element, also its natural alignment.
MRPC_SD_FN uint32_t ElemBytes(uint32_t kind) {
    if (kind == kBool) return 1;
    return kind <= kSint32 || kind == kFloat32 ? 4 : 8;
}
// Most text bytes one element takes: "-2147483648", "4294967295",
// "-9223372036854775808", "18446744073709551615", "false", and a double's
// shortest_double::kMaxJsonDoubleChars.
MRPC_SD_FN uint32_t MaxElemChars(uint32_t kind) {
    switch (kind) {
    case kInt32:
    case kSint32: return 11;
    case kUint32: return 10;
    case kInt64:
    case kUint64:
    case kSint64: return 20;
    case kBool: return 5;
    default: return (uint32_t)shortest_double::kMaxJsonDoubleChars;
    }
}
constexpr uint32_t kMaxElemChars = (uint32_t)shortest_double::kMaxJsonDoubleChars;  // of any kind
constexpr uint32_t kMaxLead = 3, kMaxTrail = 2;                                    // "],[" and "]]"

// Decimal digits of v (1 for 0, 20 for 10^19 and above).
MRPC_SD_FN uint32_t DecimalLength(uint64_t v) {
    uint32_t n = 1;
    uint64_t p = 10;
    while (n < 20 && v >= p) {
        if (++n < 20) p *= 10;  // 10^19 fits, 10^20 is never formed
    }
    return n;
}

// An integer element as magnitude and sign.
struct Integer {
    uint64_t mag;
    bool negative;
};
MRPC_SD_FN Integer FromSigned(int64_t v) {
    Integer r;
    r.negative = v < 0;
    r.mag = r.negative ? 0 - (uint64_t)v : (uint64_t)v;  // INT64_MIN: 2^63
    return r;
}
// Element i of an integer kind (not kBool, not a float kind); src is
// naturally aligned.
MRPC_SD_FN Integer LoadInteger(const void* src, uint64_t i, uint32_t kind) {
    switch (kind) {
    case kInt32:
    case kSint32: return FromSigned(static_cast<const int32_t*>(src)[i]);
    case kUint32: {
        Integer r;
        r.mag = static_cast<const uint32_t*>(src)[i];
        r.negative = false;
        return r;
    }
    case kUint64: {
        Integer r;
        r.mag = static_cast<const uint64_t*>(src)[i];
        r.negative = false;
        return r;
    }
    default: return FromSigned(static_cast<const int64_t*>(src)[i]);
    }
}
MRPC_SD_FN uint32_t IntegerLength(const Integer& v) { return DecimalLength(v.mag) + (v.negative ? 1u : 0u); }
// Writes IntegerLength(v) bytes at out and returns their number.
MRPC_SD_FN uint32_t FormatInteger(const Integer& v, char* out) {
    const uint32_t n = IntegerLength(v);
    uint64_t m = v.mag;
    for (uint32_t k = n; k-- > (v.negative ? 1u : 0u);) {
        out[k] = (char)('0' + m % 10);
        m /= 10;
    }
    if (v.negative) out[0] = '-';
    return n;
}

MRPC_SD_FN uint32_t BoolLength(bool b) { return b ? 4u : 5u; }
MRPC_SD_FN uint32_t FormatBool(bool b, char* out) {
    if (b) {
        out[0] = 't', out[1] = 'r', out[2] = 'u', out[3] = 'e';
        return 4;
    }
    out[0] = 'f', out[1] = 'a', out[2] = 'l', out[3] = 's', out[4] = 'e';
    return 5;
}

// The punctuation in front of element i (row_start: i > 0 begins a row of the
// nested form) and behind it (last: i == count - 1).
MRPC_SD_FN uint32_t LeadLength(uint32_t form, bool first, bool row_start) {
    if (first) return form;  // "", "[", "[["
    return row_start ? 3u : 1u;
}
MRPC_SD_FN uint32_t FormatLead(uint32_t form, bool first, bool row_start, char* out) {
    if (first) {
        for (uint32_t k = 0; k < form; ++k) out[k] = '[';
        return form;
    }
    if (!row_start) {
        out[0] = ',';
        return 1;
    }
    out[0] = ']', out[1] = ',', out[2] = '[';
    return 3;
}
MRPC_SD_FN uint32_t TrailLength(uint32_t form, bool last) { return last ? form : 0u; }  // "", "]", "]]"
MRPC_SD_FN uint32_t FormatTrail(uint32_t form, bool last, char* out) {
    if (!last) return 0;
    for (uint32_t k = 0; k < form; ++k) out[k] = ']';
    return form;
}

// Whether row r breaks the rules of a table of `rows` ends over `count`
// elements: prev = row_ends[r - 1] (0 for r = 0), end = row_ends[r]. A table
// is malformed at its lowest such row.
MRPC_SD_FN bool RowEndBad(uint32_t prev, uint32_t end, uint64_t r, uint64_t rows, uint64_t count) {
    return end <= prev || end > count || (r + 1 == rows && end != count);
}

// Most bytes the text can take; it always suffices as a capacity. 0 for a
// kind there is not. rows == 0: a flat form (the brackets are counted).
MRPC_SD_FN uint64_t WorstCaseBytes(uint32_t kind, uint64_t count, uint64_t rows) {
    if (!KindValid(kind)) return 0;
    // an answer above 2^32 - 1 is all a caller needs from counts this large
    if (count > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return ~0ull;
    const uint64_t text = count * MaxElemChars(kind);
    if (rows) return text + count + 2 * rows + 1;
    return count ? text + count + 1 : 2;  // "[]"
}

}  // namespace number_print
}  // namespace mrpc
