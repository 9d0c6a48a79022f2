// The text of one JSON number to its value without libc and without
// allocation, in integer arithmetic only, compiled for the host (g++) and
// for the device (hipcc): one converter behind json::Reader's number arrays
// and the device parser of float / double arrays (gpu/json_kernels.hip).
// It is the inverse of base/shortest_double.h.
//
// The result mirrors what json::Reader::number makes of the same text: an
// int64 (a literal -?digits that fits), a uint64 (above INT64_MAX), or the
// correctly rounded double (nearest, ties to even; subnormals, underflow to
// +-0 and overflow to +-Infinity included), bit-equal to std::from_chars /
// strtod. The accepted grammar is RFC 8259's,
//   -? (0 | [1-9][0-9]*) (\.[0-9]+)? ([eE][+-]?[0-9]+)?
// which is narrower than the host reader's (it takes "01" and "1."):
// everything else is kMalformed here and the caller's general path decides.
// Whatever is accepted converts exactly as the host does.
//
// Method: the Eisel-Lemire algorithm (Lemire, "Number parsing at a gigabyte
// per second", SPE 2021). The decimal significand w (at most 19 digits, so
// it fits 64 bits) is shifted to 64 bits and multiplied by the 128-bit power
// of five of tools/gen_decimal_to_double_table.py; the second 64 x 64 product
// is taken when the first leaves the low bits undecided. For a w that is the
// exact significand this needs no fallback (Mushtak & Lemire, "Fast number
// parsing without fallback", SPE 2023). With more than 19 significant digits
// and a nonzero digit among those dropped, the value lies strictly between
// w * 10^q and (w + 1) * 10^q: when both convert to one double, rounding
// being monotonic, that is the answer; otherwise the class is kNeedsExact and
// the caller uses exact arithmetic (the host's from_chars / strtod).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRPC_DD_FN __host__ __device__ inline
#else
#define MRPC_DD_FN inline
#endif
// constexpr tables: hipcc emits a device copy of a constant-initialized
// constexpr array that device code indexes
#define MRPC_DD_TABLE static constexpr

#include "base/decimal_to_double_table.h"

namespace mrpc {
namespace decimal_to_double {

// Longer texts are kNeedsExact unread, so the work of one device lane is
// bounded: "-" + 17 digits + "." + "e-308" is 24, a 40-digit literal fits.
constexpr int kMaxDeviceNumberChars = 48;

enum NumberClass : uint8_t {
    kInt64 = 0,       // bits: the int64
    kUInt64 = 1,      // bits: a value above INT64_MAX
    kDouble = 2,      // bits: the IEEE binary64 image
    kNeedsExact = 3,  // a legal number (or a text too long to read) this code does not decide
    kMalformed = 4,   // not in the grammar above
};

struct NumberResult {
    uint64_t bits;
    uint8_t cls;
};

namespace detail {

typedef unsigned __int128 u128;

// w * 10^q, 0 < w, to the nearest double's bits (sign clear). Exact for the
// w and q given; see the header comment for a truncated w.
MRPC_DD_FN uint64_t scale_to_double(uint64_t w, int64_t q) {
    constexpr int kMantBits = 52;
    constexpr uint64_t kInf = 0x7FF0000000000000ull;
    if (q < kSmallestPow10) return 0;  // below half the smallest subnormal for any 64-bit w
    if (q > kLargestPow10) return kInf;
    const int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t* five = kPow5_128[q - kSmallestPow10];
    u128 first = (u128)w * five[0];
    uint64_t hi = (uint64_t)(first >> 64), lo = (uint64_t)first;
    if ((hi & 0x1FF) == 0x1FF) {  // the 55 bits kept may still change: refine with the low word
        const uint64_t second_hi = (uint64_t)(((u128)w * five[1]) >> 64);
        lo += second_hi;
        if (second_hi > lo) ++hi;
    }
    const int upperbit = (int)(hi >> 63);
    const int shift = upperbit + 64 - kMantBits - 3;
    uint64_t m = hi >> shift;
    // floor(log2 10^q) + 63, then the bias
    int power2 = (int)((217706 * q) >> 16) + 63 + upperbit - lz + 1023;
    if (power2 <= 0) {  // subnormal
        if (-power2 + 1 >= 64) return 0;
        m >>= -power2 + 1;
        m += m & 1;
        m >>= 1;
        // a carry into bit 52 is the smallest normal, whose image this is
        return m;
    }
    // exactly halfway between two doubles only for small powers of five
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << kMantBits)) {
        m = 1ull << kMantBits;
        ++power2;
    }
    m &= ~(1ull << kMantBits);
    if (power2 >= 0x7FF) return kInf;
    return ((uint64_t)power2 << kMantBits) | m;
}

}  // namespace detail

// The number whose text is at(b) .. at(e - 1), already trimmed; `at` maps a
// position to its character (a device lane reads LDS or memory through it).
template <typename At>
MRPC_DD_FN void ParseJsonNumberAt(const At& at, uint32_t b, uint32_t e, NumberResult* out) {
    out->bits = 0;
    out->cls = kMalformed;
    if (b >= e) return;
    if (e - b > (uint32_t)kMaxDeviceNumberChars) {
        out->cls = kNeedsExact;
        return;
    }
    uint32_t i = b;
    const bool neg = at(i) == '-';
    if (neg) ++i;
    uint64_t w = 0;        // the first 19 significant digits
    int nd = 0;            // significant digits seen (leading zeros are none)
    int exp10 = 0;         // value = w * 10^exp10 (+ what was dropped)
    uint32_t d20 = 0;      // the 20th significant digit
    bool dropped = false;  // a nonzero digit beyond the 19th
    if (i >= e) return;
    uint32_t d = (uint32_t)(unsigned char)at(i) - '0';
    if (d > 9) return;
    ++i;
    if (d == 0) {
        if (i < e && (uint32_t)(unsigned char)at(i) - '0' <= 9) return;  // a leading zero
    } else {
        w = d;
        nd = 1;
        for (; i < e; ++i) {
            d = (uint32_t)(unsigned char)at(i) - '0';
            if (d > 9) break;
            if (nd < 19) {
                w = w * 10 + d;
            } else {
                if (nd == 19) d20 = d;
                dropped = dropped || d != 0;
                ++exp10;
            }
            ++nd;
        }
    }
    bool is_float = false;
    if (i < e && at(i) == '.') {
        is_float = true;
        ++i;
        const uint32_t first = i;
        for (; i < e; ++i) {
            d = (uint32_t)(unsigned char)at(i) - '0';
            if (d > 9) break;
            if (nd == 0 && d == 0) {
                --exp10;  // 0.000ddd
            } else if (nd < 19) {
                w = w * 10 + d;
                ++nd;
                --exp10;
            } else {
                dropped = dropped || d != 0;
                ++nd;
            }
        }
        if (i == first) return;  // "1."
    }
    int64_t ex = 0;
    if (i < e && (at(i) == 'e' || at(i) == 'E')) {
        is_float = true;
        ++i;
        bool eneg = false;
        if (i < e && (at(i) == '+' || at(i) == '-')) {
            eneg = at(i) == '-';
            ++i;
        }
        const uint32_t first = i;
        for (; i < e; ++i) {
            d = (uint32_t)(unsigned char)at(i) - '0';
            if (d > 9) break;
            if (ex < 100000000) ex = ex * 10 + d;  // clamped: far past any representable exponent
        }
        if (i == first) return;  // "1e", "1e+"
        if (eneg) ex = -ex;
    }
    if (i != e) return;
    if (!is_float) {
        if (nd <= 19) {  // w is the literal
            if (neg) {
                if (w <= 0x8000000000000000ull) {
                    out->bits = (uint64_t)0 - w;  // "-0" is the integer 0
                    out->cls = kInt64;
                    return;
                }
            } else {
                out->bits = w;
                out->cls = w <= 0x7FFFFFFFFFFFFFFFull ? kInt64 : kUInt64;
                return;
            }
        } else if (nd == 20 && !neg && w <= (0xFFFFFFFFFFFFFFFFull - d20) / 10) {
            out->bits = w * 10 + d20;
            out->cls = kUInt64;
            return;
        }
        // out of both integer ranges: the double
    }
    const uint64_t sign = neg ? 0x8000000000000000ull : 0;
    if (w == 0) {
        out->bits = sign;
        out->cls = kDouble;
        return;
    }
    const int64_t q = ex + exp10;
    const uint64_t r = detail::scale_to_double(w, q);
    if (dropped && detail::scale_to_double(w + 1, q) != r) {  // w + 1 <= 10^19 fits
        out->cls = kNeedsExact;
        return;
    }
    out->bits = sign | r;
    out->cls = kDouble;
}

struct PointerAt {
    const char* base;
    MRPC_DD_FN char operator()(uint32_t k) const { return base[k]; }
};

// The trimmed text [b, e) of one element.
MRPC_DD_FN void ParseJsonNumber(const char* b, const char* e, NumberResult* out) {
    if (e < b || (uint64_t)(e - b) > (uint64_t)kMaxDeviceNumberChars) {
        out->bits = 0;
        out->cls = e <= b ? kMalformed : kNeedsExact;
        return;
    }
    ParseJsonNumberAt(PointerAt{b}, 0, (uint32_t)(e - b), out);
}

// The bits of (float)x for the double whose bits are d: round to nearest
// even, float subnormals, overflow to Infinity, a NaN quieted with the top of
// its payload kept (integer only: device float conversions may flush
// subnormals). The inverse of shortest_double::WidenFloatBits.
MRPC_DD_FN uint32_t NarrowDoubleBits(uint64_t d) {
    const uint32_t sign = (uint32_t)(d >> 63) << 31;
    const int e = (int)((d >> 52) & 0x7FF);
    const uint64_t frac = d & ((1ull << 52) - 1);
    if (e == 0x7FF) {
        if (frac == 0) return sign | 0x7F800000u;
        return sign | 0x7FC00000u | (uint32_t)(frac >> 29);
    }
    if (e == 0) return sign;  // a double subnormal is far below half the smallest float
    const uint64_t m = frac | (1ull << 52);
    const int E = e - 1023;
    if (E > 127) return sign | 0x7F800000u;
    if (E >= -126) {
        uint64_t r = m >> 29;
        const uint64_t rem = m & ((1ull << 29) - 1), half = 1ull << 28;
        if (rem > half || (rem == half && (r & 1))) ++r;
        // a carry out of the significand lands in the exponent field
        const uint32_t v = ((uint32_t)(E + 127) << 23) + (uint32_t)(r - (1ull << 23));
        return sign | (v >= 0x7F800000u ? 0x7F800000u : v);
    }
    const int shift = 29 + (-126 - E);
    if (shift > 63) return sign;
    uint64_t r = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    return sign | (uint32_t)r;  // 0x800000 is the smallest normal's image
}

// The double an integer class converts to (json::Value::as_double: a cast),
// in integer arithmetic: round to nearest even at 53 bits.
MRPC_DD_FN uint64_t IntegerToDoubleBits(uint64_t mag, bool negative) {
    const uint64_t sign = negative ? 0x8000000000000000ull : 0;
    if (mag == 0) return 0;  // (double)(int64_t)0 is +0.0, "-0" included
    const int lz = __builtin_clzll(mag);
    const uint64_t n = mag << lz;  // bit 63 set
    uint64_t r = n >> 11;
    const uint64_t rem = n & 0x7FF, half = 0x400;
    if (rem > half || (rem == half && (r & 1))) ++r;
    // r in [2^52, 2^53]; a carry to 2^53 lands in the exponent field
    return sign | (((uint64_t)(1023 + 63 - lz) << 52) + (r - (1ull << 52)));
}

// The double of a parsed element of class kInt64 / kUInt64 / kDouble.
MRPC_DD_FN uint64_t NumberToDoubleBits(const NumberResult& r) {
    if (r.cls == kDouble) return r.bits;
    if (r.cls == kUInt64) return IntegerToDoubleBits(r.bits, false);
    const bool neg = (int64_t)r.bits < 0;
    return IntegerToDoubleBits(neg ? (uint64_t)0 - r.bits : r.bits, neg);
}

}  // namespace decimal_to_double
}  // namespace mrpc
