// JSON text of a double without libc and without allocation, byte-equal to
// json::AppendShortestDouble / json::Value::write (json/json.cc), compiled
// for the host (g++) and for the device (hipcc): one formatter behind
// pb2json's host printer and the device printer of float / double arrays
// (gpu/json_kernels.hip).
//
// The rule is AppendShortestDouble's: the smallest p in 1..17 for which the
// correctly rounded p-digit decimal of d (ties to even on exact halves)
// converts back to d; trailing zeros stripped. That is not quite "shortest
// decimal in the rounding interval" (Ryu, Schubfach, repr): below a power of
// two the interval is asymmetric, the closest p-digit decimal can fall
// outside it while another p-digit decimal lies inside, and this rule then
// moves on to p + 1 (2^-1017 prints 7.1202363472230444e-307, not
// 7.120236347223045e-307).
//
// Method: the Ryu scaling (Adams, "Ryu: fast float-to-string conversion",
// PLDI 2018): with d = m2 * 2^(e2 + 2), the value v = 4 m2 and the ends of
// its rounding interval lo = 4 m2 - 1 (- 1 more when the neighbour below is
// as far as the one above) and hi = 4 m2 + 2 are scaled by one power of ten
// 10^-e10 chosen so that floor(v) keeps every digit that can matter; the
// three floors come from one 64 x 128-bit multiplication each with the
// tables of tools/gen_shortest_double_table.py, and whether each scaled
// number is an integer (needed for exact halves and for closed interval
// ends) from divisibility by 5^q or 2^q. Then digits are dropped one at a
// time from all three: at every length the value is rounded correctly from
// the dropped digits and tested against the ends, and the shortest length
// that passes wins (dropping stops once no integer lies between the scaled
// ends: ten times an integer that fits later would fit now). At least one
// digit is always dropped unless the scaled
// value is an integer, so a correctly rounded candidate never needs more
// than floor(v), the last dropped digit and "everything below it is zero".
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRPC_SD_FN __host__ __device__ inline
#else
#define MRPC_SD_FN inline
#endif
// constexpr tables: hipcc emits a device copy of a constant-initialized
// constexpr array that device code indexes
#define MRPC_SD_TABLE static constexpr

#include "base/shortest_double_table.h"

namespace mrpc {
namespace shortest_double {

// "-0.00000" + 17 digits; also covers "-" + 21 digits + ".0",
// "-d." + 16 digits + "e-308" and "\"-Infinity\""
constexpr int kMaxJsonDoubleChars = 25;

enum DecimalClass : uint8_t { kFinite = 0, kZero = 1, kNaN = 2, kInfinity = 3 };

// value = digits * 10^exp10 with `ndigits` decimal digits and no trailing
// zero (finite, nonzero values; the other classes carry only the sign)
struct alignas(16) Decimal {
    uint64_t digits;
    int32_t exp10;
    uint8_t ndigits;
    uint8_t negative;
    uint8_t cls;
    uint8_t pad;
};
static_assert(sizeof(Decimal) == 16, "one 16-byte scratch slot per element");

namespace detail {

typedef unsigned __int128 u128;

MRPC_SD_FN int pow5bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }   // bits of 5^e, e <= 3528
MRPC_SD_FN int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }       // floor(log10 2^e), e <= 1650
MRPC_SD_FN int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }      // floor(log10 5^e), e <= 2620

// (m * {lo, hi}) >> j, 64 < j < 128 (m < 2^58, the factor < 2^126)
MRPC_SD_FN uint64_t mul_shift(uint64_t m, const uint64_t* mul, int j) {
    const u128 b0 = (u128)m * mul[0];
    const u128 b2 = (u128)m * mul[1];
    return (uint64_t)(((b0 >> 64) + b2) >> (j - 64));
}

MRPC_SD_FN bool multiple_of_pow5(uint64_t v, int p) {
    if (p > 24) return false;  // v < 2^58 < 5^25
    for (int k = 0; k < p; ++k) {
        if (v % 5 != 0) return false;
        v /= 5;
    }
    return true;
}

// decimal digits of v, 1 <= v < 10^20
MRPC_SD_FN int decimal_length(uint64_t v) {
    uint64_t p = 10;
    for (int n = 1; n < 20; ++n) {
        if (v < p) return n;
        p *= 10;  // 10^19 fits; the product after it is not used
    }
    return 20;
}

MRPC_SD_FN bool multiple_of_pow2(uint64_t v, int p) { return p < 64 && (v & ((1ull << p) - 1)) == 0; }

}  // namespace detail

// The double with the value of the float whose bits are f (integer only:
// device float conversions may flush subnormals).
MRPC_SD_FN uint64_t WidenFloatBits(uint32_t f) {
    const uint64_t sign = (uint64_t)(f >> 31) << 63;
    const uint32_t e = (f >> 23) & 0xFF;
    uint32_t m = f & 0x7FFFFF;
    if (e == 0xFF) return sign | 0x7FF0000000000000ull | ((uint64_t)m << 29);
    if (e != 0) return sign | ((uint64_t)(e + 896) << 52) | ((uint64_t)m << 29);
    if (m == 0) return sign;
    const int lz = __builtin_clz(m) - 8;  // shifts that bring the top set bit to bit 23
    m = (m << lz) & 0x7FFFFF;
    return sign | ((uint64_t)(897 - lz) << 52) | ((uint64_t)m << 29);
}

// Digits, exponent and class of the double whose bits are `bits`.
MRPC_SD_FN Decimal ShortestDigits(uint64_t bits) {
    using namespace detail;
    Decimal r{0, 0, 0, (uint8_t)(bits >> 63), kFinite, 0};
    const uint64_t frac = bits & ((1ull << 52) - 1);
    const uint32_t expo = (uint32_t)(bits >> 52) & 0x7FF;
    if (expo == 0x7FF) {
        r.cls = frac ? kNaN : kInfinity;
        return r;
    }
    if (expo == 0 && frac == 0) {
        r.cls = kZero;
        return r;
    }
    const int e2 = (expo ? (int)expo : 1) - 1075 - 2;
    const uint64_t m2 = expo ? frac | (1ull << 52) : frac;
    const bool closed = (m2 & 1) == 0;  // an interval end itself converts back (ties to even)
    const uint64_t mv = 4 * m2;
    const uint64_t mlo = mv - 1 - (frac != 0 || expo <= 1 ? 1 : 0), mhi = mv + 2;
    uint64_t vr, vlo, vhi;
    bool vr_int, vlo_int, vhi_int;  // the scaled number is an integer
    int e10;
    if (e2 >= 0) {
        const int q = log10_pow2(e2) - (e2 > 3);
        e10 = q;
        const int j = -e2 + q + kPow5InvBits + pow5bits(q) - 1;
        vr = mul_shift(mv, kPow5Inv[q], j);
        vlo = mul_shift(mlo, kPow5Inv[q], j);
        vhi = mul_shift(mhi, kPow5Inv[q], j);
        vr_int = multiple_of_pow5(mv, q);  // x * 2^(e2 - q) / 5^q, e2 >= q
        vlo_int = multiple_of_pow5(mlo, q);
        vhi_int = multiple_of_pow5(mhi, q);
    } else {
        const int q = log10_pow5(-e2) - (-e2 > 1);
        e10 = q + e2;
        const int i = -e2 - q;
        const int j = q - (pow5bits(i) - kPow5Bits);
        vr = mul_shift(mv, kPow5[i], j);
        vlo = mul_shift(mlo, kPow5[i], j);
        vhi = mul_shift(mhi, kPow5[i], j);
        vr_int = multiple_of_pow2(mv, q);  // x * 5^i / 2^q
        vlo_int = multiple_of_pow2(mlo, q);
        vhi_int = multiple_of_pow2(mhi, q);
    }
    // Drop digits. At every length: c = vr rounded by the dropped digits,
    // accepted when lo <= c <= hi (ends open unless `closed`), in integers:
    // ceil(lo) is vlo (+1 unless lo is an integer), floor(hi) is vhi.
    uint64_t best = 0;
    int best_drop = -1;
    uint32_t last = 0;       // the digit dropped last
    bool below_zero = vr_int;  // everything below that digit is zero
    for (int drop = 0; vr != 0; ++drop) {
        bool ok = true;
        uint64_t c = vr;
        if (drop == 0) {
            ok = vr_int;
        } else if (last > 5 || (last == 5 && (!below_zero || (vr & 1)))) {
            c = vr + 1;
        }
        const uint64_t cmin = closed && vlo_int ? vlo : vlo + 1;
        const uint64_t cmax = !closed && vhi_int ? vhi - 1 : vhi;
        // no integer fits at this length: none fits at a shorter one either
        // (c at the next length is 10 c at this one)
        if (cmin > cmax) break;
        if (ok && c >= cmin && c <= cmax) {
            best = c;
            best_drop = drop;
        }
        below_zero = below_zero && last == 0;
        last = (uint32_t)(vr % 10);
        vr /= 10;
        vlo_int = vlo_int && vlo % 10 == 0;
        vlo /= 10;
        vhi_int = vhi_int && vhi % 10 == 0;
        vhi /= 10;
    }
    // strip trailing zeros (a carry such as 9.96 -> 10.0 makes them)
    int exp10 = e10 + best_drop;
    while (best != 0 && best % 10 == 0) {  // 17 digits always pass, so best is never 0
        best /= 10;
        ++exp10;
    }
    r.digits = best;
    r.exp10 = exp10;
    r.ndigits = (uint8_t)decimal_length(best);
    return r;
}

// Characters FormatJsonDecimal writes for d.
MRPC_SD_FN int JsonDecimalLength(const Decimal& d) {
    if (d.cls == kNaN) return 5;
    if (d.cls == kInfinity) return 10 + d.negative;
    if (d.cls == kZero) return 3 + d.negative;
    const int length = d.ndigits;
    const int kk = length + d.exp10;  // position of the decimal point
    int n = d.negative;
    if (d.exp10 >= 0 && kk <= 21) return n + kk + 2;
    if (kk > 0 && kk <= 21) return n + length + 1;
    if (kk > -6 && kk <= 0) return n + 2 - kk + length;
    int e = kk - 1;
    n += length + (length > 1 ? 1 : 0) + 1;
    if (e < 0) {
        ++n;
        e = -e;
    }
    return n + (e >= 100 ? 3 : e >= 10 ? 2 : 1);
}

// The four layouts of AppendShortestDouble; non-finite values as the quoted
// strings Value::write prints. Returns the length, at most
// kMaxJsonDoubleChars; no terminator.
MRPC_SD_FN int FormatJsonDecimal(const Decimal& d, char* out) {
    char* o = out;
    if (d.cls == kNaN) {
        const char s[] = "\"NaN\"";
        for (int i = 0; i < 5; ++i) o[i] = s[i];
        return 5;
    }
    if (d.negative) *o++ = '-';
    if (d.cls == kInfinity) {
        const char s[] = "Infinity\"";
        // the quote goes before the sign
        out[0] = '"';
        o = out + 1;
        if (d.negative) *o++ = '-';
        for (int i = 0; i < 9; ++i) *o++ = s[i];
        return (int)(o - out);
    }
    if (d.cls == kZero) {
        *o++ = '0';
        *o++ = '.';
        *o++ = '0';
        return (int)(o - out);
    }
    const int length = d.ndigits;
    const int kk = length + d.exp10;
    uint64_t v = d.digits;
    if (d.exp10 >= 0 && kk <= 21) {  // 2.0, 1230000.0
        for (int i = length - 1; i >= 0; --i) {
            o[i] = (char)('0' + v % 10);
            v /= 10;
        }
        for (int i = length; i < kk; ++i) o[i] = '0';
        o[kk] = '.';
        o[kk + 1] = '0';
        return (int)(o - out) + kk + 2;
    }
    if (kk > 0 && kk <= 21) {  // 123.45
        for (int i = length; i > 0; --i) {
            o[i > kk ? i : i - 1] = (char)('0' + v % 10);
            v /= 10;
        }
        o[kk] = '.';
        return (int)(o - out) + length + 1;
    }
    if (kk > -6 && kk <= 0) {  // 0.000123
        const int lead = 2 - kk;
        o[0] = '0';
        o[1] = '.';
        for (int i = 2; i < lead; ++i) o[i] = '0';
        for (int i = length - 1; i >= 0; --i) {
            o[lead + i] = (char)('0' + v % 10);
            v /= 10;
        }
        return (int)(o - out) + lead + length;
    }
    // 1e22, 1.5e-7
    if (length == 1) {
        *o++ = (char)('0' + v);
    } else {
        for (int i = length; i > 0; --i) {
            o[i > 1 ? i : 0] = (char)('0' + v % 10);
            v /= 10;
        }
        o[1] = '.';
        o += length + 1;
    }
    *o++ = 'e';
    int e = kk - 1;
    if (e < 0) {
        *o++ = '-';
        e = -e;
    }
    if (e >= 100) *o++ = (char)('0' + e / 100);
    if (e >= 10) *o++ = (char)('0' + e / 10 % 10);
    *o++ = (char)('0' + e % 10);
    return (int)(o - out);
}

MRPC_SD_FN int FormatJsonDoubleBits(uint64_t bits, char* out) { return FormatJsonDecimal(ShortestDigits(bits), out); }

// `out` needs room for kMaxJsonDoubleChars.
MRPC_SD_FN int FormatJsonDouble(double d, char* out) {
    uint64_t bits;
    __builtin_memcpy(&bits, &d, sizeof(bits));
    return FormatJsonDoubleBits(bits, out);
}

}  // namespace shortest_double
}  // namespace mrpc
