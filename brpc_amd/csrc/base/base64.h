// Base64 (RFC 4648, the standard alphabet with '=' padding) in integer
// arithmetic only, with no table in memory, compiled for the host (g++) and
// for the device (hipcc): one coder behind base64_encode / base64_decode
// (base/util.h) and the device kernels (gpu/base64_kernels.hip). The
// reference goes through butil/base64.h (modp_b64's tables).
//
// Symbols travel four at a time in one uint32_t, the first symbol in the low
// byte (the order they have in little-endian memory); three data bytes travel
// as a 24-bit number, the first byte on top (the order base64 cuts them in).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRPC_B64_FN __host__ __device__ inline
#else
#define MRPC_B64_FN inline
#endif

namespace mrpc {
namespace base64 {

// Text size of n data bytes, padding included.
MRPC_B64_FN uint64_t Base64EncodedBytes(uint64_t n) { return (n + 2) / 3 * 4; }
// Most data bytes L symbols can carry (a lone trailing symbol carries none).
MRPC_B64_FN uint64_t Base64DecodedMaxBytes(uint64_t L) { return L / 4 * 3 + (L % 4) * 3 / 4; }

// value 0..63 -> its symbol
MRPC_B64_FN char Symbol(uint32_t v) {
    uint32_t c = v + 'A';            // A-Z
    c += v >= 26 ? 6u : 0u;          // a-z: 'a' - 'Z' - 1
    c -= v >= 52 ? 75u : 0u;         // 0-9: 'z' + 1 - '0'
    c -= v >= 62 ? 15u : 0u;         // '+': '9' + 1 - '+'
    c += v >= 63 ? 3u : 0u;          // '/'
    return (char)c;
}

// symbol -> its value, -1 for a byte outside the alphabet
MRPC_B64_FN int Value(uint8_t c) {
    int v = -1;
    v = (uint32_t)(c - 'A') < 26u ? (int)c - 'A' : v;
    v = (uint32_t)(c - 'a') < 26u ? (int)c - 'a' + 26 : v;
    v = (uint32_t)(c - '0') < 10u ? (int)c - '0' + 52 : v;
    v = c == '+' ? 62 : v;
    v = c == '/' ? 63 : v;
    return v;
}

// The bytes of a word (W: uint32_t, four of them, or uint64_t, eight) all at
// once. For bytes below 128, bit 7 of (x + 128 - k) is set in exactly the
// bytes that are >= k and no byte carries into the next; the sums below are
// taken over the whole word, which is exact because every byte's own result
// stays within 0..255.
//
// Values 0..63, one per byte -> their symbols.
template <typename W>
MRPC_B64_FN W SymbolsN(W x) {
    const W ones = (W) ~(W)0 / 255;
    const W ge26 = ((x + 102 * ones) >> 7) & ones;
    const W ge52 = ((x + 76 * ones) >> 7) & ones;
    const W ge62 = ((x + 66 * ones) >> 7) & ones;
    const W ge63 = ((x + 65 * ones) >> 7) & ones;
    return x + 'A' * ones + ge26 * 6 - ge52 * 75 - ge62 * 15 + ge63 * 3;
}
MRPC_B64_FN uint32_t Symbols4(uint32_t x) { return SymbolsN<uint32_t>(x); }

// Symbols, one per byte -> their values; *ok is false when a byte is outside
// the alphabet (its value is then unspecified, but below 64). The offset from
// symbol to value steps down at '/', '0', 'A' and 'a' (+19, +16, +4, -65,
// -71); whether every byte was a symbol is decided by mapping the values back.
template <typename W>
MRPC_B64_FN W ValuesN(W s, bool* ok) {
    const W ones = (W) ~(W)0 / 255;
    const W x = s & (127 * ones);
    const W ge47 = ((x + 81 * ones) >> 7) & ones;
    const W ge48 = ((x + 80 * ones) >> 7) & ones;
    const W ge65 = ((x + 63 * ones) >> 7) & ones;
    const W ge97 = ((x + 31 * ones) >> 7) & ones;
    const W v = (x + 19 * ones - ge47 * 3 - ge48 * 12 - ge65 * 69 - ge97 * 6) & (63 * ones);
    *ok = SymbolsN<W>(v) == s;
    return v;
}

// v24 = b0 << 16 | b1 << 8 | b2 -> the four symbols
MRPC_B64_FN uint32_t Encode3(uint32_t v24) {
    return Symbols4(((v24 >> 18) & 63) | ((v24 >> 12) & 63) << 8 | ((v24 >> 6) & 63) << 16 | (v24 & 63) << 24);
}
// The same from the three bytes as they lie in memory (b0 in the low byte;
// the top byte of `le` is ignored).
MRPC_B64_FN uint32_t Encode3LE(uint32_t le) { return Encode3(__builtin_bswap32(le) >> 8); }

// Four symbols -> v24; *ok is false when one of them is outside the alphabet
// (v24 is then unspecified).
MRPC_B64_FN uint32_t Decode4(uint32_t s, bool* ok) {
    const uint32_t v = ValuesN<uint32_t>(s, ok);
    // 6-bit values in bytes -> two 12-bit halves -> 24 bits
    const uint32_t t = (v & 0x003F003Fu) << 6 | ((v >> 8) & 0x003F003Fu);
    return (t & 0xFFFFu) << 12 | t >> 16;
}
// Eight symbols (the first in the low byte) -> their six bytes as a 48-bit
// number, the first byte on top; *ok as above.
MRPC_B64_FN uint64_t Decode8(uint64_t s, bool* ok) {
    const uint64_t v = ValuesN<uint64_t>(s, ok);
    const uint64_t t = (v & 0x003F003F003F003Full) << 6 | ((v >> 8) & 0x003F003F003F003Full);
    return (t & 0xFFFF) << 36 | ((t >> 16) & 0xFFFF) << 24 | ((t >> 32) & 0xFFFF) << 12 | t >> 48;
}
// v24 -> the three bytes as they lie in memory (b0 in the low byte, top byte 0)
MRPC_B64_FN uint32_t Bytes3LE(uint32_t v24) { return __builtin_bswap32(v24) >> 8; }

}  // namespace base64
}  // namespace mrpc
