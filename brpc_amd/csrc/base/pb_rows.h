// Wire rules of a repeated field whose occurrences ("rows") are cut out of one
// flat array by a table of row ends: `repeated Row rows = N` with
// `message Row { repeated T v = I [packed = true]; }`, or `repeated bytes`.
// Compiled for the host (g++) and for the device (hipcc): one set of rules
// behind pb::SerializeRows (pb/rows.h) and the device builder
// gpu::DeviceBuildRows (gpu/pb_kernels.hip). The reference serializes such a
// batch message by message on the host (SerializeToString).
//
// With inner != 0 a row whose payload P is p bytes is
//   varint(number << 3 | 2) varint(s) varint(inner << 3 | 2) varint(p) P
// where s counts everything after it. A row without elements of a packed kind
// is varint(number << 3 | 2) 0x00: the host serializer omits an empty packed
// field, so the sub-message is empty. A row of kind bytes always carries its
// inner field (an empty one is tag 0x02 innertag 0x00), as a bytes field of
// length 0 is tag + 0x00 in the flat builder.
// With inner == 0 (kind bytes only) a row is varint(number << 3 | 2)
// varint(p) P: `repeated bytes` / `repeated string`, or rows that already are
// serialized sub-messages.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRPC_ROWS_FN __host__ __device__ inline
#else
#define MRPC_ROWS_FN inline
#endif

namespace mrpc {
namespace pb_rows {

// Element kinds: gpu::PbRunKind 0..6 (int32, uint32, sint32, int64, uint64,
// sint64, bool: varints), then raw bytes and the two fixed widths (8 and 9 are
// the values the JSON printers use for float and double).
constexpr uint32_t kKindBool = 6, kKindBytes = 7, kKindFixed32 = 8, kKindFixed64 = 9;
constexpr uint32_t kMaxFieldNumber = (1u << 29) - 1;
constexpr uint32_t kMaxHeaderBytes = 20;  // two tags of 5 bytes, two lengths below 2^32

MRPC_ROWS_FN uint32_t VarintLen(uint64_t v) { return (uint32_t)((64 - __builtin_clzll(v | 1) + 6) / 7); }

MRPC_ROWS_FN uint32_t PutVarint(uint8_t* o, uint64_t v) {
    uint32_t n = 0;
    while (v >= 0x80) {
        o[n++] = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    o[n++] = (uint8_t)v;
    return n;
}

// Elements whose wire size depends on their value.
MRPC_ROWS_FN bool IsVarintKind(uint32_t kind) { return kind < kKindBool; }

// Bytes of an element in the source array (the field's vector layout).
MRPC_ROWS_FN uint32_t SourceBytes(uint32_t kind) {
    return kind == kKindBool || kind == kKindBytes ? 1 : (kind <= 2 || kind == kKindFixed32 ? 4 : 8);
}

// Most wire bytes of an element.
MRPC_ROWS_FN uint32_t MaxWireBytes(uint32_t kind) {
    return IsVarintKind(kind) ? (kind == 1 || kind == 2 ? 5 : 10) : SourceBytes(kind);
}

// Element i of src as the number that goes on the wire: signed 32-bit kinds
// sign-extended, zigzag applied, bools as 0 / 1, the fixed kinds' bits.
MRPC_ROWS_FN uint64_t WireValue(const void* src, uint64_t i, uint32_t kind) {
    switch (kind) {
    case 0: return (uint64_t)(int64_t) static_cast<const int32_t*>(src)[i];
    case 1:
    case kKindFixed32: return static_cast<const uint32_t*>(src)[i];
    case 2: {
        const int32_t v = static_cast<const int32_t*>(src)[i];
        return (uint32_t)(((uint32_t)v << 1) ^ (uint32_t)(v >> 31));
    }
    case 5: {
        const uint64_t v = static_cast<const uint64_t*>(src)[i];
        return (v << 1) ^ (uint64_t)((int64_t)v >> 63);
    }
    case kKindBool: return static_cast<const uint8_t*>(src)[i] ? 1 : 0;
    case kKindBytes: return static_cast<const uint8_t*>(src)[i];
    default: return static_cast<const uint64_t*>(src)[i];
    }
}

// Wire bytes of an element whose wire value is v.
MRPC_ROWS_FN uint32_t WireBytes(uint64_t v, uint32_t kind) { return IsVarintKind(kind) ? VarintLen(v) : SourceBytes(kind); }

// number, inner and kind a job may carry.
MRPC_ROWS_FN bool FieldsOk(uint32_t number, uint32_t inner, uint32_t kind) {
    return number >= 1 && number <= kMaxFieldNumber && inner <= kMaxFieldNumber && kind <= kKindFixed64 &&
           (inner != 0 || kind == kKindBytes);
}

// Whether a row of `nelems` elements carries its inner field.
MRPC_ROWS_FN bool HasInner(uint32_t inner, uint32_t kind, uint64_t nelems) {
    return inner != 0 && (nelems > 0 || kind == kKindBytes);
}

// Bytes in front of a row's payload of p bytes.
MRPC_ROWS_FN uint32_t HeaderBytes(uint32_t number, uint32_t inner, uint32_t kind, uint64_t nelems, uint64_t p) {
    const uint32_t tag = VarintLen((uint64_t)number << 3);
    if (inner == 0) return tag + VarintLen(p);
    if (!HasInner(inner, kind, nelems)) return tag + 1;
    const uint32_t in = VarintLen((uint64_t)inner << 3) + VarintLen(p);
    return tag + VarintLen(in + p) + in;
}

// Writes them (at most kMaxHeaderBytes); returns HeaderBytes().
MRPC_ROWS_FN uint32_t PutHeader(uint8_t* o, uint32_t number, uint32_t inner, uint32_t kind, uint64_t nelems,
                                uint64_t p) {
    uint32_t n = PutVarint(o, ((uint64_t)number << 3) | 2);
    if (inner == 0) return n + PutVarint(o + n, p);
    if (!HasInner(inner, kind, nelems)) {
        o[n] = 0;
        return n + 1;
    }
    const uint64_t itag = ((uint64_t)inner << 3) | 2;
    n += PutVarint(o + n, VarintLen(itag) + VarintLen(p) + p);
    n += PutVarint(o + n, itag);
    return n + PutVarint(o + n, p);
}

// Most bytes `rows` rows over `count` elements can take; 0 when the fields
// are refused, there is no row, or the size (or count) is above 2^32 - 1.
MRPC_ROWS_FN uint64_t WorstCaseBytes(uint32_t number, uint32_t inner, uint32_t kind, uint64_t count, uint64_t rows) {
    if (!FieldsOk(number, inner, kind) || rows == 0 || count > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return 0;
    const uint64_t pay = count * MaxWireBytes(kind);
    const uint64_t per_row = VarintLen((uint64_t)number << 3) + VarintLen(pay + 10) +
                             (inner ? VarintLen((uint64_t)inner << 3) + VarintLen(pay) : 0);
    const uint64_t total = pay + rows * per_row;
    return total > 0xFFFFFFFFull ? 0 : total;
}

}  // namespace pb_rows
}  // namespace mrpc
