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

// ---- the way back: a message that holds such rows, split into the flat array
// and the row ends again (pb::SplitRows in pb/rows.h, gpu::DeviceSplitRows).

// Elements that are varints on the wire. Unlike IsVarintKind this includes
// bool: a peer may send a true as any nonzero varint.
MRPC_ROWS_FN bool WireIsVarint(uint32_t kind) { return kind <= kKindBool; }

// A varint of at most ten bytes, the tenth at most 1, at w[0, avail);
// over-long encodings are accepted (gpu/device_pb.h read_varint). Reads
// w[0, min(avail, 10)) at most.
MRPC_ROWS_FN bool GetVarint(const uint8_t* w, uint64_t avail, uint32_t* used, uint64_t* v) {
    uint64_t x = 0;
    for (uint32_t i = 0; i < 10; ++i) {
        if (i >= avail) return false;
        const uint64_t c = w[i];
        x |= (c & 0x7f) << (7 * i);
        if (!(c & 0x80)) {
            *used = i + 1;
            *v = x;
            return i < 9 || c <= 1;
        }
    }
    return false;
}

constexpr uint32_t kSpecReadBytes = 20;  // a tag and a value or length, ten bytes each
struct Field {
    uint64_t next = 0;            // the offset just past the field
    uint64_t vpos = 0, vlen = 0;  // wire type 2: the value
    uint32_t tag = 0;
    bool valid = false;
};

// The speculative parse of a top-level field at ANY byte offset p of a message
// of n bytes, w pointing at byte p: what devpb::scan_message decides when it
// arrives at p (a tag is a varint of at most 2^32-1, field number 0 and wire
// types 3, 4, 6, 7 are invalid, so is a field that ends beyond n or a length
// above 2^32-1). The device calls it at every offset, garbage ones included,
// and follows the chains of `next`, so two things hold for any bytes:
//   1. it reads w[0, min(n - p, kSpecReadBytes)) at most, never a byte at or
//      beyond n (a canonical tag has five bytes, but scan_message takes an
//      over-long one of ten, hence 20 and not 15);
//   2. a valid field has p < next <= n: every chain of `next` increases
//      strictly and ends.
MRPC_ROWS_FN Field SpecFieldAt(const uint8_t* w, uint64_t p, uint64_t n) {
    Field f;
    if (p >= n) return f;
    const uint64_t avail = n - p;
    uint32_t tn = 0, vn = 0;
    uint64_t tag = 0, v = 0;
    if (!GetVarint(w, avail, &tn, &tag) || tag > 0xFFFFFFFFull || (tag >> 3) == 0) return f;
    const uint32_t wire = (uint32_t)(tag & 7);
    uint64_t size;  // bytes after the tag
    if (wire == 0) {
        if (!GetVarint(w + tn, avail - tn, &vn, &v)) return f;
        size = vn;
    } else if (wire == 1 || wire == 5) {
        size = wire == 1 ? 8 : 4;
    } else if (wire == 2) {
        if (!GetVarint(w + tn, avail - tn, &vn, &v) || v > 0xFFFFFFFFull) return f;
        size = vn + v;
        f.vpos = p + tn + vn;
        f.vlen = v;
    } else {
        return f;
    }
    if (size > avail - tn) return f;
    f.tag = (uint32_t)tag;
    f.next = p + tn + size;
    f.valid = true;
    return f;
}
MRPC_ROWS_FN Field SpecField(const uint8_t* b, uint64_t p, uint64_t n) { return SpecFieldAt(b + p, p, n); }

// Codes of a split: 0 done, 1 malformed wire, 2 refused arguments, 5 more
// elements or rows than the outputs hold, 6 well-formed wire of a shape that
// is not split (the host parser takes it).
constexpr int kSplitMalformed = 1, kSplitRefused = 2, kSplitShort = 5, kSplitUnsupported = 6;

// The verdict on one occurrence of the rows field (wire type 2) whose value
// is b[v, v + s): 0 and the payload's place, 1 or 6. With inner == 0 the
// payload is the value. With inner != 0 the value is empty (a row of no
// element, for every kind) or exactly one field `inner` of wire type 2 that
// fills it; any other sub-message is walked to its end and is 6 when all of
// it is wire (a second field, the inner field unpacked or twice), 1 when not.
// Then the payload: the fixed kinds need whole elements, the varint kinds a
// last byte without a continuation bit. Whether every varint is one the
// packed-run decoder takes (at most ten bytes, the tenth at most 1) is
// VarintsOk below on the host, and the place pass's twin on the device.
// The walk reads only b[v, v + s) and takes at most s / 2 steps.
MRPC_ROWS_FN int RowShape(const uint8_t* b, uint64_t v, uint64_t s, uint32_t inner, uint32_t kind, uint64_t* poff,
                          uint64_t* plen) {
    uint64_t po = v, pl = s;
    if (inner != 0 && s > 0) {
        const uint64_t end = v + s;
        const Field f = SpecField(b, v, end);
        if (!f.valid) return kSplitMalformed;
        if (f.tag != ((inner << 3) | 2) || f.next != end) {
            uint64_t p = f.next;
            while (p < end) {
                const Field g = SpecField(b, p, end);
                if (!g.valid) return kSplitMalformed;
                p = g.next;
            }
            return kSplitUnsupported;
        }
        po = f.vpos;
        pl = f.vlen;
    }
    if (WireIsVarint(kind)) {
        if (pl > 0 && (b[po + pl - 1] & 0x80)) return kSplitMalformed;
    } else if (pl % SourceBytes(kind)) {
        return kSplitMalformed;
    }
    *poff = po;
    *plen = pl;
    return 0;
}

// A payload of varints that ends without a continuation bit: false when the
// packed-run decoder refuses one of them, else their number.
MRPC_ROWS_FN bool VarintsOk(const uint8_t* p, uint64_t len, uint64_t* count) {
    uint64_t n = 0, start = 0;
    for (uint64_t i = 0; i < len; ++i) {
        if (p[i] & 0x80) continue;
        const uint64_t bytes = i - start + 1;
        if (bytes > 10 || (bytes == 10 && p[i] > 1)) return false;
        ++n;
        start = i + 1;
    }
    *count = n;
    return true;
}

// The element a varint of `raw` is in the kind's vector layout, as the
// packed-run decoder stores it: truncated to 32 bits, zigzag undone, a bool
// 0 or 1.
MRPC_ROWS_FN void StoreVarintElem(void* dst, uint64_t i, uint32_t kind, uint64_t raw) {
    switch (kind) {
    case 0:
    case 1: static_cast<uint32_t*>(dst)[i] = (uint32_t)raw; break;
    case 2: {
        const uint32_t u = (uint32_t)raw;
        static_cast<uint32_t*>(dst)[i] = (u >> 1) ^ (0u - (u & 1));
        break;
    }
    case 5: static_cast<uint64_t*>(dst)[i] = (raw >> 1) ^ (0ull - (raw & 1)); break;
    case kKindBool: static_cast<uint8_t*>(dst)[i] = raw ? 1 : 0; break;
    default: static_cast<uint64_t*>(dst)[i] = raw; break;
    }
}

}  // namespace pb_rows
}  // namespace mrpc
