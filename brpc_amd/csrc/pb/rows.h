// The host twin of gpu::DeviceBuildRows (gpu/device_codec.h): the
// occurrences of one repeated field, cut out of a flat host array by a table
// of row ends, appended to a string. The rules are base/pb_rows.h, the code
// the device kernels run; this is the oracle of their tests and what a caller
// falls back to when the device declined a job.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "base/pb_rows.h"

namespace mrpc {
namespace pb {

// src: `count` elements in the kind's vector layout (base/pb_rows.h), rows
// back to back; row_ends[r]: the elements in rows 0..r. Returns 0 and appends
// the bytes; 1 when row_ends decreases at row *first_bad or its last entry is
// not count (*first_bad = rows - 1); 2 when the arguments are refused (as the
// device entry refuses them). Nothing is appended on 1 or 2.
inline int SerializeRows(uint32_t number, uint32_t inner, uint32_t kind, const void* src, uint64_t count,
                         const uint32_t* row_ends, uint64_t rows, std::string* out, uint32_t* first_bad = nullptr) {
    if (first_bad) *first_bad = 0xFFFFFFFFu;
    if (!out || !row_ends || (count > 0 && !src) || pb_rows::WorstCaseBytes(number, inner, kind, count, rows) == 0) {
        return 2;
    }
    uint64_t prev = 0;
    for (uint64_t r = 0; r < rows; ++r) {
        if (row_ends[r] < prev || (r + 1 == rows && row_ends[r] != count)) {
            if (first_bad) *first_bad = (uint32_t)r;
            return 1;
        }
        prev = row_ends[r];
    }
    const bool varints = kind <= pb_rows::kKindBool;  // bools are normalized to 0 / 1
    const uint32_t eb = pb_rows::SourceBytes(kind);
    uint64_t at = 0;
    for (uint64_t r = 0; r < rows; ++r) {
        const uint64_t end = row_ends[r];
        uint64_t p = (end - at) * eb;
        if (pb_rows::IsVarintKind(kind)) {
            p = 0;
            for (uint64_t i = at; i < end; ++i) p += pb_rows::VarintLen(pb_rows::WireValue(src, i, kind));
        }
        uint8_t head[pb_rows::kMaxHeaderBytes];
        const uint32_t hn = pb_rows::PutHeader(head, number, inner, kind, end - at, p);
        out->append(reinterpret_cast<const char*>(head), hn);
        if (p > 0 && !varints) {
            out->append(static_cast<const char*>(src) + at * eb, (size_t)p);
        } else if (p > 0) {
            const size_t base = out->size();
            out->resize(base + (size_t)p);
            uint8_t* o = reinterpret_cast<uint8_t*>(&(*out)[base]);
            for (uint64_t i = at; i < end; ++i) o += pb_rows::PutVarint(o, pb_rows::WireValue(src, i, kind));
        }
        at = end;
    }
    return 0;
}

// The way back, the host twin of gpu::DeviceSplitRows: one sequential walk of
// msg[0, n) that takes every occurrence of field `number` as a row
// (pb_rows::RowShape says which rows it takes) and skips every other
// top-level field, counted in *others: `Batch { string model = 1; repeated
// Row rows = 4; }` splits as it is. values_out gets the elements of all rows
// in the kind's vector layout (cap elements), row_ends_out[r] the elements in
// rows 0..r (row_cap entries). Returns
//   0  done; *count elements, *rows rows
//   1  malformed wire; *first_bad is the offset of the top-level field that
//      offends (a row whose payload is malformed: the row's tag)
//   2  refused: fields that pb_rows::FieldsOk refuses, a null pointer with a
//      nonzero size, n above 2^32-1
//   5  more than cap elements or row_cap rows: *count and *rows say what is
//      needed
//   6  well-formed, but a shape that is not split (field `number` with another
//      wire type, or a row RowShape calls unsupported); *first_bad as for 1
// The walk stops at the first offender, so 1 and 6 describe the lowest
// offending offset. Only 0 writes to the outputs. SerializeRows of what it
// returns gives back every canonical message of rows alone byte for byte.
inline int SplitRows(uint32_t number, uint32_t inner, uint32_t kind, const void* msg, uint64_t n, void* values_out,
                     uint64_t cap, uint32_t* row_ends_out, uint64_t row_cap, uint64_t* count, uint64_t* rows,
                     uint64_t* others, uint64_t* first_bad) {
    *count = *rows = *others = 0;
    *first_bad = ~0ull;
    if (!pb_rows::FieldsOk(number, inner, kind) || (n > 0 && !msg) || (cap > 0 && !values_out) ||
        (row_cap > 0 && !row_ends_out) || n > 0xFFFFFFFFull) {
        return pb_rows::kSplitRefused;
    }
    const uint8_t* b = static_cast<const uint8_t*>(msg);
    const bool varints = pb_rows::WireIsVarint(kind);
    const uint32_t eb = pb_rows::SourceBytes(kind);
    uint64_t nelems = 0, nrows = 0, nothers = 0;
    for (int pass = 0; pass < 2; ++pass) {  // count and validate, then write
        uint64_t at = 0, r = 0;
        for (uint64_t p = 0; p < n;) {
            const pb_rows::Field f = pb_rows::SpecField(b, p, n);
            int code = f.valid ? 0 : pb_rows::kSplitMalformed;
            uint64_t po = 0, pl = 0, ne = 0;
            const bool row = code == 0 && (f.tag >> 3) == number;
            if (row) {
                code = (f.tag & 7) != 2 ? pb_rows::kSplitUnsupported : pb_rows::RowShape(b, f.vpos, f.vlen, inner, kind, &po, &pl);
                if (code == 0 && varints && !pb_rows::VarintsOk(b + po, pl, &ne)) code = pb_rows::kSplitMalformed;
                if (code == 0 && !varints) ne = pl / eb;
            }
            if (code != 0) {
                *first_bad = p;
                return code;
            }
            if (!row) {
                nothers += pass == 0;
            } else if (pass == 0) {
                nelems += ne;
                ++nrows;
            } else {
                if (!varints) {
                    if (pl > 0) memcpy(static_cast<char*>(values_out) + at * eb, b + po, (size_t)pl);
                } else {
                    uint64_t v = 0, i = at;
                    uint32_t shift = 0;
                    for (uint64_t k = 0; k < pl; ++k) {
                        if (shift < 64) v |= (uint64_t)(b[po + k] & 0x7f) << shift;
                        shift += 7;
                        if (b[po + k] & 0x80) continue;
                        pb_rows::StoreVarintElem(values_out, i++, kind, v);
                        v = 0;
                        shift = 0;
                    }
                }
                at += ne;
                row_ends_out[r++] = (uint32_t)at;
            }
            p = f.next;
        }
        if (pass == 0) {
            *count = nelems;
            *rows = nrows;
            *others = nothers;
            if (nelems > cap || nrows > row_cap) return pb_rows::kSplitShort;
        }
    }
    return 0;
}

}  // namespace pb
}  // namespace mrpc
