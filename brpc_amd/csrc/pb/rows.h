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

}  // namespace pb
}  // namespace mrpc
