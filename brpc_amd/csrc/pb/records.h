// The host twin of gpu::DeviceBuildRecords (gpu/device_codec.h): the
// occurrences of one repeated sub-message with several fields, each field a
// column of host arrays, appended to a string. The rules are
// base/pb_records.h, the code the device kernels run; this is the oracle of
// their tests and what a caller falls back to when the device declined a job.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "base/pb_records.h"

namespace mrpc {
namespace pb {

// One sequential walk. Returns 0 and appends the bytes; 1 when some column's
// row_ends decreases or its last entry is not that column's count
// (*first_bad: the lowest such row over all columns, *bad_column: the lowest
// column that offends at that row); 2 when the job is refused (as the device
// entry refuses it). Nothing is appended on 1 or 2.
inline int SerializeRecords(const pb_records::Job& job, std::string* out, uint32_t* first_bad = nullptr,
                            uint32_t* bad_column = nullptr) {
    if (first_bad) *first_bad = 0xFFFFFFFFu;
    if (bad_column) *bad_column = 0xFFFFFFFFu;
    if (!out || pb_records::WorstCaseBytes(job) == 0) return 2;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        if (job.columns[c].count > 0 && !job.columns[c].src) return 2;
    }
    uint64_t bad_row = ~0ull;
    uint32_t bad_col = 0;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const pb_records::Column& col = job.columns[c];
        if (!col.row_ends) continue;
        uint64_t prev = 0;
        for (uint64_t r = 0; r < job.rows && r < bad_row; ++r) {
            if (col.row_ends[r] < prev || (r + 1 == job.rows && col.row_ends[r] != col.count)) {
                bad_row = r;
                bad_col = c;
                break;
            }
            prev = col.row_ends[r];
        }
    }
    if (bad_row != ~0ull) {
        if (first_bad) *first_bad = (uint32_t)bad_row;
        if (bad_column) *bad_column = bad_col;
        return 1;
    }
    uint64_t pay[pb_records::kRecordMaxColumns];
    for (uint64_t r = 0; r < job.rows; ++r) {
        uint64_t s = 0;
        for (uint32_t c = 0; c < job.ncols; ++c) {
            const pb_records::Column& col = job.columns[c];
            const uint64_t at = col.row_ends ? (r ? col.row_ends[r - 1] : 0) : r;
            const uint64_t end = col.row_ends ? col.row_ends[r] : r + 1;
            uint64_t p = 0;
            for (uint64_t i = at; i < end; ++i) p += pb_rows::WireBytes(pb_rows::WireValue(col.src, i, col.kind), col.kind);
            pay[c] = p;
            s += p + pb_records::FieldHeaderBytes(col.inner, col.kind, !col.row_ends, p);
        }
        uint8_t head[pb_records::kMaxRowHeaderBytes];
        out->append(reinterpret_cast<const char*>(head), pb_records::PutRowHeader(head, job.number, s));
        for (uint32_t c = 0; c < job.ncols; ++c) {
            const pb_records::Column& col = job.columns[c];
            const uint64_t at = col.row_ends ? (r ? col.row_ends[r - 1] : 0) : r;
            const uint64_t end = col.row_ends ? col.row_ends[r] : r + 1;
            out->append(reinterpret_cast<const char*>(head),
                        pb_records::PutFieldHeader(head, col.inner, col.kind, !col.row_ends, pay[c]));
            if (pay[c] == 0) continue;
            const size_t base = out->size();
            out->resize(base + (size_t)pay[c]);
            uint8_t* o = reinterpret_cast<uint8_t*>(&(*out)[base]);
            if (pb_rows::IsVarintKind(col.kind)) {
                for (uint64_t i = at; i < end; ++i) o += pb_rows::PutVarint(o, pb_rows::WireValue(col.src, i, col.kind));
            } else if (col.kind == pb_rows::kKindBool) {  // normalized to 0 / 1
                for (uint64_t i = at; i < end; ++i) *o++ = (uint8_t)pb_rows::WireValue(col.src, i, col.kind);
            } else {
                memcpy(o, static_cast<const char*>(col.src) + at * pb_rows::SourceBytes(col.kind), (size_t)pay[c]);
            }
        }
    }
    return 0;
}

}  // namespace pb
}  // namespace mrpc
