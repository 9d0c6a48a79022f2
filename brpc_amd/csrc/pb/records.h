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

// The way back, the host twin of gpu::DeviceSplitRecords: one sequential walk
// of msg[0, n) that takes every occurrence of field `number` with wire type 2
// as a record (pb_records::RecordShape says which records it takes) and skips
// every other top-level field, counted in `others`; field `number` with
// another wire type is 6.
struct SplitRecordsColumn {
    uint32_t inner = 0, kind = 0;
    bool scalar = false;
    void* values = nullptr;        // cap elements in the kind's vector layout; a scalar column: one per record
    uint64_t cap = 0;
    uint32_t* row_ends = nullptr;  // ragged columns: row_cap entries, row_ends[r] = the elements in records 0..r
    // out
    uint64_t count = 0;   // elements (a scalar column: the records)
    uint64_t absent = 0;  // scalar columns: the records without the field, whose element is 0
};
struct SplitRecordsJob {
    uint32_t number = 0;
    SplitRecordsColumn* columns = nullptr;
    uint32_t ncols = 0;
    const void* msg = nullptr;
    uint64_t n = 0;
    uint64_t row_cap = 0;  // one value for every ragged column
    // out
    uint64_t rows = 0, others = 0, first_bad = ~0ull;
};
// Returns
//   0  done
//   1  malformed wire; first_bad is the offset of the top-level field that
//      offends (for a fault inside a record: the record's tag)
//   2  refused: a bad number, inner or kind, a bytes column flagged scalar,
//      ncols 0 or above 8, a duplicate inner, a null pointer with a nonzero
//      size, n above 2^32-1
//   5  rows > row_cap, or some column's count above its cap (a scalar
//      column's count is rows). rows is always exact; the column counts are
//      exact when rows <= row_cap and all 0 otherwise, which lets the device
//      keep a record table sized by row_cap
//   6  well-formed wire of a shape that is not split; first_bad as for 1
// The walk stops at the lowest offender, and 1 and 6 win over 5. A record
// that is both 6 and 1 is 1. Only 0 writes to values and row_ends.
// SerializeRecords of what it returns gives back every canonical
// SerializeRecords output byte for byte.
inline int SplitRecords(SplitRecordsJob* job) {
    job->rows = job->others = 0;
    job->first_bad = ~0ull;
    pb_records::SplitColumn cols[pb_records::kRecordMaxColumns];
    if (!job->columns || job->ncols < 1 || job->ncols > pb_records::kRecordMaxColumns) return pb_rows::kSplitRefused;
    const uint32_t ncols = job->ncols;
    for (uint32_t c = 0; c < ncols; ++c) {
        SplitRecordsColumn& col = job->columns[c];
        col.count = col.absent = 0;
        cols[c].inner = col.inner;
        cols[c].kind = col.kind;
        cols[c].scalar = col.scalar;
    }
    if (!pb_records::SplitColumnsOk(job->number, cols, ncols) || (job->n > 0 && !job->msg) || job->n > 0xFFFFFFFFull) {
        return pb_rows::kSplitRefused;
    }
    for (uint32_t c = 0; c < ncols; ++c) {
        const SplitRecordsColumn& col = job->columns[c];
        if ((col.cap > 0 && !col.values) || (!col.scalar && job->row_cap > 0 && !col.row_ends)) return pb_rows::kSplitRefused;
    }
    const uint8_t* b = static_cast<const uint8_t*>(job->msg);
    const uint64_t n = job->n;
    uint64_t counts[pb_records::kRecordMaxColumns] = {0}, absent[pb_records::kRecordMaxColumns] = {0};
    uint64_t nrows = 0, nothers = 0;
    for (int pass = 0; pass < 2; ++pass) {  // count and validate, then write
        uint64_t at[pb_records::kRecordMaxColumns] = {0};
        uint64_t r = 0;
        for (uint64_t p = 0; p < n;) {
            const pb_rows::Field f = pb_rows::SpecField(b, p, n);
            int code = f.valid ? 0 : pb_rows::kSplitMalformed;
            const bool record = code == 0 && (f.tag >> 3) == job->number;
            uint64_t off[pb_records::kRecordMaxColumns], len[pb_records::kRecordMaxColumns];
            uint32_t taken = 0;
            if (record && (f.tag & 7) != 2) code = pb_rows::kSplitUnsupported;
            if (record && code == 0) {
                code = pb_records::RecordShape(b, f.vpos, f.vlen, cols, ncols, [&](uint32_t c, uint64_t o, uint64_t l) {
                    taken |= 1u << c;
                    off[c] = o;
                    len[c] = l;
                });
                // also of a record that is 6: one with both faults is 1
                for (uint32_t c = 0; c < ncols && code != pb_rows::kSplitMalformed && pass == 0; ++c) {
                    uint64_t ne = 0;
                    if ((taken >> c & 1) && !cols[c].scalar && pb_rows::WireIsVarint(cols[c].kind) &&
                        !pb_rows::VarintsOk(b + off[c], len[c], &ne)) {
                        code = pb_rows::kSplitMalformed;
                    }
                }
            }
            if (code != 0) {
                job->first_bad = p;
                return code;
            }
            if (!record) {
                nothers += pass == 0;
                p = f.next;
                continue;
            }
            for (uint32_t c = 0; c < ncols; ++c) {
                const SplitRecordsColumn& col = job->columns[c];
                const bool has = taken >> c & 1;
                const uint32_t eb = pb_rows::SourceBytes(col.kind);
                if (col.scalar) {
                    if (pass == 0) {
                        absent[c] += !has;
                        continue;
                    }
                    if (!has) {
                        memset(static_cast<char*>(col.values) + r * eb, 0, eb);
                    } else if (pb_rows::WireIsVarint(col.kind)) {
                        uint32_t used = 0;
                        uint64_t raw = 0;
                        pb_rows::GetVarint(b + off[c], len[c], &used, &raw);
                        pb_rows::StoreVarintElem(col.values, r, col.kind, raw);
                    } else {
                        memcpy(static_cast<char*>(col.values) + r * eb, b + off[c], eb);
                    }
                    continue;
                }
                const uint64_t pl = has ? len[c] : 0;
                uint64_t ne = pl / eb;
                if (pb_rows::WireIsVarint(col.kind)) {
                    ne = 0;
                    if (pl > 0) pb_rows::VarintsOk(b + off[c], pl, &ne);
                }
                if (pass == 0) {
                    counts[c] += ne;
                    continue;
                }
                if (!pb_rows::WireIsVarint(col.kind)) {
                    if (pl > 0) memcpy(static_cast<char*>(col.values) + at[c] * eb, b + off[c], (size_t)pl);
                } else {
                    uint64_t val = 0, i = at[c];
                    uint32_t shift = 0;
                    for (uint64_t k = 0; k < pl; ++k) {
                        const uint8_t byte = b[off[c] + k];
                        if (shift < 64) val |= (uint64_t)(byte & 0x7f) << shift;
                        shift += 7;
                        if (byte & 0x80) continue;
                        pb_rows::StoreVarintElem(col.values, i++, col.kind, val);
                        val = 0;
                        shift = 0;
                    }
                }
                at[c] += ne;
                col.row_ends[r] = (uint32_t)at[c];
            }
            if (pass == 0) ++nrows;
            ++r;
            p = f.next;
        }
        if (pass == 0) {
            job->rows = nrows;
            job->others = nothers;
            if (nrows > job->row_cap) return pb_rows::kSplitShort;
            bool fits = true;
            for (uint32_t c = 0; c < ncols; ++c) {
                SplitRecordsColumn& col = job->columns[c];
                col.count = col.scalar ? nrows : counts[c];
                col.absent = col.scalar ? absent[c] : 0;
                fits = fits && col.count <= col.cap;
            }
            if (!fits) return pb_rows::kSplitShort;
        }
    }
    return 0;
}

}  // namespace pb
}  // namespace mrpc
