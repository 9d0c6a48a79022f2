// Wire rules of a repeated sub-message with several fields, each field a
// column of a batch: `repeated Example examples = N` with
//   message Example { repeated int64 input_ids = 1 [packed = true];
//                     repeated float weights   = 2 [packed = true];
//                     optional int32 label     = 3;
//                     optional bytes blob      = 4; }
// On top of base/pb_rows.h (element kinds, wire values, varints) and, like
// it, compiled for the host (g++) and the device (hipcc): one set of rules
// behind pb::SerializeRecords (pb/records.h) and gpu::DeviceBuildRecords
// (gpu/pb_kernels.hip).
//
// A record job is the field number of the repeated field, rows >= 1 and 1 to
// kRecordMaxColumns columns, written into every record in the order given.
// A column is {inner, kind, src, count, row_ends}; its wire form follows from
// the kind and from whether it has row ends:
//   packed  kinds 0..6, 8, 9 with row_ends: varint(inner << 3 | 2) varint(p) P,
//           P the row's elements as DeviceBuildRows encodes them; omitted when
//           the row has no element (the host serializer omits an empty packed
//           field)
//   bytes   kind 7 with row_ends: varint(inner << 3 | 2) varint(p) P; an empty
//           one is tag 0x00 (present, as pb_rows::HasInner)
//   scalar  kinds 0..6, 8, 9 without row_ends, count == rows: kinds 0..6 are
//           varint(inner << 3 | 0) varint(WireValue), kind 8 is
//           varint(inner << 3 | 5) and 4 bytes, kind 9 varint(inner << 3 | 1)
//           and 8 bytes. Always written: explicit presence, a zero stays.
// Kind 7 without row_ends is refused. Record r is
//   varint(number << 3 | 2) varint(s) F0 F1 .. Fk-1
// with s the bytes of its fields; a record whose fields are all omitted is
// tag 0x00. A job of one packed (or one bytes) column is the pb_rows output
// for the same number / inner / kind byte for byte.
#pragma once

#include <cstddef>
#include <cstdint>

#include "base/pb_rows.h"

namespace mrpc {
namespace pb_records {

constexpr uint32_t kRecordMaxColumns = 8;
constexpr uint32_t kMaxFieldHeaderBytes = 10;  // a tag of 5 bytes, a length below 2^32
constexpr uint32_t kMaxRowHeaderBytes = 10;

struct Column {
    uint32_t inner = 0;  // the field inside the record, 1 .. 2^29-1 (numbers may repeat: the wire allows it)
    uint32_t kind = 0;   // base/pb_rows.h
    const void* src = nullptr;           // count elements in the kind's vector layout
    uint64_t count = 0;
    const uint32_t* row_ends = nullptr;  // rows entries; null: a scalar column, element r belongs to record r
};
struct Job {
    uint32_t number = 0;  // the repeated field, 1 .. 2^29-1
    const Column* columns = nullptr;
    uint32_t ncols = 0;
    uint64_t rows = 0;
};

// inner, kind and form a column may carry.
MRPC_ROWS_FN bool ColumnOk(uint32_t inner, uint32_t kind, bool scalar) {
    return inner >= 1 && inner <= pb_rows::kMaxFieldNumber && kind <= pb_rows::kKindFixed64 &&
           !(scalar && kind == pb_rows::kKindBytes);
}

MRPC_ROWS_FN uint32_t WireType(uint32_t kind, bool scalar) {
    if (!scalar) return 2;
    return kind <= pb_rows::kKindBool ? 0 : (kind == pb_rows::kKindFixed32 ? 5 : 1);
}

// Whether a record carries the column's field when the row's payload is p
// bytes (an element takes at least one byte, so p == 0 is a row without one).
MRPC_ROWS_FN bool HasField(uint32_t kind, bool scalar, uint64_t p) {
    return scalar || kind == pb_rows::kKindBytes || p > 0;
}

// Bytes in front of the field's payload of p bytes; 0 when it is omitted.
MRPC_ROWS_FN uint32_t FieldHeaderBytes(uint32_t inner, uint32_t kind, bool scalar, uint64_t p) {
    if (!HasField(kind, scalar, p)) return 0;
    const uint32_t tag = pb_rows::VarintLen((uint64_t)inner << 3);
    return scalar ? tag : tag + pb_rows::VarintLen(p);
}

// Writes them (at most kMaxFieldHeaderBytes); returns FieldHeaderBytes().
MRPC_ROWS_FN uint32_t PutFieldHeader(uint8_t* o, uint32_t inner, uint32_t kind, bool scalar, uint64_t p) {
    if (!HasField(kind, scalar, p)) return 0;
    const uint32_t n = pb_rows::PutVarint(o, ((uint64_t)inner << 3) | WireType(kind, scalar));
    return scalar ? n : n + pb_rows::PutVarint(o + n, p);
}

// The record's own header in front of s bytes of fields.
MRPC_ROWS_FN uint32_t RowHeaderBytes(uint32_t number, uint64_t s) {
    return pb_rows::VarintLen((uint64_t)number << 3) + pb_rows::VarintLen(s);
}
MRPC_ROWS_FN uint32_t PutRowHeader(uint8_t* o, uint32_t number, uint64_t s) {
    const uint32_t n = pb_rows::PutVarint(o, ((uint64_t)number << 3) | 2);
    return n + pb_rows::PutVarint(o + n, s);
}

// number, column count and every column's inner / kind / form; a scalar
// column holds one element per record.
MRPC_ROWS_FN bool FieldsOk(const Job& job) {
    if (job.number < 1 || job.number > pb_rows::kMaxFieldNumber || !job.columns || job.ncols < 1 ||
        job.ncols > kRecordMaxColumns) {
        return false;
    }
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const Column& col = job.columns[c];
        const bool scalar = col.row_ends == nullptr;
        if (!ColumnOk(col.inner, col.kind, scalar) || (scalar && col.count != job.rows)) return false;
    }
    return true;
}

// Most bytes the job's records can take for any values; 0 when the job is
// refused, there is no row, or a count, rows or the total is above 2^32 - 1.
MRPC_ROWS_FN uint64_t WorstCaseBytes(const Job& job) {
    if (!FieldsOk(job) || job.rows == 0 || job.rows > 0xFFFFFFFFull) return 0;
    uint64_t pay = 0, per_row = 0;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const Column& col = job.columns[c];
        if (col.count > 0xFFFFFFFFull) return 0;
        const uint64_t p = col.count * pb_rows::MaxWireBytes(col.kind);
        pay += p;
        per_row += pb_rows::VarintLen((uint64_t)col.inner << 3) + (col.row_ends ? pb_rows::VarintLen(p) : 0);
    }
    // a record's length is below pay + per_row
    per_row += pb_rows::VarintLen((uint64_t)job.number << 3) + pb_rows::VarintLen(pay + per_row);
    const uint64_t total = pay + job.rows * per_row;
    return total > 0xFFFFFFFFull ? 0 : total;
}

}  // namespace pb_records
}  // namespace mrpc
