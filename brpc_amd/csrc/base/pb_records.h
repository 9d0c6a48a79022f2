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
// for the same number / inner / kind byte for byte, and the device builds it
// as one: gpu::DeviceBuildRows runs a one-column record job.
//
// The headerless column: inner == 0, kind bytes, ragged, the job's only
// column. Its payload follows the record header with no field header in
// between (HasFieldHeader), so record r is varint(number << 3 | 2) varint(p)
// P: pb_rows' `repeated bytes`. Only the header rules below know it.
// ColumnOk, FieldsOk, WorstCaseBytes and SplitColumnsOk refuse inner == 0, so
// no caller of pb::SerializeRecords, DeviceBuildRecords or a splitter can
// pass one; the rows entry point does, behind pb_rows::WorstCaseBytes.
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

// Whether a tag (and, for a ragged column, a length) stands in front of the
// field's payload: not when the field is omitted, and never for the
// headerless column.
MRPC_ROWS_FN bool HasFieldHeader(uint32_t inner, uint32_t kind, bool scalar, uint64_t p) {
    return inner != 0 && HasField(kind, scalar, p);
}

// Bytes in front of the field's payload of p bytes; 0 when there is none.
MRPC_ROWS_FN uint32_t FieldHeaderBytes(uint32_t inner, uint32_t kind, bool scalar, uint64_t p) {
    if (!HasFieldHeader(inner, kind, scalar, p)) return 0;
    const uint32_t tag = pb_rows::VarintLen((uint64_t)inner << 3);
    return scalar ? tag : tag + pb_rows::VarintLen(p);
}

// Writes them (at most kMaxFieldHeaderBytes); returns FieldHeaderBytes().
MRPC_ROWS_FN uint32_t PutFieldHeader(uint8_t* o, uint32_t inner, uint32_t kind, bool scalar, uint64_t p) {
    if (!HasFieldHeader(inner, kind, scalar, p)) return 0;
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

// ---- the way back: a message that holds such records, split into the
// columns again (pb::SplitRecords in pb/records.h, gpu::DeviceSplitRecords).
// The codes are pb_rows' (kSplitMalformed 1, kSplitRefused 2, kSplitShort 5,
// kSplitUnsupported 6).
//
// A split column is {inner, kind, scalar}. Column numbers must be distinct:
// the builder allows repeats, the splitter cannot attribute them, and as it
// cannot tell a packed form from an unpacked one either, one number must not
// appear with two wire forms. SplitColumnsOk refuses duplicates (code 2).
struct SplitColumn {
    uint32_t inner = 0;
    uint32_t kind = 0;
    uint32_t scalar = 0;  // 1: one element per record, no row ends
};

MRPC_ROWS_FN bool SplitColumnsOk(uint32_t number, const SplitColumn* cols, uint32_t ncols) {
    if (number < 1 || number > pb_rows::kMaxFieldNumber || !cols || ncols < 1 || ncols > kRecordMaxColumns) return false;
    for (uint32_t c = 0; c < ncols; ++c) {
        if (!ColumnOk(cols[c].inner, cols[c].kind, cols[c].scalar != 0)) return false;
        for (uint32_t d = 0; d < c; ++d) {
            if (cols[d].inner == cols[c].inner) return false;
        }
    }
    return true;
}

// The verdict on one record whose value is b[v, v + s): 0, 1 or 6. For every
// field that column c takes, take(c, offset, bytes) is called with the place
// of its payload (a ragged column) or of its value (a scalar: the varint, or
// the 4 or 8 bytes); a column that is never taken is absent from the record.
//   - a field pb_rows::SpecField calls invalid makes the record 1;
//   - a field is taken by column c when its number is the column's inner, its
//     wire type is WireType(kind, scalar) and c was not taken earlier in this
//     record; fields may come in any order;
//   - a taken ragged payload of a fixed kind (or of bytes) must be whole
//     elements, one of a varint kind must end in a byte without a
//     continuation bit; a breach makes the record 1;
//   - every other well-formed field (an unknown number, a column's number
//     with another wire type, which is an unpacked repeated field, a column
//     taken twice) makes the record 6, unless something in it is 1.
// take() is called for the taken fields of a record that is 6 too (and for
// those in front of the offender of one that is 1): whether a taken varint
// payload holds only varints the packed-run decoder takes is
// pb_rows::VarintsOk on the host and the check pass on the device, both of
// which must see the payloads of a record that has both faults (it is 1).
// An absent ragged column is a row of no element, an absent bytes field and
// an empty one are the same row, an absent scalar reads as 0 (the proto3 rule
// and the proto2 default) and is counted; an empty record is valid.
// The walk reads only b[v, v + s) and takes at most s / 2 steps: both of
// SpecField's invariants hold with the record's end in the place of n.
template <typename Take>
MRPC_ROWS_FN int RecordShape(const uint8_t* b, uint64_t v, uint64_t s, const SplitColumn* cols, uint32_t ncols,
                             Take&& take) {
    const uint64_t end = v + s;
    uint32_t taken = 0;
    int code = 0;
    for (uint64_t p = v; p < end;) {
        const pb_rows::Field f = pb_rows::SpecField(b, p, end);
        if (!f.valid) return pb_rows::kSplitMalformed;
        const uint32_t number = f.tag >> 3, wire = f.tag & 7;
        uint32_t c = 0;
        while (c < ncols && cols[c].inner != number) ++c;
        if (c == ncols || wire != WireType(cols[c].kind, cols[c].scalar != 0) || (taken >> c & 1)) {
            code = pb_rows::kSplitUnsupported;
        } else if (cols[c].scalar) {
            // the value ends the field; a varint's tag may be over-long, so its end is parsed again
            uint64_t at = f.next - (wire == 1 ? 8 : 4);
            if (wire == 0) {
                uint32_t tn = 0;
                uint64_t tag = 0;
                pb_rows::GetVarint(b + p, end - p, &tn, &tag);
                at = p + tn;
            }
            taken |= 1u << c;
            take(c, at, f.next - at);
        } else {
            if (pb_rows::WireIsVarint(cols[c].kind)) {
                if (f.vlen > 0 && (b[f.vpos + f.vlen - 1] & 0x80)) return pb_rows::kSplitMalformed;
            } else if (f.vlen % pb_rows::SourceBytes(cols[c].kind)) {
                return pb_rows::kSplitMalformed;
            }
            taken |= 1u << c;
            take(c, f.vpos, f.vlen);
        }
        p = f.next;
    }
    return code;
}

}  // namespace pb_records
}  // namespace mrpc
