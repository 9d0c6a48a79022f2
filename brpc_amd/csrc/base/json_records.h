// Records as a JSON array of objects, each field a column of a batch:
//   [{"label":3,"ids":[1,2],"scores":[0.5,0.25],"text":"..."}, ...]
// compiled for the host (g++) and the device (hipcc): one set of rules behind
// json::FormatRecordObjects (json/json.h) and gpu::DevicePrintRecordObjects
// (gpu/json_records_kernels.hip). Nothing here formats a value by itself: a
// number is base/number_print.h and base/shortest_double.h, a string byte is
// json_string::EscapeByte, three bytes of a blob are base64::Encode3.
//
// A job is `rows` records over 1 to kMaxColumns columns, the columns of
// base/pb_records.h with a key in the place of a field number. A column is
// {key, key_len, kind, text, src, count, row_ends}; the cell of record r is
//   scalar   kinds 0..6, 8, 9 (number_print::Kind) without row_ends, count ==
//            rows: element r as DevicePrintNumbers prints it (a non-finite
//            float as the quoted "NaN" / "Infinity" / "-Infinity")
//   numbers  the same kinds with row_ends: [v,v,...,v], [] for a row of no
//            element
//   string   kind 7 with row_ends, text kString: '"', the row's bytes through
//            EscapeByte, '"'. No UTF-8 verdict, as with the escaper.
//   base64   kind 7 with row_ends, text kBase64: '"', the padded canonical
//            base64 of the row, '"'
// Empty rows are legal. Row r of a ragged column is [row_ends[r - 1],
// row_ends[r]) (row_ends[-1] = 0); a table is bad at a row whose end lies
// below its predecessor or above `count`, and at the last row when its end is
// not `count`.
//
// Record r is {"k0":cell,"k1":cell,...}: every key in every record, in column
// order, nothing omitted. Records are joined by ',' and, with `brackets`,
// wrapped in '[' ']'. No whitespace. No row: "[]" or nothing.
//
// Keys are raw bytes. They are escaped once per job (EscapeByte, what
// json::EscapeStringBody writes) into the column's fixed prefix: {"k": for
// column 0, ,"k": behind it. An escaped key above kMaxEscapedKey bytes and two
// equal keys in one job are refused.
//
// Verdicts, in this order: 2 refused (before anything is read), 1 a bad
// table (the lowest offending row over all columns, then the lowest column
// that offends there), 3 longer than the capacity, 4 a source or table
// changed between the device's passes. 1 wins over 3.
#pragma once

#include <cstddef>
#include <cstdint>

#include "base/base64.h"
#include "base/json_string.h"
#include "base/number_print.h"
#include "base/pb_records.h"
#include "base/shortest_double.h"

namespace mrpc {
namespace json_records {

constexpr uint32_t kMaxColumns = pb_records::kRecordMaxColumns;
constexpr uint32_t kKindBytes = 7;  // pb_rows::kKindBytes: one source byte per element
enum Text : uint32_t { kNumber = 0, kString = 1, kBase64 = 2 };  // kNumber: every kind but 7
constexpr uint32_t kMaxEscapedKey = 255;
constexpr uint32_t kMaxPrefixBytes = kMaxEscapedKey + 4;  // {" or ," in front, ": behind
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kKindBytes == pb_rows::kKindBytes, "the byte kind of the record builder");

struct Column {
    const void* key = nullptr;  // key_len raw bytes
    uint32_t key_len = 0;
    uint32_t kind = 0;
    uint32_t text = kNumber;
    const void* src = nullptr;  // count elements, naturally aligned
    uint64_t count = 0;
    const uint32_t* row_ends = nullptr;  // rows entries; null: a scalar column
};
struct Job {
    const Column* columns = nullptr;
    uint32_t ncols = 0;
    uint64_t rows = 0;
    bool brackets = false;
};

// kind, text form and shape a column may carry.
MRPC_SD_FN bool ColumnOk(uint32_t kind, uint32_t text, bool scalar) {
    if (kind == kKindBytes) return !scalar && (text == kString || text == kBase64);
    return number_print::KindValid(kind) && text == kNumber;
}
// Bytes of one source element, also its alignment.
MRPC_SD_FN uint32_t ElemBytes(uint32_t kind) { return kind == kKindBytes ? 1u : number_print::ElemBytes(kind); }

// Column count and every column's kind / text / shape; a scalar column holds
// one element per record.
MRPC_SD_FN bool FieldsOk(const Job& job) {
    if (!job.columns || job.ncols < 1 || job.ncols > kMaxColumns) return false;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const Column& col = job.columns[c];
        const bool scalar = col.row_ends == nullptr;
        if (!ColumnOk(col.kind, col.text, scalar) || (scalar && col.count != job.rows)) return false;
    }
    return true;
}

// Whether row r of a ragged column breaks the table rule: prev = row_ends[r -
// 1] (0 for r = 0), end = row_ends[r].
MRPC_SD_FN bool RowEndBad(uint32_t prev, uint32_t end, uint64_t r, uint64_t rows, uint64_t count) {
    return end < prev || end > count || (r + 1 == rows && end != count);
}

// ---- keys and prefixes
MRPC_SD_FN uint64_t EscapedKeyBytes(const uint8_t* key, uint32_t n) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; ++i) s += json_string::EscapedSize(key[i]);
    return s;
}
// Bytes of a column's prefix around an escaped key of `escaped` bytes.
MRPC_SD_FN uint32_t PrefixBytes(uint32_t escaped) { return escaped + 4; }
// Writes the prefix of column c (room for kMaxPrefixBytes) around the
// already escaped key; returns PrefixBytes(escaped).
MRPC_SD_FN uint32_t PutPrefix(uint32_t c, const char* escaped_key, uint32_t escaped, uint8_t* out) {
    out[0] = c == 0 ? '{' : ',';
    out[1] = '"';
    for (uint32_t i = 0; i < escaped; ++i) out[2 + i] = (uint8_t)escaped_key[i];
    out[2 + escaped] = '"';
    out[3 + escaped] = ':';
    return escaped + 4;
}

// ---- sizes
// What every record takes besides its cells: the prefixes and '}'.
MRPC_SD_FN uint64_t RecordFixedBytes(uint64_t prefix_bytes) { return prefix_bytes + 1; }
// The punctuation in front of record r (',' or the outer '[') and behind it
// (the outer ']' behind the last).
MRPC_SD_FN uint32_t LeadBytes(uint64_t r, bool brackets) { return r > 0 || brackets ? 1u : 0u; }
MRPC_SD_FN uint32_t TrailBytes(uint64_t r, uint64_t rows, bool brackets) { return brackets && r + 1 == rows ? 1u : 0u; }
// A cell is its inner bytes and, unless the column is scalar, two wrappers:
// [ ] or " ".
MRPC_SD_FN uint32_t WrapperBytes(bool scalar) { return scalar ? 0u : 2u; }
// Inner bytes of a number row of n elements whose texts sum to `text`.
MRPC_SD_FN uint32_t NumberRowInner(uint32_t text, uint32_t n) { return text + (n ? n - 1 : 0u); }
// Inner bytes of a base64 cell of a row of `len` bytes: no element pass.
MRPC_SD_FN uint32_t Base64Inner(uint32_t len) { return 4 * ((len + 2) / 3); }
MRPC_SD_FN uint32_t Base64CellBytes(uint32_t len) { return 2 + Base64Inner(len); }

// Text bytes of element i of a number column (kNumber) or of byte i of a
// string column.
MRPC_SD_FN uint32_t ElemTextBytes(const void* src, uint64_t i, uint32_t kind) {
    namespace np = number_print;
    namespace sd = shortest_double;
    if (kind == kKindBytes) return json_string::EscapedSize(static_cast<const uint8_t*>(src)[i]);
    if (kind == np::kBool) return np::BoolLength(static_cast<const uint8_t*>(src)[i] != 0);
    if (kind == np::kFloat32)
        return (uint32_t)sd::JsonDecimalLength(sd::ShortestDigits(sd::WidenFloatBits(static_cast<const uint32_t*>(src)[i])));
    if (kind == np::kFloat64) return (uint32_t)sd::JsonDecimalLength(sd::ShortestDigits(static_cast<const uint64_t*>(src)[i]));
    return np::IntegerLength(np::LoadInteger(src, i, kind));
}
// Writes them (at most number_print::kMaxElemChars); returns their number.
MRPC_SD_FN uint32_t FormatElem(const void* src, uint64_t i, uint32_t kind, char* out) {
    namespace np = number_print;
    namespace sd = shortest_double;
    if (kind == kKindBytes) return json_string::EscapeByte(static_cast<const uint8_t*>(src)[i], out);
    if (kind == np::kBool) return np::FormatBool(static_cast<const uint8_t*>(src)[i] != 0, out);
    if (kind == np::kFloat32)
        return (uint32_t)sd::FormatJsonDoubleBits(sd::WidenFloatBits(static_cast<const uint32_t*>(src)[i]), out);
    if (kind == np::kFloat64) return (uint32_t)sd::FormatJsonDoubleBits(static_cast<const uint64_t*>(src)[i], out);
    return np::FormatInteger(np::LoadInteger(src, i, kind), out);
}
// The four symbols of the group that begins at byte k (a multiple of 3) of a
// row of `len` bytes, k < len, '=' where the row has no byte: the first
// symbol in the low byte.
MRPC_SD_FN uint32_t Base64Group(const uint8_t* row, uint32_t k, uint32_t len) {
    const uint32_t left = len - k;
    const uint32_t v24 = (uint32_t)row[k] << 16 | (left > 1 ? (uint32_t)row[k + 1] << 8 : 0u) |
                         (left > 2 ? (uint32_t)row[k + 2] : 0u);
    uint32_t s = base64::Encode3(v24);
    if (left < 3) s = (s & 0x00FFFFFFu) | (uint32_t)'=' << 24;
    if (left < 2) s = (s & 0x0000FFFFu) | (uint32_t)'=' << 16 | (uint32_t)'=' << 24;
    return s;
}

// Most bytes the job's text can take for any values and any table;
// prefix_bytes: the prefixes of all columns together. It always suffices as a
// cap. 0 when the job is refused; ~0 when a count, rows or the total is above
// 2^32 - 1. A number element takes at most MaxElemChars and a comma, a string
// byte at most 6, a blob the base64 formula (rounding up once per row), and a
// ragged cell two wrappers.
MRPC_SD_FN uint64_t WorstCaseBytes(const Job& job, uint64_t prefix_bytes) {
    if (!FieldsOk(job)) return 0;
    if (job.rows == 0) return job.brackets ? 2 : 0;
    if (job.rows > 0xFFFFFFFFull) return ~0ull;
    uint64_t pay = 0, per_row = RecordFixedBytes(prefix_bytes) + 1;  // the ',' or a bracket
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const Column& col = job.columns[c];
        if (col.count > 0xFFFFFFFFull) return ~0ull;
        if (col.text == kString) pay += 6 * col.count;
        else if (col.text == kBase64) pay += 4 * (col.count / 3) + 4 * job.rows;  // sum of ceil <= floor of sum + rows
        else pay += col.count * (number_print::MaxElemChars(col.kind) + 1);
        per_row += WrapperBytes(col.row_ends == nullptr);
    }
    const uint64_t total = pay + job.rows * per_row + 1;
    return total > 0xFFFFFFFFull ? ~0ull : total;
}

}  // namespace json_records
}  // namespace mrpc
