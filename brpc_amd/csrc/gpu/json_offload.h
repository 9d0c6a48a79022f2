// GPU structural index for large JSON bodies (see json_offload.cc):
// installs gpu::JsonIndex behind json2pb's SetJsonIndexOffload for bodies of
// at least min_bytes, so http+json and json2pb parses cut strings at
// device-found quotes instead of scanning them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mrpc {
namespace gpu {

int EnableGpuJsonIndex(int device, size_t min_bytes, std::string* error = nullptr);
void DisableGpuJsonIndex();

// Synchronous structural index of host bytes on `device` (fiber-friendly
// wait): ascending offsets of unescaped quotes and of {}[]:, outside
// strings. -1 on a device error or an unterminated string.
int JsonIndex(const char* data, size_t n, std::vector<uint32_t>* out, int device);

// ---- float / double arrays as JSON text (the reference prints them element
// by element on the host, src/json2pb/pb_to_json.cpp). Each element is
// printed exactly as json::Value prints a double (a float is widened first;
// "NaN" / "Infinity" / "-Infinity" quoted), elements joined by ',' with no
// brackets; the formatter is base/shortest_double.h, the one pb2json's host
// printer runs.
constexpr uint32_t kJsonFloat32 = 8, kJsonFloat64 = 9;  // json2pb::kArrayKindFloat / kArrayKindDouble
struct DeviceFloatPrintJob {
    const void* src = nullptr;  // device or pinned host; naturally aligned (4 / 8 bytes)
    uint64_t count = 0;         // elements
    uint32_t kind = 0;          // kJsonFloat32 or kJsonFloat64
    void* dst = nullptr;        // device-writable, cap bytes
    uint64_t cap = 0;
    uint64_t len = 0;  // out: text size (with err 3: the size it needs)
    // out, the codes of DeviceMessageJob: 0 printed; 2 refused before any
    // launch (null src or dst with count > 0, bad kind, misaligned src, a
    // worst case above 2^32-1 bytes); 3 longer than cap (dst untouched); 4 a
    // chunk's text was not the size measured for it (nothing of it written)
    int err = 0;
};
// Most bytes `count` elements can take (25 per element and the commas
// between them); 0 for count 0.
uint64_t FloatPrintWorstCaseBytes(uint64_t count);
// All jobs share three launches on a pool stream (size, prefix, place; no
// host size pass: an element's size is known once it is formatted) and one
// fiber-friendly wait. Returns -1 only on a device error; per-job codes in
// jobs[i].err. A job of count 0 prints nothing (len 0, err 0).
int DevicePrintFloatArrays(DeviceFloatPrintJob* jobs, int n, int device);
// Host values -> *out through the device, the shape of EncodeRunOnDevice:
// the values are staged in pinned memory, the text is written to pinned
// memory by the place pass, one wait. 0 on success (then *out holds exactly
// the text), -1 on a bad argument or a device error (*out unchanged).
int PrintFloatsOnDevice(const void* values, size_t n, uint32_t kind, std::string* out, int device);

// ---- JSON number arrays parsed on the device, the inverse of the printer
// above (the reference converts every element on the host through
// rapidjson). Element i is the text between separators seps[i] and
// seps[i+1] (a separator of 0xFFFFFFFF stands for one before the first
// byte), trimmed of JSON whitespace and converted by
// base/decimal_to_double.h exactly as json::Reader converts it.
constexpr uint32_t kJsonParseNumbers = 0, kJsonParseFloat64 = 1, kJsonParseFloat32 = 2;  // gpu::JSON_PARSE_*
struct DeviceNumberParseJob {
    const char* text = nullptr;      // device or pinned host
    const uint32_t* seps = nullptr;  // count + 1 offsets into text, ascending; device or pinned host
    uint64_t count = 0;              // elements
    uint32_t mode = 0;
    // kJsonParseNumbers: 8 bytes of payload per element and a class byte in
    // `classes` (0 int64, 1 uint64 above INT64_MAX, 2 the bits of a double).
    // kJsonParseFloat64 / kJsonParseFloat32: a plain array of double / float
    // (an integer class becomes the double of its value, so "-0" is +0.0;
    // float32 is (float) of the double, as json2pb narrows it).
    void* out = nullptr;         // device-writable, 8-byte aligned (4 for float32)
    uint8_t* classes = nullptr;  // kJsonParseNumbers only
    // elements the device does not decide (more than 19 significant digits
    // whose truncation leaves the rounding open, or a text longer than
    // decimal_to_double::kMaxDeviceNumberChars): nothing is written to out
    // for them, their indices are listed here in no particular order
    uint32_t* redo = nullptr;  // redo_cap entries, device-writable
    uint32_t redo_cap = 0;
    uint32_t n_redo = 0;              // out: how many there are (also beyond redo_cap)
    uint32_t first_bad = 0xFFFFFFFFu;  // out: lowest index of a malformed element
    // out: 0 parsed; 1 a malformed element (trust nothing of out); 2 refused
    // before any launch (null pointers with count > 0, bad mode, misaligned
    // out, count above 2^32 - 2); 3 more than redo_cap elements need exact
    // arithmetic (the first redo_cap are listed)
    int err = 0;
};
// All jobs in one launch on a pool stream, one fiber-friendly wait. Returns
// -1 only on a device error; per-job codes in jobs[i].err. A job of count 0
// parses nothing (err 0).
int DeviceParseNumberArrays(DeviceNumberParseJob* jobs, int n, int device);
// Host text through the device, the shape of the integer array offload: the
// text between the outer separators and the separators go to pinned memory,
// payload[nseps - 1] and classes[nseps - 1] come back as
// json::ParseNumberArray gives them. Elements on the redo list (a fixed
// small capacity) are repaired on the host from the host text by the exact
// route. False on a malformed element, on a redo overflow or on a device
// error; *n_redo (optional) receives the number of repaired elements.
bool ParseNumbersOnDevice(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload, uint8_t* classes,
                          int device, uint32_t* n_redo = nullptr);

// ---- JSON number text parsed on the device with no separator table: the
// caller has bytes in HBM (a string field, a peer's printed embedding, the
// text behind a "key": prefix) and nothing else. Accepted, with JSON
// whitespace wherever JSON allows it:
//   depth 0  v,v,...,v
//   depth 1  [v,v,...,v]
//   depth 2  [[v,..],[v,..],..]   rows of any (nonzero) lengths
// every v a number of the RFC 8259 grammar. Empty text, whitespace and "[ ]"
// are count 0. Everything else is malformed: first_bad is the lowest index
// of a piece (the text between consecutive commas or the ends) that does not
// fit. json::ParseNumberText is the host twin: the same scanner
// (base/number_text.h), the same verdicts.
struct DeviceNumberTextJob {
    const char* text = nullptr;  // device or pinned host, any byte alignment
    uint64_t n = 0;              // bytes, below 2^32 - 1
    uint32_t mode = 0;           // kJsonParse*: out / classes exactly as in DeviceNumberParseJob
    void* out = nullptr;         // cap elements, 8-byte aligned (4 for float32)
    uint8_t* classes = nullptr;  // kJsonParseNumbers only, cap bytes
    uint64_t cap = 0;
    // depth 2: row_ends[r] = the elements in rows 0..r. Null: nested text is
    // malformed (first_bad 0).
    uint32_t* row_ends = nullptr;
    uint64_t row_cap = 0;
    // elements the device does not decide (see DeviceNumberParseJob): nothing
    // is written to out for them; each takes a pair {element index, offset of
    // the first byte after the element's preceding separator} (0 for the
    // first element), in no particular order. The element is the number in
    // the piece that starts there, within its brackets and whitespace.
    uint32_t* redo = nullptr;  // 2 * redo_cap entries, device-writable
    uint32_t redo_cap = 0;
    // out
    uint32_t depth = 0;
    uint64_t count = 0;  // elements (with err 5: what the text holds; with err 1: its pieces)
    uint64_t rows = 0;   // depth 2 only
    uint32_t n_redo = 0;
    uint32_t first_bad = 0xFFFFFFFFu;
    // 0 parsed; 1 malformed (trust nothing of out); 2 refused before any
    // launch (null text with n > 0, bad mode, null out with cap > 0,
    // misaligned out / row_ends / redo, n above 2^32 - 2, classes missing in
    // numbers mode, redo_cap without redo, row_cap without row_ends); 3 more
    // than redo_cap undecided elements (n_redo is the true number); 5 more
    // than cap elements or more than row_cap rows (count and rows are what is
    // needed; nothing is written beyond the capacities). 5 is reported
    // before 3.
    int err = 0;
};
// All jobs share one launch sequence (count, prefix, parse, publish) on a
// pool stream and one fiber-friendly wait; nothing is read back in between.
// Returns -1 only on a device error; per-job codes in jobs[i].err. A job of
// n 0 launches nothing (count 0, err 0).
int DeviceParseNumberText(DeviceNumberTextJob* jobs, int n, int device);
// Bytes of text one workgroup takes (tests aim at its edges).
uint32_t JsonTextChunkBytes();

// ---- number arrays and nested number rows as JSON text, the inverse of
// DeviceParseNumberText: `count` elements of one kind plus an optional table
// of row ends (the pair DeviceParseNumberText, DeviceSplitRows and
// DeviceBuildRows use: row_ends[r] = the elements in rows 0..r) become
//   row_ends null, brackets false   v,v,...,v
//   row_ends null, brackets true    [v,v,...,v]          "[]" for count 0
//   row_ends given                  [[v,..],[v,..],..]   brackets ignored
// with no whitespace. Kinds: gpu::PbRunKind 0..6 (int32 and sint32, uint32,
// int64 and sint64, uint64 print as the decimal number of their type, never
// as a wire form; bool reads one byte per element, nonzero prints true) and
// kJsonFloat32 / kJsonFloat64, printed exactly as DevicePrintFloatArrays
// prints them. Rows are not empty, as DeviceParseNumberText refuses an empty
// row. json::FormatNumberRows is the host twin: the same rules
// (base/number_print.h), the same bytes, the same verdicts.
struct DeviceNumberPrintJob {
    const void* src = nullptr;  // device or pinned host; naturally aligned (1 / 4 / 8 bytes)
    uint64_t count = 0;         // elements
    uint32_t kind = 0;
    const uint32_t* row_ends = nullptr;  // device or pinned host, `rows` entries; the host never reads it
    uint64_t rows = 0;
    bool brackets = false;
    void* dst = nullptr;  // device-writable, cap bytes
    uint64_t cap = 0;
    uint64_t len = 0;  // out: text size (with err 3: the size it needs)
    // out, with err 1: the lowest row r with row_ends[r] <= row_ends[r - 1]
    // (row_ends[-1] = 0), row_ends[r] > count, or r the last row and
    // row_ends[r] != count. Found on the device.
    uint32_t first_bad = 0xFFFFFFFFu;
    // out: 0 printed; 1 bad row_ends (dst untouched); 2 refused before any
    // launch (a null src where elements are read, a null dst where bytes are
    // written, a kind there is not, a src not naturally aligned, a row_ends
    // not 4-byte aligned, rows without row_ends, row_ends without rows, a dst
    // that overlaps src or row_ends, a worst case above 2^32 - 1 bytes); 3
    // longer than cap (dst untouched); 4 the source changed between the
    // passes: a chunk's text was not the size measured for it (nothing of
    // that chunk written)
    int err = 0;
};
// Most bytes the text of `count` elements in `rows` rows (0: a flat form) can
// take; always suffices as a cap. 0 for a kind there is not.
uint64_t NumberPrintWorstCaseBytes(uint32_t kind, uint64_t count, uint64_t rows);
// All jobs share one launch sequence (size, rows, prefix, place) on a pool
// stream and one fiber-friendly wait; the host reads nothing but the result
// words. Returns -1 only on a device error; per-job codes in jobs[i].err. A
// flat job of count 0 without brackets writes nothing and launches nothing
// (len 0, err 0).
int DevicePrintNumbers(DeviceNumberPrintJob* jobs, int n, int device);
// Elements one workgroup takes, and rows (tests aim at its edges).
uint32_t JsonNumberPrintChunkElems();

// ---- records as JSON objects: the columns DeviceSplitRecords gives (or
// DeviceBuildRecords takes), each with a key, become
//   [{"k0":cell,"k1":cell,...},{...},...]
// in device memory, the shape http+json model APIs return. Every key appears
// in every record, in column order; nothing is omitted (this is not pb2json's
// omission rule). No whitespace; without brackets the records are only joined
// by ','. The cell of record r:
//   kinds 0..6, 8, 9 without row_ends (count == rows)   element r, as DevicePrintNumbers prints it
//   the same kinds with row_ends                        [v,v,...,v], [] for a row of no element
//   kind 7 with row_ends, text kJsonRecordString        the row's bytes as DeviceEscapeJsonStrings escapes them, quoted
//   kind 7 with row_ends, text kJsonRecordBase64        the row as padded base64, quoted
// Empty rows are legal. base/json_records.h has the rules,
// json::FormatRecordObjects is the host twin: the same bytes, the same codes.
constexpr uint32_t kJsonRecordNumber = 0, kJsonRecordString = 1, kJsonRecordBase64 = 2;  // json_records::Text
struct DeviceRecordPrintColumn {
    const void* key = nullptr;  // host memory, key_len raw bytes; escaped once per job
    uint32_t key_len = 0;
    uint32_t kind = 0;
    uint32_t text = kJsonRecordNumber;
    const void* src = nullptr;  // device or pinned host; naturally aligned (1 / 4 / 8 bytes)
    uint64_t count = 0;         // elements (bytes for kind 7)
    const uint32_t* row_ends = nullptr;  // device or pinned host, `rows` entries, 4-byte aligned; null: a scalar column
};
struct DeviceRecordPrintJob {
    const DeviceRecordPrintColumn* columns = nullptr;
    uint32_t ncols = 0;  // 1 .. 8
    uint64_t rows = 0;
    bool brackets = false;
    void* dst = nullptr;  // device-writable, cap bytes, any alignment
    uint64_t cap = 0;
    uint64_t len = 0;  // out: text size (with err 3: the size it needs; 0 with err 1)
    // out, with err 1: the lowest row whose end lies below its predecessor or
    // above count, or is the last and not count, over all columns, and the
    // lowest column that offends there. Found on the device.
    uint32_t first_bad = 0xFFFFFFFFu, bad_column = 0xFFFFFFFFu;
    // out: 0 printed; 1 a bad table (dst untouched); 2 refused before any
    // launch (a null pointer with a nonzero size, a misaligned src or
    // row_ends, a kind or text form there is not, kind 7 without row_ends, a
    // text form on a number kind, ncols 0 or above 8, a scalar column whose
    // count is not rows, a key whose escaped form is above 255 bytes, two
    // equal keys, a dst that overlaps a source or a table, a worst case above
    // 2^32 - 1); 3 longer than cap (dst untouched); 4 a source or table
    // changed between the passes (nothing of that chunk is written). 1 wins
    // over 3.
    int err = 0;
};
// Most bytes the job's text can take for any values and tables (dst and cap
// are not looked at); always suffices as a cap. 0 for a job that is refused,
// ~0 when it is above 2^32 - 1.
uint64_t RecordObjectsWorstCaseBytes(const DeviceRecordPrintJob& job);
// All jobs share one launch sequence (init, size, prefix, measure, prefix,
// heads, place: kernels.h) on a pool stream and one fiber-friendly wait; the
// host reads no table and no value, only the result words. Returns -1 only on
// a device error; per-job codes in jobs[i].err. A job of no row launches
// nothing: its text is "[]" (copied to dst) or nothing.
int DevicePrintRecordObjects(DeviceRecordPrintJob* jobs, int n, int device);
// Elements one workgroup of the element passes takes, and records one of the
// record passes takes (tests aim at their edges).
uint32_t JsonRecordsChunkElems();
uint32_t JsonRecordsBlockRows();

struct GpuJsonStats {
    int64_t record_print_jobs = 0, record_print_rows = 0;  // DevicePrintRecordObjects: jobs and records printed
    // json2pb number arrays (floats) parsed on the device; fallbacks: arrays the device declined
    int64_t number_arrays = 0, number_elems = 0, number_array_fallbacks = 0, number_redo_elems = 0;
    int64_t indexed_bodies = 0, indexed_bytes = 0, failures = 0;
    int64_t pb2json_arrays = 0, pb2json_elems = 0, pb2json_failures = 0;  // number arrays printed on the device
    int64_t pb2json_float_arrays = 0, pb2json_float_elems = 0;  // float / double arrays (not counted above)
    int64_t int_arrays = 0, int_array_fallbacks = 0;  // json2pb integer arrays parsed on the device
    int64_t sparse_skips = 0;  // bodies left to the host parser by the density check
};
GpuJsonStats GetGpuJsonStats();

}  // namespace gpu
}  // namespace mrpc
