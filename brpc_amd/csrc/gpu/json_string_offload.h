// JSON string bodies that live in device memory (gpu/json_string_kernels.hip):
// escape, unescape, the text of an array of strings back into bytes and row
// ends, and the UTF-8 verdict, HBM -> HBM. A handler that holds text
// in HBM (a string field found by DevicePayloadField, the rows DeviceSplitRows
// produced for a repeated string, a prompt or completion buffer) turns it into
// the body of a JSON string, or a body back into text, without a trip to the
// host; the reference goes through rapidjson's Writer and Reader on the host.
// The rules are base/json_string.h and base/json_string_rows.h;
// json::EscapeStringBody, EscapeStringRows, UnescapeStringBody,
// UnescapeStringRows and Utf8FirstBad (json/json.h) are the host twins. A
// repeated string goes both ways: DeviceEscapeJsonStrings with row_ends writes
// "r0","r1",..., DeviceUnescapeJsonStringRows turns that text, or the
// ["r0","r1",...] a peer sends, back into (bytes, row_ends), the pair
// DeviceBuildRows takes. Host-resident strings stay with the twins: there is
// no staged path through the device and no pb2json / json2pb hook.
//
// Codes of all entries: 0 done; 1 see each entry, first_bad is set;
// 2 refused before any launch (a null pointer where bytes are to be read or
// written, n above 2^32 - 2 or a worst-case output above 2^32 - 1, src and dst
// ranges that overlap, row_ends that is not 4-byte aligned, rows without
// row_ends, row_ends without rows for n > 0); 3 cap too small, len says what
// is needed. An escape job of n 0 with quote set writes "" and so needs a dst;
// every other job of n 0 writes nothing (len 0, code 0). With 1 and 3 dst is untouched; no store ever
// goes beyond cap. All jobs of a call share the launches, on one pool stream
// with one fiber-friendly wait; the host reads nothing but the result words.
// Each returns -1 only on a device error.
#pragma once

#include <cstdint>

#include "base/json_string_rows.h"
#include "gpu/kernels.h"

namespace mrpc {
namespace gpu {

// 6n + 2 for a single string (quotes included), 6n + 3 rows - 1 for rows.
constexpr uint64_t JsonEscapeWorstCaseBytes(uint64_t n, uint64_t rows) {
    return rows ? 6 * n + 3 * rows - 1 : 6 * n + 2;
}

struct DeviceJsonEscapeJob {
    const void* src = nullptr;  // device, any alignment
    uint64_t n = 0;
    // null: one string. Else `rows` uint32 in device memory, row_ends[r] the
    // bytes in rows 0..r (equal neighbours: an empty row), as DeviceSplitRows
    // and DeviceBuildRows use them for repeated string: the output is
    // "r0","r1",...,"r(rows-1)" and quote is ignored. A decrease, or a last
    // entry that is not n, is code 1 with first_bad the row (found on the
    // device).
    const void* row_ends = nullptr;
    uint64_t rows = 0;
    bool quote = true;    // one string: surrounding quotes
    void* dst = nullptr;  // device-writable, any alignment, cap bytes; must not overlap src
    uint64_t cap = 0;
    uint64_t len = 0;        // out: bytes written (code 3: the size needed)
    uint64_t first_bad = 0;  // out, code 1
    int err = 0;
};
// The size is known only after a pass over the data: cap may be anything from
// the true size up; JsonEscapeWorstCaseBytes always suffices.
int DeviceEscapeJsonStrings(DeviceJsonEscapeJob* jobs, int njobs, int device);

struct DeviceJsonUnescapeJob {
    const void* src = nullptr;  // the body between the quotes
    uint64_t n = 0;
    void* dst = nullptr;
    uint64_t cap = 0;        // at least n, else code 3 before any launch
    uint64_t len = 0;        // out
    uint64_t first_bad = 0;  // out, code 1: the lowest offset of an offending backslash or quote
    int err = 0;             // 1: not for the device, json::Reader decides
};
int DeviceUnescapeJsonStrings(DeviceJsonUnescapeJob* jobs, int njobs, int device);

// The worst cases of DeviceUnescapeJsonStringRows for a text of n bytes: n - 2
// decoded bytes, (n + 1) / 3 strings.
constexpr uint64_t JsonStringRowsMaxBytes(uint64_t n) { return json_string_rows::JsonStringRowsMaxBytes(n); }
constexpr uint64_t JsonStringRowsMaxRows(uint64_t n) { return json_string_rows::JsonStringRowsMaxRows(n); }

// "r0","r1",... or ["r0","r1",...] (base/json_string_rows.h has the grammar)
// -> the decoded bytes of all strings at dst and row_ends[r], the bytes in
// strings 0..r: the inverse of an escape job with row_ends. Codes as above,
// with these particulars. 1: the text is not for the device (json::Reader
// decides), first_bad is the offset at which a parser reading from the left
// cannot go on; len, rows and depth are 0. 2 also: a null dst with cap > 0, a
// null row_ends with row_cap > 0, dst or row_ends overlapping src or each
// other. 3: more than cap bytes or more than row_cap strings, found on the
// device since both depend on the data; len and rows say what the text holds.
// 4: the source changed between the passes. With 1 and 3 dst and row_ends are
// untouched, and no store goes beyond either capacity. n == 0 is code 0, no
// rows, nothing written, no launch.
struct DeviceJsonStringRowsJob {
    const void* src = nullptr;  // device, any alignment
    uint64_t n = 0;             // at most 2^32 - 2
    void* dst = nullptr;        // decoded bytes, any alignment; must not overlap src
    uint64_t cap = 0;           // JsonStringRowsMaxBytes(n) always suffices
    void* row_ends = nullptr;   // uint32[row_cap], 4-byte aligned
    uint64_t row_cap = 0;       // JsonStringRowsMaxRows(n) always suffices
    uint64_t len = 0, rows = 0, first_bad = 0;  // out
    uint32_t depth = 0;                         // out: 1 when the text is bracketed
    int err = 0;
};
int DeviceUnescapeJsonStringRows(DeviceJsonStringRowsJob* jobs, int njobs, int device);

struct DeviceUtf8Job {
    const void* src = nullptr;
    uint64_t n = 0;
    uint64_t first_bad = 0;  // out, code 1: the first offset where no well-formed sequence starts
    int err = 0;             // 0 well-formed, 1 ill-formed, 2 refused
};
int DeviceValidateUtf8(DeviceUtf8Job* jobs, int njobs, int device);

}  // namespace gpu
}  // namespace mrpc
