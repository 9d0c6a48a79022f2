// Base64 of bytes that live in device memory (gpu/base64_kernels.hip): the
// form pb2json / json2pb give a `bytes` field by default
// (Pb2JsonOptions::bytes_to_base64, Json2PbOptions::base64_to_bytes; the
// reference codes it on the host through butil/base64.h). A handler that
// holds a tensor or a scanned bytes field in HBM turns it into JSON text, or
// text back into bytes, without a trip to the host. Host-resident strings
// stay with base64_encode / base64_decode (base/util.h): there is no staged
// path through the device and no json2pb hook.
#pragma once

#include <cstdint>

#include "base/base64_rows.h"

namespace mrpc {
namespace gpu {

struct DeviceBase64Job {
    const void* src = nullptr;  // device or pinned host, any alignment
    uint64_t n = 0;             // bytes at src: data (encode), text (decode)
    void* dst = nullptr;        // device-writable, any alignment, cap bytes; must not overlap src
    uint64_t cap = 0;
    uint64_t len = 0;  // out: bytes written (with err 3: the size needed)
    // out, decode with err 1: the lowest offset of a body byte outside the
    // alphabet, or n when only the length rule fails
    uint64_t first_odd = 0;
    // out, the codes of the other device jobs: 0 done; 1 (decode) the text is
    // not canonical, trust nothing of dst, the host decoder decides; 2 refused
    // before any launch (a null pointer with n > 0, n or the output size above
    // 2^32 - 1, text of exactly 2^32 - 1 bytes too, src and dst ranges that
    // overlap); 3 cap too small, decided before any launch (dst untouched)
    int err = 0;
};

// n data bytes -> Base64EncodedBytes(n) = (n + 2) / 3 * 4 symbols, '='
// padded; err 3 when cap is smaller. All jobs share one launch on a pool
// stream and one fiber-friendly wait. Returns -1 only on a device error;
// per-job codes in jobs[i].err. A job of n 0 writes nothing (len 0, err 0).
int DeviceBase64Encode(DeviceBase64Job* jobs, int njobs, int device);

// Canonical text only: a body of m alphabet symbols followed by p = 0, 1 or 2
// '=' (n = m + p), m % 4 != 1, and p == 0 or n % 4 == 0 (unpadded text is
// canonical; so are trailing bits that are not zero, which are dropped as the
// host drops them). len = m / 4 * 3 + (m % 4) * 3 / 4. On such text device
// and host agree; everything else, the whitespace the host decoder skips
// included, is err 1 with first_odd set, and the caller asks base64_decode.
// cap must hold Base64DecodedMaxBytes(n) = n / 4 * 3 + (n % 4) * 3 / 4, the
// size before the padding is known (err 3 otherwise). Launches, wait and
// return value as above.
int DeviceBase64Decode(DeviceBase64Job* jobs, int njobs, int device);

// ---- rows: `repeated bytes`, or a bytes column of records, to and from the
// text of a JSON array of base64 strings, HBM -> HBM. The rules are
// base/base64_rows.h; json::EncodeBase64Rows / DecodeBase64Rows (json/json.h)
// are the host twins. (bytes, row_ends) is the pair DeviceSplitRows /
// DeviceSplitRecords give and DeviceBuildRows / DeviceBuildRecords take.
//
// Codes of both entries: 0 done; 1 see each entry, first_bad is set; 2 refused
// before any launch (a null pointer where something is to be read or written,
// n above 2^32 - 2 or an output above 2^32 - 1, ranges that overlap, row_ends
// that is not 4-byte aligned, rows without row_ends); 3 cap or row_cap too
// small, found on the device, len and rows say what is needed; 4 (decode) the
// source changed between the passes. With 1, 3 and 4 dst and row_ends are
// untouched apart from what code 4 had placed before it was found; no store
// ever goes beyond a capacity. All jobs of a call share the launches, on one
// pool stream with one fiber-friendly wait; the host reads nothing but the
// result words, row_ends neither. Each returns -1 only on a device error.

// The text of `rows` rows holding n bytes in all is never longer than this.
constexpr uint64_t Base64RowsWorstCaseBytes(uint64_t n, uint64_t rows, bool brackets) {
    return base64_rows::Base64RowsWorstCaseBytes(n, rows, brackets);
}
// A text of n bytes never decodes to more bytes, or holds more strings.
constexpr uint64_t Base64RowsMaxBytes(uint64_t n) { return base64_rows::Base64RowsMaxBytes(n); }
constexpr uint64_t Base64RowsMaxRows(uint64_t n) { return base64_rows::Base64RowsMaxRows(n); }

// Row r is src[row_ends[r - 1], row_ends[r]) (row_ends[-1] = 0, equal
// neighbours: an empty row); the output is "b0","b1",...,"b(rows-1)", wrapped
// in '[' ']' with brackets, no whitespace. rows == 0 writes "[]" or nothing;
// n == 0 with rows > 0 writes "","",.. . Code 1: row_ends decreases at row
// first_bad, rises above n, or does not end at n (the lowest such row, found
// on the device). The table is read once, into a copy the later passes use.
// The size depends on every row length: cap may be anything from the true
// size up, Base64RowsWorstCaseBytes always suffices.
struct DeviceBase64RowsEncodeJob {
    const void* src = nullptr;       // device, any alignment
    uint64_t n = 0;                  // at most 2^32 - 2
    const void* row_ends = nullptr;  // uint32[rows], device, 4-byte aligned
    uint64_t rows = 0;
    bool brackets = true;
    void* dst = nullptr;  // device-writable, any alignment, cap bytes; overlaps neither src nor row_ends
    uint64_t cap = 0;
    uint64_t len = 0;        // out: bytes written (code 3: the size needed)
    uint64_t first_bad = 0;  // out, code 1
    int err = 0;
};
int DeviceBase64EncodeRows(DeviceBase64RowsEncodeJob* jobs, int njobs, int device);

// "b0","b1",... or ["b0","b1",...], JSON whitespace wherever JSON allows it,
// every body canonical base64 -> the decoded bytes of all strings at dst and
// row_ends[r], the bytes in strings 0..r. Code 1: the text is not for the
// device (json::Reader and base64_decode are laxer), first_bad is the offset
// at which a parser reading from the left cannot go on; len, rows and depth
// are 0. Code 2 also: dst or row_ends overlapping src or each other. n == 0 is
// code 0, no rows, nothing written, no launch.
struct DeviceBase64RowsDecodeJob {
    const void* src = nullptr;  // device, any alignment
    uint64_t n = 0;             // at most 2^32 - 2
    void* dst = nullptr;        // decoded bytes, any alignment
    uint64_t cap = 0;           // Base64RowsMaxBytes(n) always suffices
    void* row_ends = nullptr;   // uint32[row_cap], 4-byte aligned
    uint64_t row_cap = 0;       // Base64RowsMaxRows(n) always suffices
    uint64_t len = 0, rows = 0, first_bad = 0;  // out
    uint32_t depth = 0;                         // out: 1 when the text is bracketed
    int err = 0;
};
int DeviceBase64DecodeRows(DeviceBase64RowsDecodeJob* jobs, int njobs, int device);

}  // namespace gpu
}  // namespace mrpc
