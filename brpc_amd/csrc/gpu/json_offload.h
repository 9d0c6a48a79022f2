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

struct GpuJsonStats {
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
