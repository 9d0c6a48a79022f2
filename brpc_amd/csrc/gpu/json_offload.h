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

struct GpuJsonStats {
    int64_t indexed_bodies = 0, indexed_bytes = 0, failures = 0;
    int64_t pb2json_arrays = 0, pb2json_elems = 0, pb2json_failures = 0;  // number arrays printed on the device
    int64_t pb2json_float_arrays = 0, pb2json_float_elems = 0;  // float / double arrays (not counted above)
    int64_t int_arrays = 0, int_array_fallbacks = 0;  // json2pb integer arrays parsed on the device
    int64_t sparse_skips = 0;  // bodies left to the host parser by the density check
};
GpuJsonStats GetGpuJsonStats();

}  // namespace gpu
}  // namespace mrpc
