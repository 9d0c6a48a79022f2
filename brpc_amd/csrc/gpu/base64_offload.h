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

}  // namespace gpu
}  // namespace mrpc
