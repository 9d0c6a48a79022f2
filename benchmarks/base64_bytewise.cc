// Helper of benchmarks/base64_bw.py, built by it into a shared library and
// called through ctypes: the byte-wise base64 coder base/util.cc had before
// it moved onto base/base64.h (four push_backs per three bytes; a reverse
// table rebuilt per call and one push_back per byte), next to today's coder,
// both timed inside C++ around one call so that no binding is in the number.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>

#include "base/util.h"

namespace {

const char* kB64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

std::string bytewise_encode(const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    std::string out;
    out.reserve((n + 2) / 3 * 4);
    size_t i = 0;
    for (; i + 2 < n; i += 3) {
        uint32_t v = (p[i] << 16) | (p[i + 1] << 8) | p[i + 2];
        out.push_back(kB64[v >> 18]);
        out.push_back(kB64[(v >> 12) & 63]);
        out.push_back(kB64[(v >> 6) & 63]);
        out.push_back(kB64[v & 63]);
    }
    if (i < n) {
        uint32_t v = p[i] << 16;
        if (i + 1 < n) v |= p[i + 1] << 8;
        out.push_back(kB64[v >> 18]);
        out.push_back(kB64[(v >> 12) & 63]);
        out.push_back(i + 1 < n ? kB64[(v >> 6) & 63] : '=');
        out.push_back('=');
    }
    return out;
}

bool bytewise_decode(const std::string& in, std::string* out) {
    int8_t rev[256];
    memset(rev, -1, sizeof(rev));
    for (int i = 0; i < 64; ++i) rev[(uint8_t)kB64[i]] = (int8_t)i;
    out->clear();
    uint32_t acc = 0;
    int bits = 0;
    size_t n = 0, pad = 0;
    for (char c : in) {
        if (c == '\n' || c == '\r' || c == ' ') continue;
        if (c == '=') {
            ++pad;
            continue;
        }
        if (pad) return false;
        int v = rev[(uint8_t)c];
        if (v < 0) return false;
        ++n;
        acc = (acc << 6) | (uint32_t)v;
        bits += 6;
        if (bits >= 8) {
            bits -= 8;
            out->push_back((char)((acc >> bits) & 0xff));
        }
    }
    if (n % 4 == 1 || pad > 2 || (pad && (n + pad) % 4 != 0)) return false;
    return true;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// One call of the coder `which` (0 byte-wise, 1 today's) in direction
// `decode` over in[0, n): the seconds it took; the result goes to
// out[0, *out_len) (cap bytes) outside the timed span. -1 when the decoder
// refused or the result does not fit.
extern "C" double base64_bw_time(int which, int decode, const char* in, size_t n, char* out, size_t cap,
                                 size_t* out_len) {
    std::string result;
    double t;
    if (decode) {
        const std::string text(in, n);
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = which == 0 ? bytewise_decode(text, &result) : mrpc::base64_decode(text, &result);
        t = seconds_since(t0);
        if (!ok) return -1;
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        result = which == 0 ? bytewise_encode(in, n) : mrpc::base64_encode(in, n);
        t = seconds_since(t0);
    }
    if (result.size() > cap) return -1;
    memcpy(out, result.data(), result.size());
    *out_len = result.size();
    return t;
}

// Today's coder between the caller's buffers (pinned memory in the
// benchmark), as a handler calls it after a D2H copy: the bytes written, or
// (size_t)-1 when the decoder refused or dst is too small.
extern "C" size_t base64_bw_host(int decode, const char* src, size_t n, char* dst, size_t cap) {
    if (!decode) {
        const size_t len = (n + 2) / 3 * 4;
        if (len > cap) return (size_t)-1;
        mrpc::base64_encode_to(src, n, dst);
        return len;
    }
    std::string out;
    if (!mrpc::base64_decode(src, n, &out) || out.size() > cap) return (size_t)-1;
    memcpy(dst, out.data(), out.size());
    return out.size();
}
