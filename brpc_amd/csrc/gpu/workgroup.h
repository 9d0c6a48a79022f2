// Workgroup idioms shared by the offload kernels (base64, JSON strings, JSON
// number text, float print, packed runs, row builder and splitter, varint).
// Device only: include it from .hip files. Where a size matters the helper
// is templated on the workgroup size, so its loops over waves and rounds
// unroll. Every lane of the workgroup calls a helper that holds a barrier.
//
// Barriers. block_excl_scan and block_sum hold exactly one, between writing
// and reading `part`; nothing precedes the write and nothing follows the
// read. A caller that hands the same `part` words to a second call (or
// rewrites them in a loop) puts its own barrier in between. scan_post /
// scan_rank are the two halves of block_excl_scan for callers that post
// several scans (one `part` row each) in front of a single barrier.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mrpc {
namespace gpu {
namespace wg {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The job that owns block (or chunk, or row block) x: the last one whose
// kFirst field is not past x. A job without blocks shares its start with the
// next job, which then owns them. (Searches of other tables keep their own
// code: find_segment and the MFMA CRC kernel's in kernels.hip, over arrays of
// starts on the copy/CRC path, and the row searches inside a job in
// pb_kernels.hip and json_string_kernels.hip, which are lower bounds over
// row ends.)
template <auto kFirst, class Job>
__device__ __forceinline__ int job_of(const Job* __restrict__ jobs, int njobs, uint32_t x) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (jobs[mid].*kFirst <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Dwords lo, hi as they follow each other in memory -> the dword that starts
// `sh` bits (0, 8, 16, 24) into lo.
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// Stages [p, p + n) into lds as the whole 16-byte units that hold a byte of
// it (so the loads stay inside pages the span touches): aligned 16-byte
// loads, all issued before the first is stored. At most kRounds * kThreads
// units; byte p lands at lds byte (p & 15), which is returned. The caller
// synchronizes before reading lds.
template <int kThreads, int kRounds>
__device__ __forceinline__ uint32_t stage16(const uint8_t* p, uint32_t n, u32x4* lds) {
    const uint32_t a = (uint32_t)((uintptr_t)p & 15);
    const u32x4* src = reinterpret_cast<const u32x4*>(p - a);
    const uint32_t n16 = (a + n + 15) >> 4;
    u32x4 v[kRounds];
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const uint32_t i = threadIdx.x + (uint32_t)k * kThreads;
        if (i < n16) v[k] = src[i];
    }
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const uint32_t i = threadIdx.x + (uint32_t)k * kThreads;
        if (i < n16) lds[i] = v[k];
    }
    return a;
}

// The copy-outs: an LDS image -> dst at any alignment, as bytes up to dst's
// first 16-byte boundary, 16-byte stores, bytes for the rest. The caller has
// synchronized the image. They are named for what they assume of it.
//
// copy_out_phased: image bytes [sh, sh + total) -> dst, where the 16-byte
// aligned image was laid out at dst's phase (dst = sh mod 16), so the body is
// 16-byte LDS reads.
template <int kThreads>
__device__ __forceinline__ void copy_out_phased(const uint8_t* image, uint32_t sh, uint8_t* dst, uint32_t total) {
    const uint32_t t = threadIdx.x;
    uint32_t head = (16 - sh) & 15;
    if (head > total) head = total;
    if (t < head) dst[t] = image[sh + t];
    const uint32_t nv = (total - head) / 16;
    const u32x4* from = reinterpret_cast<const u32x4*>(image + sh + head);
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    for (uint32_t w = t; w < nv; w += kThreads) body[w] = from[w];
    for (uint32_t j = head + 16 * nv + t; j < total; j += kThreads) dst[j] = image[sh + j];
}

// copy_out_shifted: bytes [ioff, ioff + total) of a 16-byte aligned image ->
// dst, whatever the two phases: a unit is one 16-byte LDS read when it starts
// on a 16-byte boundary of the image, four dwords when on a dword, else five
// dwords funnel-shifted into four. The image is readable through the dword
// that holds byte ioff + total: one dword past the last unit.
template <int kThreads>
__device__ __forceinline__ void copy_out_shifted(const uint32_t* image, uint32_t ioff, uint8_t* __restrict__ dst,
                                                 uint32_t total) {
    const uint32_t t = threadIdx.x;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(image) + ioff;
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15)) & 15;
    if (head > total) head = total;
    if (t < head) dst[t] = bytes[t];
    const uint32_t nv = (total - head) / 16;
    const uint32_t at = ioff + head;     // uniform: where the first unit starts in the image
    const uint32_t sh = (at & 3) * 8;
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    for (uint32_t v = t; v < nv; v += kThreads) {
        const uint32_t w = (at + 16 * v) >> 2;
        u32x4 x;
        if ((at & 15) == 0) {
            x = reinterpret_cast<const u32x4*>(image)[w >> 2];
        } else if (sh == 0) {
            x.x = image[w];
            x.y = image[w + 1];
            x.z = image[w + 2];
            x.w = image[w + 3];
        } else {
            const uint32_t d0 = image[w], d1 = image[w + 1], d2 = image[w + 2], d3 = image[w + 3], d4 = image[w + 4];
            x.x = funnel(d0, d1, sh);
            x.y = funnel(d1, d2, sh);
            x.z = funnel(d2, d3, sh);
            x.w = funnel(d3, d4, sh);
        }
        body[v] = x;
    }
    for (uint32_t j = head + 16 * nv + t; j < total; j += kThreads) dst[j] = bytes[j];
}

// copy_out_bytes: image[0, total) -> dst, nothing assumed: the image starts
// at any byte and ends with its last byte, and every dword of a unit is put
// together from four byte reads of LDS. The packed-run and row kernels keep
// it: with copy_out_shifted in its place pb_run_encode_kernel and
// pb_run_decode_kernel each need enough more VGPRs to lose a wave per SIMD.
template <int kThreads>
__device__ __forceinline__ void copy_out_bytes(const uint8_t* image, uint8_t* dst, uint32_t total) {
    const uint32_t t = threadIdx.x;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > total) head = total;
    if (t < head) dst[t] = image[t];
    const uint32_t nv = (total - head) / 16;
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    for (uint32_t w = t; w < nv; w += kThreads) {
        const uint8_t* q = image + head + 16 * w;
        u32x4 v;
        v.x = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        v.y = (uint32_t)q[4] | ((uint32_t)q[5] << 8) | ((uint32_t)q[6] << 16) | ((uint32_t)q[7] << 24);
        v.z = (uint32_t)q[8] | ((uint32_t)q[9] << 8) | ((uint32_t)q[10] << 16) | ((uint32_t)q[11] << 24);
        v.w = (uint32_t)q[12] | ((uint32_t)q[13] << 8) | ((uint32_t)q[14] << 16) | ((uint32_t)q[15] << 24);
        body[w] = v;
    }
    for (uint32_t j = head + 16 * nv + t; j < total; j += kThreads) dst[j] = image[j];
}

// ---- scans and sums over a wave (64 lanes), then over the workgroup

struct Add {
    template <class T>
    __device__ __forceinline__ T operator()(T earlier, T later) const {
        return earlier + later;
    }
};

// v of the lane below (lane 0 of a wave keeps its own).
template <class T>
__device__ __forceinline__ T wave_prev(T v) {
    return __shfl_up(v, 1, 64);
}

// Inclusive scan over the wave: op(earlier lanes, this lane), a sum by default.
template <class T, class Op = Add>
__device__ __forceinline__ T wave_incl_scan(T v, Op op = Op()) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v = op(y, v);
    }
    return v;
}

// Sum over the wave, in every lane.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// First half of a workgroup scan: the wave's inclusive scan of v; its total
// goes to part[wave]. part: kThreads / 64 words of LDS.
template <class T>
__device__ __forceinline__ T scan_post(T v, T* part) {
    const T incl = wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
    return incl;
}

// Second half, after a barrier: the sum of v over the lanes before this one;
// the workgroup's sum is added to *total.
template <int kThreads, class T>
__device__ __forceinline__ T scan_rank(T incl, T v, const T* part, T* total) {
    const uint32_t wave = threadIdx.x >> 6;
    T before = incl - v;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kThreads / 64; ++k) {
        const T x = part[k];
        if (k < wave) before += x;
        *total += x;
    }
    return before;
}

// Exclusive scan of v over the workgroup; *total its sum. One barrier.
template <int kThreads, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* part, T* total) {
    const T incl = scan_post(v, part);
    __syncthreads();
    *total = 0;
    return scan_rank<kThreads>(incl, v, part, total);
}

// Sum of v over the workgroup, in every lane. One barrier.
template <int kThreads, class T>
__device__ __forceinline__ T block_sum(T v, T* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) total += part[k];
    return total;
}

}  // namespace wg
}  // namespace gpu
}  // namespace mrpc
