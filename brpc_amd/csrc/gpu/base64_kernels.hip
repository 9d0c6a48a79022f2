// Base64 of bytes in device memory on gfx950, both directions (kernels.h
// Base64Job; the reference codes bytes fields on the host through
// butil/base64.h in pb_to_json.cpp / json_to_pb.cpp). The arithmetic is
// base/base64.h, the code the host coder runs.
//
// A job is cut into chunks of kBase64ChunkBytes data bytes <->
// kBase64ChunkSymbols symbols; a workgroup of 256 lanes takes one chunk of one
// job, a lane 12 bytes <-> 16 symbols. src and dst may have any byte
// alignment: global loads and the stores of whole 16-byte units are aligned,
// the shift happens on chip.
//
//  encode  the chunk's source span is staged in LDS (wg::stage16). A lane
//          reads its 12 bytes as four dwords (stride 3 dwords: conflict-free)
//          and funnel-shifts them, forms its 16 symbols in registers and,
//          when dst is 16-byte aligned and the chunk whole, stores them at
//          once. Otherwise the symbols go through an LDS image and leave
//          through wg::copy_out_shifted. Only the job's last lane that holds
//          data writes '='.
//  decode  a lane loads its 16 symbols (one aligned 16-byte load, or the two
//          that cover them), converts them and puts its 12 bytes into the LDS
//          image, which leaves through wg::copy_out_shifted. Every workgroup
//          reads the job's last two bytes to learn the padding p, so the body
//          is [0, n - p) for all of them; a body byte outside the alphabet
//          records its offset with atomicMin on the job's result in device
//          memory, a body length the padding rule forbids records n there.
//          The first workgroup of a job writes the decoded length.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "base/base64.h"
#include "gpu/kernels.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

namespace b64 = ::mrpc::base64;
using wg::u32x4;
constexpr int kB64Threads = 256;
constexpr uint32_t kLaneBytes = 12, kLaneSymbols = 16;
static_assert(kB64Threads * kLaneBytes == kBase64ChunkBytes, "a lane per 12 bytes");
static_assert(kB64Threads * kLaneSymbols == kBase64ChunkSymbols, "a lane per 16 symbols");

constexpr int kEncStage16 = (int)(kBase64ChunkBytes + 15 + 15) / 16 + 1;  // the span at any phase, and a dword to spare
constexpr int kEncImage16 = (int)kBase64ChunkSymbols / 16 + 1;            // copy_out_shifted reads one dword past

__global__ void __launch_bounds__(kB64Threads) base64_encode_kernel(const Base64Job* __restrict__ jobs, int njobs) {
    __shared__ u32x4 staged[kEncStage16];
    __shared__ u32x4 image16[kEncImage16];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&Base64Job::first_block>(jobs, njobs, blockIdx.x);
    const Base64Job job = jobs[ji];
    const uint64_t at = (uint64_t)(blockIdx.x - job.first_block) * kBase64ChunkBytes;
    if (at >= job.n) return;  // uniform: a block the host did not mean for this job
    const uint32_t left = job.n - (uint32_t)at;
    const uint32_t len = left < kBase64ChunkBytes ? left : kBase64ChunkBytes;  // data bytes of this chunk
    const uint8_t* src = job.src + at;
    uint8_t* dst = job.dst + (at / 3) * 4;
    const uint32_t a = wg::stage16<kB64Threads, 1>(src, len, staged);  // at most 193 units
    __syncthreads();
    const uint32_t* stage = reinterpret_cast<const uint32_t*>(staged);
    const uint32_t mine = 12 * t < len ? (len - 12 * t < 12 ? len - 12 * t : 12u) : 0u;  // data bytes of this lane
    const uint32_t w = (a + 12 * t) >> 2, sh = (a & 3) * 8;
    const uint32_t d0 = stage[w], d1 = stage[w + 1], d2 = stage[w + 2], d3 = stage[w + 3];
    uint32_t b0 = wg::funnel(d0, d1, sh), b1 = wg::funnel(d1, d2, sh), b2 = wg::funnel(d2, d3, sh);
    if (mine < 12) {  // what lies past the data counts as zero bits
        const uint64_t keep01 = mine >= 8 ? ~0ull : ((1ull << (8 * mine)) - 1);
        b0 &= (uint32_t)keep01;
        b1 &= (uint32_t)(keep01 >> 32);
        b2 &= mine > 8 ? (1u << (8 * (mine - 8))) - 1 : 0u;
    }
    u32x4 sym;
    sym.x = b64::Encode3LE(b0);
    sym.y = b64::Encode3LE((b0 >> 24) | (b1 << 8));
    sym.z = b64::Encode3LE((b1 >> 16) | (b2 << 16));
    sym.w = b64::Encode3LE(b2 >> 8);
    const uint32_t rem = mine % 3;
    if (mine < 12 && rem != 0) {  // the job's last lane: pad its last group
        const uint32_t keep = rem == 1 ? 0x0000FFFFu : 0x00FFFFFFu, pad = rem == 1 ? 0x3D3D0000u : 0x3D000000u;
        const uint32_t g = mine / 3;
        if (g == 0) sym.x = (sym.x & keep) | pad;
        if (g == 1) sym.y = (sym.y & keep) | pad;
        if (g == 2) sym.z = (sym.z & keep) | pad;
        if (g == 3) sym.w = (sym.w & keep) | pad;
    }
    const uint32_t total = (len + 2) / 3 * 4;  // symbols of this chunk
    if (((uintptr_t)dst & 15) == 0 && len == kBase64ChunkBytes) {
        reinterpret_cast<u32x4*>(dst)[t] = sym;
        return;
    }
    image16[t] = sym;
    __syncthreads();
    wg::copy_out_shifted<kB64Threads>(reinterpret_cast<const uint32_t*>(image16), 0, dst, total);
}

constexpr int kDecImage16 = (int)kBase64ChunkBytes / 16 + 1;  // copy_out_shifted reads one dword past

__global__ void __launch_bounds__(kB64Threads) base64_decode_kernel(const Base64Job* __restrict__ jobs, int njobs,
                                                                    JsonNumberResult* __restrict__ res) {
    __shared__ u32x4 image16[kDecImage16];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&Base64Job::first_block>(jobs, njobs, blockIdx.x);
    const Base64Job job = jobs[ji];
    const uint32_t n = job.n;
    const uint64_t at = (uint64_t)(blockIdx.x - job.first_block) * kBase64ChunkSymbols;
    if (at >= n) return;  // uniform
    // the padding, and with it the body [0, m), from the text's last two bytes
    uint32_t p = 0;
    if (job.src[n - 1] == '=') p = n >= 2 && job.src[n - 2] == '=' ? 2 : 1;
    const uint32_t m = n - p;
    if (at == 0 && t == 0) {
        if (m % 4 == 1 || (p != 0 && n % 4 != 0)) atomicMin(&res[ji].bad, n);
        res[ji].n_redo = m / 4 * 3 + (m % 4) * 3 / 4;  // the decoded length
    }
    const uint8_t* src = job.src + at;
    const uint32_t left = n - (uint32_t)at;                                     // text bytes from here
    const uint32_t body = m > at ? (uint32_t)(m - at) : 0u;                     // body symbols from here
    const uint32_t text_mine = 16 * t < left ? (left - 16 * t < 16 ? left - 16 * t : 16u) : 0u;
    const uint32_t mine = 16 * t < body ? (body - 16 * t < 16 ? body - 16 * t : 16u) : 0u;  // body symbols of this lane
    uint32_t s[4] = {0x41414141u, 0x41414141u, 0x41414141u, 0x41414141u};  // 'A': zero bits
    if (text_mine == 16) {
        const uint8_t* mp = src + 16 * t;
        const uint32_t a = (uint32_t)((uintptr_t)mp & 15);  // uniform
        const u32x4* lo = reinterpret_cast<const u32x4*>(mp - a);
        const u32x4 x = lo[0];
        if (a == 0) {
            s[0] = x.x, s[1] = x.y, s[2] = x.z, s[3] = x.w;
        } else {
            // the second unit starts before this lane's last symbol: it holds text
            const u32x4 y = lo[1];
            const uint32_t d[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
            const uint32_t w = a >> 2, sh = (a & 3) * 8;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t lo32 = 0, hi32 = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {  // static indices: w selects without a private array
                    if (w == (uint32_t)q) {
                        lo32 = d[q + k];
                        hi32 = d[q + k + 1 < 8 ? q + k + 1 : 7];
                    }
                }
                s[k] = wg::funnel(lo32, hi32, sh);
            }
        }
    } else if (text_mine != 0) {  // the text's last lane: byte by byte
        const uint8_t* mp = src + 16 * t;
        for (uint32_t k = 0; k < text_mine; ++k) {
            const uint32_t c = mp[k], q = k >> 2, b = (k & 3) * 8;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (q == (uint32_t)g) s[g] = (s[g] & ~(0xFFu << b)) | (c << b);
            }
        }
    }
    if (mine < 16) {  // padding and what lies past the body count as zero bits
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t have = mine > 4 * (uint32_t)g ? mine - 4 * (uint32_t)g : 0u;  // body symbols in this group
            if (have < 4) {
                const uint32_t keep = have == 0 ? 0u : (1u << (8 * have)) - 1;
                s[g] = (s[g] & keep) | (0x41414141u & ~keep);
            }
        }
    }
    uint32_t x[4];
    bool all_ok = true;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bool ok;
        x[g] = b64::Bytes3LE(b64::Decode4(s[g], &ok));
        all_ok = all_ok && ok;
    }
    if (!all_ok) {  // the lowest offset of a byte outside the alphabet
        uint32_t first = 16;
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            if (b64::Value((uint8_t)(s[k >> 2] >> ((k & 3) * 8))) < 0) first = (uint32_t)k;
        }
        if (first < mine) atomicMin(&res[ji].bad, (uint32_t)at + 16 * t + first);
    }
    uint32_t* image = reinterpret_cast<uint32_t*>(image16);
    image[3 * t] = x[0] | x[1] << 24;
    image[3 * t + 1] = x[1] >> 8 | x[2] << 16;
    image[3 * t + 2] = x[2] >> 16 | x[3] << 8;
    __syncthreads();
    const uint32_t chunk_syms = body < kBase64ChunkSymbols ? body : kBase64ChunkSymbols;
    const uint32_t total = chunk_syms / 4 * 3 + (chunk_syms % 4) * 3 / 4;
    wg::copy_out_shifted<kB64Threads>(image, 0, job.dst + (at / 4) * 3, total);
}

}  // namespace

int LaunchBase64Encode(const Base64Job* jobs, int njobs, uint32_t nblocks, hipStream_t s) {
    if (njobs <= 0 || nblocks == 0) return 0;
    if (!jobs) return -1;
    hipLaunchKernelGGL(base64_encode_kernel, dim3(nblocks), dim3(kB64Threads), 0, s, jobs, njobs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchBase64Decode(const Base64Job* jobs, int njobs, uint32_t nblocks, JsonNumberResult* res_dev,
                       JsonNumberResult* res_out, hipStream_t s) {
    if (njobs <= 0 || nblocks == 0) return 0;
    if (!jobs || !res_dev || !res_out) return -1;
    if (LaunchJsonNumberResultInit(res_dev, njobs, s) != 0) return -1;
    hipLaunchKernelGGL(base64_decode_kernel, dim3(nblocks), dim3(kB64Threads), 0, s, jobs, njobs, res_dev);
    if (hipGetLastError() != hipSuccess) return -1;
    return LaunchJsonNumberResultPublish(res_dev, res_out, njobs, s);
}

}  // namespace gpu
}  // namespace mrpc
