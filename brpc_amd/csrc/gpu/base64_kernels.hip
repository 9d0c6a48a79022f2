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
#include "base/base64_rows.h"
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

// ------------------------------------------------------------------- rows
// (bytes, row_ends) <-> the text of a JSON array of base64 strings; kernels.h
// Base64RowsJob has the passes, base/base64_rows.h the rules.

namespace {

namespace br = ::mrpc::base64_rows;
namespace jr = ::mrpc::json_string_rows;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kEC = kBase64RowsEncodeChunkBytes, kDC = kBase64RowsDecodeChunkBytes;
static_assert(kB64Threads * kLaneBytes == kEC, "a lane per 12 bytes");
static_assert(kB64Threads * 16 == kDC, "a lane per 16 bytes of text");
static_assert(kB64Threads == kBase64RowsBlockRows, "a lane per row of a row block");

// ---- encode

__device__ __forceinline__ uint32_t b64r_row_blocks(uint32_t rows) {
    return (uint32_t)(((uint64_t)rows + kBase64RowsBlockRows - 1) / kBase64RowsBlockRows);
}

__global__ void __launch_bounds__(kB64Threads) b64r_rows_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                                                uint32_t* __restrict__ ends, uint32_t* __restrict__ rowoff,
                                                                uint32_t* __restrict__ prefix, uint32_t* __restrict__ bad) {
    __shared__ uint32_t part[kB64Threads / 64];
    const int ji = wg::job_of<&Base64RowsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const Base64RowsJob job = jobs[ji];
    const uint64_t r = (uint64_t)(blockIdx.x - job.first_rblock) * kBase64RowsBlockRows + threadIdx.x;
    const bool live = r < job.rows;
    uint32_t symbols = 0;
    if (live) {
        const uint32_t end = job.row_ends[r], prev = r ? job.row_ends[r - 1] : 0u;
        ends[job.first_row + r] = end;
        if (end < prev || end > job.n || (r == job.rows - 1 && end != job.n)) atomicMin(&bad[ji], (uint32_t)r);
        else symbols = (uint32_t)b64::Base64EncodedBytes(end - prev);
    }
    uint32_t total;
    const uint32_t before = wg::block_excl_scan<kB64Threads>(symbols, part, &total);
    if (live) rowoff[job.first_row + r] = before;
    if (threadIdx.x == 0) prefix[blockIdx.x] = total;
}

__global__ void b64r_encode_verdict_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                           const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ bad,
                                           int32_t* __restrict__ ok, Base64RowsResult* __restrict__ res) {
    const int ji = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (ji >= njobs) return;
    const Base64RowsJob job = jobs[ji];
    const uint64_t symbols = (uint32_t)(prefix[job.first_rblock + b64r_row_blocks(job.rows)] - prefix[job.first_rblock]);
    Base64RowsResult r;
    r.len = (job.rows ? symbols + 3ull * job.rows - 1 : 0ull) + (job.brackets ? 2u : 0u);
    r.rows = r.first_bad = r.depth = 0;
    r.err = 0;
    const uint32_t b = bad[ji];
    if (b != kNone) {
        r.err = 1;
        r.first_bad = b;
        r.len = 0;
    } else if (r.len > job.cap) {
        r.err = 3;
    } else if (job.brackets) {
        job.dst[0] = '[';
        job.dst[r.len - 1] = ']';
    }
    ok[ji] = r.err == 0;
    res[ji] = r;
}

// Where the text of row r begins (its opening quote), r < rows.
__device__ __forceinline__ uint64_t b64r_row_text(const Base64RowsJob& job, const uint32_t* __restrict__ prefix,
                                                  const uint32_t* __restrict__ rowoff, uint32_t r) {
    const uint32_t symbols = prefix[job.first_rblock + r / kBase64RowsBlockRows] - prefix[job.first_rblock] +
                             rowoff[job.first_row + r];
    return (uint64_t)symbols + 3ull * r + (job.brackets ? 1u : 0u);
}

__global__ void __launch_bounds__(kB64Threads) b64r_punct_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                                                 const uint32_t* __restrict__ ends,
                                                                 const uint32_t* __restrict__ rowoff,
                                                                 const uint32_t* __restrict__ prefix,
                                                                 const int32_t* __restrict__ ok) {
    const int ji = wg::job_of<&Base64RowsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const Base64RowsJob job = jobs[ji];
    if (!ok[ji]) return;
    const uint64_t r64 = (uint64_t)(blockIdx.x - job.first_rblock) * kBase64RowsBlockRows + threadIdx.x;
    if (r64 >= job.rows) return;
    const uint32_t r = (uint32_t)r64;
    const uint32_t* e = ends + job.first_row;
    const uint32_t start = r ? e[r - 1] : 0u, end = e[r];
    const uint64_t o = b64r_row_text(job, prefix, rowoff, r);
    const uint64_t close = o + br::Base64RowTextBytes(end >= start ? end - start : 0u) - 1;
    if (o < job.cap) job.dst[o] = '"';
    if (close < job.cap) job.dst[close] = '"';
    if (r + 1 < job.rows && close + 1 < job.cap) job.dst[close + 1] = ',';
}

// The first row of [lo, hi] whose end lies beyond byte x; hi when none does.
__device__ __forceinline__ uint32_t b64r_row_of(const uint32_t* __restrict__ e, uint32_t lo, uint32_t hi, uint32_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (e[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

constexpr int kRowsEncStage16 = (int)(kEC + 2 + 15 + 15) / 16 + 1;  // the span with two bytes beyond, and a dword to spare

__global__ void __launch_bounds__(kB64Threads) b64r_encode_place_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                                                        const uint32_t* __restrict__ ends,
                                                                        const uint32_t* __restrict__ rowoff,
                                                                        const uint32_t* __restrict__ prefix,
                                                                        const int32_t* __restrict__ ok) {
    __shared__ u32x4 staged[kRowsEncStage16];
    __shared__ u32x4 image16[kEncImage16];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&Base64RowsJob::first_chunk>(jobs, njobs, blockIdx.x);
    const Base64RowsJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks || !ok[ji] || job.rows == 0) return;  // uniform
    const uint32_t at = c * kEC, left = job.n - at, len = left < kEC ? left : kEC;
    const uint32_t span = left < kEC + 2 ? left : kEC + 2;  // a group that starts in the chunk may end beyond it
    const uint32_t a = wg::stage16<kB64Threads, 2>(job.src + at, span, staged);
    __syncthreads();
    const uint32_t* e = ends + job.first_row;
    // ok: the ends ascend to n, so a row ends beyond every byte of the chunk
    const uint32_t r0 = b64r_row_of(e, 0, job.rows - 1, at);
    const uint32_t r1 = b64r_row_of(e, r0, job.rows - 1, at + len - 1);
    if (r1 - r0 < kBase64RowsSegmentRows) {  // few rows: the symbols of each row's part leave as one segment
        const uint32_t* stage = reinterpret_cast<const uint32_t*>(staged);
        for (uint32_t r = r0; r <= r1; ++r) {
            const uint32_t start = r ? e[r - 1] : 0u, end = e[r];
            const uint32_t lo = start > at ? start : at, hi = end < at + len ? end : at + len;
            if (hi <= lo) continue;                         // uniform
            const uint32_t g0 = (lo - start + 2) / 3;       // the first group that starts in the chunk
            const uint32_t s0 = start + 3 * g0;
            if (s0 >= hi) continue;                         // uniform
            const uint32_t ng = (hi - s0 + 2) / 3;          // groups that start in [s0, hi): at most kEC / 3
            const uint32_t groups = 4 * t < ng ? (ng - 4 * t < 4 ? ng - 4 * t : 4u) : 0u;
            if (groups) {
                const uint32_t from = s0 + 12 * t;
                const uint32_t upto = from + 3 * groups < end ? from + 3 * groups : end;
                const uint32_t mine = upto - from;  // 1..12, cut by the row's end only
                const uint32_t q = a + (from - at);
                const uint32_t w = q >> 2, sh = (q & 3) * 8;
                const uint32_t d0 = stage[w], d1 = stage[w + 1], d2 = stage[w + 2], d3 = stage[w + 3];
                uint32_t b0 = wg::funnel(d0, d1, sh), b1 = wg::funnel(d1, d2, sh), b2 = wg::funnel(d2, d3, sh);
                if (mine < 12) {
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
                if (rem != 0) {  // the row's last group: pad it
                    const uint32_t keep = rem == 1 ? 0x0000FFFFu : 0x00FFFFFFu, pad = rem == 1 ? 0x3D3D0000u : 0x3D000000u;
                    const uint32_t g = mine / 3;
                    if (g == 0) sym.x = (sym.x & keep) | pad;
                    if (g == 1) sym.y = (sym.y & keep) | pad;
                    if (g == 2) sym.z = (sym.z & keep) | pad;
                    if (g == 3) sym.w = (sym.w & keep) | pad;
                }
                image16[t] = sym;
            }
            __syncthreads();
            const uint64_t o = b64r_row_text(job, prefix, rowoff, r) + 1 + 4ull * g0;
            if (o + 4ull * ng <= job.cap)
                wg::copy_out_shifted<kB64Threads>(reinterpret_cast<const uint32_t*>(image16), 0, job.dst + o, 4 * ng);
            __syncthreads();  // the image is rewritten for the next row
        }
        return;
    }
    // many rows: every lane stores the groups that start in its own bytes
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(staged) + a;  // bytes[i - at] is job byte i
    uint32_t pos = at + kLaneBytes * t;
    const uint32_t stop = pos + kLaneBytes < at + len ? pos + kLaneBytes : at + len;
    if (pos >= stop) return;
    uint32_t r = b64r_row_of(e, r0, r1, pos);
    uint32_t start = r ? e[r - 1] : 0u, end = e[r];
    uint64_t text = b64r_row_text(job, prefix, rowoff, r);
    while (pos < stop) {
        if (pos >= end) {  // into a later row: one search past every row that ends here
            if (r >= r1) return;  // cannot be: the last row of the chunk ends beyond it
            r = b64r_row_of(e, r + 1, r1, pos);
            start = e[r - 1], end = e[r];
            text = b64r_row_text(job, prefix, rowoff, r);
            if (pos >= end || pos < start) return;  // cannot be while ends[] ascends to n
        }
        const uint32_t off = pos - start, phase = off % 3;
        if (phase != 0) {  // a group the lane below, or the chunk before, owns
            const uint32_t next = pos + (3 - phase);
            pos = next < end ? next : end;
            continue;
        }
        const uint32_t nb = end - pos < 3 ? end - pos : 3u;
        uint32_t le = 0;
        for (uint32_t k = 0; k < nb; ++k) le |= (uint32_t)bytes[pos - at + k] << (8 * k);
        uint32_t sym = b64::Encode3LE(le);
        if (nb == 1) sym = (sym & 0x0000FFFFu) | 0x3D3D0000u;
        if (nb == 2) sym = (sym & 0x00FFFFFFu) | 0x3D000000u;
        const uint64_t o = text + 1 + 4ull * (off / 3);
        if (o + 4 <= job.cap) {
            uint8_t* d = job.dst + o;
            d[0] = (uint8_t)sym, d[1] = (uint8_t)(sym >> 8), d[2] = (uint8_t)(sym >> 16), d[3] = (uint8_t)(sym >> 24);
        }
        pos += nb;
    }
}

// ---- decode

// The carried state: 0..4 outside a string after that kind of token (jr::Kind),
// 5..8 inside one at body offset mod 4. A chunk's exit may also be kDrRel
// (entered inside and no quote met: the entry's phase moves on by the chunk's
// length) or kDrPass (entered outside and no token met: the entry's kind stays).
constexpr uint32_t kDrInside = 5, kDrStates = 9, kDrRel = 14, kDrPass = 15;
enum { kDwSize = 0, kDwClose = 1, kDwBad = 2, kDwFirst = 3, kDwBracket = 4, kDwExit = 5 };
constexpr uint32_t kDwEntry = 6, kDwLeadSize = 12, kDwLeadBad = 16, kDwChosen = 20;
static_assert(kDwChosen < kBase64RowsInfoWords, "the info words of a chunk");

// The staged text of a chunk: job bytes [at - 4, at + len + 4) cut to [0, n),
// behind one unit nobody reads a valid byte from, so that a lane may load the
// four bytes in front of byte 0. lds byte pos0 + (i - at) is job byte i.
constexpr int kRowsDecStage16 = 1 + (int)(4 + 15 + kDC + 4 + 15) / 16 + 1;
__device__ __forceinline__ uint32_t b64r_stage_text(u32x4* lds, const uint8_t* src, uint32_t n, uint32_t at, uint32_t len) {
    const uint32_t lo = at < 4 ? 0u : at - 4;
    const uint64_t want = (uint64_t)at + len + 4;
    const uint32_t hi = want > n ? n : (uint32_t)want;
    const uint32_t a = wg::stage16<kB64Threads, 2>(src + lo, hi - lo, lds + 1);
    return 16 + a + (at - lo);
}

// A bit per byte of the lane's window, the 24 bytes from four in front of its
// own 16: bit k is job byte i0 - 4 + k; bytes outside the job are nothing.
struct DrBits {
    uint32_t sym, eq, quote, ws, lb, comma, rb, own;
};
__device__ __forceinline__ DrBits b64r_lane_bits(const u32x4* lds, uint32_t pos0, uint32_t at, uint32_t len, uint32_t n) {
    const uint32_t t = threadIdx.x;
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(lds);
    const uint32_t q = pos0 + 16 * t - 4, w = q >> 2, sh = (q & 3) * 8;
    uint32_t d[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] = dw[w + k];
    const uint64_t i0 = (uint64_t)at + 16 * t;
    DrBits b = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 24; ++k) {
        const uint32_t word = wg::funnel(d[k >> 2], d[(k >> 2) + 1], sh);
        const uint8_t ch = (uint8_t)(word >> (8 * (k & 3)));
        const bool valid = i0 + k >= 4 && i0 + k - 4 < n;
        b.sym |= (uint32_t)(valid && br::IsSymbol(ch)) << k;
        b.eq |= (uint32_t)(valid && ch == '=') << k;
        b.quote |= (uint32_t)(valid && ch == '"') << k;
        b.ws |= (uint32_t)(valid && number_text::IsSpace((char)ch)) << k;
        b.lb |= (uint32_t)(valid && ch == '[') << k;
        b.comma |= (uint32_t)(valid && ch == ',') << k;
        b.rb |= (uint32_t)(valid && ch == ']') << k;
    }
    const uint32_t o = 16 * t, mine = o < len ? (len - o < 16 ? len - o : 16u) : 0u;
    b.own = ((1u << mine) - 1) << 4;
    return b;
}

// What lies in front of the lane within its chunk: the parity of the quotes,
// and the last quote as its offset in the chunk + 1 (0: none). *chunk_par and
// *chunk_last are those of the whole chunk. One barrier.
__device__ __forceinline__ void b64r_quotes_before(const DrBits& b, uint32_t* wave_par, uint32_t* wave_last, uint32_t* par,
                                                   uint32_t* last, uint32_t* chunk_par, uint32_t* chunk_last) {
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t mq = b.quote & b.own;
    const uint64_t odd = __ballot(__popc(mq) & 1);
    const uint32_t my_last = mq ? 16 * t + (31 - (uint32_t)__builtin_clz(mq)) - 4 + 1 : 0u;
    const uint32_t incl = wg::wave_incl_scan(my_last, [](uint32_t p, uint32_t q) { return p > q ? p : q; });
    if (lane == 63) wave_last[wave] = incl;
    if (lane == 0) wave_par[wave] = (uint32_t)__popcll(odd) & 1;
    __syncthreads();
    uint32_t p = (uint32_t)__popcll(odd & ((1ull << lane) - 1)) & 1;
    uint32_t l = wg::wave_prev(incl);
    if (lane == 0) l = 0;
    uint32_t cp = 0, cl = 0;
#pragma unroll
    for (uint32_t k = 0; k < kB64Threads / 64; ++k) {
        if (k < wave) {
            p ^= wave_par[k];
            l = l > wave_last[k] ? l : wave_last[k];
        }
        cp ^= wave_par[k];
        cl = cl > wave_last[k] ? cl : wave_last[k];
    }
    *par = p, *last = l, *chunk_par = cp, *chunk_last = cl;
}

struct DrLane {
    uint32_t size, nclose, bad, first, last, rb;
    uint32_t groups, s1, s2, s3, closing;  // window bits: group starts, and how far each group's symbols go
};
// What the lane's bytes hold when its byte 0 lies inside a string (inside != 0)
// at body offset a0 mod 4, or outside one. A token is the word
// (offset in the chunk) << 3 | kind; first / last: the lane's, kNone / 0 when
// it has none. Tokens after its first are judged here, against the token
// before them; bad and rb are job offsets.
__device__ __forceinline__ DrLane b64r_lane(const DrBits& b, uint32_t at, uint32_t a0, uint32_t inside) {
    const uint32_t t = threadIdx.x;
    const uint32_t mq = b.quote & b.own;
    // the in-string mask: the state in front, flipped by every quote below the byte
    uint32_t px = mq;
    px ^= px << 1;
    px ^= px << 2;
    px ^= px << 4;
    px ^= px << 8;
    px ^= px << 16;
    const uint32_t in = ((px << 1) ^ (inside ? ~0u : 0u)) & b.own;
    // the body offset mod 4 of every byte as two bit planes: bit k holds (k + a) mod 4, a set anew behind a quote
    uint32_t lo = 0xAAAAAAAAu >> (a0 & 3), hi = 0xCCCCCCCCu >> (a0 & 3);
    for (uint32_t qs = mq; qs; qs &= qs - 1) {
        const uint32_t q = (uint32_t)__builtin_ctz(qs), above = ~((2u << q) - 1), a = ~q & 3;
        lo = (lo & ~above) | ((0xAAAAAAAAu >> a) & above);
        hi = (hi & ~above) | ((0xCCCCCCCCu >> a) & above);
    }
    const uint32_t p0 = ~lo & ~hi, p1 = lo & ~hi;
    const uint32_t content = in & ~mq, closing = mq & in;
    const uint32_t prev_sym = b.sym << 1, prev_eq = b.eq << 1;
    const uint32_t outside = ~in & ~mq & b.own;
    const uint32_t faults = (content & ((b.sym & prev_eq) | (b.eq & ~hi) | ~(b.sym | b.eq))) |
                            (closing & ((prev_sym & p1) | (prev_eq & ~p0))) |
                            (outside & ~(b.ws | b.lb | b.comma | b.rb));
    DrLane r;
    const uint32_t i0 = at + 16 * t;
    r.bad = faults ? i0 + (uint32_t)__builtin_ctz(faults) - 4 : kNone;
    r.nclose = (uint32_t)__popc(closing);
    r.closing = closing;
    r.groups = content & b.sym & p0;
    r.s1 = b.sym >> 1;
    r.s2 = r.s1 & (b.sym >> 2);
    r.s3 = r.s2 & (b.sym >> 3);
    r.size = 3 * (uint32_t)__popc(r.groups & r.s3) + 2 * (uint32_t)__popc(r.groups & r.s2 & ~r.s3) +
             (uint32_t)__popc(r.groups & r.s1 & ~r.s2);
    r.first = kNone;
    r.last = 0;
    r.rb = kNone;
    uint32_t pred = 0;  // no token of this lane yet (kStart is no token)
    for (uint32_t tokens = mq | (outside & (b.lb | b.comma | b.rb)); tokens; tokens &= tokens - 1) {
        const uint32_t k = (uint32_t)__builtin_ctz(tokens), bit = 1u << k;
        const uint32_t kind = (mq & bit)        ? ((in & bit) ? jr::kCloseQuote : jr::kOpenQuote)
                              : (b.lb & bit)    ? jr::kOpenBracket
                              : (b.comma & bit) ? jr::kComma
                                                : jr::kCloseBracket;
        const uint32_t where = i0 + k - 4;
        r.last = (16 * t + k - 4) << 3 | kind;
        if (pred == 0) r.first = r.last;
        else if (!jr::Follows(pred, kind) && where < r.bad) r.bad = where;
        if (kind == jr::kCloseBracket && r.rb == kNone) r.rb = where;
        pred = kind;
    }
    return r;
}

__device__ __forceinline__ uint32_t b64r_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

__global__ void __launch_bounds__(kB64Threads) b64r_scan_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                                                uint32_t* __restrict__ info) {
    __shared__ u32x4 stage16[kRowsDecStage16];
    __shared__ uint32_t wave_par[4], wave_lastq[4];
    __shared__ uint32_t wave_last[2][4];  // the last token of each wave, per entry
    __shared__ uint32_t acc[kBase64RowsInfoWords];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ji = wg::job_of<&Base64RowsJob::first_chunk>(jobs, njobs, blockIdx.x);
    const Base64RowsJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks) return;  // uniform
    const uint32_t at = c * kDC, left = job.n - at, len = left < kDC ? left : kDC;
    const uint32_t pos0 = b64r_stage_text(stage16, job.src, job.n, at, len);
    if (t < kBase64RowsInfoWords) {
        const uint32_t k = t < kDwLeadSize ? t % kDwEntry : 0;
        const bool lowest = t < kDwLeadSize ? (k == kDwBad || k == kDwFirst || k == kDwBracket) : (t >= kDwLeadBad && t < kDwChosen);
        acc[t] = lowest ? kNone : 0u;
    }
    __syncthreads();
    const DrBits b = b64r_lane_bits(stage16, pos0, at, len, job.n);
    uint32_t par, lastq, chunk_par, chunk_lastq;
    b64r_quotes_before(b, wave_par, wave_lastq, &par, &lastq, &chunk_par, &chunk_lastq);
    // entry 0: the chunk begins outside a string. entry 1: inside one, every state the other way round; the lanes
    // in front of the chunk's first quote (lead) then count their body offsets from the entry's phase
    const bool lead = lastq == 0;
    const uint32_t a_lane = (16 * t - lastq) & 3;  // body offset of the lane's byte 0 behind the last quote
    DrLane v[2];
    v[0] = b64r_lane(b, at, a_lane, par);
    v[1] = b64r_lane(b, at, lead ? 0u : a_lane, par ^ 1u);
    if (b.own != 0) {
        if (v[0].size) atomicAdd(&acc[kDwSize], v[0].size);
        if (v[0].bad != kNone) atomicMin(&acc[kDwBad], v[0].bad);
        if (!lead) {
            if (v[1].size) atomicAdd(&acc[kDwEntry + kDwSize], v[1].size);
            if (v[1].bad != kNone) atomicMin(&acc[kDwEntry + kDwBad], v[1].bad);
        } else {
#pragma unroll
            for (uint32_t ph = 0; ph < 4; ++ph) {
                const DrLane x = ph == 0 ? v[1] : b64r_lane(b, at, ph, 1u);
                if (x.size) atomicAdd(&acc[kDwLeadSize + ph], x.size);
                if (x.bad != kNone) atomicMin(&acc[kDwLeadBad + ph], x.bad);
            }
        }
    }
    uint32_t prev[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t nclose = wg::wave_sum(v[e].nclose);
        if (lane == 0 && nclose) atomicAdd(&acc[e * kDwEntry + kDwClose], nclose);
        if (v[e].rb != kNone) atomicMin(&acc[e * kDwEntry + kDwBracket], v[e].rb);
        // the last token in front of the lane: tokens ascend with the lanes, so the highest word below it
        const uint32_t incl = wg::wave_incl_scan(v[e].last, [](uint32_t p, uint32_t q) { return b64r_max(p, q); });
        if (lane == 63) wave_last[e][wave] = incl;
        prev[e] = wg::wave_prev(incl);
        if (lane == 0) prev[e] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        uint32_t last = 0;
#pragma unroll
        for (uint32_t k = 0; k < kB64Threads / 64; ++k) {
            if (k < wave) prev[e] = b64r_max(prev[e], wave_last[e][k]);
            last = b64r_max(last, wave_last[e][k]);
        }
        if (v[e].first != kNone) {
            // the lane's first token: judged against the token before it in the chunk; the chunk's first is the
            // carry kernel's to judge
            if (prev[e] == 0) atomicMin(&acc[e * kDwEntry + kDwFirst], v[e].first);
            else if (!jr::Follows(prev[e] & 7, v[e].first & 7)) atomicMin(&acc[e * kDwEntry + kDwBad], at + (v[e].first >> 3));
        }
        if (t == 0) {
            const uint32_t inside = (uint32_t)e ^ chunk_par;
            uint32_t exit = last ? (last & 7) : kDrPass;
            if (inside) exit = chunk_lastq ? kDrInside + ((len - chunk_lastq) & 3) : kDrRel;
            acc[e * kDwEntry + kDwExit] = exit;
        }
    }
    __syncthreads();
    if (t < kBase64RowsInfoWords) info[(uint64_t)blockIdx.x * kBase64RowsInfoWords + t] = acc[t];
}

// maps of the nine states to themselves, four bits per image
__device__ __forceinline__ uint64_t b64r_then(uint64_t f, uint64_t g) {  // first f, then g
    uint64_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < kDrStates; ++s) r |= ((g >> (4 * ((f >> (4 * s)) & 15))) & 15) << (4 * s);
    return r;
}
constexpr uint64_t kDrIdentity = 0x876543210ull;

__global__ void __launch_bounds__(kB64Threads) b64r_carry_kernel(const Base64RowsJob* __restrict__ jobs,
                                                                 uint32_t* __restrict__ info, uint32_t* __restrict__ prefix,
                                                                 uint32_t nchunks_all, uint32_t* __restrict__ state) {
    __shared__ uint64_t wave_map[kB64Threads / 64];
    __shared__ uint32_t low[3];  // lowest offender, first ']' outside, depth
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const Base64RowsJob job = jobs[blockIdx.x];
    if (t < 3) low[t] = t == 2 ? 0u : kNone;
    uint32_t carry = jr::kStart, lowest = kNone, bracket = kNone;
    for (uint32_t base = 0; base < job.nchunks; base += kB64Threads) {
        const uint32_t c = base + t;
        uint32_t* mine = info + (uint64_t)(job.first_chunk + c) * kBase64RowsInfoWords;
        uint64_t map = kDrIdentity;
        if (c < job.nchunks) {
            const uint32_t e0 = mine[kDwExit], e1 = mine[kDwEntry + kDwExit];
            const uint32_t left = job.n - c * kDC, len = left < kDC ? left : kDC;
            map = 0;
#pragma unroll
            for (uint32_t s = 0; s < kDrInside; ++s) map |= (uint64_t)(e0 == kDrPass ? s : e0) << (4 * s);
#pragma unroll
            for (uint32_t ph = 0; ph < 4; ++ph)
                map |= (uint64_t)(e1 == kDrRel ? kDrInside + ((ph + len) & 3) : e1) << (4 * (kDrInside + ph));
        }
        const uint64_t incl = wg::wave_incl_scan(map, [](uint64_t f, uint64_t g) { return b64r_then(f, g); });
        if (lane == 63) wave_map[wave] = incl;
        __syncthreads();
        uint64_t excl = wg::wave_prev(incl);
        if (lane == 0) excl = kDrIdentity;
        uint64_t front = kDrIdentity, tile = kDrIdentity;
        for (uint32_t k = 0; k < kB64Threads / 64; ++k) {
            if (k < wave) front = b64r_then(front, wave_map[k]);
            tile = b64r_then(tile, wave_map[k]);
        }
        const uint32_t st = (uint32_t)(b64r_then(front, excl) >> (4 * carry)) & 15;
        if (c < job.nchunks) {
            const uint32_t* w = mine + (st < kDrInside ? 0u : kDwEntry);
            uint32_t size = w[kDwSize], bad = w[kDwBad];
            if (st >= kDrInside) {
                size += mine[kDwLeadSize + st - kDrInside];
                bad = bad < mine[kDwLeadBad + st - kDrInside] ? bad : mine[kDwLeadBad + st - kDrInside];
            }
            prefix[job.first_chunk + c] = size;
            prefix[nchunks_all + 1 + job.first_chunk + c] = w[kDwClose];
            mine[kDwChosen] = st;
            if (bad < lowest) lowest = bad;
            if (w[kDwBracket] < bracket) bracket = w[kDwBracket];
            if (st < kDrInside && w[kDwFirst] != kNone) {  // the chunk's first token, against its true predecessor
                const uint32_t kind = w[kDwFirst] & 7, where = c * kDC + (w[kDwFirst] >> 3);
                if (!jr::Follows(st, kind) && where < lowest) lowest = where;
                if (st == jr::kStart && kind == jr::kOpenBracket) low[2] = 1;  // the text's first token
            }
        }
        carry = (uint32_t)(tile >> (4 * carry)) & 15;
        __syncthreads();  // wave_map is rewritten by the next tile
    }
    if (lowest != kNone) atomicMin(&low[0], lowest);
    if (bracket != kNone) atomicMin(&low[1], bracket);
    __syncthreads();
    if (t == 0) {
        uint32_t* st = state + (uint64_t)blockIdx.x * kBase64RowsStateWords;
        st[0] = low[0];
        st[1] = carry;
        st[2] = low[2];
        st[3] = low[1];
    }
}

// a lane per job, after the prefix scan over both tables
__global__ void b64r_decode_verdict_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                           const uint32_t* __restrict__ prefix, uint32_t nchunks_all,
                                           const uint32_t* __restrict__ state, int32_t* __restrict__ ok,
                                           Base64RowsResult* __restrict__ res) {
    const int ji = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (ji >= njobs) return;
    const Base64RowsJob job = jobs[ji];
    const uint32_t* bytes = prefix + job.first_chunk;
    const uint32_t* quotes = bytes + nchunks_all + 1;
    const uint32_t* st = state + (uint64_t)ji * kBase64RowsStateWords;
    const uint32_t depth = st[2];
    uint32_t bad = st[0];
    if (depth == 0 && st[3] < bad) bad = st[3];                    // a ']' without its '['
    if (bad == kNone && !jr::EndsWell(st[1], depth)) bad = job.n;  // the text ends too soon, inside a string too
    Base64RowsResult r;
    r.len = (uint32_t)(bytes[job.nchunks] - bytes[0]);
    r.rows = quotes[job.nchunks] - quotes[0];
    r.depth = depth;
    r.first_bad = 0;
    r.err = 0;
    if (bad != kNone) {
        r.err = 1;
        r.first_bad = bad;
        r.len = 0;
        r.rows = r.depth = 0;
    } else if (r.len > job.cap || r.rows > job.rows) {
        r.err = 3;
    }
    ok[ji] = r.err == 0;
    res[ji] = r;
}

constexpr int kRowsDecImage16 = (int)(kDC / 4 * 3 + 16) / 16 + 1;  // a group per four bytes at most; one dword past

__global__ void __launch_bounds__(kB64Threads) b64r_decode_place_kernel(const Base64RowsJob* __restrict__ jobs, int njobs,
                                                                        const uint32_t* __restrict__ info,
                                                                        const uint32_t* __restrict__ prefix,
                                                                        uint32_t nchunks_all, const int32_t* __restrict__ ok,
                                                                        Base64RowsResult* __restrict__ res) {
    __shared__ u32x4 stage16[kRowsDecStage16];
    __shared__ u32x4 image16[kRowsDecImage16];
    __shared__ uint32_t wave_par[4], wave_lastq[4];
    __shared__ uint32_t part[2][kB64Threads / 64];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&Base64RowsJob::first_chunk>(jobs, njobs, blockIdx.x);
    const Base64RowsJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks || !ok[ji]) return;  // uniform
    const uint32_t at = c * kDC, left = job.n - at, len = left < kDC ? left : kDC;
    const uint32_t pos0 = b64r_stage_text(stage16, job.src, job.n, at, len);
    __syncthreads();
    const uint32_t* bytes = prefix + blockIdx.x;
    const uint32_t* quotes = bytes + nchunks_all + 1;
    const uint32_t want = bytes[1] - bytes[0], want_rows = quotes[1] - quotes[0];
    const uint32_t out0 = bytes[0] - prefix[job.first_chunk];
    const uint32_t row0 = quotes[0] - prefix[nchunks_all + 1 + job.first_chunk];
    const uint32_t entry = info[(uint64_t)blockIdx.x * kBase64RowsInfoWords + kDwChosen];
    const uint32_t enters_inside = entry >= kDrInside ? 1u : 0u;
    const DrBits b = b64r_lane_bits(stage16, pos0, at, len, job.n);
    uint32_t par, lastq, chunk_par, chunk_lastq;
    b64r_quotes_before(b, wave_par, wave_lastq, &par, &lastq, &chunk_par, &chunk_lastq);
    const uint32_t a0 = lastq == 0 ? entry - kDrInside : 16 * t - lastq;  // read only where the byte lies inside
    const DrLane v = b64r_lane(b, at, a0 & 3, par ^ enters_inside);
    const uint32_t incl_bytes = wg::scan_post(v.size, part[0]), incl_rows = wg::scan_post(v.nclose, part[1]);
    __syncthreads();
    uint32_t total = 0, total_rows = 0;
    const uint32_t bytes_before = wg::scan_rank<kB64Threads>(incl_bytes, v.size, part[0], &total);
    const uint32_t rows_before = wg::scan_rank<kB64Threads>(incl_rows, v.nclose, part[1], &total_rows);
    if (total != want || total_rows != want_rows || __syncthreads_or(v.bad != kNone)) {  // uniform: the source changed
        if (t == 0) res[ji].err = 4;
        return;
    }
    // groups and closing quotes of the lane in the order they stand: a group's bytes into the image, a row end per quote
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(stage16);
    uint8_t* image = reinterpret_cast<uint8_t*>(image16);
    uint32_t* ends = const_cast<uint32_t*>(job.row_ends);
    uint32_t run = bytes_before, row = row0 + rows_before;
    for (uint32_t todo = v.groups | v.closing; todo; todo &= todo - 1) {
        const uint32_t k = (uint32_t)__builtin_ctz(todo), bit = 1u << k;
        if (v.closing & bit) {
            if (row < job.rows) ends[row] = out0 + run;
            ++row;
            continue;
        }
        const uint32_t s = (v.s3 & bit) ? 4u : (v.s2 & bit) ? 3u : (v.s1 & bit) ? 2u : 1u;
        if (s < 2) continue;  // a lone symbol carries nothing (and is refused)
        const uint32_t q = pos0 + 16 * t + k - 4;
        uint32_t word = wg::funnel(dw[q >> 2], dw[(q >> 2) + 1], (q & 3) * 8);
        if (s < 4) {
            const uint32_t keep = (1u << (8 * s)) - 1;
            word = (word & keep) | (0x41414141u & ~keep);  // 'A': zero bits
        }
        bool fine;
        const uint32_t le = b64::Bytes3LE(b64::Decode4(word, &fine));
        const uint32_t nb = br::GroupBytes(s);
        for (uint32_t x = 0; x < nb; ++x) image[run + x] = (uint8_t)(le >> (8 * x));
        run += nb;
    }
    __syncthreads();
    if ((uint64_t)out0 + total <= job.cap)
        wg::copy_out_shifted<kB64Threads>(reinterpret_cast<const uint32_t*>(image16), 0, job.dst + out0, total);
}

int b64r_begin(const Base64RowsTables& t, size_t prefix_words, hipStream_t s) {
    if (!t.jobs || !t.jobs_dev || !t.bad || !t.ok || !t.res || !t.prefix) return -1;
    if (hipMemcpyAsync(t.jobs_dev, t.jobs, (size_t)t.njobs * sizeof(Base64RowsJob), hipMemcpyHostToDevice, s) != hipSuccess)
        return -1;
    if (hipMemsetAsync(t.bad, 0xFF, (size_t)t.njobs * sizeof(uint32_t), s) != hipSuccess) return -1;
    if (hipMemsetAsync(t.ok, 0, (size_t)t.njobs * sizeof(int32_t), s) != hipSuccess) return -1;
    // a job without blocks reads two equal entries, the last job the one past the end
    if (hipMemsetAsync(t.prefix, 0, prefix_words * sizeof(uint32_t), s) != hipSuccess) return -1;
    return 0;
}

bool b64r_launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

int LaunchBase64EncodeRows(const Base64RowsTables& t, hipStream_t s) {
    if (t.njobs <= 0) return 0;
    if ((t.nrows && (!t.ends || !t.rowoff)) || b64r_begin(t, (size_t)t.nrblocks + 1, s) != 0) return -1;
    const dim3 threads(kB64Threads), per_job((t.njobs + 63) / 64);
    if (t.nrblocks) {
        hipLaunchKernelGGL(b64r_rows_kernel, dim3(t.nrblocks), threads, 0, s, t.jobs_dev, t.njobs, t.ends, t.rowoff, t.prefix,
                           t.bad);
        if (!b64r_launched()) return -1;
        if (LaunchPbRunPrefix(t.prefix, (int)t.nrblocks + 1, s) != 0) return -1;
    }
    hipLaunchKernelGGL(b64r_encode_verdict_kernel, per_job, dim3(64), 0, s, t.jobs_dev, t.njobs, t.prefix, t.bad, t.ok, t.res);
    if (!b64r_launched()) return -1;
    if (t.nrblocks) {
        hipLaunchKernelGGL(b64r_punct_kernel, dim3(t.nrblocks), threads, 0, s, t.jobs_dev, t.njobs, t.ends, t.rowoff, t.prefix,
                           t.ok);
        if (!b64r_launched()) return -1;
    }
    if (t.nchunks) {
        hipLaunchKernelGGL(b64r_encode_place_kernel, dim3(t.nchunks), threads, 0, s, t.jobs_dev, t.njobs, t.ends, t.rowoff,
                           t.prefix, t.ok);
        if (!b64r_launched()) return -1;
    }
    return 0;
}

int LaunchBase64DecodeRows(const Base64RowsTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (!t.info || !t.state || b64r_begin(t, 2 * ((size_t)t.nchunks + 1), s) != 0) return -1;
    const dim3 threads(kB64Threads), chunks(t.nchunks);
    hipLaunchKernelGGL(b64r_scan_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info);
    if (!b64r_launched()) return -1;
    hipLaunchKernelGGL(b64r_carry_kernel, dim3(t.njobs), threads, 0, s, t.jobs_dev, t.info, t.prefix, t.nchunks, t.state);
    if (!b64r_launched()) return -1;
    if (LaunchPbRunPrefix(t.prefix, 2 * ((int)t.nchunks + 1), s) != 0) return -1;
    hipLaunchKernelGGL(b64r_decode_verdict_kernel, dim3((t.njobs + 63) / 64), dim3(64), 0, s, t.jobs_dev, t.njobs, t.prefix,
                       t.nchunks, t.state, t.ok, t.res);
    if (!b64r_launched()) return -1;
    hipLaunchKernelGGL(b64r_decode_place_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info, t.prefix, t.nchunks, t.ok,
                       t.res);
    return b64r_launched() ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
