// JSON structural index on gfx950 (K6 of SURVEY §3, the device half of
// json2pb for large http+json bodies): the positions of every structural
// character ({ } [ ] : ,) outside strings and of every unescaped quote, plus
// validation that all strings are terminated — the stage-1 index a parser
// walks instead of scanning bytes (the reference's json2pb tokenizes on the
// CPU, src/json2pb/json_to_pb.cpp via rapidjson).
//
// Each lane owns 64 input bytes and turns them into 64-bit masks (quote,
// backslash, structural) with SWAR byte compares; the bytes are read once,
// everything after works on masks. The two sequential dependencies of
// tokenizing are carried with scans instead of a serial walk:
//  * escapes: whether byte i is escaped depends on the parity of the
//    backslash run before it, which may start in an earlier lane or tile.
//    A lane maps its carry-in (byte 0 escaped?) to a carry-out; the map is
//    composable, so lanes and tiles scan it.
//  * strings: inside/outside flips at every unescaped quote, so the state
//    at a byte is the XOR of the quote parities before it (prefix XOR in a
//    lane), and a lane's parity depends on its escape carry-in.
// A lane therefore has 4 possible start states (carry, in-string), and so
// does a tile (256 lanes x 64 B = 16 KiB). Three launches:
//  1. per tile: masks, the tile's transfer table T(c) = (carry-out, quote
//     parity), each lane's prefix table and its exclusive position offset
//     for each of the 4 tile start states (4 x u16 packed in one u64 and
//     scanned with plain 64-bit adds) and the tile's 4 counts;
//  2. one block: scan the tile tables to each tile's actual start state,
//     pick its count, scan the counts to output offsets;
//  3. per tile: each lane resolves its position mask with no further scan
//     and writes positions through an LDS window, so global stores are
//     contiguous 1 KiB rows instead of 64 scattered lanes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "base/decimal_to_double.h"
#include "base/number_text.h"
#include "base/shortest_double.h"
#include "gpu/kernels.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

constexpr int kJThreads = 256;
constexpr int kJWaves = kJThreads / 64;
constexpr uint64_t kLaneBytes = 64;
constexpr uint64_t kJTile = kJThreads * kLaneBytes;  // 16 KiB
constexpr uint32_t kEmitWindow = 4096;               // positions staged in LDS per round (16 KiB)

// Transfer table for escape carry-in c in {0,1}, packed in 4 bits:
// bit c = carry-out for carry-in c, bit 2+c = quote parity for carry-in c.
__device__ __forceinline__ uint32_t xf_next(uint32_t x, int c) { return (x >> c) & 1; }
__device__ __forceinline__ uint32_t xf_flip(uint32_t x, int c) { return (x >> (2 + c)) & 1; }
__device__ __forceinline__ uint32_t xf_make(uint32_t n0, uint32_t n1, uint32_t f0, uint32_t f1) {
    return n0 | (n1 << 1) | (f0 << 2) | (f1 << 3);
}
constexpr uint32_t kXfIdentity = 0x2;  // next = c, no flips

// a then b
__device__ __forceinline__ uint32_t xf_compose(uint32_t a, uint32_t b) {
    const uint32_t m0 = xf_next(a, 0), m1 = xf_next(a, 1);
    return xf_make(xf_next(b, m0), xf_next(b, m1), xf_flip(a, 0) ^ xf_flip(b, m0), xf_flip(a, 1) ^ xf_flip(b, m1));
}

// Start state k = carry | in_string << 1 after applying prefix table x to
// start state k0.
__device__ __forceinline__ int xf_apply(uint32_t x, int k0) {
    const int c = k0 & 1;
    return (int)xf_next(x, c) | ((((k0 >> 1) & 1) ^ (int)xf_flip(x, c)) << 1);
}

// High bit of each byte of w set iff that byte equals the byte broadcast in
// pat (exact, no cross-byte carries).
__device__ __forceinline__ uint32_t bytes_eq(uint32_t w, uint32_t pat) {
    const uint32_t t = w ^ pat;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}
// Gather the 4 byte-high-bits into bits 0..3.
__device__ __forceinline__ uint32_t gather4(uint32_t m) { return ((m >> 7) & 0x01010101u) * 0x01020408u >> 24; }

struct LaneMasks {
    uint64_t quote, backslash, structural;
};

__device__ __forceinline__ void word_masks(uint32_t w, int shift, LaneMasks& m) {
    const uint32_t lw = w | 0x20202020u;  // '[' -> '{', ']' -> '}'
    const uint32_t q = bytes_eq(w, 0x22222222u);
    const uint32_t b = bytes_eq(w, 0x5C5C5C5Cu);
    const uint32_t s = bytes_eq(lw, 0x7B7B7B7Bu) | bytes_eq(lw, 0x7D7D7D7Du) | bytes_eq(w, 0x3A3A3A3Au) |
                       bytes_eq(w, 0x2C2C2C2Cu);
    m.quote |= (uint64_t)gather4(q) << shift;
    m.backslash |= (uint64_t)gather4(b) << shift;
    m.structural |= (uint64_t)gather4(s) << shift;
}

// Masks of the lane's 64 bytes (zero past the end: neither quote nor
// backslash nor structural).
__device__ __forceinline__ LaneMasks lane_masks(const uint8_t* __restrict__ in, uint64_t n, uint64_t base) {
    LaneMasks m{0, 0, 0};
    if (base + kLaneBytes <= n && ((reinterpret_cast<uintptr_t>(in) + base) & 15) == 0) {
        const uint4* p = reinterpret_cast<const uint4*>(in + base);
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            word_masks(v[k].x, 16 * k + 0, m);
            word_masks(v[k].y, 16 * k + 4, m);
            word_masks(v[k].z, 16 * k + 8, m);
            word_masks(v[k].w, 16 * k + 12, m);
        }
    } else if (base < n) {
        for (int j = 0; j < (int)kLaneBytes; j += 4) {
            uint32_t w = 0;
            for (int t = 0; t < 4; ++t)
                if (base + j + t < n) w |= (uint32_t)in[base + j + t] << (8 * t);
            word_masks(w, j, m);
        }
    }
    return m;
}

// Escaped-byte mask of a lane for carry-in c (byte 0 escaped), walking the
// backslash runs (JSON has few); *carry_out = whether the next lane's byte 0
// is escaped.
__device__ __forceinline__ uint64_t escaped_mask(uint64_t bs, int c, int* carry_out) {
    uint64_t esc = 0;
    int co = 0;
    if (c) {
        esc = 1;
        bs &= ~1ull;  // an escaped backslash escapes nothing
    }
    while (bs) {
        const int s = __builtin_ctzll(bs);
        const uint64_t rest = ~(bs >> s);
        const int len = rest ? __builtin_ctzll(rest) : 64 - s;
        const int e = s + len;
        if (len & 1) {
            if (e < 64) esc |= 1ull << e;
            else co = 1;
        }
        bs = e >= 64 ? 0 : bs & (~0ull << e);
    }
    *carry_out = co;
    return esc;
}

// Inclusive prefix XOR of the bits of x (bit i = XOR of bits 0..i).
__device__ __forceinline__ uint64_t prefix_xor(uint64_t x) {
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;
    return x;
}

// Reported positions of a lane given its unescaped quotes q and start
// in-string flag: quotes always, structurals outside strings. The in-string
// mask (inclusive prefix XOR) runs from an opening quote to the byte before
// its closing quote.
__device__ __forceinline__ uint64_t position_mask(uint64_t q, uint64_t structural, int in_string) {
    const uint64_t inside = (prefix_xor(q) ^ (in_string ? ~0ull : 0ull)) & ~q;
    return (structural & ~inside) | q;
}

// Block-wide scan of transfer tables, the shape of wg::block_excl_scan with
// xf_compose in place of the sum: one barrier, between writing and reading
// `wtot`, a kJWaves-entry LDS array owned by the caller.
__device__ __forceinline__ uint32_t block_xf_scan(uint32_t v, uint32_t* wtot, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wg::wave_incl_scan(v, [](uint32_t a, uint32_t b) { return xf_compose(a, b); });
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t before = kXfIdentity, all = kXfIdentity;
#pragma unroll
    for (int w = 0; w < kJWaves; ++w) {
        if (w < wave) before = xf_compose(before, wtot[w]);
        all = xf_compose(all, wtot[w]);
    }
    uint32_t ex = wg::wave_prev(inc);
    if (lane == 0) ex = kXfIdentity;
    *total = all;
    return xf_compose(before, ex);
}

// Scratch layout (lanes = tiles * 256):
//   u64 quote0[lanes], quote1[lanes], structural[lanes]  unescaped quotes for carry-in 0/1
//   u64 lane_off[lanes]       exclusive offset in the tile, u16 per tile start state
//   u8  lane_prefix[lanes]    prefix transfer table of the lanes before it in the tile
//   u32 tile_xfer[tiles]      then, after pass 2, tile start state
//   u64 tile_cnt[tiles]       u16 x 4 counts by start state; after pass 2, output offset
struct Scratch {
    uint64_t *q0, *q1, *st, *lane_off, *tile_cnt;
    uint8_t* lane_prefix;
    uint32_t* tile_xfer;
};

__host__ __device__ inline Scratch carve(void* p, uint64_t tiles) {
    const uint64_t lanes = tiles * kJThreads;
    Scratch s;
    uint64_t* u = static_cast<uint64_t*>(p);
    s.q0 = u;
    s.q1 = u + lanes;
    s.st = u + 2 * lanes;
    s.lane_off = u + 3 * lanes;
    s.tile_cnt = u + 4 * lanes;
    s.tile_xfer = reinterpret_cast<uint32_t*>(s.tile_cnt + tiles);
    s.lane_prefix = reinterpret_cast<uint8_t*>(s.tile_xfer + tiles);
    return s;
}

// Pass 1.
__global__ void __launch_bounds__(kJThreads) json_tile_kernel(const uint8_t* __restrict__ in, uint64_t n,
                                                              Scratch sc, int* err) {
    __shared__ uint32_t xf_wtot[kJWaves];
    __shared__ uint64_t sum_wtot[kJWaves];
    const uint64_t lane = (uint64_t)blockIdx.x * kJThreads + threadIdx.x;
    const LaneMasks m = lane_masks(in, n, lane * kLaneBytes);
    int c0, c1;
    const uint64_t e0 = escaped_mask(m.backslash, 0, &c0);
    uint64_t e1;
    if (m.backslash & 1) {
        e1 = escaped_mask(m.backslash, 1, &c1);
    } else {  // byte 0 is no backslash: an escape carried in only escapes byte 0
        e1 = e0 | 1;
        c1 = c0;
    }
    const uint64_t q0 = m.quote & ~e0;
    const uint64_t q1 = m.quote & ~e1;
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = 0;  // pass 2 is the first to set it
    const uint32_t mine = xf_make((uint32_t)c0, (uint32_t)c1, (uint32_t)(__popcll(q0) & 1),
                                  (uint32_t)(__popcll(q1) & 1));
    uint32_t tile_xf;
    const uint32_t before = block_xf_scan(mine, xf_wtot, &tile_xf);
    // the lane's position count for each tile start state k
    uint64_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ls = xf_apply(before, k);
        const uint64_t pos = position_mask(ls & 1 ? q1 : q0, m.structural, ls >> 1);
        packed |= (uint64_t)__popcll(pos) << (16 * k);
    }
    uint64_t tile_cnt;
    const uint64_t off = wg::block_excl_scan<kJThreads>(packed, sum_wtot, &tile_cnt);  // no u16 field exceeds 16384
    sc.q0[lane] = q0;
    sc.q1[lane] = q1;
    sc.st[lane] = m.structural;
    sc.lane_off[lane] = off;
    sc.lane_prefix[lane] = (uint8_t)before;
    if (threadIdx.x == 0) {
        sc.tile_xfer[blockIdx.x] = tile_xf;
        sc.tile_cnt[blockIdx.x] = tile_cnt;
    }
}

// Pass 2 (one block): tile start states from (carry 0, outside strings),
// output offsets, total count; err |= 1 for a string open at the end. The
// tile arrays stream through LDS in coalesced chunks of kScanPer tiles per
// thread; the state and the running offset carry from chunk to chunk.
constexpr int kScanThreads = 1024;
constexpr int kScanPer = 4;
constexpr int kScanChunk = kScanThreads * kScanPer;

__global__ void __launch_bounds__(kScanThreads) json_scan_kernel(Scratch sc, uint64_t ntiles, uint64_t* total,
                                                                 int* err) {
    __shared__ uint32_t sx[kScanChunk];
    __shared__ uint64_t scnt[kScanChunk];
    __shared__ uint32_t xpart[kScanThreads];
    __shared__ uint64_t cpart[kScanThreads];
    const int t = threadIdx.x;
    int k_carry = 0;
    uint64_t off_carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kScanChunk) {
        const uint64_t m = ntiles - base < (uint64_t)kScanChunk ? ntiles - base : (uint64_t)kScanChunk;
        for (int j = t; j < kScanChunk; j += kScanThreads) {
            sx[j] = (uint64_t)j < m ? sc.tile_xfer[base + j] : kXfIdentity;
            scnt[j] = (uint64_t)j < m ? sc.tile_cnt[base + j] : 0;
        }
        __syncthreads();
        uint32_t acc = kXfIdentity;
#pragma unroll
        for (int i = 0; i < kScanPer; ++i) acc = xf_compose(acc, sx[t * kScanPer + i]);
        xpart[t] = acc;
        __syncthreads();
        for (int off = 1; off < kScanThreads; off <<= 1) {
            const uint32_t y = t >= off ? xpart[t - off] : kXfIdentity;
            __syncthreads();
            xpart[t] = xf_compose(y, xpart[t]);
            __syncthreads();
        }
        int k = xf_apply(t ? xpart[t - 1] : kXfIdentity, k_carry);
        uint64_t sum = 0;
#pragma unroll
        for (int i = 0; i < kScanPer; ++i) {
            const int j = t * kScanPer + i;
            const uint32_t x = sx[j];
            const uint64_t cnt = (scnt[j] >> (16 * k)) & 0xFFFF;
            sx[j] = (uint32_t)k;  // now: the tile's start state
            scnt[j] = cnt;
            sum += cnt;
            k = xf_apply(x, k);
        }
        cpart[t] = sum;
        __syncthreads();
        for (int off = 1; off < kScanThreads; off <<= 1) {
            const uint64_t y = t >= off ? cpart[t - off] : 0;
            __syncthreads();
            cpart[t] += y;
            __syncthreads();
        }
        uint64_t run = off_carry + (t ? cpart[t - 1] : 0);
#pragma unroll
        for (int i = 0; i < kScanPer; ++i) {
            const int j = t * kScanPer + i;
            const uint64_t c = scnt[j];
            scnt[j] = run;
            run += c;
        }
        __syncthreads();
        for (int j = t; (uint64_t)j < m; j += kScanThreads) {
            sc.tile_xfer[base + j] = sx[j];
            sc.tile_cnt[base + j] = scnt[j];
        }
        k_carry = xf_apply(xpart[kScanThreads - 1], k_carry);
        off_carry += cpart[kScanThreads - 1];
        __syncthreads();  // the next chunk reuses the LDS arrays
    }
    if (t == 0) {
        *total = off_carry;
        if (k_carry >> 1) atomicOr(err, 1);
    }
}

// Pass 3: positions through an LDS window, written as contiguous rows.
__global__ void __launch_bounds__(kJThreads) json_emit_kernel(Scratch sc, uint64_t ntiles, const uint64_t* total_dev,
                                                              uint32_t* __restrict__ out, uint64_t max_out, int* err) {
    __shared__ uint32_t win[kEmitWindow];
    const uint64_t lane = (uint64_t)blockIdx.x * kJThreads + threadIdx.x;
    const int tk = (int)sc.tile_xfer[blockIdx.x];
    const int ls = xf_apply(sc.lane_prefix[lane], tk);
    uint64_t m = position_mask(ls & 1 ? sc.q1[lane] : sc.q0[lane], sc.st[lane], ls >> 1);
    uint32_t idx = (uint32_t)((sc.lane_off[lane] >> (16 * tk)) & 0xFFFF);
    const uint64_t tile_off = sc.tile_cnt[blockIdx.x];
    const uint64_t tile_end = blockIdx.x + 1 < ntiles ? sc.tile_cnt[blockIdx.x + 1] : *total_dev;
    const uint32_t count = (uint32_t)(tile_end - tile_off);
    const uint32_t base = (uint32_t)(lane * kLaneBytes);
    for (uint32_t w0 = 0; w0 < count; w0 += kEmitWindow) {  // uniform trip count
        const uint32_t wend = w0 + kEmitWindow;
        while (m && idx < wend) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            win[idx - w0] = base + (uint32_t)i;
            ++idx;
        }
        __syncthreads();
        const uint32_t nwin = count - w0 < kEmitWindow ? count - w0 : kEmitWindow;
        for (uint32_t j = threadIdx.x; j < nwin; j += kJThreads) {
            const uint64_t g = tile_off + w0 + j;
            if (g < max_out) out[g] = win[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && tile_end > max_out && tile_off < tile_end) atomicOr(err, 2);
}

// json2pb integer arrays (the reference converts them element by element
// from rapidjson values, src/json2pb/json_to_pb.cpp).
// One lane per element; a workgroup's 256 elements are one contiguous span
// of text, staged into LDS with loads that are all issued before any is
// used (the text is pinned host memory: a lane walking its element byte by
// byte would pay a PCIe round trip per character). Spans longer than the
// LDS window (long runs of whitespace) are read from memory directly.
constexpr uint32_t kIntSpan = 16384;

__device__ __forceinline__ bool json_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

__global__ void __launch_bounds__(256) json_int_array_kernel(const char* __restrict__ text,
                                                             const uint32_t* __restrict__ seps, uint32_t n,
                                                             int64_t* __restrict__ out, int32_t* __restrict__ bad) {
    __shared__ char span[kIntSpan];
    __shared__ uint32_t lo_s, hi_s;
    const uint32_t first = blockIdx.x * blockDim.x;
    const uint32_t i = first + threadIdx.x;
    const uint32_t last = min(first + blockDim.x, n);  // elements [first, last)
    uint32_t b = 0, e = 0;
    if (i < n) {
        b = seps[i] + 1;
        e = seps[i + 1];
    }
    if (threadIdx.x == 0) lo_s = seps[first] + 1;
    if (i + 1 == last) hi_s = e;
    __syncthreads();
    const uint32_t lo = lo_s, hi = hi_s;
    const bool staged = hi - lo <= kIntSpan;
    if (staged) {
        constexpr int kPer = kIntSpan / 256;
        char v[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t j = threadIdx.x + (uint32_t)k * 256;
            v[k] = lo + j < hi ? text[lo + j] : 0;
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t j = threadIdx.x + (uint32_t)k * 256;
            if (lo + j < hi) span[j] = v[k];
        }
    }
    __syncthreads();
    if (i >= n) return;
    // positions stay absolute; an LDS pointer must never be offset below the
    // array (a flat address below the LDS aperture is a global address)
    auto at = [&](uint32_t k) -> char { return staged ? span[k - lo] : text[k]; };
    while (b < e && json_ws(at(b))) ++b;
    while (e > b && json_ws(at(e - 1))) --e;
    bool neg = false;
    if (b < e && at(b) == '-') {
        neg = true;
        ++b;
    }
    bool ok = b < e && e - b <= 20;
    uint64_t v = 0;
    for (uint32_t k = b; ok && k < e; ++k) {
        const uint32_t d = (uint32_t)(unsigned char)at(k) - '0';
        if (d > 9 || v > (0xFFFFFFFFFFFFFFFFull - d) / 10) {
            ok = false;
            break;
        }
        v = v * 10 + d;
    }
    if (ok) ok = neg ? v <= 0x8000000000000000ull : v <= 0x7FFFFFFFFFFFFFFFull;
    if (!ok) {
        *bad = 1;
        return;
    }
    out[i] = neg ? (int64_t)((uint64_t)0 - v) : (int64_t)v;
}

// json2pb number arrays, floats among them (kernels.h JsonNumberJob; the
// reference converts every element with rapidjson's number parser on the
// host). The shape is json_int_array_kernel's; the conversion is
// base/decimal_to_double.h, the code json::Reader runs. A separator of
// 0xFFFFFFFF stands for one before the text's first byte (seps[i] + 1 is
// taken mod 2^32), so bare "v,v,...,v" text needs no bracket.
namespace dd = ::mrpc::decimal_to_double;

__global__ void __launch_bounds__(256) json_number_init_kernel(JsonNumberResult* __restrict__ res, int njobs) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < njobs) res[j] = JsonNumberResult{0xFFFFFFFFu, 0u};
}

__global__ void __launch_bounds__(256) json_number_publish_kernel(const JsonNumberResult* __restrict__ res,
                                                                  JsonNumberResult* __restrict__ out, int njobs) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < njobs) out[j] = res[j];
}

__global__ void __launch_bounds__(256) json_number_array_kernel(const JsonNumberJob* __restrict__ jobs, int njobs,
                                                                JsonNumberResult* __restrict__ res) {
    __shared__ char span[kIntSpan];
    __shared__ uint32_t lo_s, hi_s;
    const int ja = wg::job_of<&JsonNumberJob::first_block>(jobs, njobs, blockIdx.x);
    const JsonNumberJob job = jobs[ja];
    const char* __restrict__ text = job.text;
    const uint32_t* __restrict__ seps = job.seps;
    const uint32_t n = job.count;
    const uint64_t first64 = (uint64_t)(blockIdx.x - job.first_block) * 256;
    if (first64 >= n) return;  // uniform: a block the host did not mean for this job
    const uint32_t first = (uint32_t)first64;
    const uint64_t i64 = first64 + threadIdx.x;
    const uint32_t i = (uint32_t)i64;
    const uint32_t last = (uint32_t)(first64 + 256 < n ? first64 + 256 : n);  // elements [first, last)
    uint32_t b = 0, e = 0;
    if (i64 < n) {
        b = seps[i] + 1;
        e = seps[i + 1];
    }
    if (threadIdx.x == 0) lo_s = seps[first] + 1;
    if (i64 + 1 == last) hi_s = e;
    __syncthreads();
    const uint32_t lo = lo_s, hi = hi_s;
    const bool staged = hi >= lo && hi - lo <= kIntSpan;
    if (staged) {
        constexpr int kPer = kIntSpan / 256;
        char v[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t j = threadIdx.x + (uint32_t)k * 256;
            v[k] = j < hi - lo ? text[lo + j] : 0;
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t j = threadIdx.x + (uint32_t)k * 256;
            if (j < hi - lo) span[j] = v[k];
        }
    }
    __syncthreads();
    if (i64 >= n) return;
    // separators that do not ascend: never index LDS outside the staged span
    if (b > e || (staged && (b < lo || e > hi))) b = e = lo;
    // positions stay absolute; an LDS pointer must never be offset below the
    // array (a flat address below the LDS aperture is a global address)
    auto at = [&](uint32_t k) -> char { return staged ? span[k - lo] : text[k]; };
    while (b < e && json_ws(at(b))) ++b;
    while (e > b && json_ws(at(e - 1))) --e;
    dd::NumberResult r;
    dd::ParseJsonNumberAt(at, b, e, &r);
    if (r.cls == dd::kMalformed) {
        atomicMin(&res[ja].bad, i);
        return;
    }
    if (r.cls == dd::kNeedsExact) {
        const uint32_t slot = atomicAdd(&res[ja].n_redo, 1u);
        if (slot < job.redo_cap) job.redo[slot] = i;
        return;
    }
    if (job.mode == JSON_PARSE_NUMBERS) {
        static_cast<uint64_t*>(job.out)[i] = r.bits;
        job.classes[i] = r.cls;
    } else if (job.mode == JSON_PARSE_FLOAT64) {
        static_cast<uint64_t*>(job.out)[i] = dd::NumberToDoubleBits(r);
    } else {
        static_cast<uint32_t*>(job.out)[i] = dd::NarrowDoubleBits(dd::NumberToDoubleBits(r));
    }
}

// Number text without a separator table (kernels.h JsonTextJob): the text is
// cut into chunks of kJsonTextChunkBytes, a workgroup per chunk in both
// passes, a lane per 16 bytes of it. The scanner and every rule of the shape
// are base/number_text.h, the code json::ParseNumberText runs.
namespace nt = ::mrpc::number_text;
using wg::u32x4;
static_assert(sizeof(nt::TextState) == kJsonTextStateBytes, "kernels.h sizes the state table");
constexpr uint32_t kJtChunk = kJsonTextChunkBytes;
constexpr int kJtThreads = 256;
constexpr uint32_t kJtPer = kJtChunk / kJtThreads;  // 16: one 128-bit LDS read
constexpr uint32_t kJtPre = 16, kJtPost = 112;      // staged before / after the chunk
constexpr uint32_t kJtWin = kJtPre + kJtChunk + kJtPost;
static_assert(kJtPer == 16 && kJtPre % 16 == 0 && kJtChunk < 65536, "a lane's bytes are one aligned uint4; offsets fit 16 bits");

// Reads of the staged window, eight bytes per LDS access: a scan walks its
// piece byte by byte, and every byte fetched alone is a round trip to LDS the
// next step waits for. k - wlo is below kJtWin, a multiple of 8.
struct JtWindowAt {
    const uint64_t* win8;  // the window, 16-byte aligned
    uint32_t wlo;
    mutable uint32_t have = 0xFFFFFFFFu;
    mutable uint64_t word = 0;
    __device__ __forceinline__ char operator()(uint32_t k) const {
        const uint32_t j = k - wlo;
        if ((j >> 3) != have) {
            have = j >> 3;
            word = win8[have];
        }
        return (char)(word >> ((j & 7) * 8));
    }
};
static_assert(kJtWin % 16 == 0 && kJtWin / 16 <= 2 * kJtThreads, "the window is read in 8-byte words and staged in at most two 16-byte loads a lane");

// commas in the low half, ']' bytes in the high half (a chunk has at most 4096 of each)
__device__ __forceinline__ uint32_t jt_tally(char c) { return c == ',' ? 1u : c == ']' ? 0x10000u : 0u; }

// how many of the 16 bytes equal the byte broadcast in pat
__device__ __forceinline__ uint32_t jt_count_eq(u32x4 q, uint32_t pat) {
    return (uint32_t)(__builtin_popcount(bytes_eq(q.x, pat)) + __builtin_popcount(bytes_eq(q.y, pat)) +
                      __builtin_popcount(bytes_eq(q.z, pat)) + __builtin_popcount(bytes_eq(q.w, pat)));
}

// prefix[0, nchunks]: commas per chunk and a 0; prefix[nchunks + 1, 2 * nchunks + 2): the same for ']'
__global__ void __launch_bounds__(kJtThreads) json_text_count_kernel(const JsonTextJob* __restrict__ jobs, int njobs,
                                                                     JsonTextJob* __restrict__ jobs_dev,
                                                                     uint32_t nchunks, uint32_t* __restrict__ prefix,
                                                                     nt::TextState* __restrict__ state,
                                                                     uint32_t* __restrict__ n_redo) {
    __shared__ uint32_t wave_tot[kJtThreads / 64];
    __shared__ JsonTextJob job_s;
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    // the table is host memory: one lane reads the job once, the later
    // kernels find it in device memory (a field read where it is used would
    // cross the bus every time)
    if (t == 0) {
        const int ja = wg::job_of<&JsonTextJob::first_chunk>(jobs, njobs, ci);
        job_s = jobs[ja];
        if (ci == 0) prefix[nchunks] = prefix[2 * nchunks + 1] = 0;  // become the totals under the scan
        if (ci == job_s.first_chunk) {
            jobs_dev[ja] = job_s;
            state[ja] = nt::TextState{nt::kNone, nt::kNone, 0u, 0u, 0u};
            n_redo[ja] = 0;
        }
    }
    __syncthreads();
    const JsonTextJob& job = job_s;
    const uint64_t s64 = (uint64_t)(ci - job.first_chunk) * kJtChunk;
    uint32_t v = 0;
    if (s64 < job.n) {
        const uint32_t s = (uint32_t)s64, len = job.n - s < kJtChunk ? job.n - s : kJtChunk;
        if (len == kJtChunk && ((uintptr_t)(job.text + s) & 15) == 0) {  // a whole chunk, aligned: one load a lane
            const u32x4 q = reinterpret_cast<const u32x4*>(job.text + s)[t];
            v = jt_count_eq(q, 0x2C2C2C2Cu) | jt_count_eq(q, 0x5D5D5D5Du) << 16;
        } else {
            char c[kJtPer];
#pragma unroll
            for (uint32_t k = 0; k < kJtPer; ++k) {
                const uint32_t j = t + k * kJtThreads;
                c[k] = j < len ? job.text[s + j] : 0;
            }
#pragma unroll
            for (uint32_t k = 0; k < kJtPer; ++k) v += jt_tally(c[k]);
        }
    }
    const uint32_t total = wg::block_sum<kJtThreads>(v, wave_tot);
    if (t == 0) {
        prefix[ci] = total & 0xFFFFu;
        prefix[nchunks + 1 + ci] = total >> 16;
    }
}

__global__ void __launch_bounds__(kJtThreads) json_text_parse_kernel(const JsonTextJob* __restrict__ jobs, int njobs,
                                                                     uint32_t nchunks,
                                                                     const uint32_t* __restrict__ prefix,
                                                                     nt::TextState* __restrict__ state,
                                                                     uint32_t* __restrict__ n_redo) {
    __shared__ __attribute__((aligned(16))) char win[kJtWin];
    __shared__ uint16_t cpos[kJtChunk];  // the chunk's commas, as offsets into it
    __shared__ uint32_t wave_tot[kJtThreads / 64];
    __shared__ JsonTextJob job_s;
    __shared__ int ja_s;
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        ja_s = wg::job_of<&JsonTextJob::first_chunk>(jobs, njobs, ci);
        job_s = jobs[ja_s];
    }
    __syncthreads();
    const int ja = ja_s;
    const JsonTextJob& job = job_s;
    const char* __restrict__ text = job.text;
    const uint32_t n = job.n;
    const uint32_t lc = ci - job.first_chunk;
    const uint64_t s64 = (uint64_t)lc * kJtChunk;
    if (s64 >= n) return;  // uniform: a chunk the host did not mean for this job
    const uint32_t s = (uint32_t)s64, e = n - s < kJtChunk ? n : s + kJtChunk;  // the chunk [s, e)
    // the scan runs over every job's chunks (mod 2^32): differences within a
    // job are its own counts. Loaded here so that they arrive with the text.
    const uint32_t* __restrict__ cprefix = prefix;
    const uint32_t* __restrict__ rprefix = prefix + nchunks + 1;
    const uint32_t commas_before = cprefix[ci] - cprefix[job.first_chunk];
    const uint32_t closes_before = rprefix[ci] - rprefix[job.first_chunk];
    const uint32_t closes_all = rprefix[job.first_chunk + job.nchunks] - rprefix[job.first_chunk];
    // the staged window [wlo, whi), text[k] at win[k - wlo]
    const uint32_t wlo = s >= kJtPre ? s - kJtPre : 0, whi = n - e < kJtPost ? n : e + kJtPost;
    if (whi - wlo == kJtWin && ((uintptr_t)(text + wlo) & 15) == 0) {  // a whole window, aligned: 16 bytes a load
        constexpr uint32_t kWin16 = kJtWin / 16;
        const u32x4* from = reinterpret_cast<const u32x4*>(text + wlo);
        u32x4* to = reinterpret_cast<u32x4*>(win);
        const u32x4 a = from[t];
        u32x4 b = {0, 0, 0, 0};
        if (t + kJtThreads < kWin16) b = from[t + kJtThreads];
        to[t] = a;
        if (t + kJtThreads < kWin16) to[t + kJtThreads] = b;
    } else {
        constexpr uint32_t kLoads = (kJtWin + kJtThreads - 1) / kJtThreads;
        char v[kLoads];
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const uint32_t j = t + k * kJtThreads;
            v[k] = j < whi - wlo ? text[wlo + j] : 0;
        }
#pragma unroll
        for (uint32_t k = 0; k < kLoads; ++k) {
            const uint32_t j = t + k * kJtThreads;
            if (j < kJtWin) win[j] = v[k];  // zeros past whi: never a comma or a bracket
        }
    }
    __syncthreads();
    // this lane's 16 bytes of the chunk: s - wlo is 0 or kJtPre, so they are
    // one aligned uint4. One bit per byte for ',' and for ']' (the SWAR
    // compares of the structural index), bytes past the chunk masked off.
    const uint32_t lo = s - wlo + t * kJtPer;  // index into win
    const uint32_t mine = s + t * kJtPer < e ? (e - (s + t * kJtPer) < kJtPer ? e - (s + t * kJtPer) : kJtPer) : 0;
    const u32x4 own = *reinterpret_cast<const u32x4*>(win + lo);
    const uint32_t keep = mine >= kJtPer ? 0xFFFFu : (1u << mine) - 1u;
    uint32_t comma_bits = (gather4(bytes_eq(own.x, 0x2C2C2C2Cu)) | gather4(bytes_eq(own.y, 0x2C2C2C2Cu)) << 4 |
                           gather4(bytes_eq(own.z, 0x2C2C2C2Cu)) << 8 | gather4(bytes_eq(own.w, 0x2C2C2C2Cu)) << 12) & keep;
    uint32_t close_bits = (gather4(bytes_eq(own.x, 0x5D5D5D5Du)) | gather4(bytes_eq(own.y, 0x5D5D5D5Du)) << 4 |
                           gather4(bytes_eq(own.z, 0x5D5D5D5Du)) << 8 | gather4(bytes_eq(own.w, 0x5D5D5D5Du)) << 12) & keep;
    const uint32_t own_commas = comma_bits;
    const uint32_t tally = (uint32_t)__builtin_popcount(comma_bits) | (uint32_t)__builtin_popcount(close_bits) << 16;
    uint32_t total;
    const uint32_t before = wg::block_excl_scan<kJtThreads>(tally, wave_tot, &total);
    const uint32_t ncommas = total & 0xFFFFu;  // of this chunk
    {
        uint32_t c_at = before & 0xFFFFu;
        for (; comma_bits; comma_bits &= comma_bits - 1) cpos[c_at++] = (uint16_t)(t * kJtPer + __builtin_ctz(comma_bits));
        // the k-th ']' of the text ends row k; the last one closes the outer array
        uint32_t r = closes_before + (before >> 16);
        for (; close_bits; close_bits &= close_bits - 1, ++r) {
            const uint32_t k = (uint32_t)__builtin_ctz(close_bits);
            const uint32_t commas_to_here = (before & 0xFFFFu) + (uint32_t)__builtin_popcount(own_commas & ((1u << k) - 1u));
            if (job.row_ends && r + 1 < closes_all && r < job.row_cap) job.row_ends[r] = commas_before + commas_to_here + 1;
        }
    }
    __syncthreads();
    // positions stay absolute; an LDS pointer must never be offset below the
    // array (a flat address below the LDS aperture is a global address)
    auto at = [&](uint32_t k) -> char { return k >= wlo && k < whi ? win[k - wlo] : text[k]; };
    // nearly every piece lies inside the window: it is scanned as if the text ended at whi, from LDS alone
    const JtWindowAt at_win{reinterpret_cast<const uint64_t*>(win), wlo};
    nt::TextState* __restrict__ st = state + ja;
    // piece q + 1 of the chunk follows its comma q; the text's first chunk
    // also owns the piece before any comma (q = -1). A chunk holds 0 to
    // kJtChunk commas, so the lanes go round.
    for (int q = (int)t - (lc == 0 ? 1 : 0); q < (int)ncommas; q += kJtThreads) {
        const uint32_t b = q < 0 ? 0 : s + cpos[q] + 1;  // <= n
        const uint32_t idx = q < 0 ? 0 : commas_before + (uint32_t)q + 1;
        nt::Piece piece;
        bool inside = b <= whi;  // b >= s >= wlo
        if (inside) {
            nt::ScanPiece(at_win, b, whi, &piece);
            inside = !piece.fits || piece.end < whi || whi == n;  // a refusal is one whatever follows
        }
        if (!inside) nt::ScanPiece(at, b, n, &piece);
        bool closes = false;
        if (q >= 0) {  // nt::ClosesBefore(at, b - 1), in the window as far as it reaches
            uint32_t k = b - 1;
            while (k > wlo && nt::IsSpace(win[k - 1 - wlo])) --k;
            closes = k > wlo ? win[k - 1 - wlo] == ']' : nt::ClosesBefore(at, k);
        }
        const uint32_t verdict = nt::JudgePiece(piece, idx, n, closes);
        if (verdict & nt::kPieceBad) {
            atomicMin(&st->bad, idx);
            continue;
        }
        if (idx == 0) st->lead0 = piece.lead;
        if (piece.end == n) st->trail_last = piece.trail;
        if (verdict & nt::kPieceBlank) {
            st->blank = 1;
            continue;
        }
        if (verdict & nt::kPieceNested) atomicMin(&st->nested_min, idx);
        dd::NumberResult r;
        if (inside) dd::ParseJsonNumberAt(at_win, piece.nb, piece.ne, &r);
        else dd::ParseJsonNumberAt(at, piece.nb, piece.ne, &r);
        if (r.cls == dd::kMalformed) {
            atomicMin(&st->bad, idx);
            continue;
        }
        if (r.cls == dd::kNeedsExact) {
            const uint32_t slot = atomicAdd(&n_redo[ja], 1u);
            if (slot < job.redo_cap) {
                job.redo[2 * (uint64_t)slot] = idx;
                job.redo[2 * (uint64_t)slot + 1] = b;
            }
            continue;
        }
        if (idx >= job.cap) continue;  // counted, not stored: the publish step reports it
        if (job.mode == JSON_PARSE_NUMBERS) {
            static_cast<uint64_t*>(job.out)[idx] = r.bits;
            job.classes[idx] = r.cls;
        } else if (job.mode == JSON_PARSE_FLOAT64) {
            static_cast<uint64_t*>(job.out)[idx] = dd::NumberToDoubleBits(r);
        } else {
            static_cast<uint32_t*>(job.out)[idx] = dd::NarrowDoubleBits(dd::NumberToDoubleBits(r));
        }
    }
}

__global__ void __launch_bounds__(256) json_text_publish_kernel(const JsonTextJob* __restrict__ jobs, int njobs,
                                                                uint32_t nchunks,
                                                                const uint32_t* __restrict__ prefix,
                                                                const nt::TextState* __restrict__ state,
                                                                const uint32_t* __restrict__ n_redo,
                                                                JsonTextResult* __restrict__ res) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= njobs) return;
    const JsonTextJob job = jobs[j];
    const uint32_t* rprefix = prefix + nchunks + 1;
    const uint32_t commas = prefix[job.first_chunk + job.nchunks] - prefix[job.first_chunk];
    const uint32_t closes = rprefix[job.first_chunk + job.nchunks] - rprefix[job.first_chunk];
    const nt::TextVerdict v = nt::CombineNumberText(state[j], commas, closes, job.row_ends != nullptr);
    res[j] = JsonTextResult{v.first_bad, n_redo[j], v.depth, v.count, v.rows, 0u};
}

// pb2json float / double arrays (kernels.h: size, prefix, place). The
// reference prints them element by element on the host through rapidjson's
// Writer (src/json2pb/pb_to_json.cpp); here one lane formats one element
// with base/shortest_double.h, the same code the host printer runs.
namespace sd = ::mrpc::shortest_double;
constexpr int kJfThreads = (int)kJsonFloatChunkElems;  // a lane per element
constexpr int kJfWaves = kJfThreads / 64;
constexpr uint32_t kJfElemMax = (uint32_t)sd::kMaxJsonDoubleChars + 1;                // with its comma
constexpr int kJfImage16 = (int)(kJsonFloatChunkElems * kJfElemMax + 16 + 15) / 16;  // at any 16-byte phase

__device__ __forceinline__ uint32_t jf_count(const JsonFloatChunk& c) {
    return c.count < kJsonFloatChunkElems ? c.count : kJsonFloatChunkElems;
}

__device__ __forceinline__ uint64_t jf_load_bits(const JsonFloatChunk& c, uint32_t i) {
    if (c.kind == JSON_FLOAT32) return sd::WidenFloatBits(static_cast<const uint32_t*>(c.src)[i]);
    return static_cast<const uint64_t*>(c.src)[i];
}

// the element's text size, its comma included (none after an array's last)
__device__ __forceinline__ uint32_t jf_elem_len(const sd::Decimal& d, const JsonFloatChunk& c, uint32_t i,
                                                uint32_t count) {
    return (uint32_t)sd::JsonDecimalLength(d) + (c.last && i + 1 == count ? 0u : 1u);
}

__global__ void __launch_bounds__(kJfThreads) json_float_size_kernel(const JsonFloatChunk* __restrict__ chunks,
                                                                     int nchunks, uint32_t* __restrict__ sizes,
                                                                     sd::Decimal* __restrict__ digits) {
    __shared__ uint32_t wave_tot[kJfWaves];
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    const JsonFloatChunk c = chunks[ci];
    const uint32_t count = jf_count(c);
    if (ci == 0 && t == 0) sizes[nchunks] = 0;  // becomes the total under the scan
    uint32_t n = 0;
    if (t < count) {
        const sd::Decimal d = sd::ShortestDigits(jf_load_bits(c, t));
        n = jf_elem_len(d, c, t, count);
        digits[(uint64_t)ci * kJsonFloatChunkElems + t] = d;
    }
    const uint32_t total = wg::block_sum<kJfThreads>(n, wave_tot);
    if (t == 0) sizes[ci] = total;
}

__global__ void __launch_bounds__(kJfThreads) json_float_place_kernel(const JsonFloatJob* __restrict__ jobs,
                                                                      const JsonFloatChunk* __restrict__ chunks,
                                                                      const uint32_t* __restrict__ prefix,
                                                                      const sd::Decimal* __restrict__ digits,
                                                                      JsonFloatResult* __restrict__ res) {
    __shared__ u32x4 image16[kJfImage16];
    __shared__ uint32_t wave_tot[kJfWaves];
    uint8_t* image = reinterpret_cast<uint8_t*>(image16);
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    const JsonFloatChunk c = chunks[ci];
    const JsonFloatJob job = jobs[c.job];
    // the host refuses arrays whose worst case passes 2^32 - 1, so the
    // differences of the scan (mod 2^32) are the sizes themselves
    const uint32_t first = prefix[job.first_chunk];
    const uint32_t job_len = prefix[job.first_chunk + job.nchunks] - first;
    const bool fits = (uint64_t)job_len <= job.cap;
    if (ci == job.first_chunk && t == 0) {
        res[c.job].len = job_len;
        if (!fits) res[c.job].err = 3;
    }
    if (!fits) return;  // the whole workgroup leaves: nothing of this array is written
    const uint32_t want = prefix[ci + 1] - prefix[ci];
    uint8_t* dst = job.dst + (uint32_t)(prefix[ci] - first);
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15);
    const uint32_t count = jf_count(c);
    sd::Decimal d;
    uint32_t len = 0;
    if (t < count) {
        d = digits[(uint64_t)ci * kJsonFloatChunkElems + t];
        len = jf_elem_len(d, c, t, count);
        if (len > kJfElemMax) len = 0;  // whatever the slot holds, never past the image
    }
    uint32_t total;
    const uint32_t pos = wg::block_excl_scan<kJfThreads>(len, wave_tot, &total);
    if (len) {
        char* o = reinterpret_cast<char*>(image + sh + pos);
        const uint32_t body = (uint32_t)sd::FormatJsonDecimal(d, o);
        if (body < len) o[body] = ',';
    }
    __syncthreads();
    if (total != want) {  // not what the size pass measured, and every later offset assumed `want`
        if (t == 0) res[c.job].err = 4;
        return;
    }
    wg::copy_out_phased<kJfThreads>(image, sh, dst, total);  // the image sits at dst's phase
}

}  // namespace

int LaunchJsonFloatPrint(const JsonFloatTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks <= 0) return 0;
    if (!t.jobs || !t.chunks || !t.prefix || !t.digits || !t.res) return -1;
    hipLaunchKernelGGL(json_float_size_kernel, dim3((unsigned)t.nchunks), dim3(kJfThreads), 0, s, t.chunks, t.nchunks,
                       t.prefix, static_cast<sd::Decimal*>(t.digits));
    if (hipGetLastError() != hipSuccess) return -1;
    if (LaunchPbRunPrefix(t.prefix, t.nchunks + 1, s) != 0) return -1;
    hipLaunchKernelGGL(json_float_place_kernel, dim3((unsigned)t.nchunks), dim3(kJfThreads), 0, s, t.jobs, t.chunks,
                       t.prefix, static_cast<const sd::Decimal*>(t.digits), t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchJsonIntArray(const char* text, const uint32_t* seps, uint32_t n, int64_t* out, int32_t* bad,
                       hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(json_int_array_kernel, dim3((n + 255) / 256), dim3(256), 0, s, text, seps, n, out, bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchJsonNumberArrays(const JsonNumberJob* jobs, int njobs, uint32_t nblocks, JsonNumberResult* res_dev,
                           JsonNumberResult* res_out, hipStream_t s) {
    if (njobs <= 0 || nblocks == 0) return 0;
    if (!jobs || !res_dev || !res_out) return -1;
    if (LaunchJsonNumberResultInit(res_dev, njobs, s) != 0) return -1;
    hipLaunchKernelGGL(json_number_array_kernel, dim3(nblocks), dim3(256), 0, s, jobs, njobs, res_dev);
    if (hipGetLastError() != hipSuccess) return -1;
    return LaunchJsonNumberResultPublish(res_dev, res_out, njobs, s);
}

int LaunchJsonNumberText(const JsonTextTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (!t.jobs || !t.jobs_dev || !t.prefix || !t.state || !t.n_redo || !t.res) return -1;
    nt::TextState* state = static_cast<nt::TextState*>(t.state);
    hipLaunchKernelGGL(json_text_count_kernel, dim3(t.nchunks), dim3(kJtThreads), 0, s, t.jobs, t.njobs, t.jobs_dev,
                       t.nchunks, t.prefix, state, t.n_redo);
    if (hipGetLastError() != hipSuccess) return -1;
    if (LaunchPbRunPrefix(t.prefix, (int)(2 * t.nchunks + 2), s) != 0) return -1;
    const JsonTextJob* jobs_dev = t.jobs_dev;
    hipLaunchKernelGGL(json_text_parse_kernel, dim3(t.nchunks), dim3(kJtThreads), 0, s, jobs_dev, t.njobs, t.nchunks,
                       t.prefix, state, t.n_redo);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(json_text_publish_kernel, dim3((unsigned)(t.njobs + 255) / 256), dim3(256), 0, s, jobs_dev,
                       t.njobs, t.nchunks, t.prefix, state, t.n_redo, t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchJsonNumberResultInit(JsonNumberResult* res_dev, int njobs, hipStream_t s) {
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(json_number_init_kernel, dim3((unsigned)(njobs + 255) / 256), dim3(256), 0, s, res_dev, njobs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int LaunchJsonNumberResultPublish(const JsonNumberResult* res_dev, JsonNumberResult* res_out, int njobs,
                                  hipStream_t s) {
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(json_number_publish_kernel, dim3((unsigned)(njobs + 255) / 256), dim3(256), 0, s, res_dev,
                       res_out, njobs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t JsonIndexScratchBytes(uint64_t n) {
    const uint64_t tiles = (n + kJTile - 1) / kJTile;
    const uint64_t lanes = tiles * kJThreads;
    return (size_t)(lanes * (4 * sizeof(uint64_t) + 1) + tiles * (sizeof(uint64_t) + sizeof(uint32_t)) + 64);
}

int LaunchJsonIndex(const uint8_t* in, uint64_t n, uint32_t* out_pos, uint64_t max_out, uint64_t* count_dev,
                    int* err_dev, void* scratch, hipStream_t s) {
    if (n > 0xFFFFFFFFull) return -1;  // positions are 32-bit
    if (n == 0) {
        if (hipMemsetAsync(err_dev, 0, sizeof(int), s) != hipSuccess) return -1;
        return hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s) == hipSuccess ? 0 : -1;
    }
    const uint64_t tiles = (n + kJTile - 1) / kJTile;
    const Scratch sc = carve(scratch, tiles);
    const dim3 grid((uint32_t)tiles), block(kJThreads);
    hipLaunchKernelGGL(json_tile_kernel, grid, block, 0, s, in, n, sc, err_dev);
    hipLaunchKernelGGL(json_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, sc, tiles, count_dev, err_dev);
    hipLaunchKernelGGL(json_emit_kernel, grid, block, 0, s, sc, tiles, (const uint64_t*)count_dev, out_pos, max_out,
                       err_dev);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
