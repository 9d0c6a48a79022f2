// JSON string bodies in device memory on gfx950: escape, unescape and the
// UTF-8 verdict (kernels.h JsonStringJob has the passes; the reference does
// all three on the host, through rapidjson's Writer and Reader). The rules
// are base/json_string.h, the code the host twins in json/json.cc run.
//
// A workgroup of 256 lanes takes one chunk of kJsonStringChunkBytes of one
// job, a lane 16 bytes. The chunk's span of the source is staged in LDS with
// aligned 16-byte loads (jstr_stage, over wg::stage16); what leaves goes
// through wg::copy_out_shifted, so the shift between the two alignments
// happens on chip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "base/json_string.h"
#include "base/json_string_rows.h"
#include "gpu/kernels.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

namespace js = ::mrpc::json_string;
using wg::u32x4;
constexpr int kJstrThreads = 256;
constexpr uint32_t kC = kJsonStringChunkBytes;
constexpr uint32_t kNone = kJsonStringNone;
static_assert(kJstrThreads * 16 == kC, "a lane per 16 bytes");
static_assert(kC / kJsonStringGroupBytes == 64, "64 groups per chunk");

// The staged span of a chunk: job bytes [at - back, at + len + fwd) cut to
// [0, n), loaded as whole 16-byte units. stage[pos0 + (i - at)] is job byte i.
struct JstrStage {
    const uint8_t* bytes;  // LDS
    int pos0;              // index of job byte `at`
    __device__ __forceinline__ uint8_t at(int64_t rel) const { return bytes[pos0 + rel]; }
};
constexpr uint32_t kStageBack = 16, kStageFwd = 12;
constexpr int kStage16 = (int)(kStageBack + 15 + kC + kStageFwd + 15) / 16 + 1;  // and a dword to spare

static_assert(kStage16 - 1 <= 2 * kJstrThreads, "two rounds of loads stage a chunk");

__device__ __forceinline__ JstrStage jstr_stage(u32x4* lds, const uint8_t* src, uint32_t n, uint32_t at, uint32_t len,
                                                uint32_t back, uint32_t fwd) {
    const uint32_t lo = at < back ? 0u : at - back;
    const uint64_t want = (uint64_t)at + len + fwd;
    const uint32_t hi = want > n ? n : (uint32_t)want;  // lo < hi: the chunk holds a byte
    const uint32_t a = wg::stage16<kJstrThreads, 2>(src + lo, hi - lo, lds);  // <= kStage16 - 1 units
    JstrStage st;
    st.bytes = reinterpret_cast<const uint8_t*>(lds);
    st.pos0 = (int)(a + (at - lo));
    return st;
}

// The lane's 16 bytes of the chunk as two words; what lies past `mine` bytes
// reads as '0' (plain, no backslash, ASCII).
__device__ __forceinline__ void jstr_words_at(const JstrStage& st, uint32_t p, uint32_t mine, uint64_t* w0,
                                              uint64_t* w1) {
    const uint32_t* dw = reinterpret_cast<const uint32_t*>(st.bytes);
    uint64_t a = 0x3030303030303030ull, b = 0x3030303030303030ull;
    if (mine != 0) {
        const uint32_t w = p >> 2, sh = (p & 3) * 8;
        const uint32_t d0 = dw[w], d1 = dw[w + 1], d2 = dw[w + 2], d3 = dw[w + 3], d4 = dw[w + 4];
        a = (uint64_t)wg::funnel(d0, d1, sh) | (uint64_t)wg::funnel(d1, d2, sh) << 32;
        b = (uint64_t)wg::funnel(d2, d3, sh) | (uint64_t)wg::funnel(d3, d4, sh) << 32;
        if (mine < 16) {
            const uint64_t keep_a = mine >= 8 ? ~0ull : (1ull << (8 * mine)) - 1;
            const uint64_t keep_b = mine <= 8 ? 0ull : (1ull << (8 * (mine - 8))) - 1;
            a = (a & keep_a) | (0x3030303030303030ull & ~keep_a);
            b = (b & keep_b) | (0x3030303030303030ull & ~keep_b);
        }
    }
    *w0 = a;
    *w1 = b;
}
__device__ __forceinline__ void jstr_lane_words(const JstrStage& st, uint32_t mine, uint64_t* w0, uint64_t* w1) {
    jstr_words_at(st, (uint32_t)st.pos0 + 16 * threadIdx.x, mine, w0, w1);
}
// a bit per byte of the two words that equals c
__device__ __forceinline__ uint32_t jstr_bits_of(uint64_t w0, uint64_t w1, uint8_t c) {
    const uint64_t spread = 0x0102040810204080ull;
    return (uint32_t)(((js::EqMask8(w0, c) >> 7) * spread) >> 56) | (uint32_t)(((js::EqMask8(w1, c) >> 7) * spread) >> 56) << 8;
}

__device__ __forceinline__ uint32_t jstr_mine(uint32_t len) {
    const uint32_t o = 16 * threadIdx.x;
    return o < len ? (len - o < 16 ? len - o : 16u) : 0u;
}

// ------------------------------------------------------------------ escape

__global__ void __launch_bounds__(kJstrThreads) jstr_escape_size_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                        uint32_t* __restrict__ prefix,
                                                                        uint32_t* __restrict__ groups) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ uint32_t part[8];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    const JstrStage st = jstr_stage(stage16, job.src, job.n, at, len, 0, 0);
    __syncthreads();
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(st, mine, &w0, &w1);
    const uint32_t size = js::EscapedSize8(w0) + js::EscapedSize8(w1) - (16 - mine);
    uint32_t total;
    const uint32_t before = wg::block_excl_scan<kJstrThreads>(size, part, &total);
    if (job.row_ends && (t & 3) == 0) groups[job.first_group + c * 64 + (t >> 2)] = before;
    if (t == 0) prefix[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kJstrThreads) jstr_rows_check_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                       uint32_t* __restrict__ bad) {
    const int ji = wg::job_of<&JsonStringJob::first_rblock>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    if (!job.row_ends) return;
    const uint64_t r = (uint64_t)(blockIdx.x - job.first_rblock) * kJsonStringBlockRows + threadIdx.x;
    if (r >= job.rows) return;
    const uint32_t end = job.row_ends[r], prev = r ? job.row_ends[r - 1] : 0u;
    if (end < prev || (r == job.rows - 1 && end != job.n)) atomicMin(&bad[ji], (uint32_t)r);
}

// a lane per job, after the prefix scan: shared by escape and unescape
__global__ void jstr_verdict_kernel(const JsonStringJob* __restrict__ jobs, int njobs, const uint32_t* __restrict__ prefix,
                                    const uint32_t* __restrict__ bad, int32_t* __restrict__ ok,
                                    JsonStringResult* __restrict__ res) {
    const int ji = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (ji >= njobs) return;
    const JsonStringJob job = jobs[ji];
    const uint64_t body = (uint32_t)(prefix[job.first_chunk + job.nchunks] - prefix[job.first_chunk]);
    uint64_t len = body;
    if (job.row_ends) len += 3ull * job.rows - 1;
    else if (job.quote) len += 2;
    JsonStringResult r;
    r.len = len;
    r.first_bad = 0;
    r.err = 0;
    const uint32_t b = bad[ji];
    if (b != kNone) {
        r.err = 1;
        r.first_bad = b;
        r.len = 0;
    } else if (len > job.cap) {
        r.err = 3;
    } else if (!job.row_ends && job.quote) {
        job.dst[0] = '"';
        job.dst[len - 1] = '"';
    }
    ok[ji] = r.err == 0;
    res[ji] = r;
}

// escaped bytes in front of source byte x of the job (x <= n)
__device__ __forceinline__ uint32_t jstr_escaped_before(const JsonStringJob& job, const uint32_t* __restrict__ prefix,
                                                        const uint32_t* __restrict__ groups, uint32_t x) {
    if (x >= job.n) return prefix[job.first_chunk + job.nchunks] - prefix[job.first_chunk];
    const uint32_t c = x / kC, g = (x % kC) / kJsonStringGroupBytes;
    uint32_t e = prefix[job.first_chunk + c] - prefix[job.first_chunk] + groups[job.first_group + c * 64 + g];
    for (uint32_t i = c * kC + g * kJsonStringGroupBytes; i < x; ++i) e += js::EscapedSize(job.src[i]);
    return e;
}

__global__ void __launch_bounds__(kJstrThreads) jstr_rows_punct_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                       const uint32_t* __restrict__ prefix,
                                                                       const uint32_t* __restrict__ groups,
                                                                       const int32_t* __restrict__ ok) {
    const int ji = wg::job_of<&JsonStringJob::first_rblock>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    if (!job.row_ends || !ok[ji]) return;
    const uint64_t r = (uint64_t)(blockIdx.x - job.first_rblock) * kJsonStringBlockRows + threadIdx.x;
    if (r >= job.rows) return;
    // ok: the ends ascend to n, so both lie inside the source
    const uint32_t start = r ? job.row_ends[r - 1] : 0u, end = job.row_ends[r];
    const uint32_t es = jstr_escaped_before(job, prefix, groups, start);
    const uint32_t ee = end == start ? es : jstr_escaped_before(job, prefix, groups, end);
    uint8_t* o = job.dst + (uint64_t)es + 3 * r;  // below cap: the verdict compared the whole length
    o[0] = '"';
    o[1 + (ee - es)] = '"';
    if (r + 1 < job.rows) o[2 + (ee - es)] = ',';
}

constexpr int kEscImage16 = (int)(6 * kC) / 16 + 1;  // copy_out_shifted reads one dword past

__global__ void __launch_bounds__(kJstrThreads) jstr_escape_place_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                         const uint32_t* __restrict__ prefix,
                                                                         const int32_t* __restrict__ ok,
                                                                         JsonStringResult* __restrict__ res) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ u32x4 image16[kEscImage16];
    __shared__ uint32_t lane_before[kJstrThreads + 1];
    __shared__ uint32_t part[8];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks || !ok[ji]) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    const JstrStage st = jstr_stage(stage16, job.src, job.n, at, len, 0, 0);
    __syncthreads();
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(st, mine, &w0, &w1);
    const uint32_t size = js::EscapedSize8(w0) + js::EscapedSize8(w1) - (16 - mine);
    uint32_t total;
    const uint32_t before = wg::block_excl_scan<kJstrThreads>(size, part, &total);
    if (total != prefix[blockIdx.x + 1] - prefix[blockIdx.x]) {  // uniform: the source changed since the size pass
        if (t == 0) res[ji].err = 4;
        return;
    }
    const uint32_t out0 = prefix[blockIdx.x] - prefix[job.first_chunk];  // escaped bytes of the job before this chunk
    const uint32_t* image = reinterpret_cast<const uint32_t*>(stage16);
    uint32_t ioff = (uint32_t)st.pos0;
    if (total != len) {  // some byte expands: build the escaped image
        char* img = reinterpret_cast<char*>(image16);
        if (size == mine) {
            for (uint32_t k = 0; k < mine; ++k) img[before + k] = (char)st.at(16 * t + k);
        } else {
            uint32_t o = before;
            for (uint32_t k = 0; k < mine; ++k) o += js::EscapeByte(st.at(16 * t + k), img + o);
        }
        image = reinterpret_cast<const uint32_t*>(image16);
        ioff = 0;
    }
    if (!job.row_ends) {
        __syncthreads();
        wg::copy_out_shifted<kJstrThreads>(image, ioff, job.dst + (job.quote ? 1 : 0) + out0, total);
        return;
    }
    lane_before[t] = before;
    if (t == 0) lane_before[kJstrThreads] = total;
    __syncthreads();
    // the rows of the chunk's first and last byte: the first row whose end lies beyond the byte
    const uint32_t* __restrict__ ends = job.row_ends;
    uint32_t ra = 0, rb = job.rows - 1;
    while (ra < rb) {
        const uint32_t mid = (ra + rb) / 2;
        if (ends[mid] > at) rb = mid;
        else ra = mid + 1;
    }
    const uint32_t r0 = ra;
    rb = job.rows - 1;
    while (ra < rb) {
        const uint32_t mid = (ra + rb) / 2;
        if (ends[mid] > at + len - 1) rb = mid;
        else ra = mid + 1;
    }
    const uint32_t r1 = ra;
    if (r1 - r0 < 8) {  // few rows: a segment of the image per row
        for (uint32_t r = r0; r <= r1; ++r) {
            const uint32_t start = r ? ends[r - 1] : 0u, end = ends[r];
            const uint32_t lo = (start > at ? start : at) - at, hi = (end < at + len ? end : at + len) - at;
            if (hi <= lo) continue;
            uint32_t xlo = lane_before[lo >> 4], xhi = lane_before[hi >> 4];
            for (uint32_t i = lo & ~15u; i < lo; ++i) xlo += js::EscapedSize(st.at(i));
            for (uint32_t i = hi & ~15u; i < hi; ++i) xhi += js::EscapedSize(st.at(i));
            wg::copy_out_shifted<kJstrThreads>(image, ioff + xlo, job.dst + (uint64_t)out0 + xlo + 3ull * r + 1, xhi - xlo);
        }
        return;
    }
    // many rows: every lane stores its own bytes
    if (mine == 0) return;
    const uint32_t i0 = at + 16 * t;
    ra = r0, rb = r1;
    while (ra < rb) {
        const uint32_t mid = (ra + rb) / 2;
        if (ends[mid] > i0) rb = mid;
        else ra = mid + 1;
    }
    uint32_t r = ra, o = before;
    for (uint32_t k = 0; k < mine; ++k) {
        while (r < r1 && ends[r] <= i0 + k) ++r;
        char b[6];
        const uint32_t nb = js::EscapeByte(st.at(16 * t + k), b);
        uint8_t* d = job.dst + (uint64_t)out0 + o + 3ull * r + 1;
        for (uint32_t q = 0; q < nb; ++q) d[q] = (uint8_t)b[q];
        o += nb;
    }
}

// ---------------------------------------------------------------- unescape

// A chunk's staged text, addressed by job offset; bytes outside the job read as 0.
struct JstrText {
    JstrStage st;
    uint32_t at, n;
    __device__ __forceinline__ uint8_t byte(int64_t i) const {  // job offset, anywhere
        return i >= 0 && i < (int64_t)n ? st.at(i - (int64_t)at) : (uint8_t)0;
    }
};

// Which bytes of the lane's window are unescaped backslashes, from a bit per
// backslash. The window is the 32 bytes [at - 16 + 16 t, at + 16 + 16 t): the
// 16 bytes in front of the lane's own, then its own. `run` is the parity of
// the backslashes right in front of the window; *mid gets the parity in front
// of the lane's own bytes.
__device__ __forceinline__ uint32_t jstr_starters(uint32_t backslashes, uint32_t run, uint32_t* mid) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        if (j == 16) *mid = run;
        if ((backslashes >> j) & 1) {
            if (!(run & 1)) m |= 1u << j;
            run ^= 1;
        } else {
            run = 0;
        }
    }
    return m;
}

// The bytes the lane's own 16 bytes give, with starter mask m of its window:
// returns their number, lowers *bad to the first offender; writes them at out
// when it is not null. kMasked (the rows kernels): only the bytes whose bit is
// set in `inside` are looked at, the bytes of a string's body; the others give
// nothing and offend nobody here.
template <bool kMasked = false>
__device__ __forceinline__ uint32_t jstr_emit(const JstrText& x, int64_t i0, uint32_t mine, uint64_t w0, uint64_t w1,
                                              uint32_t m, uint32_t* bad, char* out, uint32_t inside = 0) {
    uint32_t count = 0;
    for (uint32_t j = 0; j < mine; ++j) {
        if (kMasked && !((inside >> j) & 1)) continue;
        const int64_t i = i0 + j;
        const uint32_t before = m >> (10 + j);  // bit 6 - k: whether byte i - k starts an escape, k = 1..6
        if (before & 32u) continue;            // the letter of an escape
        if (((before & 16u) && x.byte(i - 1) == 'u') || ((before & 8u) && x.byte(i - 2) == 'u') ||
            ((before & 4u) && x.byte(i - 3) == 'u') || ((before & 2u) && x.byte(i - 4) == 'u'))
            continue;  // a hex digit of one
        const uint8_t b = (uint8_t)((j < 8 ? w0 : w1) >> (8 * (j & 7)));  // the lane's own byte j
        if (b == '\\') {
            char got[4];
            uint32_t span;
            const int k = js::DecodeEscape([&](int d) { return x.byte(i + d); }, (uint64_t)i, (uint64_t)x.n - (uint64_t)i,
                                           [&] { return (before & 1u) != 0; }, got, &span);
            if (k < 0) {
                if ((uint32_t)i < *bad) *bad = (uint32_t)i;
                continue;
            }
            if (out) {
                for (int q = 0; q < k; ++q) out[count + q] = got[q];
            }
            count += (uint32_t)k;
        } else if (b == '"') {
            if ((uint32_t)i < *bad) *bad = (uint32_t)i;
        } else {
            if (out) out[count] = (char)b;
            ++count;
        }
    }
    return count;
}

// A bit per backslash of the lane's window: bits 0..15 the 16 bytes in front
// of its own (bytes outside the job are none), bits 16..31 its own.
__device__ __forceinline__ uint32_t jstr_window_backslashes(const JstrText& x, uint32_t own) {
    const int64_t win = (int64_t)x.at - 16 + 16 * (int64_t)threadIdx.x;
    uint32_t valid = 0;  // bytes of the front 16 inside the job
    if (win >= 0 && win < (int64_t)x.n) valid = x.n - (uint32_t)win < 16 ? x.n - (uint32_t)win : 16u;
    uint64_t f0, f1;
    jstr_words_at(x.st, (uint32_t)(x.st.pos0 - 16 + 16 * (int)threadIdx.x), valid, &f0, &f1);
    return jstr_bits_of(f0, f1, '\\') | own << 16;
}

// The parity in front of each lane's window for carry-in c of the chunk, c
// the parity in front of byte at - 16. *depends: no byte other than a
// backslash lies between there and the window, so the answer is c itself
// (16 backslashes keep a parity); else it is the returned value.
__device__ __forceinline__ uint32_t jstr_window_parity(uint32_t front, uint64_t* wave_np, uint64_t* wave_odd,
                                                       bool* depends) {
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // the 16 bytes in front of the lane's own (a bit per backslash): all backslashes, or how many at their end
    const bool all = front == 0xFFFFu;
    const uint32_t trail = (uint32_t)__builtin_clz(~(front << 16));
    const uint64_t np = __ballot(!all), odd = __ballot(!all && (trail & 1));
    if (lane == 0) {
        wave_np[wave] = np;
        wave_odd[wave] = odd;
    }
    __syncthreads();
    // the nearest lane below this one whose front 16 bytes are not all backslashes: their trailing run decides,
    // the lanes between (16 backslashes each) only pass the parity on
    uint64_t mask = np & ((1ull << lane) - 1), odds = odd;
    int w = (int)wave;
    while (mask == 0 && w > 0) {
        --w;
        mask = wave_np[w];
        odds = wave_odd[w];
    }
    if (mask == 0) {
        *depends = true;
        return 0;
    }
    *depends = false;
    const int p = 63 - __builtin_clzll(mask);
    return (uint32_t)((odds >> p) & 1);
}

constexpr int kUnImage16 = (int)(kC + 16) / 16 + 1;

__global__ void __launch_bounds__(kJstrThreads) jstr_unescape_scan_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                          uint32_t* __restrict__ info) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ uint64_t wave_np[4], wave_odd[4];
    __shared__ uint32_t acc[6];  // size 0 / 1, bad 0 / 1, the map, whether any lane met a backslash or a quote
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    JstrText x;
    x.st = jstr_stage(stage16, job.src, job.n, at, len, kStageBack, kStageFwd);
    x.at = at;
    x.n = job.n;
    if (t < 6) acc[t] = t == 2 || t == 3 ? kNone : 0u;
    __syncthreads();
    const uint32_t mine = jstr_mine(len);
    uint32_t* out = info + (uint64_t)blockIdx.x * kJsonStringInfoWords;
    // a chunk with neither backslash nor quote, in the 16 bytes before it either, is copied whatever came before
    uint64_t w0, w1;
    jstr_lane_words(x.st, mine, &w0, &w1);
    uint64_t special = js::EqMask8(w0, '\\') | js::EqMask8(w0, '"') | js::EqMask8(w1, '\\') | js::EqMask8(w1, '"');
    if (t < 16 && x.byte((int64_t)at - 16 + t) == '\\') special = 1;
    if (!__syncthreads_or(special != 0)) {
        if (t == 0) {
            out[0] = out[1] = len;
            out[2] = out[3] = kNone;
            out[4] = 0;  // both carries end at 0
        }
        return;
    }
    const int64_t i0 = (int64_t)at + 16 * t;
    const uint32_t bs = jstr_window_backslashes(x, jstr_bits_of(w0, w1, '\\'));
    bool depends;
    const uint32_t par = jstr_window_parity(bs & 0xFFFFu, wave_np, wave_odd, &depends);
    uint32_t size[2], bad[2] = {kNone, kNone}, mid[2];
    const uint32_t m0 = jstr_starters(bs, depends ? 0u : par, &mid[0]);
    size[0] = jstr_emit(x, i0, mine, w0, w1, m0, &bad[0], nullptr);
    if (depends) {
        const uint32_t m1 = jstr_starters(bs, 1u, &mid[1]);
        size[1] = jstr_emit(x, i0, mine, w0, w1, m1, &bad[1], nullptr);
    } else {
        size[1] = size[0], bad[1] = bad[0], mid[1] = mid[0];
    }
    atomicAdd(&acc[0], size[0]);
    atomicAdd(&acc[1], size[1]);
    if (bad[0] != kNone) atomicMin(&acc[2], bad[0]);
    if (bad[1] != kNone) atomicMin(&acc[3], bad[1]);
    // the parity in front of the last lane's own bytes is the one in front of byte at + kC - 16: the carry
    if (t == kJstrThreads - 1) acc[4] = (mid[0] & 1) | (mid[1] & 1) << 1;
    __syncthreads();
    if (t < 5) out[t] = acc[t];
}

// maps of {0, 1} to itself in two bits: bit c = the image of c
__device__ __forceinline__ uint32_t jstr_then(uint32_t f, uint32_t g) {  // first f, then g
    return ((g >> (f & 1)) & 1) | ((g >> ((f >> 1) & 1)) & 1) << 1;
}
constexpr uint32_t kMapIdentity = 2;

__global__ void __launch_bounds__(kJstrThreads) jstr_unescape_carry_kernel(const JsonStringJob* __restrict__ jobs,
                                                                           uint32_t* __restrict__ info,
                                                                           uint32_t* __restrict__ prefix,
                                                                           uint32_t* __restrict__ bad) {
    __shared__ uint32_t wave_map[kJstrThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const JsonStringJob job = jobs[blockIdx.x];
    uint32_t carry = 0, lowest = kNone;
    for (uint32_t base = 0; base < job.nchunks; base += kJstrThreads) {
        const uint32_t c = base + t;
        uint32_t* mine = info + (uint64_t)(job.first_chunk + c) * kJsonStringInfoWords;
        const uint32_t map = c < job.nchunks ? mine[4] : kMapIdentity;
        const uint32_t incl = wg::wave_incl_scan(map, [](uint32_t f, uint32_t g) { return jstr_then(f, g); });
        if (lane == 63) wave_map[wave] = incl;
        __syncthreads();
        uint32_t excl = wg::wave_prev(incl);
        if (lane == 0) excl = kMapIdentity;
        uint32_t front = kMapIdentity, tile = kMapIdentity;
        for (uint32_t k = 0; k < kJstrThreads / 64; ++k) {
            if (k < wave) front = jstr_then(front, wave_map[k]);
            tile = jstr_then(tile, wave_map[k]);
        }
        const uint32_t cin = (jstr_then(front, excl) >> carry) & 1;
        if (c < job.nchunks) {
            prefix[job.first_chunk + c] = mine[cin];
            mine[5] = cin;
            const uint32_t b = mine[2 + cin];
            if (b < lowest) lowest = b;
        }
        carry = (tile >> carry) & 1;
        __syncthreads();  // wave_map is rewritten by the next tile
    }
    if (lowest != kNone) atomicMin(&bad[blockIdx.x], lowest);
}

__global__ void __launch_bounds__(kJstrThreads) jstr_unescape_place_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                           const uint32_t* __restrict__ info,
                                                                           const uint32_t* __restrict__ prefix,
                                                                           const int32_t* __restrict__ ok,
                                                                           JsonStringResult* __restrict__ res) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ u32x4 image16[kUnImage16];
    __shared__ uint64_t wave_np[4], wave_odd[4];
    __shared__ uint32_t part[8];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks || !ok[ji]) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    JstrText x;
    x.st = jstr_stage(stage16, job.src, job.n, at, len, kStageBack, kStageFwd);
    x.at = at;
    x.n = job.n;
    __syncthreads();
    const uint32_t want = prefix[blockIdx.x + 1] - prefix[blockIdx.x];
    uint8_t* dst = job.dst + (uint32_t)(prefix[blockIdx.x] - prefix[job.first_chunk]);
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(x.st, mine, &w0, &w1);
    uint64_t special = js::EqMask8(w0, '\\') | js::EqMask8(w0, '"') | js::EqMask8(w1, '\\') | js::EqMask8(w1, '"');
    if (t < 16 && x.byte((int64_t)at - 16 + t) == '\\') special = 1;
    if (!__syncthreads_or(special != 0)) {
        if (want != len) {
            if (t == 0) res[ji].err = 4;
            return;
        }
        wg::copy_out_shifted<kJstrThreads>(reinterpret_cast<const uint32_t*>(stage16), (uint32_t)x.st.pos0, dst, len);
        return;
    }
    const uint32_t cin = info[(uint64_t)blockIdx.x * kJsonStringInfoWords + 5] & 1;
    const int64_t i0 = (int64_t)at + 16 * t;
    const uint32_t bs = jstr_window_backslashes(x, jstr_bits_of(w0, w1, '\\'));
    bool depends;
    const uint32_t par = jstr_window_parity(bs & 0xFFFFu, wave_np, wave_odd, &depends);
    uint32_t mid, bad = kNone;
    const uint32_t m = jstr_starters(bs, depends ? cin : par, &mid);
    const uint32_t count = jstr_emit(x, i0, mine, w0, w1, m, &bad, nullptr);
    uint32_t total;
    const uint32_t before = wg::block_excl_scan<kJstrThreads>(count, part, &total);
    if (total != want || __syncthreads_or(bad != kNone)) {  // uniform: the source changed since the scan
        if (t == 0) res[ji].err = 4;
        return;
    }
    jstr_emit(x, i0, mine, w0, w1, m, &bad, reinterpret_cast<char*>(image16) + before);
    __syncthreads();
    wg::copy_out_shifted<kJstrThreads>(reinterpret_cast<const uint32_t*>(image16), 0, dst, total);
}

// ----------------------------------------------------------- unescape rows

namespace jr = ::mrpc::json_string_rows;
// The carried state: 0..4 outside a string after that kind of token (jr::Kind,
// kStart: none yet), 5 / 6 inside one after an even / odd backslash run.
constexpr uint32_t kRowsInside = 5;
constexpr uint32_t kRowsPass = 7;  // a chunk's exit only: outside and no token met, the entry's kind stays
constexpr uint32_t kRowsW = kJsonStringRowsEntryWords;
// words of an entry: size, closing quotes, lowest offender, first token, first ']', exit (in the scan: last token)
enum { kRwSize = 0, kRwClose = 1, kRwBad = 2, kRwFirst = 3, kRwBracket = 4, kRwExit = 5 };
constexpr uint32_t kRwChosen = 3 * kRowsW;  // the entry state the carry picked

// A bit per own byte of the lane.
struct JrowBits {
    uint32_t quote, ws, lb, comma, rb, backslash, valid;
};
__device__ __forceinline__ JrowBits jrow_bits(uint64_t w0, uint64_t w1, uint32_t mine) {
    JrowBits b;
    b.valid = mine >= 16 ? 0xFFFFu : (1u << mine) - 1;  // what lies past `mine` reads as '0': none of these
    b.quote = jstr_bits_of(w0, w1, '"');
    b.ws = jstr_bits_of(w0, w1, ' ') | jstr_bits_of(w0, w1, '\t') | jstr_bits_of(w0, w1, '\n') | jstr_bits_of(w0, w1, '\r');
    b.lb = jstr_bits_of(w0, w1, '[');
    b.comma = jstr_bits_of(w0, w1, ',');
    b.rb = jstr_bits_of(w0, w1, ']');
    b.backslash = jstr_bits_of(w0, w1, '\\');
    return b;
}
// The quotes of the lane's bytes that no escape covers: byte j is covered when
// byte j - 1 starts an escape (bit 15 + j of the window's starter mask).
__device__ __forceinline__ uint32_t jrow_open_quotes(const JrowBits& b, uint32_t m) { return b.quote & ~(m >> 15); }
// Bit j: whether the lane's byte j lies inside a string, seen from in front of
// it: the state in front of the lane's bytes, flipped by every uncovered quote
// below j (the prefix-xor of uq, exclusive).
__device__ __forceinline__ uint32_t jrow_inside(uint32_t uq, uint32_t before) {
    uint32_t p = uq;
    p ^= p << 1;
    p ^= p << 2;
    p ^= p << 4;
    p ^= p << 8;
    return ((p << 1) ^ (before ? 0xFFFFu : 0u)) & 0xFFFFu;
}
// The decoded bytes of the lane's `upto` first bytes, `content` the bytes of
// string bodies among them; writes them at out when it is not null.
__device__ __forceinline__ uint32_t jrow_emit(const JstrText& x, int64_t i0, uint32_t upto, uint64_t w0, uint64_t w1,
                                              uint32_t m, const JrowBits& b, uint32_t content, uint32_t* bad, char* out) {
    content &= upto >= 16 ? 0xFFFFu : (1u << upto) - 1;
    if (content == 0) return 0;
    // no escape reaches the lane's bytes (none starts in them or in the 6 before): every body byte is itself
    if (out == nullptr && (m >> 10) == 0 && (b.backslash & content) == 0) return (uint32_t)__popc(content);
    return jstr_emit<true>(x, i0, upto, w0, w1, m, bad, out, content);
}

struct JrowLane {
    uint32_t size, nclose, bad, first, last, rb;
};
// What the lane's bytes hold for one entry. m: the starter mask of its window,
// uq: its uncovered quotes, inside: jrow_inside. A token is the word
// (offset in the chunk) << 3 | kind; first / last: the lane's, kNone / 0 when
// it has none. Tokens after its first are judged here, against the token
// before them; bad and rb are job offsets.
__device__ __forceinline__ JrowLane jrow_lane(const JstrText& x, int64_t i0, uint32_t mine, uint64_t w0, uint64_t w1,
                                              uint32_t m, const JrowBits& b, uint32_t uq, uint32_t inside) {
    JrowLane r;
    r.bad = kNone;
    r.size = jrow_emit(x, i0, mine, w0, w1, m, b, inside & ~uq & b.valid, &r.bad, nullptr);
    r.nclose = (uint32_t)__popc(uq & inside);
    const uint32_t outside = ~inside & ~uq & b.valid;
    const uint32_t illegal = outside & ~(b.ws | b.lb | b.comma | b.rb);
    if (illegal) {
        const uint32_t at = (uint32_t)i0 + (uint32_t)__builtin_ctz(illegal);
        if (at < r.bad) r.bad = at;
    }
    r.first = kNone;
    r.last = 0;
    r.rb = kNone;
    uint32_t pred = 0;  // no token of this lane yet (kStart is no token)
    for (uint32_t tokens = uq | (outside & (b.lb | b.comma | b.rb)); tokens; tokens &= tokens - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(tokens), bit = 1u << j;
        const uint32_t kind = (uq & bit)        ? ((inside & bit) ? jr::kCloseQuote : jr::kOpenQuote)
                              : (b.lb & bit)    ? jr::kOpenBracket
                              : (b.comma & bit) ? jr::kComma
                                                : jr::kCloseBracket;
        const uint32_t at = (uint32_t)i0 + j;
        r.last = (16 * threadIdx.x + j) << 3 | kind;
        if (pred == 0) r.first = r.last;
        else if (!jr::Follows(pred, kind) && at < r.bad) r.bad = at;
        if (kind == jr::kCloseBracket && r.rb == kNone) r.rb = at;
        pred = kind;
    }
    return r;
}

__device__ __forceinline__ uint32_t jrow_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

__global__ void __launch_bounds__(kJstrThreads) jstr_rows_scan_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                      uint32_t* __restrict__ info) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ uint64_t wave_np[4], wave_odd[4];
    __shared__ uint32_t wave_par[2][4];   // parity of each wave's uncovered quotes, backslash carry-in 0 / 1
    __shared__ uint32_t wave_last[3][4];  // the last token of each wave, per entry
    __shared__ uint32_t acc[3][kRowsW];
    __shared__ uint32_t exit_par;  // bit c: the backslash carry-out for carry-in c
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    JstrText x;
    x.st = jstr_stage(stage16, job.src, job.n, at, len, kStageBack, kStageFwd);
    x.at = at;
    x.n = job.n;
    if (t < 3 * kRowsW) {
        const uint32_t k = t % kRowsW;
        acc[t / kRowsW][k] = k == kRwBad || k == kRwFirst || k == kRwBracket ? kNone : 0u;
    }
    __syncthreads();
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(x.st, mine, &w0, &w1);
    const JrowBits b = jrow_bits(w0, w1, mine);
    uint32_t special = b.quote | b.backslash;
    if (t < 16 && x.byte((int64_t)at - 16 + t) == '\\') special = 1;
    // starter masks of the lane's window for backslash carry-in 0 and 1; without a quote or a backslash in reach
    // nothing starts an escape and no quote flips a state
    uint32_t m0 = 0, m1 = 0, mid0 = 0, mid1 = 0;
    if (__syncthreads_or(special != 0)) {
        const uint32_t bs = jstr_window_backslashes(x, b.backslash);
        bool depends;
        const uint32_t par = jstr_window_parity(bs & 0xFFFFu, wave_np, wave_odd, &depends);
        m0 = jstr_starters(bs, depends ? 0u : par, &mid0);
        if (depends) m1 = jstr_starters(bs, 1u, &mid1);
        else m1 = m0, mid1 = mid0;
    }
    const uint32_t uq0 = jrow_open_quotes(b, m0), uq1 = jrow_open_quotes(b, m1);
    const uint64_t odd0 = __ballot(__popc(uq0) & 1), odd1 = __ballot(__popc(uq1) & 1);
    if (lane == 0) {
        wave_par[0][wave] = (uint32_t)__popcll(odd0) & 1;
        wave_par[1][wave] = (uint32_t)__popcll(odd1) & 1;
    }
    // the parity in front of the last lane's own bytes is the one in front of byte at + kC - 16: the carry
    if (t == kJstrThreads - 1) exit_par = (mid0 & 1) | (mid1 & 1) << 1;
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1;
    uint32_t before0 = (uint32_t)__popcll(odd0 & below) & 1, before1 = (uint32_t)__popcll(odd1 & below) & 1;
    uint32_t flips0 = 0, flips1 = 0;  // of the whole chunk
#pragma unroll
    for (uint32_t k = 0; k < kJstrThreads / 64; ++k) {
        if (k < wave) before0 ^= wave_par[0][k], before1 ^= wave_par[1][k];
        flips0 ^= wave_par[0][k];
        flips1 ^= wave_par[1][k];
    }
    // entry 0: outside. entry 1: inside after an even run, every state the other way round. entry 2: inside after
    // an odd run, which differs from entry 1 from the first lane on whose escapes depend on the carry-in
    const int64_t i0 = (int64_t)at + 16 * t;
    const uint32_t in0 = jrow_inside(uq0, before0), in1 = in0 ^ 0xFFFFu, in2 = jrow_inside(uq1, before1 ^ 1u);
    JrowLane v[3];
    v[0] = jrow_lane(x, i0, mine, w0, w1, m0, b, uq0, in0);
    v[1] = jrow_lane(x, i0, mine, w0, w1, m0, b, uq0, in1);
    v[2] = (m1 != m0 || in2 != in1) ? jrow_lane(x, i0, mine, w0, w1, m1, b, uq1, in2) : v[1];
    uint32_t prev[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const uint32_t size = wg::wave_sum(v[e].size), nclose = wg::wave_sum(v[e].nclose);
        if (lane == 0) {
            if (size) atomicAdd(&acc[e][kRwSize], size);
            if (nclose) atomicAdd(&acc[e][kRwClose], nclose);
        }
        if (v[e].bad != kNone) atomicMin(&acc[e][kRwBad], v[e].bad);
        if (v[e].rb != kNone) atomicMin(&acc[e][kRwBracket], v[e].rb);
        // the last token in front of the lane: tokens ascend with the lanes, so the highest word below it
        const uint32_t incl = wg::wave_incl_scan(v[e].last, [](uint32_t p, uint32_t q) { return jrow_max(p, q); });
        if (lane == 63) wave_last[e][wave] = incl;
        prev[e] = wg::wave_prev(incl);
        if (lane == 0) prev[e] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        uint32_t last = 0;
#pragma unroll
        for (uint32_t k = 0; k < kJstrThreads / 64; ++k) {
            if (k < wave) prev[e] = jrow_max(prev[e], wave_last[e][k]);
            last = jrow_max(last, wave_last[e][k]);
        }
        if (v[e].first != kNone) {
            // the lane's first token: judged against the token before it in the chunk; the chunk's first is the
            // carry kernel's to judge
            if (prev[e] == 0) atomicMin(&acc[e][kRwFirst], v[e].first);
            else if (!jr::Follows(prev[e] & 7, v[e].first & 7)) atomicMin(&acc[e][kRwBad], at + (v[e].first >> 3));
        }
        if (t == 0) {
            const uint32_t inside = (e ? 1u : 0u) ^ (e == 2 ? flips1 : flips0);
            const uint32_t carry = (exit_par >> (e == 2 ? 1 : 0)) & 1;
            acc[e][kRwExit] = inside ? kRowsInside + carry : (last ? (last & 7) : kRowsPass);
        }
    }
    __syncthreads();
    if (t < 3 * kRowsW) info[(uint64_t)blockIdx.x * kJsonStringRowsInfoWords + t] = acc[t / kRowsW][t % kRowsW];
}

// maps of the seven states to themselves, three bits per image
__device__ __forceinline__ uint32_t jrow_then(uint32_t f, uint32_t g) {  // first f, then g
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < 7; ++s) r |= ((g >> (3 * ((f >> (3 * s)) & 7))) & 7) << (3 * s);
    return r;
}
constexpr uint32_t kRowsIdentity = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12 | 5u << 15 | 6u << 18;

__global__ void __launch_bounds__(kJstrThreads) jstr_rows_carry_kernel(const JsonStringJob* __restrict__ jobs,
                                                                       uint32_t* __restrict__ info,
                                                                       uint32_t* __restrict__ prefix, uint32_t nchunks_all,
                                                                       uint32_t* __restrict__ state) {
    __shared__ uint32_t wave_map[kJstrThreads / 64];
    __shared__ uint32_t low[3];  // lowest offender, first ']' outside, depth
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const JsonStringJob job = jobs[blockIdx.x];
    if (t < 3) low[t] = t == 2 ? 0u : kNone;
    uint32_t carry = jr::kStart, lowest = kNone, bracket = kNone;
    for (uint32_t base = 0; base < job.nchunks; base += kJstrThreads) {
        const uint32_t c = base + t;
        uint32_t* mine = info + (uint64_t)(job.first_chunk + c) * kJsonStringRowsInfoWords;
        uint32_t map = kRowsIdentity;
        if (c < job.nchunks) {
            const uint32_t e0 = mine[kRwExit], e1 = mine[kRowsW + kRwExit], e2 = mine[2 * kRowsW + kRwExit];
            map = e1 << 15 | e2 << 18;
#pragma unroll
            for (uint32_t s = 0; s < kRowsInside; ++s) map |= (e0 == kRowsPass ? s : e0) << (3 * s);
        }
        const uint32_t incl = wg::wave_incl_scan(map, [](uint32_t f, uint32_t g) { return jrow_then(f, g); });
        if (lane == 63) wave_map[wave] = incl;
        __syncthreads();
        uint32_t excl = wg::wave_prev(incl);
        if (lane == 0) excl = kRowsIdentity;
        uint32_t front = kRowsIdentity, tile = kRowsIdentity;
        for (uint32_t k = 0; k < kJstrThreads / 64; ++k) {
            if (k < wave) front = jrow_then(front, wave_map[k]);
            tile = jrow_then(tile, wave_map[k]);
        }
        const uint32_t st = (jrow_then(front, excl) >> (3 * carry)) & 7;
        if (c < job.nchunks) {
            const uint32_t* w = mine + (st < kRowsInside ? 0u : st - 4u) * kRowsW;
            prefix[job.first_chunk + c] = w[kRwSize];
            prefix[nchunks_all + 1 + job.first_chunk + c] = w[kRwClose];
            mine[kRwChosen] = st;
            if (w[kRwBad] < lowest) lowest = w[kRwBad];
            if (w[kRwBracket] < bracket) bracket = w[kRwBracket];
            if (st < kRowsInside && w[kRwFirst] != kNone) {  // the chunk's first token, against its true predecessor
                const uint32_t kind = w[kRwFirst] & 7, where = c * kC + (w[kRwFirst] >> 3);
                if (!jr::Follows(st, kind) && where < lowest) lowest = where;
                if (st == jr::kStart && kind == jr::kOpenBracket) low[2] = 1;  // the text's first token
            }
        }
        carry = (tile >> (3 * carry)) & 7;
        __syncthreads();  // wave_map is rewritten by the next tile
    }
    if (lowest != kNone) atomicMin(&low[0], lowest);
    if (bracket != kNone) atomicMin(&low[1], bracket);
    __syncthreads();
    if (t == 0) {
        uint32_t* st = state + (uint64_t)blockIdx.x * kJsonStringRowsStateWords;
        st[0] = low[0];
        st[1] = carry;
        st[2] = low[2];
        st[3] = low[1];
    }
}

// a lane per job, after the prefix scan over both tables
__global__ void jstr_rows_verdict_kernel(const JsonStringJob* __restrict__ jobs, int njobs, const uint32_t* __restrict__ prefix,
                                         uint32_t nchunks_all, const uint32_t* __restrict__ state, int32_t* __restrict__ ok,
                                         JsonStringRowsResult* __restrict__ res) {
    const int ji = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (ji >= njobs) return;
    const JsonStringJob job = jobs[ji];
    const uint32_t* bytes = prefix + job.first_chunk;
    const uint32_t* quotes = bytes + nchunks_all + 1;
    const uint32_t* st = state + (uint64_t)ji * kJsonStringRowsStateWords;
    const uint32_t depth = st[2];
    uint32_t bad = st[0];
    if (depth == 0 && st[3] < bad) bad = st[3];                    // a ']' without its '['
    if (bad == kNone && !jr::EndsWell(st[1], depth)) bad = job.n;  // the text ends too soon
    JsonStringRowsResult r;
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

__global__ void __launch_bounds__(kJstrThreads) jstr_rows_place_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                       const uint32_t* __restrict__ info,
                                                                       const uint32_t* __restrict__ prefix,
                                                                       uint32_t nchunks_all, const int32_t* __restrict__ ok,
                                                                       JsonStringRowsResult* __restrict__ res) {
    __shared__ u32x4 stage16[kStage16];
    __shared__ u32x4 image16[kUnImage16];
    __shared__ uint64_t wave_np[4], wave_odd[4];
    __shared__ uint32_t wave_par[4];
    __shared__ uint32_t part[2][kJstrThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks || !ok[ji]) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    JstrText x;
    x.st = jstr_stage(stage16, job.src, job.n, at, len, kStageBack, kStageFwd);
    x.at = at;
    x.n = job.n;
    __syncthreads();
    const uint32_t* bytes = prefix + blockIdx.x;
    const uint32_t* quotes = bytes + nchunks_all + 1;
    const uint32_t want = bytes[1] - bytes[0], want_rows = quotes[1] - quotes[0];
    // decoded bytes and closing quotes of the job in front of this chunk: below cap and row_cap, the verdict
    // compared the job's totals
    const uint32_t out0 = bytes[0] - prefix[job.first_chunk];
    const uint32_t row0 = quotes[0] - prefix[nchunks_all + 1 + job.first_chunk];
    const uint32_t entry = info[(uint64_t)blockIdx.x * kJsonStringRowsInfoWords + kRwChosen];
    const uint32_t enters_inside = entry >= kRowsInside, cin = entry == kRowsInside + 1;
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(x.st, mine, &w0, &w1);
    const JrowBits b = jrow_bits(w0, w1, mine);
    uint32_t special = b.quote | b.backslash;
    if (t < 16 && x.byte((int64_t)at - 16 + t) == '\\') special = 1;
    if (!__syncthreads_or(special != 0)) {  // all copy, or all punctuation
        if (want != (enters_inside ? len : 0u) || want_rows != 0) {
            if (t == 0) res[ji].err = 4;
            return;
        }
        if (enters_inside)
            wg::copy_out_shifted<kJstrThreads>(reinterpret_cast<const uint32_t*>(stage16), (uint32_t)x.st.pos0,
                                               job.dst + out0, len);
        return;
    }
    const int64_t i0 = (int64_t)at + 16 * t;
    const uint32_t bs = jstr_window_backslashes(x, b.backslash);
    bool depends;
    const uint32_t par = jstr_window_parity(bs & 0xFFFFu, wave_np, wave_odd, &depends);
    uint32_t mid, bad = kNone;
    const uint32_t m = jstr_starters(bs, depends ? cin : par, &mid);
    const uint32_t uq = jrow_open_quotes(b, m);
    const uint64_t odd = __ballot(__popc(uq) & 1);
    if (lane == 0) wave_par[wave] = (uint32_t)__popcll(odd) & 1;
    __syncthreads();
    uint32_t before = enters_inside ^ ((uint32_t)__popcll(odd & ((1ull << lane) - 1)) & 1);
#pragma unroll
    for (uint32_t k = 0; k < kJstrThreads / 64; ++k) {
        if (k < wave) before ^= wave_par[k];
    }
    const uint32_t inside = jrow_inside(uq, before), content = inside & ~uq & b.valid, closing = uq & inside;
    const uint32_t count = jrow_emit(x, i0, mine, w0, w1, m, b, content, &bad, nullptr);
    const uint32_t nclose = (uint32_t)__popc(closing);
    const uint32_t incl_bytes = wg::scan_post(count, part[0]), incl_rows = wg::scan_post(nclose, part[1]);
    __syncthreads();
    uint32_t total = 0, total_rows = 0;
    const uint32_t bytes_before = wg::scan_rank<kJstrThreads>(incl_bytes, count, part[0], &total);
    const uint32_t rows_before = wg::scan_rank<kJstrThreads>(incl_rows, nclose, part[1], &total_rows);
    if (total != want || total_rows != want_rows || __syncthreads_or(bad != kNone)) {  // uniform: the source changed
        if (t == 0) res[ji].err = 4;
        return;
    }
    if (count) jstr_emit<true>(x, i0, mine, w0, w1, m, &bad, reinterpret_cast<char*>(image16) + bytes_before, content);
    __syncthreads();
    wg::copy_out_shifted<kJstrThreads>(reinterpret_cast<const uint32_t*>(image16), 0, job.dst + out0, total);
    // the lane that holds the k-th closing quote of the job writes row_ends[k]
    uint32_t* ends = const_cast<uint32_t*>(job.row_ends) + row0 + rows_before;
    for (uint32_t q = closing; q; q &= q - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(q);
        *ends++ = out0 + bytes_before + jrow_emit(x, i0, j, w0, w1, m, b, content, &bad, nullptr);
    }
}

// ------------------------------------------------------------------- UTF-8

__global__ void __launch_bounds__(kJstrThreads) jstr_utf8_kernel(const JsonStringJob* __restrict__ jobs, int njobs,
                                                                 uint32_t* __restrict__ bad) {
    __shared__ u32x4 stage16[kStage16];
    const uint32_t t = threadIdx.x;
    const int ji = wg::job_of<&JsonStringJob::first_chunk>(jobs, njobs, blockIdx.x);
    const JsonStringJob job = jobs[ji];
    const uint32_t c = blockIdx.x - job.first_chunk;
    if (c >= job.nchunks) return;  // uniform
    const uint32_t at = c * kC, left = job.n - at, len = left < kC ? left : kC;
    JstrText x;
    x.st = jstr_stage(stage16, job.src, job.n, at, len, 3, 3);
    x.at = at;
    x.n = job.n;
    __syncthreads();
    const uint32_t mine = jstr_mine(len);
    uint64_t w0, w1;
    jstr_lane_words(x.st, mine, &w0, &w1);
    if (((w0 | w1) & 0x8080808080808080ull) == 0) return;  // all ASCII
    const int64_t i0 = (int64_t)at + 16 * t;
    uint32_t lowest = kNone;
    for (uint32_t j = 0; j < mine && lowest == kNone; ++j) {
        const int64_t i = i0 + j;
        const uint8_t b = x.byte(i);
        if (b < 0x80) continue;
        bool fine;
        if (js::Utf8IsCont(b)) {
            fine = js::Utf8ContCovered(x.byte(i - 1), x.byte(i - 2), x.byte(i - 3), (uint64_t)i);
        } else {
            fine = js::Utf8SequenceLen(b, x.byte(i + 1), x.byte(i + 2), x.byte(i + 3), (uint64_t)job.n - (uint64_t)i) != 0;
        }
        if (!fine) lowest = (uint32_t)i;
    }
    if (lowest != kNone) atomicMin(&bad[ji], lowest);
}

__global__ void jstr_utf8_publish_kernel(const uint32_t* __restrict__ bad, int njobs, JsonStringResult* __restrict__ res) {
    const int ji = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (ji >= njobs) return;
    JsonStringResult r;
    r.len = 0;
    r.first_bad = bad[ji] == kNone ? 0u : bad[ji];
    r.err = bad[ji] != kNone;
    res[ji] = r;
}

// the job table to device memory, the counters to their start values
int jstr_begin(const JsonStringTables& t, hipStream_t s) {
    if (!t.jobs || !t.jobs_dev || !t.bad || (!t.res && !t.rows_res)) return -1;
    if (hipMemcpyAsync(t.jobs_dev, t.jobs, (size_t)t.njobs * sizeof(JsonStringJob), hipMemcpyHostToDevice, s) != hipSuccess)
        return -1;
    if (hipMemsetAsync(t.bad, 0xFF, (size_t)t.njobs * sizeof(uint32_t), s) != hipSuccess) return -1;
    if (t.ok && hipMemsetAsync(t.ok, 0, (size_t)t.njobs * sizeof(int32_t), s) != hipSuccess) return -1;
    // a job without chunks reads two equal entries, the last job the one past the end
    if (t.prefix && hipMemsetAsync(t.prefix, 0, ((size_t)t.nchunks + 1) * sizeof(uint32_t), s) != hipSuccess) return -1;
    return 0;
}

bool jstr_launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

int LaunchJsonStringEscape(const JsonStringTables& t, hipStream_t s) {
    if (t.njobs <= 0) return 0;
    if (!t.prefix || !t.ok || (t.ngroups && !t.groups) || jstr_begin(t, s) != 0) return -1;
    const dim3 threads(kJstrThreads), per_job((t.njobs + 63) / 64);
    if (t.nchunks) {
        hipLaunchKernelGGL(jstr_escape_size_kernel, dim3(t.nchunks), threads, 0, s, t.jobs_dev, t.njobs, t.prefix, t.groups);
        if (!jstr_launched()) return -1;
    }
    if (t.nrblocks) {
        hipLaunchKernelGGL(jstr_rows_check_kernel, dim3(t.nrblocks), threads, 0, s, t.jobs_dev, t.njobs, t.bad);
        if (!jstr_launched()) return -1;
    }
    if (t.nchunks && LaunchPbRunPrefix(t.prefix, (int)t.nchunks + 1, s) != 0) return -1;
    hipLaunchKernelGGL(jstr_verdict_kernel, per_job, dim3(64), 0, s, t.jobs_dev, t.njobs, t.prefix, t.bad, t.ok, t.res);
    if (!jstr_launched()) return -1;
    if (t.nrblocks) {
        hipLaunchKernelGGL(jstr_rows_punct_kernel, dim3(t.nrblocks), threads, 0, s, t.jobs_dev, t.njobs, t.prefix, t.groups,
                           t.ok);
        if (!jstr_launched()) return -1;
    }
    if (t.nchunks) {
        hipLaunchKernelGGL(jstr_escape_place_kernel, dim3(t.nchunks), threads, 0, s, t.jobs_dev, t.njobs, t.prefix, t.ok,
                           t.res);
        if (!jstr_launched()) return -1;
    }
    return 0;
}

int LaunchJsonStringUnescape(const JsonStringTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (!t.prefix || !t.ok || !t.info || jstr_begin(t, s) != 0) return -1;
    const dim3 threads(kJstrThreads), chunks(t.nchunks);
    hipLaunchKernelGGL(jstr_unescape_scan_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info);
    if (!jstr_launched()) return -1;
    hipLaunchKernelGGL(jstr_unescape_carry_kernel, dim3(t.njobs), threads, 0, s, t.jobs_dev, t.info, t.prefix, t.bad);
    if (!jstr_launched()) return -1;
    if (LaunchPbRunPrefix(t.prefix, (int)t.nchunks + 1, s) != 0) return -1;
    hipLaunchKernelGGL(jstr_verdict_kernel, dim3((t.njobs + 63) / 64), dim3(64), 0, s, t.jobs_dev, t.njobs, t.prefix, t.bad,
                       t.ok, t.res);
    if (!jstr_launched()) return -1;
    hipLaunchKernelGGL(jstr_unescape_place_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info, t.prefix, t.ok, t.res);
    return jstr_launched() ? 0 : -1;
}

int LaunchJsonStringValidate(const JsonStringTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (jstr_begin(t, s) != 0) return -1;
    hipLaunchKernelGGL(jstr_utf8_kernel, dim3(t.nchunks), dim3(kJstrThreads), 0, s, t.jobs_dev, t.njobs, t.bad);
    if (!jstr_launched()) return -1;
    hipLaunchKernelGGL(jstr_utf8_publish_kernel, dim3((t.njobs + 63) / 64), dim3(64), 0, s, t.bad, t.njobs, t.res);
    return jstr_launched() ? 0 : -1;
}

int LaunchJsonStringUnescapeRows(const JsonStringTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (!t.prefix || !t.ok || !t.info || !t.state || !t.rows_res || jstr_begin(t, s) != 0) return -1;
    // the second size table, behind the first
    if (hipMemsetAsync(t.prefix + t.nchunks + 1, 0, ((size_t)t.nchunks + 1) * sizeof(uint32_t), s) != hipSuccess) return -1;
    const dim3 threads(kJstrThreads), chunks(t.nchunks);
    hipLaunchKernelGGL(jstr_rows_scan_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info);
    if (!jstr_launched()) return -1;
    hipLaunchKernelGGL(jstr_rows_carry_kernel, dim3(t.njobs), threads, 0, s, t.jobs_dev, t.info, t.prefix, t.nchunks, t.state);
    if (!jstr_launched()) return -1;
    if (LaunchPbRunPrefix(t.prefix, 2 * ((int)t.nchunks + 1), s) != 0) return -1;
    hipLaunchKernelGGL(jstr_rows_verdict_kernel, dim3((t.njobs + 63) / 64), dim3(64), 0, s, t.jobs_dev, t.njobs, t.prefix,
                       t.nchunks, t.state, t.ok, t.rows_res);
    if (!jstr_launched()) return -1;
    hipLaunchKernelGGL(jstr_rows_place_kernel, chunks, threads, 0, s, t.jobs_dev, t.njobs, t.info, t.prefix, t.nchunks, t.ok,
                       t.rows_res);
    return jstr_launched() ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
