// Number arrays and nested number rows printed to JSON text on gfx950
// (kernels.h: size, rows, prefix, place), the inverse of the number-text
// parser in json_kernels.hip. The reference prints such fields element by
// element on the host through rapidjson's Writer
// (src/json2pb/pb_to_json.cpp); here a lane formats one element with
// base/number_print.h and base/shortest_double.h, the code the host twin
// json::FormatNumberRows runs, and the punctuation of the nested form comes
// from the table of row ends without a look at any other element's text.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "base/number_print.h"
#include "base/shortest_double.h"
#include "gpu/kernels.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

namespace np = ::mrpc::number_print;
namespace sd = ::mrpc::shortest_double;
using wg::u32x4;

constexpr int kNpThreads = (int)kJsonNumberPrintChunkElems;  // a lane per element, or per row
constexpr int kNpWaves = kNpThreads / 64;
constexpr uint32_t kNpSlot = np::kMaxLead + np::kMaxElemChars + np::kMaxTrail;  // an element with its punctuation
constexpr int kNpImage16 = (int)(kJsonNumberPrintChunkElems * kNpSlot + 16 + 15) / 16;  // at any 16-byte phase

static_assert(JSON_FLOAT32 == (uint32_t)np::kFloat32 && JSON_FLOAT64 == (uint32_t)np::kFloat64 &&
                  (uint32_t)PB_RUN_BOOL == (uint32_t)np::kBool && (uint32_t)PB_RUN_SINT64 == (uint32_t)np::kSint64,
              "base/number_print.h numbers the kinds as kernels.h does");

// The chunk a workgroup owns: elements [start, start + n) of its job.
struct NpChunk {
    int ja;
    uint32_t index;  // within the job
    uint32_t start, n;
};

__device__ __forceinline__ NpChunk np_chunk(const JsonNumberPrintJob* __restrict__ jobs, int njobs, uint32_t ci,
                                            JsonNumberPrintJob* job) {
    NpChunk c;
    c.ja = wg::job_of<&JsonNumberPrintJob::first_chunk>(jobs, njobs, ci);
    *job = jobs[c.ja];
    c.index = ci - job->first_chunk;
    c.start = c.index * kJsonNumberPrintChunkElems;
    const uint32_t left = job->count > c.start ? job->count - c.start : 0;  // 0: the chunk of "[]"
    c.n = left < kJsonNumberPrintChunkElems ? left : kJsonNumberPrintChunkElems;
    return c;
}

// starts[k] = 1 where element c.start + k begins a row after the first. One
// lower-bound search, the same in every lane, finds the first row end that is
// not before the chunk; of an ascending table only the 256 entries from there
// on can fall into it, a lane each. A table that does not ascend marks what
// it marks: its job is refused by the rows pass and prints nothing. Holds two
// barriers; starts is readable afterwards.
__device__ __forceinline__ void np_row_starts(const JsonNumberPrintJob& job, const NpChunk& c, uint8_t* starts) {
    const uint32_t t = threadIdx.x;
    starts[t] = 0;
    __syncthreads();
    if (job.form == np::kNested && c.n > 0) {
        uint32_t lo = 0, hi = job.rows;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (job.row_ends[mid] < c.start) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t r = (uint64_t)lo + t;
        if (r < job.rows) {
            const uint32_t e = job.row_ends[r];
            if (e > 0 && e >= c.start && e - c.start < c.n) starts[e - c.start] = 1;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ uint64_t np_float_bits(const JsonNumberPrintJob& job, uint32_t g) {
    if (job.kind == np::kFloat32) return sd::WidenFloatBits(static_cast<const uint32_t*>(job.src)[g]);
    return static_cast<const uint64_t*>(job.src)[g];
}

__global__ void __launch_bounds__(kNpThreads) json_number_size_kernel(const JsonNumberPrintJob* __restrict__ jobs,
                                                                      int njobs, uint32_t nchunks,
                                                                      uint32_t* __restrict__ sizes,
                                                                      uint32_t* __restrict__ bad,
                                                                      sd::Decimal* __restrict__ digits) {
    __shared__ uint32_t wave_tot[kNpWaves];
    __shared__ uint8_t starts[kNpThreads];
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    JsonNumberPrintJob job;
    const NpChunk c = np_chunk(jobs, njobs, ci, &job);
    if (ci == 0 && t == 0) sizes[nchunks] = 0;  // becomes the total under the scan
    if (c.index == 0 && t == 0) bad[c.ja] = np::kNone;  // the rows pass lowers it
    np_row_starts(job, c, starts);
    uint32_t len = 0;
    if (t < c.n) {
        const uint32_t g = c.start + t;
        if (job.kind == np::kBool) {
            len = np::BoolLength(static_cast<const uint8_t*>(job.src)[g] != 0);
        } else if (np::KindIsFloat(job.kind)) {
            const sd::Decimal d = sd::ShortestDigits(np_float_bits(job, g));
            digits[(uint64_t)ci * kJsonNumberPrintChunkElems + t] = d;
            len = (uint32_t)sd::JsonDecimalLength(d);
        } else {
            len = np::IntegerLength(np::LoadInteger(job.src, g, job.kind));
        }
        len += np::LeadLength(job.form, g == 0, starts[t] != 0) + np::TrailLength(job.form, g + 1 == job.count);
    } else if (t == 0 && job.count == 0 && job.form == np::kBracketed) {
        len = 2;  // "[]"
    }
    const uint32_t total = wg::block_sum<kNpThreads>(len, wave_tot);
    if (t == 0) sizes[ci] = total;
}

__global__ void __launch_bounds__(kNpThreads) json_number_rows_kernel(const JsonNumberPrintJob* __restrict__ jobs,
                                                                      int njobs, uint32_t* __restrict__ bad) {
    const uint32_t rb = blockIdx.x, t = threadIdx.x;
    const int ja = wg::job_of<&JsonNumberPrintJob::first_row_block>(jobs, njobs, rb);
    const JsonNumberPrintJob job = jobs[ja];
    const uint64_t r = (uint64_t)(rb - job.first_row_block) * kJsonNumberPrintChunkElems + t;
    if (r >= job.rows) return;
    const uint32_t prev = r ? job.row_ends[r - 1] : 0u;
    if (np::RowEndBad(prev, job.row_ends[r], r, job.rows, job.count)) atomicMin(&bad[ja], (uint32_t)r);
}

__global__ void __launch_bounds__(kNpThreads) json_number_place_kernel(const JsonNumberPrintJob* __restrict__ jobs,
                                                                       int njobs,
                                                                       const uint32_t* __restrict__ prefix,
                                                                       const uint32_t* __restrict__ bad,
                                                                       const sd::Decimal* __restrict__ digits,
                                                                       JsonNumberPrintResult* __restrict__ res) {
    __shared__ u32x4 image16[kNpImage16];
    __shared__ uint32_t wave_tot[kNpWaves];
    __shared__ uint8_t starts[kNpThreads];
    uint8_t* image = reinterpret_cast<uint8_t*>(image16);
    const uint32_t ci = blockIdx.x, t = threadIdx.x;
    JsonNumberPrintJob job;
    const NpChunk c = np_chunk(jobs, njobs, ci, &job);
    // the host refuses jobs whose worst case passes 2^32 - 1, so the
    // differences of the scan (mod 2^32) are the sizes themselves
    const uint32_t first = prefix[job.first_chunk];
    const uint32_t job_len = prefix[job.first_chunk + job.nchunks] - first;
    const uint32_t bad_row = bad[c.ja];
    const bool fits = (uint64_t)job_len <= job.cap;
    if (c.index == 0 && t == 0) {
        if (bad_row != np::kNone) {
            res[c.ja].first_bad = bad_row;
            res[c.ja].err = 1;
        } else {
            res[c.ja].len = job_len;
            if (!fits) res[c.ja].err = 3;
        }
    }
    if (bad_row != np::kNone || !fits) return;  // the whole workgroup leaves: nothing of this job is written
    const uint32_t want = prefix[ci + 1] - prefix[ci];
    uint8_t* dst = job.dst + (uint32_t)(prefix[ci] - first);
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15);
    np_row_starts(job, c, starts);
    const uint32_t g = c.start + t;
    const bool is_float = np::KindIsFloat(job.kind);
    sd::Decimal d;
    np::Integer v = {0, false};
    bool b = false;
    uint32_t text = 0, lead = 0, trail = 0, len = 0;
    if (t < c.n) {
        if (job.kind == np::kBool) {
            b = static_cast<const uint8_t*>(job.src)[g] != 0;
            text = np::BoolLength(b);
        } else if (is_float) {
            d = digits[(uint64_t)ci * kJsonNumberPrintChunkElems + t];
            text = (uint32_t)sd::JsonDecimalLength(d);
        } else {
            v = np::LoadInteger(job.src, g, job.kind);
            text = np::IntegerLength(v);
        }
        lead = np::LeadLength(job.form, g == 0, starts[t] != 0);
        trail = np::TrailLength(job.form, g + 1 == job.count);
        len = lead + text + trail;
        if (text > np::kMaxElemChars) len = 0;  // whatever the slot holds, never past the image
    } else if (t == 0 && job.count == 0 && job.form == np::kBracketed) {
        len = 2;
    }
    uint32_t total;
    const uint32_t pos = wg::block_excl_scan<kNpThreads>(len, wave_tot, &total);
    if (len) {
        char* o = reinterpret_cast<char*>(image + sh + pos);
        if (t >= c.n) {
            o[0] = '[';
            o[1] = ']';
        } else {
            o += np::FormatLead(job.form, g == 0, starts[t] != 0, o);
            if (job.kind == np::kBool) o += np::FormatBool(b, o);
            else if (is_float) o += sd::FormatJsonDecimal(d, o);
            else o += np::FormatInteger(v, o);
            np::FormatTrail(job.form, g + 1 == job.count, o);
        }
    }
    __syncthreads();
    if (total != want) {  // not what the size pass measured, and every later offset assumed `want`
        if (t == 0) res[c.ja].err = 4;
        return;
    }
    wg::copy_out_phased<kNpThreads>(image, sh, dst, total);  // the image sits at dst's phase
}

}  // namespace

int LaunchJsonNumberPrint(const JsonNumberPrintTables& t, hipStream_t s) {
    if (t.njobs <= 0 || t.nchunks == 0) return 0;
    if (!t.jobs || !t.prefix || !t.bad || !t.res) return -1;
    hipLaunchKernelGGL(json_number_size_kernel, dim3(t.nchunks), dim3(kNpThreads), 0, s, t.jobs, t.njobs, t.nchunks,
                       t.prefix, t.bad, static_cast<sd::Decimal*>(t.digits));
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.nrow_blocks) {
        hipLaunchKernelGGL(json_number_rows_kernel, dim3(t.nrow_blocks), dim3(kNpThreads), 0, s, t.jobs, t.njobs,
                           t.bad);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    if (LaunchPbRunPrefix(t.prefix, (int)t.nchunks + 1, s) != 0) return -1;
    hipLaunchKernelGGL(json_number_place_kernel, dim3(t.nchunks), dim3(kNpThreads), 0, s, t.jobs, t.njobs, t.prefix,
                       t.bad, static_cast<const sd::Decimal*>(t.digits), t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
