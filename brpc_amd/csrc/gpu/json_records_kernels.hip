// Records printed as JSON objects on gfx950 (kernels.h: init, size, prefix,
// measure, prefix, heads, place), the record builder's plan with a key prefix
// in the place of a field header. The reference prints such a batch field by
// field on the host through rapidjson's Writer (src/json2pb/pb_to_json.cpp);
// here a lane sizes and stores one element with the rules of
// base/json_records.h, the code the host twin json::FormatRecordObjects runs,
// and a record's lane composes the object around the cells.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "base/json_records.h"
#include "gpu/kernels.h"
#include "gpu/workgroup.h"

namespace mrpc {
namespace gpu {

namespace {

namespace jr = ::mrpc::json_records;
namespace np = ::mrpc::number_print;
namespace sd = ::mrpc::shortest_double;

constexpr int kJrThreads = (int)kJsonRecordsChunkElems;  // a lane per element
constexpr int kJrRows = (int)kJsonRecordsBlockRows;      // a lane per record
constexpr unsigned long long kJrNoRecord = ~0ull;        // the offender key: row << 4 | column
constexpr uint32_t kJrPrefixWords = kJsonRecordsPrefixStride / 4;

static_assert(kJsonRecordsGroupElems == 64 && kJrThreads % 64 == 0, "a group is a wave");
static_assert(kJsonRecordsPrefixStride >= jr::kMaxPrefixBytes && kJsonRecordsPrefixStride % 4 == 0, "prefix slots");
static_assert(64 * np::kMaxElemChars <= 0xFFFF, "a group's text fits elem_incl");
static_assert(jr::kMaxColumns <= 16, "the offender key keeps the column in four bits");

__device__ __forceinline__ bool jr_sized(const JsonRecordsColumn& col) { return col.text != jr::kBase64; }

// Text bytes of the column's elements before element e, e <= count.
__device__ __forceinline__ uint32_t jr_text_before(const JsonRecordsColumn& col, const uint32_t* __restrict__ groups,
                                                   const uint16_t* __restrict__ elem_incl, uint32_t e) {
    const uint32_t g = groups[col.first_group + e / 64] - groups[col.first_group];
    return (e & 63) ? g + elem_incl[col.first_elem + e - 1] : g;
}

// The job's text size, from the scanned block sums.
__device__ __forceinline__ uint32_t jr_job_total(const JsonRecordsJob& job, int j, const uint32_t* block_off) {
    const uint32_t first = job.first_rblock + (uint32_t)j;
    const uint32_t nblocks = (uint32_t)(((uint64_t)job.rows + kJsonRecordsBlockRows - 1) / kJsonRecordsBlockRows);
    return block_off[first + nblocks] - block_off[first];
}

// The first row in [lo, hi) whose end is above e, hi when there is none: the
// row element e lies in when the table ascends.
__device__ __forceinline__ uint32_t jr_row_above(const uint32_t* __restrict__ row_ends, uint32_t lo, uint32_t hi,
                                                 uint32_t e) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (row_ends[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kJrThreads) json_records_init_kernel(
    const JsonRecordsJob* __restrict__ jobs, int njobs, const JsonRecordsColumn* __restrict__ cols, int ncols,
    const uint32_t* __restrict__ prefixes, JsonRecordsJob* __restrict__ jobs_dev,
    JsonRecordsColumn* __restrict__ cols_dev, uint32_t* __restrict__ prefixes_dev, uint32_t* __restrict__ groups,
    unsigned long long* __restrict__ bad) {
    const uint32_t i = blockIdx.x * kJrThreads + threadIdx.x;
    if (i < (uint32_t)ncols * kJrPrefixWords) prefixes_dev[i] = prefixes[i];
    if (i < (uint32_t)njobs) {
        jobs_dev[i] = jobs[i];
        bad[i] = kJrNoRecord;
    }
    if (i >= (uint32_t)ncols) return;
    const JsonRecordsColumn col = cols[i];
    cols_dev[i] = col;
    // the group behind the last element: written again by the size pass when
    // it holds elements; its prefix is the column's total when it holds none
    if (jr_sized(col)) groups[col.first_group + col.count / 64] = 0;
}

__global__ void __launch_bounds__(kJrThreads) json_records_size_kernel(const JsonRecordsColumn* __restrict__ cols,
                                                                       int ncols, uint32_t* __restrict__ groups,
                                                                       uint16_t* __restrict__ elem_incl,
                                                                       sd::Decimal* __restrict__ digits) {
    const JsonRecordsColumn col = cols[wg::job_of<&JsonRecordsColumn::first_chunk>(cols, ncols, blockIdx.x)];
    if (!jr_sized(col)) return;  // the whole workgroup
    const uint32_t e = (blockIdx.x - col.first_chunk) * kJsonRecordsChunkElems + threadIdx.x;
    const bool live = e < col.count;
    uint32_t len = 0;
    if (live) {
        if (np::KindIsFloat(col.kind)) {
            const uint64_t bits = col.kind == np::kFloat32
                                      ? sd::WidenFloatBits(static_cast<const uint32_t*>(col.src)[e])
                                      : static_cast<const uint64_t*>(col.src)[e];
            const sd::Decimal d = sd::ShortestDigits(bits);
            digits[col.first_digit + e] = d;
            len = (uint32_t)sd::JsonDecimalLength(d);
        } else {
            len = jr::ElemTextBytes(col.src, e, col.kind);
        }
    }
    const uint32_t incl = wg::wave_incl_scan(len);
    if (live) elem_incl[col.first_elem + e] = (uint16_t)incl;
    // lane 63 holds the group's sum; the group has an element when its first lane is live
    if ((threadIdx.x & 63) == 63 && e - 63 < col.count) groups[col.first_group + e / 64] = incl;
}

__global__ void __launch_bounds__(kJrRows) json_records_measure_kernel(
    const JsonRecordsJob* __restrict__ jobs, int njobs, const JsonRecordsColumn* __restrict__ cols,
    const uint32_t* __restrict__ groups, const uint16_t* __restrict__ elem_incl, uint32_t* __restrict__ row_size,
    uint32_t* __restrict__ col_cell, uint32_t* __restrict__ col_delta, uint32_t* __restrict__ block_off,
    unsigned long long* __restrict__ bad) {
    __shared__ uint32_t wave_tot[kJrRows / 64];
    const int j = wg::job_of<&JsonRecordsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const JsonRecordsJob job = jobs[j];
    const uint32_t block = blockIdx.x - job.first_rblock;
    const uint64_t r64 = (uint64_t)block * kJsonRecordsBlockRows + threadIdx.x;
    const uint32_t r = (uint32_t)r64;
    uint32_t size = 0;
    if (r64 < job.rows) {
        size = job.fixed + jr::LeadBytes(r, job.brackets != 0) + jr::TrailBytes(r, job.rows, job.brackets != 0);
        for (uint32_t c = 0; c < job.ncols; ++c) {
            const JsonRecordsColumn col = cols[job.first_col + c];
            const bool scalar = col.row_ends == nullptr;
            uint32_t s = r, e = r + 1;  // a scalar column: host-checked count == rows
            if (!scalar) {
                s = r ? col.row_ends[r - 1] : 0;
                e = col.row_ends[r];
                if (jr::RowEndBad(s, e, r, job.rows, col.count)) atomicMin(&bad[j], ((unsigned long long)r << 4) | c);
                // a bad table gets nothing written; until then it must not
                // make a lane read past the source or the scratch
                s = s < col.count ? s : col.count;
                e = e < col.count ? e : col.count;
                e = e < s ? s : e;
            }
            uint32_t before = 0, inner;
            if (col.text == jr::kBase64) {
                inner = jr::Base64Inner(e - s);
            } else {
                before = jr_text_before(col, groups, elem_incl, s);
                inner = jr_text_before(col, groups, elem_incl, e) - before;
                if (!scalar && col.text == jr::kNumber) {
                    inner = jr::NumberRowInner(inner, e - s);
                    before += s;  // a comma in front of every element but the row's first
                }
            }
            const uint32_t at = col.first_row + r;
            col_cell[at] = inner;
            col_delta[at] = before;
            size += inner + jr::WrapperBytes(scalar);
        }
        row_size[job.first_row + r] = size;
    }
    uint32_t sum;
    wg::block_excl_scan<kJrRows>(size, wave_tot, &sum);
    if (threadIdx.x == 0) {
        // the job's blocks, then one entry that becomes its total under the scan
        const uint32_t at = blockIdx.x + (uint32_t)j;
        block_off[at] = sum;
        if ((uint64_t)(block + 1) * kJsonRecordsBlockRows >= job.rows) block_off[at + 1] = 0;
    }
}

__global__ void __launch_bounds__(kJrRows) json_records_heads_kernel(
    const JsonRecordsJob* __restrict__ jobs, int njobs, const JsonRecordsColumn* __restrict__ cols,
    const uint8_t* __restrict__ prefixes, const uint32_t* __restrict__ row_size, const uint32_t* __restrict__ col_cell,
    uint32_t* __restrict__ col_delta, const uint32_t* __restrict__ block_off,
    const unsigned long long* __restrict__ bad, JsonRecordsResult* __restrict__ res) {
    __shared__ uint32_t wave_tot[kJrRows / 64];
    const int j = wg::job_of<&JsonRecordsJob::first_rblock>(jobs, njobs, blockIdx.x);
    const JsonRecordsJob job = jobs[j];
    const uint64_t r64 = (uint64_t)(blockIdx.x - job.first_rblock) * kJsonRecordsBlockRows + threadIdx.x;
    const bool live = r64 < job.rows;
    const uint32_t r = (uint32_t)r64;
    const unsigned long long key = bad[j];
    const uint32_t total = jr_job_total(job, j, block_off);
    const bool ok = key == kJrNoRecord && total <= job.cap;
    if (r64 == 0) {
        res[j] = JsonRecordsResult{key != kJrNoRecord ? 0u : total, key != kJrNoRecord ? (uint32_t)(key >> 4) : jr::kNone,
                                   key != kJrNoRecord ? (uint32_t)(key & 15) : jr::kNone,
                                   key != kJrNoRecord ? 1 : (total > job.cap ? 3 : 0)};
    }
    if (!ok) return;  // the whole workgroup
    const uint32_t size = live ? row_size[job.first_row + r] : 0u;
    uint32_t block_size;
    uint32_t at = wg::block_excl_scan<kJrRows>(size, wave_tot, &block_size);
    if (!live) return;
    at += block_off[blockIdx.x + (uint32_t)j] - block_off[job.first_rblock + (uint32_t)j];
    if ((uint64_t)at + size > total) return;  // nothing leaves the text
    uint8_t* const dst = job.dst;
    // total <= cap: a store below total is a store inside dst
    auto put = [&](uint32_t where, uint8_t b) {
        if (where < total) dst[where] = b;
    };
    if (jr::LeadBytes(r, job.brackets != 0)) put(at++, r > 0 ? ',' : '[');
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const JsonRecordsColumn col = cols[job.first_col + c];
        const uint8_t* prefix = prefixes + (size_t)(job.first_col + c) * kJsonRecordsPrefixStride;
        const uint32_t pn = col.prefix_len <= kJsonRecordsPrefixStride ? col.prefix_len : kJsonRecordsPrefixStride;
        for (uint32_t k = 0; k < pn; ++k) put(at + k, prefix[k]);
        at += pn;
        const bool scalar = col.row_ends == nullptr;
        const uint32_t inner = col_cell[col.first_row + r];
        const uint8_t open = col.text == jr::kNumber ? '[' : '"', close = col.text == jr::kNumber ? ']' : '"';
        if (!scalar) put(at++, open);
        col_delta[col.first_row + r] = at - col_delta[col.first_row + r];
        at += inner;
        if (!scalar) put(at++, close);
    }
    put(at++, '}');
    if (jr::TrailBytes(r, job.rows, job.brackets != 0)) put(at, ']');
}

__global__ void __launch_bounds__(kJrThreads) json_records_place_kernel(
    const JsonRecordsJob* __restrict__ jobs, const JsonRecordsColumn* __restrict__ cols, int ncols,
    const uint32_t* __restrict__ groups, const uint16_t* __restrict__ elem_incl,
    const sd::Decimal* __restrict__ digits, const uint32_t* __restrict__ block_off,
    const uint32_t* __restrict__ col_delta, const unsigned long long* __restrict__ bad,
    JsonRecordsResult* __restrict__ res) {
    __shared__ uint32_t wave_tot[kJrThreads / 64];
    const JsonRecordsColumn col = cols[wg::job_of<&JsonRecordsColumn::first_chunk>(cols, ncols, blockIdx.x)];
    const int j = (int)col.job;
    const JsonRecordsJob job = jobs[j];
    if (bad[j] != kJrNoRecord) return;  // the whole workgroup, here and below
    const uint32_t total = jr_job_total(job, j, block_off);
    if (total > job.cap) return;
    const uint32_t start = (blockIdx.x - col.first_chunk) * kJsonRecordsChunkElems;
    const uint32_t e = start + threadIdx.x;
    const bool live = e < col.count;
    const bool scalar = col.row_ends == nullptr;
    // the row of element e and where it starts
    uint32_t r = e, s = e, row_len = 1;
    uint32_t changed = 0;
    if (!scalar) {
        const uint32_t last = col.count - start > kJsonRecordsChunkElems ? start + kJsonRecordsChunkElems - 1 : col.count - 1;
        const uint32_t lo = jr_row_above(col.row_ends, 0, job.rows, start);  // the same in every lane
        const uint32_t hi = jr_row_above(col.row_ends, lo, job.rows, last);
        if (live) {
            r = jr_row_above(col.row_ends, lo, hi, e);
            if (r >= job.rows) {
                changed = 1;  // the table is not the one the measure pass saw
                r = 0;
            }
            s = r ? col.row_ends[r - 1] : 0;
            const uint32_t end = col.row_ends[r];
            if (s > e || end <= e || end > col.count) changed = 1;
            row_len = end - s;
        }
    }
    // what the lane stores: `len` bytes at `pos`, measured as `want` bytes
    uint32_t len = 0, want = 0, pos = 0;
    np::Integer v = {0, false};
    uint8_t byte = 0;
    sd::Decimal d;
    d.cls = sd::kZero;
    const bool is_float = np::KindIsFloat(col.kind);
    const bool comma = live && !scalar && col.text == jr::kNumber && e > s;
    if (live && !changed) {
        const uint32_t delta = col_delta[col.first_row + r];
        if (col.text == jr::kBase64) {
            const uint32_t k = e - s;
            if (k % 3 == 0) {
                len = want = 4;
                pos = delta + 4 * (k / 3);
            }
        } else {
            const uint32_t in_group = (e & 63) ? elem_incl[col.first_elem + e - 1] : 0u;
            want = elem_incl[col.first_elem + e] - in_group;
            pos = delta + groups[col.first_group + e / 64] - groups[col.first_group] + in_group;
            if (!scalar && col.text == jr::kNumber) pos += e;
            if (col.kind == jr::kKindBytes) {
                byte = static_cast<const uint8_t*>(col.src)[e];
                len = json_string::EscapedSize(byte);
            } else if (col.kind == np::kBool) {
                byte = static_cast<const uint8_t*>(col.src)[e] != 0;
                len = np::BoolLength(byte != 0);
            } else if (is_float) {
                d = digits[col.first_digit + e];
                len = (uint32_t)sd::JsonDecimalLength(d);
            } else {
                v = np::LoadInteger(col.src, e, col.kind);
                len = np::IntegerLength(v);
            }
        }
        // a comma stands at pos - 1: pos >= 1 behind the cell's '['
        if (len != want || (uint64_t)pos + len > total || (comma && pos == 0)) changed = 1;
    }
    if (wg::block_sum<kJrThreads>(changed, wave_tot) != 0) {
        if (threadIdx.x == 0) res[j].err = 4;
        return;
    }
    if (!live || len == 0) return;
    char* o = reinterpret_cast<char*>(job.dst) + pos;
    if (comma) o[-1] = ',';
    if (col.text == jr::kBase64) {
        const uint32_t sym = jr::Base64Group(static_cast<const uint8_t*>(col.src) + s, e - s, row_len);
        o[0] = (char)sym;
        o[1] = (char)(sym >> 8);
        o[2] = (char)(sym >> 16);
        o[3] = (char)(sym >> 24);
    } else if (col.kind == jr::kKindBytes) {
        json_string::EscapeByte(byte, o);
    } else if (col.kind == np::kBool) {
        np::FormatBool(byte != 0, o);
    } else if (is_float) {
        sd::FormatJsonDecimal(d, o);
    } else {
        np::FormatInteger(v, o);
    }
}

}  // namespace

int LaunchJsonRecordsPrint(const JsonRecordsTables& t, hipStream_t s) {
    if (t.njobs <= 0) return 0;
    if (!t.jobs || !t.cols || t.ncols <= 0 || !t.prefixes || !t.jobs_dev || !t.cols_dev || !t.prefixes_dev ||
        !t.row_size || !t.col_cell || !t.col_delta || !t.block_off || !t.bad || !t.res || t.nrblocks == 0 ||
        (t.ngroups > 0 && !t.groups) || (t.nelems > 0 && !t.elem_incl) || (t.ndigits > 0 && !t.digits) ||
        t.ngroups > 0x7FFFFFFFu) {
        return -1;
    }
    const unsigned init_lanes = (unsigned)t.ncols * kJrPrefixWords;  // above the column and job counts
    hipLaunchKernelGGL(json_records_init_kernel, dim3((init_lanes + kJrThreads - 1) / kJrThreads), dim3(kJrThreads), 0,
                       s, t.jobs, t.njobs, t.cols, t.ncols, reinterpret_cast<const uint32_t*>(t.prefixes), t.jobs_dev,
                       t.cols_dev, reinterpret_cast<uint32_t*>(t.prefixes_dev), t.groups, t.bad);
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.ngroups > 0) {
        if (t.nchunks > 0) {
            hipLaunchKernelGGL(json_records_size_kernel, dim3(t.nchunks), dim3(kJrThreads), 0, s, t.cols_dev, t.ncols,
                               t.groups, t.elem_incl, static_cast<sd::Decimal*>(t.digits));
            if (hipGetLastError() != hipSuccess) return -1;
        }
        if (LaunchPbRunPrefix(t.groups, (int)t.ngroups, s) != 0) return -1;
    }
    hipLaunchKernelGGL(json_records_measure_kernel, dim3(t.nrblocks), dim3(kJrRows), 0, s, t.jobs_dev, t.njobs,
                       t.cols_dev, t.groups, t.elem_incl, t.row_size, t.col_cell, t.col_delta, t.block_off, t.bad);
    if (hipGetLastError() != hipSuccess) return -1;
    if (LaunchPbRunPrefix(t.block_off, (int)(t.nrblocks + (uint32_t)t.njobs), s) != 0) return -1;
    hipLaunchKernelGGL(json_records_heads_kernel, dim3(t.nrblocks), dim3(kJrRows), 0, s, t.jobs_dev, t.njobs,
                       t.cols_dev, t.prefixes_dev, t.row_size, t.col_cell, t.col_delta, t.block_off, t.bad, t.res);
    if (hipGetLastError() != hipSuccess) return -1;
    if (t.nchunks == 0) return 0;
    hipLaunchKernelGGL(json_records_place_kernel, dim3(t.nchunks), dim3(kJrThreads), 0, s, t.jobs_dev, t.cols_dev,
                       t.ncols, t.groups, t.elem_incl, static_cast<const sd::Decimal*>(t.digits), t.block_off,
                       t.col_delta, t.bad, t.res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
