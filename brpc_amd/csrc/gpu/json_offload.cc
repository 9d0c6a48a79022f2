// Device half of json2pb for large bodies (the reference parses
// every http+json body on the CPU, src/json2pb/json_to_pb.cpp): the body is
// copied into a pinned buffer, LaunchJsonIndex (gpu/json_kernels.hip) reads
// it there and writes every structural position straight into pinned
// memory, and json::ParseWithIndex walks the positions: one launch and one
// fiber-friendly wait per body. (-json_index_direct_host=false keeps the
// older staging through HBM: a copy kernel in, the index, a second wait for
// the count, a copy of count * 4 bytes back.)
#include "gpu/json_offload.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstring>

#include "base/decimal_to_double.h"
#include "base/flags.h"
#include "base/json_records.h"
#include "base/number_print.h"
#include "base/shortest_double.h"
#include "base/time.h"
#include "gpu/gpu.h"
#include "gpu/hbm_pool.h"
#include "gpu/kernels.h"
#include "gpu/scoped.h"
#include "gpu/snappy_offload.h"
#include "json/json.h"
#include "json/json2pb.h"
#include "rpc/span.h"
#include "var/var.h"

DEFINE_int32(gpu_pb2json_min_elems, 4096,
             "repeated integer/bool fields with at least this many elements are printed by the device in pb2json "
             "(pb_run_encode_kernel, decimal format) and integer arrays of at least as many elements are parsed by "
             "json_int_array_kernel in json2pb, while the GPU JSON path is enabled");
DEFINE_int32(gpu_pb2json_float_min_elems, 4096,
             "repeated float / double fields with at least this many elements are printed by the device in pb2json "
             "(json_float_size_kernel / json_float_place_kernel) while the GPU JSON path is enabled; shorter ones by "
             "the host printer (4096: the smallest size measured, where the device already wins, "
             "profiles/json_float_print.txt). 0: never. Reloadable");
MRPC_VALIDATE_FLAG(gpu_pb2json_float_min_elems, ::mrpc::PassValidator);
DEFINE_int32(gpu_json2pb_float_min_elems, 4096,
             "JSON arrays of numbers that are not all int64 (floats) with at least this many elements are parsed by "
             "the device in json2pb (json_number_array_kernel) while the GPU JSON path is enabled; shorter ones by "
             "the host's packed pass (4096: the smallest size measured, where the device already wins, "
             "profiles/json_float_parse.txt). 0: never. Reloadable");
MRPC_VALIDATE_FLAG(gpu_json2pb_float_min_elems, ::mrpc::PassValidator);
DEFINE_int32(json_index_min_density, 8,
             "structural characters per KiB (sampled in three windows) a JSON body needs before the GPU index is "
             "used; sparser bodies (long strings) parse faster on the host; 0: always offload");
DEFINE_bool(json_index_direct_host, true,
            "the JSON index kernel reads the pinned body and writes positions to pinned memory directly");

namespace mrpc {
namespace gpu {

namespace {

int g_device = -1;
std::atomic<int64_t> g_bodies{0}, g_bytes{0}, g_failures{0};
std::atomic<int64_t> g_sparse{0};

// Structural characters per KiB in three 1 KiB windows (start, middle,
// end). A body that is mostly one long string (the http_json_64KB leg)
// has almost none: the host parser crosses it with memchr faster than a
// device round trip returns its index, so such bodies are not offloaded.
bool structurally_sparse(const char* data, size_t n) {
    const int need = FLAGS_json_index_min_density;
    if (need <= 0 || n < 3 * 1024) return false;
    int hits = 0;
    for (size_t w : {(size_t)0, n / 2 - 512, n - 1024}) {
        for (size_t i = w; i < w + 1024; ++i) {
            const char c = data[i];
            hits += c == '"' || c == ',' || c == ':' || c == '{' || c == '[';
        }
    }
    return hits < 3 * need;
}

bool offload(const char* data, size_t n, std::vector<uint32_t>* index) {
    if (g_device < 0) return false;
    if (structurally_sparse(data, n)) {
        g_sparse.fetch_add(1, std::memory_order_relaxed);
        return false;
    }
    Span* span = IsRpczEnabled() ? Span::tls_parent() : nullptr;
    const int64_t t0 = span ? monotonic_us() : 0;
    const int rc = JsonIndex(data, n, index, g_device);
    if (rc != 0) {
        g_failures.fetch_add(1, std::memory_order_relaxed);
        return false;  // malformed or no device: the CPU parser reports it
    }
    g_bodies.fetch_add(1, std::memory_order_relaxed);
    g_bytes.fetch_add((int64_t)n, std::memory_order_relaxed);
    if (span) {
        span->AnnotateDevice(string_printf("json index %zu B -> %zu positions dev%d", n, index->size(), g_device),
                             (float)(monotonic_us() - t0) / 1000.0f);
    }
    return true;
}

}  // namespace

int JsonIndex(const char* data, size_t n, std::vector<uint32_t>* out, int device) {
    out->clear();
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull || device < 0) return -1;
    if (FLAGS_json_index_direct_host) {
        PinnedBlock body(n), pos(n * sizeof(uint32_t)), meta(16);  // every byte could be a position
        HbmBlock scratch(JsonIndexScratchBytes(n), device);
        if (!body || !pos || !meta || !scratch) return -1;
        memcpy(body.p, data, n);
        uint64_t* count = meta.as<uint64_t>();
        int* err = reinterpret_cast<int*>(count + 1);
        const int rc = RunOnPoolStream(device, [&](hipStream_t s) {
            return LaunchJsonIndex(body.as<uint8_t>(), n, pos.as<uint32_t>(), n, count, err, scratch.p, s);
        });
        if (rc != 0 || *err != 0 || *count > n) return -1;
        out->assign(pos.as<uint32_t>(), pos.as<uint32_t>() + *count);
        return 0;
    }
    // every byte could be a position; the count decides what comes back
    HbmBlock in(n, device), pos(n * sizeof(uint32_t), device), scratch(JsonIndexScratchBytes(n), device);
    PinnedBlock bounce(n), meta(16);
    if (!in || !pos || !scratch || !bounce || !meta) return -1;
    memcpy(bounce.p, data, n);
    uint64_t* count = meta.as<uint64_t>();
    int* err = reinterpret_cast<int*>(count + 1);
    int rc = RunOnPoolStream(device, [&](hipStream_t s) {
        Segment seg{bounce.p, in.p, n};
        if (LaunchBatchedCopy(&seg, 1, s) != 0) return -1;
        return LaunchJsonIndex(in.as<uint8_t>(), n, pos.as<uint32_t>(), n, count, err, scratch.p, s);
    });
    if (rc != 0 || *err != 0) return -1;
    if (*count == 0) return 0;
    const size_t bytes = (size_t)*count * sizeof(uint32_t);
    PinnedBlock back(bytes);
    if (!back) return -1;
    rc = RunOnPoolStream(device, [&](hipStream_t s) {
        Segment seg{pos.p, back.p, bytes};
        return LaunchBatchedCopy(&seg, 1, s);
    });
    if (rc != 0) return -1;
    out->assign(back.as<uint32_t>(), back.as<uint32_t>() + *count);
    return 0;
}

uint64_t FloatPrintWorstCaseBytes(uint64_t count) {
    return count ? count * (uint64_t)(shortest_double::kMaxJsonDoubleChars + 1) - 1 : 0;
}

int DevicePrintFloatArrays(DeviceFloatPrintJob* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    // refuse what must not reach a kernel; count the chunks of the rest
    uint64_t nchunks = 0;
    std::vector<int> live;  // the jobs that go to the device, in order
    for (int i = 0; i < n; ++i) {
        DeviceFloatPrintJob& j = jobs[i];
        j.len = 0;
        j.err = 0;
        if (j.count == 0) continue;
        const size_t eb = j.kind == kJsonFloat32 ? 4 : 8;
        if ((j.kind != kJsonFloat32 && j.kind != kJsonFloat64) || !j.src || !j.dst ||
            ((uintptr_t)j.src & (eb - 1)) != 0 || j.count > 0xFFFFFFFFull / (shortest_double::kMaxJsonDoubleChars + 1)) {
            j.err = 2;
            continue;
        }
        nchunks += (j.count + kJsonFloatChunkElems - 1) / kJsonFloatChunkElems;
        live.push_back(i);
    }
    if (live.empty()) return 0;
    if (nchunks > 0x3FFFFFFFull) return -1;  // the tables are indexed with int
    const int nlive = (int)live.size();
    const size_t jobs_bytes = live.size() * sizeof(JsonFloatJob);
    const size_t chunks_bytes = (size_t)nchunks * sizeof(JsonFloatChunk);
    const size_t res_bytes = live.size() * sizeof(JsonFloatResult);
    PinnedBlock tables(jobs_bytes + chunks_bytes + res_bytes);
    HbmBlock prefix((size_t)(nchunks + 1) * sizeof(uint32_t), device);
    HbmBlock digits((size_t)nchunks * kJsonFloatChunkElems * sizeof(shortest_double::Decimal), device);
    if (!tables || !prefix || !digits) return -1;
    JsonFloatJob* tj = tables.as<JsonFloatJob>();
    JsonFloatChunk* tc = reinterpret_cast<JsonFloatChunk*>(tables.p + jobs_bytes);
    JsonFloatResult* tr = reinterpret_cast<JsonFloatResult*>(tables.p + jobs_bytes + chunks_bytes);
    uint32_t ci = 0;
    for (int k = 0; k < nlive; ++k) {
        const DeviceFloatPrintJob& j = jobs[live[k]];
        const size_t eb = j.kind == kJsonFloat32 ? 4 : 8;
        const uint32_t nc = (uint32_t)((j.count + kJsonFloatChunkElems - 1) / kJsonFloatChunkElems);
        tj[k] = JsonFloatJob{static_cast<uint8_t*>(j.dst), j.cap, ci, nc};
        tr[k] = JsonFloatResult{0, 0, 0};
        for (uint32_t c = 0; c < nc; ++c) {
            const uint64_t at = (uint64_t)c * kJsonFloatChunkElems;
            const uint64_t left = j.count - at;
            tc[ci + c] = JsonFloatChunk{static_cast<const char*>(j.src) + at * eb,
                                        (uint32_t)std::min<uint64_t>(left, kJsonFloatChunkElems), j.kind, (uint32_t)k,
                                        c + 1 == nc ? 1u : 0u};
        }
        ci += nc;
    }
    JsonFloatTables t;
    t.jobs = tj;
    t.njobs = nlive;
    t.chunks = tc;
    t.nchunks = (int)nchunks;
    t.prefix = prefix.as<uint32_t>();
    t.digits = digits.p;
    t.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonFloatPrint(t, s); }) != 0) return -1;
    for (int k = 0; k < nlive; ++k) {
        jobs[live[k]].len = tr[k].len;
        jobs[live[k]].err = tr[k].err;
    }
    return 0;
}

int PrintFloatsOnDevice(const void* values, size_t n, uint32_t kind, std::string* out, int device) {
    if (!out || device < 0 || (kind != kJsonFloat32 && kind != kJsonFloat64)) return -1;
    if (n == 0) {
        out->clear();
        return 0;
    }
    if (!values) return -1;
    const size_t eb = kind == kJsonFloat32 ? 4 : 8;
    const uint64_t cap = FloatPrintWorstCaseBytes(n);
    if (cap > 0xFFFFFFFFull) return -1;
    PinnedBlock stage(n * eb), text((size_t)cap);
    if (!stage || !text) return -1;
    memcpy(stage.p, values, n * eb);
    DeviceFloatPrintJob job;
    job.src = stage.p;
    job.count = n;
    job.kind = kind;
    job.dst = text.p;
    job.cap = cap;
    if (DevicePrintFloatArrays(&job, 1, device) != 0 || job.err != 0 || job.len > cap) return -1;
    out->assign(text.p, (size_t)job.len);
    return 0;
}

uint64_t NumberPrintWorstCaseBytes(uint32_t kind, uint64_t count, uint64_t rows) {
    return number_print::WorstCaseBytes(kind, count, rows);
}

uint32_t JsonNumberPrintChunkElems() { return kJsonNumberPrintChunkElems; }

int DevicePrintNumbers(DeviceNumberPrintJob* jobs, int n, int device) {
    namespace np = number_print;
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    // refuse what must not reach a kernel; count the chunks and row blocks of the rest
    uint64_t nchunks = 0, nrow_blocks = 0;
    bool any_float = false;
    std::vector<int> live;  // the jobs that go to the device, in order
    auto overlaps = [](const void* a, uint64_t an, const void* b, uint64_t bn) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return an > 0 && bn > 0 && x < y + bn && y < x + an;
    };
    for (int i = 0; i < n; ++i) {
        DeviceNumberPrintJob& j = jobs[i];
        j.len = 0;
        j.first_bad = np::kNone;
        j.err = 0;
        if (!np::KindValid(j.kind) || (j.row_ends == nullptr) != (j.rows == 0)) {
            j.err = 2;
            continue;
        }
        if (j.count == 0 && !j.row_ends && !j.brackets) continue;
        const uint64_t eb = np::ElemBytes(j.kind);
        if ((!j.src && j.count > 0) || !j.dst || ((uintptr_t)j.src & (eb - 1)) != 0 || ((uintptr_t)j.row_ends & 3) != 0 ||
            np::WorstCaseBytes(j.kind, j.count, j.rows) > 0xFFFFFFFFull ||
            overlaps(j.dst, j.cap, j.src, j.count * eb) || overlaps(j.dst, j.cap, j.row_ends, j.rows * 4)) {
            j.err = 2;
            continue;
        }
        nchunks += std::max<uint64_t>(1, (j.count + kJsonNumberPrintChunkElems - 1) / kJsonNumberPrintChunkElems);
        nrow_blocks += (j.rows + kJsonNumberPrintChunkElems - 1) / kJsonNumberPrintChunkElems;
        any_float |= np::KindIsFloat(j.kind);
        live.push_back(i);
    }
    if (live.empty()) return 0;
    if (nchunks > 0x3FFFFFFFull || nrow_blocks > 0x3FFFFFFFull) return -1;  // one grid each; the tables are indexed with int
    const int nlive = (int)live.size();
    const size_t jobs_bytes = live.size() * sizeof(JsonNumberPrintJob);
    PinnedBlock tables(jobs_bytes + live.size() * sizeof(JsonNumberPrintResult));
    HbmBlock words((size_t)(nchunks + 1 + live.size()) * sizeof(uint32_t), device);  // the prefix, then bad[]
    HbmBlock digits(any_float ? (size_t)nchunks * kJsonNumberPrintChunkElems * sizeof(shortest_double::Decimal) : 16,
                    device);
    if (!tables || !words || !digits) return -1;
    JsonNumberPrintJob* tj = tables.as<JsonNumberPrintJob>();
    JsonNumberPrintResult* tr = reinterpret_cast<JsonNumberPrintResult*>(tables.p + jobs_bytes);
    uint32_t chunk = 0, row_block = 0;
    for (int k = 0; k < nlive; ++k) {
        const DeviceNumberPrintJob& j = jobs[live[k]];
        const uint32_t nc = (uint32_t)std::max<uint64_t>(
            1, (j.count + kJsonNumberPrintChunkElems - 1) / kJsonNumberPrintChunkElems);
        const uint32_t nrb = (uint32_t)((j.rows + kJsonNumberPrintChunkElems - 1) / kJsonNumberPrintChunkElems);
        const uint32_t form = j.row_ends ? np::kNested : j.brackets ? np::kBracketed : np::kBare;
        tj[k] = JsonNumberPrintJob{j.src, j.row_ends, static_cast<uint8_t*>(j.dst), j.cap, (uint32_t)j.count,
                                   (uint32_t)j.rows, j.kind, form, chunk, nc, row_block, nrb};
        tr[k] = JsonNumberPrintResult{0, np::kNone, 0};
        chunk += nc;
        row_block += nrb;
    }
    JsonNumberPrintTables t;
    t.jobs = tj;
    t.njobs = nlive;
    t.nchunks = chunk;
    t.nrow_blocks = row_block;
    t.prefix = words.as<uint32_t>();
    t.bad = words.as<uint32_t>() + nchunks + 1;
    t.digits = any_float ? digits.p : nullptr;
    t.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonNumberPrint(t, s); }) != 0) return -1;
    for (int k = 0; k < nlive; ++k) {
        jobs[live[k]].len = tr[k].len;
        jobs[live[k]].first_bad = tr[k].first_bad;
        jobs[live[k]].err = tr[k].err;
    }
    return 0;
}

namespace {

std::atomic<int64_t> g_record_print_jobs{0}, g_record_print_rows{0};

static_assert(kJsonRecordNumber == json_records::kNumber && kJsonRecordString == json_records::kString &&
                  kJsonRecordBase64 == json_records::kBase64,
              "one numbering of the text forms");

// The job as the rules see it (cols: room for kMaxColumns); false when it
// has no column table to look at.
bool record_print_view(const DeviceRecordPrintJob& j, json_records::Column* cols, json_records::Job* out) {
    if (!j.columns || j.ncols < 1 || j.ncols > json_records::kMaxColumns) return false;
    for (uint32_t c = 0; c < j.ncols; ++c) {
        const DeviceRecordPrintColumn& in = j.columns[c];
        cols[c].key = in.key;
        cols[c].key_len = in.key_len;
        cols[c].kind = in.kind;
        cols[c].text = in.text;
        cols[c].src = in.src;
        cols[c].count = in.count;
        cols[c].row_ends = in.row_ends;
    }
    out->columns = cols;
    out->ncols = j.ncols;
    out->rows = j.rows;
    out->brackets = j.brackets;
    return true;
}

// The job's key prefixes and its worst case (json_records::WorstCaseBytes);
// false for a job the rules refuse.
bool record_print_worst(const DeviceRecordPrintJob& j, std::vector<std::string>* prefixes, uint64_t* worst) {
    namespace jr = json_records;
    jr::Column cols[jr::kMaxColumns];
    jr::Job view;
    if (!record_print_view(j, cols, &view) || !jr::FieldsOk(view) || !json::RecordObjectPrefixes(view, prefixes))
        return false;
    uint64_t prefix_bytes = 0;
    for (const std::string& p : *prefixes) prefix_bytes += p.size();
    *worst = jr::WorstCaseBytes(view, prefix_bytes);
    return true;
}

// Everything the host can say about a job without reading device memory; the
// prefixes and the worst case come back for a job that passes.
bool record_print_ok(const DeviceRecordPrintJob& j, std::vector<std::string>* prefixes, uint64_t* worst) {
    namespace jr = json_records;
    if (!record_print_worst(j, prefixes, worst) || *worst > 0xFFFFFFFFull || (!j.dst && j.cap > 0)) return false;
    // a cap above the worst case can claim no more of dst than that
    const uint64_t reach = j.cap < *worst ? j.cap : *worst;
    auto overlaps = [](const void* a, uint64_t an, const void* b, uint64_t bn) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return an > 0 && bn > 0 && x < y + bn && y < x + an;
    };
    for (uint32_t c = 0; c < j.ncols; ++c) {
        const DeviceRecordPrintColumn& col = j.columns[c];
        const uint64_t eb = jr::ElemBytes(col.kind);
        if ((!col.src && col.count > 0) || ((uintptr_t)col.src & (eb - 1)) != 0 || ((uintptr_t)col.row_ends & 3) != 0 ||
            overlaps(j.dst, reach, col.src, col.count * eb) || overlaps(j.dst, reach, col.row_ends, j.rows * 4))
            return false;
    }
    return true;
}

}  // namespace

uint64_t RecordObjectsWorstCaseBytes(const DeviceRecordPrintJob& job) {
    std::vector<std::string> prefixes;
    uint64_t worst = 0;
    return record_print_worst(job, &prefixes, &worst) ? worst : 0;
}

uint32_t JsonRecordsChunkElems() { return kJsonRecordsChunkElems; }
uint32_t JsonRecordsBlockRows() { return kJsonRecordsBlockRows; }

int DevicePrintRecordObjects(DeviceRecordPrintJob* jobs, int n, int device) {
    namespace jr = json_records;
    namespace np = number_print;
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    std::vector<int> live;   // the jobs that go to the device, in order
    std::vector<int> empty;  // those of no row that get "[]"
    std::vector<std::vector<std::string>> prefixes((size_t)n);
    uint64_t nchunks = 0, nrblocks = 0, ngroups = 0, nrows = 0, ncolrows = 0, ncols = 0, nelems = 0, ndigits = 0;
    for (int i = 0; i < n; ++i) {
        DeviceRecordPrintJob& j = jobs[i];
        j.len = 0;
        j.first_bad = j.bad_column = jr::kNone;
        j.err = 0;
        uint64_t worst = 0;
        if (!record_print_ok(j, &prefixes[i], &worst)) {
            j.err = 2;
            continue;
        }
        if (j.rows == 0) {
            j.len = worst;  // 2 or 0
            if (j.len > j.cap) j.err = 3;
            else if (j.len) empty.push_back(i);
            continue;
        }
        for (uint32_t c = 0; c < j.ncols; ++c) {
            const DeviceRecordPrintColumn& col = j.columns[c];
            nchunks += (col.count + kJsonRecordsChunkElems - 1) / kJsonRecordsChunkElems;
            if (col.text != jr::kBase64) {
                ngroups += col.count / kJsonRecordsGroupElems + 1;
                nelems += col.count;
            }
            if (np::KindIsFloat(col.kind)) ndigits += col.count;
        }
        nrblocks += (j.rows + kJsonRecordsBlockRows - 1) / kJsonRecordsBlockRows;
        nrows += j.rows;
        ncolrows += j.rows * j.ncols;
        ncols += j.ncols;
        live.push_back(i);
    }
    if (live.empty() && empty.empty()) return 0;
    // one grid per pass, 32-bit table indices
    if (nchunks > 0x7FFFFFFFull || nrblocks > 0x7FFFFFFFull || ngroups > 0x7FFFFFFFull || ncolrows > 0x7FFFFFFFull ||
        nelems > 0x7FFFFFFFull) {
        return -1;
    }
    const size_t nlive = live.size();
    // the most aligned first: digits are 16-byte, jobs, columns and offender words 8-byte
    const size_t jobs_bytes = nlive * sizeof(JsonRecordsJob), cols_bytes = (size_t)ncols * sizeof(JsonRecordsColumn);
    const size_t prefix_bytes = (size_t)ncols * kJsonRecordsPrefixStride;
    PinnedBlock tables(jobs_bytes + cols_bytes + nlive * sizeof(JsonRecordsResult) + prefix_bytes + 4);
    const size_t digits_bytes = (size_t)ndigits * sizeof(shortest_double::Decimal);
    const size_t words = (size_t)ngroups + (size_t)nrows + 2 * (size_t)ncolrows + (size_t)nrblocks + nlive;
    HbmBlock scratch(digits_bytes + jobs_bytes + cols_bytes + nlive * sizeof(uint64_t) + words * sizeof(uint32_t) +
                         prefix_bytes + (size_t)nelems * sizeof(uint16_t) + 16,
                     device);
    if (!tables || !scratch) return -1;
    JsonRecordsJob* tj = tables.as<JsonRecordsJob>();
    JsonRecordsColumn* tc = reinterpret_cast<JsonRecordsColumn*>(tj + nlive);
    JsonRecordsResult* tr = reinterpret_cast<JsonRecordsResult*>(tc + ncols);
    uint8_t* tp = reinterpret_cast<uint8_t*>(tr + nlive);
    char* two = reinterpret_cast<char*>(tp + prefix_bytes);  // "[]" for the jobs of no row
    two[0] = '[';
    two[1] = ']';
    memset(tp, 0, prefix_bytes);
    JsonRecordsTables t;
    for (size_t k = 0; k < nlive; ++k) {
        const DeviceRecordPrintJob& j = jobs[live[k]];
        JsonRecordsJob& o = tj[k];
        o.dst = static_cast<uint8_t*>(j.dst);
        o.cap = j.cap;
        o.rows = (uint32_t)j.rows;
        o.brackets = j.brackets ? 1 : 0;
        o.ncols = j.ncols;
        o.first_col = (uint32_t)t.ncols;
        o.first_rblock = t.nrblocks;
        o.first_row = t.nrows;
        o.fixed = 1;  // '}'
        o.pad = 0;
        for (uint32_t c = 0; c < o.ncols; ++c) {
            const DeviceRecordPrintColumn& in = j.columns[c];
            const std::string& prefix = prefixes[live[k]][c];
            memcpy(tp + (size_t)t.ncols * kJsonRecordsPrefixStride, prefix.data(), prefix.size());
            o.fixed += (uint32_t)prefix.size();
            JsonRecordsColumn& col = tc[t.ncols++];
            col.src = in.src;
            col.row_ends = in.row_ends;
            col.count = (uint32_t)in.count;
            col.kind = in.kind;
            col.text = in.text;
            col.job = (uint32_t)k;
            col.first_chunk = t.nchunks;
            col.nchunks = (uint32_t)((in.count + kJsonRecordsChunkElems - 1) / kJsonRecordsChunkElems);
            col.first_row = t.ncolrows;
            col.first_group = t.ngroups;
            col.first_elem = t.nelems;
            col.first_digit = t.ndigits;
            col.prefix_len = (uint32_t)prefix.size();
            col.pad = 0;
            t.nchunks += col.nchunks;
            t.ncolrows += o.rows;
            if (in.text != jr::kBase64) {
                t.ngroups += col.count / kJsonRecordsGroupElems + 1;
                t.nelems += col.count;
            }
            if (np::KindIsFloat(in.kind)) t.ndigits += col.count;
        }
        t.nrblocks += (uint32_t)((j.rows + kJsonRecordsBlockRows - 1) / kJsonRecordsBlockRows);
        t.nrows += o.rows;
        tr[k] = JsonRecordsResult{0, jr::kNone, jr::kNone, 0};
    }
    t.jobs = tj;
    t.njobs = (int)nlive;
    t.cols = tc;
    t.prefixes = tp;
    t.digits = scratch.p;
    t.jobs_dev = reinterpret_cast<JsonRecordsJob*>(static_cast<char*>(scratch.p) + digits_bytes);
    t.cols_dev = reinterpret_cast<JsonRecordsColumn*>(t.jobs_dev + nlive);
    t.bad = reinterpret_cast<unsigned long long*>(t.cols_dev + t.ncols);
    t.groups = reinterpret_cast<uint32_t*>(t.bad + nlive);
    t.row_size = t.groups + t.ngroups;
    t.col_cell = t.row_size + t.nrows;
    t.col_delta = t.col_cell + t.ncolrows;
    t.block_off = t.col_delta + t.ncolrows;
    t.prefixes_dev = reinterpret_cast<uint8_t*>(t.block_off + t.nrblocks + nlive);
    t.elem_incl = reinterpret_cast<uint16_t*>(t.prefixes_dev + prefix_bytes);
    t.res = tr;
    const int rc = RunOnPoolStream(device, [&](hipStream_t s) {
        for (int i : empty) {
            if (hipMemcpyAsync(jobs[i].dst, two, 2, hipMemcpyDefault, s) != hipSuccess) return -1;
        }
        return LaunchJsonRecordsPrint(t, s);
    });
    if (rc != 0) return -1;
    for (size_t k = 0; k < nlive; ++k) {
        DeviceRecordPrintJob& j = jobs[live[k]];
        j.len = tr[k].len;
        j.err = tr[k].err;
        if (j.err == 1) {
            j.first_bad = tr[k].first_bad;
            j.bad_column = tr[k].bad_column;
        }
        if (j.err) continue;
        g_record_print_jobs.fetch_add(1, std::memory_order_relaxed);
        g_record_print_rows.fetch_add((int64_t)j.rows, std::memory_order_relaxed);
    }
    return 0;
}

int DeviceParseNumberArrays(DeviceNumberParseJob* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    // refuse what must not reach a kernel; count the blocks of the rest
    uint64_t nblocks = 0;
    std::vector<int> live;  // the jobs that go to the device, in order
    for (int i = 0; i < n; ++i) {
        DeviceNumberParseJob& j = jobs[i];
        j.n_redo = 0;
        j.first_bad = 0xFFFFFFFFu;
        j.err = 0;
        if (j.count == 0) continue;
        const size_t align = j.mode == kJsonParseFloat32 ? 4 : 8;
        if (j.mode > kJsonParseFloat32 || !j.text || !j.seps || !j.out ||
            (j.mode == kJsonParseNumbers && !j.classes) || (j.redo_cap > 0 && !j.redo) ||
            ((uintptr_t)j.out & (align - 1)) != 0 || ((uintptr_t)j.seps & 3) != 0 ||
            ((uintptr_t)j.redo & 3) != 0 || j.count > 0xFFFFFFFEull) {
            j.err = 2;
            continue;
        }
        nblocks += (j.count + 255) / 256;
        live.push_back(i);
    }
    if (live.empty()) return 0;
    if (nblocks > 0x7FFFFFFFull) return -1;  // one grid
    const int nlive = (int)live.size();
    PinnedBlock tables(live.size() * (sizeof(JsonNumberJob) + sizeof(JsonNumberResult)));
    HbmBlock counters(live.size() * sizeof(JsonNumberResult), device);
    if (!tables || !counters) return -1;
    JsonNumberJob* tj = tables.as<JsonNumberJob>();
    JsonNumberResult* tr = reinterpret_cast<JsonNumberResult*>(tj + nlive);
    uint32_t block = 0;
    for (int k = 0; k < nlive; ++k) {
        const DeviceNumberParseJob& j = jobs[live[k]];
        tj[k] = JsonNumberJob{j.text, j.seps, j.out, j.classes, j.redo, (uint32_t)j.count, j.mode, j.redo_cap, block};
        tr[k] = JsonNumberResult{0xFFFFFFFFu, 0};
        block += (uint32_t)((j.count + 255) / 256);
    }
    const int rc = RunOnPoolStream(device, [&](hipStream_t s) {
        return LaunchJsonNumberArrays(tj, nlive, block, counters.as<JsonNumberResult>(), tr, s);
    });
    if (rc != 0) return -1;
    for (int k = 0; k < nlive; ++k) {
        DeviceNumberParseJob& j = jobs[live[k]];
        j.first_bad = tr[k].bad;
        j.n_redo = tr[k].n_redo;
        if (j.first_bad != 0xFFFFFFFFu) j.err = 1;
        else if (j.n_redo > j.redo_cap) j.err = 3;
    }
    return 0;
}

uint32_t JsonTextChunkBytes() { return kJsonTextChunkBytes; }

int DeviceParseNumberText(DeviceNumberTextJob* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    // refuse what must not reach a kernel; count the chunks of the rest
    uint64_t nchunks = 0;
    std::vector<int> live;  // the jobs that go to the device, in order
    for (int i = 0; i < n; ++i) {
        DeviceNumberTextJob& j = jobs[i];
        j.depth = 0;
        j.count = j.rows = 0;
        j.n_redo = 0;
        j.first_bad = 0xFFFFFFFFu;
        j.err = 0;
        const size_t align = j.mode == kJsonParseFloat32 ? 4 : 8;
        if (j.mode > kJsonParseFloat32 || (!j.text && j.n > 0) || (!j.out && j.cap > 0) ||
            (j.mode == kJsonParseNumbers && !j.classes && j.cap > 0) || (j.redo_cap > 0 && !j.redo) ||
            (j.row_cap > 0 && !j.row_ends) || ((uintptr_t)j.out & (align - 1)) != 0 ||
            ((uintptr_t)j.row_ends & 3) != 0 || ((uintptr_t)j.redo & 3) != 0 || j.n > 0xFFFFFFFEull) {
            j.err = 2;
            continue;
        }
        if (j.n == 0) continue;
        nchunks += (j.n + kJsonTextChunkBytes - 1) / kJsonTextChunkBytes;
        live.push_back(i);
    }
    if (live.empty()) return 0;
    if (nchunks > 0x3FFFFFFFull) return -1;  // one grid, and 2 * nchunks + 2 table entries
    const int nlive = (int)live.size();
    const size_t prefix_bytes = (2 * (size_t)nchunks + 2) * sizeof(uint32_t);
    PinnedBlock tables(live.size() * (sizeof(JsonTextJob) + sizeof(JsonTextResult)));
    const size_t jobs_bytes = live.size() * sizeof(JsonTextJob);  // first: the most aligned
    HbmBlock scratch(jobs_bytes + prefix_bytes + live.size() * (kJsonTextStateBytes + sizeof(uint32_t)), device);
    if (!tables || !scratch) return -1;
    JsonTextJob* tj = tables.as<JsonTextJob>();
    JsonTextResult* tr = reinterpret_cast<JsonTextResult*>(tj + nlive);
    uint32_t chunk = 0;
    for (int k = 0; k < nlive; ++k) {
        const DeviceNumberTextJob& j = jobs[live[k]];
        const uint32_t nc = (uint32_t)((j.n + kJsonTextChunkBytes - 1) / kJsonTextChunkBytes);
        auto clamp = [](uint64_t v) { return (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull); };
        tj[k] = JsonTextJob{j.text,      j.out,        j.classes,        j.row_ends, j.redo, (uint32_t)j.n, j.mode,
                            clamp(j.cap), clamp(j.row_cap), j.redo_cap, chunk,      nc};
        tr[k] = JsonTextResult{0xFFFFFFFFu, 0, 0, 0, 0, 0};
        chunk += nc;
    }
    JsonTextTables t;
    t.jobs = tj;
    t.njobs = nlive;
    t.nchunks = chunk;
    t.jobs_dev = scratch.as<JsonTextJob>();
    t.prefix = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch.p) + jobs_bytes);
    t.state = static_cast<char*>(scratch.p) + jobs_bytes + prefix_bytes;
    t.n_redo = reinterpret_cast<uint32_t*>(static_cast<char*>(t.state) + live.size() * kJsonTextStateBytes);
    t.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonNumberText(t, s); }) != 0) return -1;
    for (int k = 0; k < nlive; ++k) {
        DeviceNumberTextJob& j = jobs[live[k]];
        j.depth = tr[k].depth;
        j.count = tr[k].count;
        j.rows = tr[k].rows;
        j.n_redo = tr[k].n_redo;
        j.first_bad = tr[k].first_bad;
        if (j.first_bad != 0xFFFFFFFFu) j.err = 1;
        else if (j.count > j.cap || j.rows > j.row_cap) j.err = 5;
        else if (j.n_redo > j.redo_cap) j.err = 3;
    }
    return 0;
}

namespace {
// elements of one array the device may hand back for exact arithmetic before
// the whole array goes to the host (they are rare: a 20-digit number whose
// 19-digit truncation straddles a rounding boundary)
constexpr uint32_t kRedoCap = 64;
}  // namespace

bool ParseNumbersOnDevice(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload, uint8_t* classes,
                          int device, uint32_t* n_redo) {
    if (n_redo) *n_redo = 0;
    if (device < 0 || nseps < 2 || !base || !seps || !payload || !classes) return false;
    const size_t n = nseps - 1;
    if (n > 0xFFFFFFFEull) return false;
    // the text from the byte after the first separator up to the last one
    const uint32_t lo = seps[0] + 1, hi = seps[nseps - 1];
    if (hi < lo) return false;
    const size_t vals_bytes = n * sizeof(uint64_t);
    PinnedBlock text((size_t)(hi - lo) + 1), sep(nseps * sizeof(uint32_t)),
        vals(vals_bytes + kRedoCap * sizeof(uint32_t) + n);
    if (!text || !sep || !vals) return false;
    memcpy(text.p, base + lo, hi - lo);
    uint32_t* sp = sep.as<uint32_t>();
    for (size_t i = 0; i < nseps; ++i) sp[i] = seps[i] - lo;  // the first becomes 0xFFFFFFFF
    DeviceNumberParseJob job;
    job.text = text.p;
    job.seps = sp;
    job.count = n;
    job.mode = kJsonParseNumbers;
    job.out = vals.p;
    job.redo = reinterpret_cast<uint32_t*>(vals.p + vals_bytes);
    job.redo_cap = kRedoCap;
    job.classes = reinterpret_cast<uint8_t*>(job.redo + kRedoCap);
    if (DeviceParseNumberArrays(&job, 1, device) != 0 || job.err != 0) return false;
    memcpy(payload, vals.p, vals_bytes);
    memcpy(classes, job.classes, n);
    for (uint32_t r = 0; r < job.n_redo; ++r) {
        const uint32_t i = job.redo[r];
        if (i >= n) return false;
        const char* b = base + (uint32_t)(seps[i] + 1);
        const char* e = base + seps[i + 1];
        while (b < e && (*b == ' ' || *b == '\t' || *b == '\n' || *b == '\r')) ++b;
        while (e > b && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\n' || e[-1] == '\r')) --e;
        if (!json::ParseNumberExact(b, e, &payload[i], &classes[i])) return false;
    }
    if (n_redo) *n_redo = job.n_redo;
    return true;
}

namespace {

std::atomic<int64_t> g_arrays{0}, g_array_elems{0}, g_array_failures{0};
std::atomic<int64_t> g_float_arrays{0}, g_float_elems{0};

// pb2json number arrays: pb_run_encode_kernel prints the
// field's values in the codec batch (gpu/snappy_offload.h
// EncodeRunOnDevice), the host only sizes them and wraps the brackets.
bool array_offload(const void* values, size_t n, uint32_t kind, std::string* text) {
    const int dev = g_device;
    if (dev < 0) return false;
    if (kind == kJsonFloat32 || kind == kJsonFloat64) {
        const int min_elems = FLAGS_gpu_pb2json_float_min_elems;
        if (min_elems <= 0 || n < (size_t)min_elems) return false;  // the host printer takes it
        if (PrintFloatsOnDevice(values, n, kind, text, dev) != 0) {
            g_array_failures.fetch_add(1, std::memory_order_relaxed);
            return false;
        }
        g_float_arrays.fetch_add(1, std::memory_order_relaxed);
        g_float_elems.fetch_add((int64_t)n, std::memory_order_relaxed);
        return true;
    }
    if (EncodeRunOnDevice(values, n, kind, PB_RUN_DECIMAL, text, dev) != 0) {
        g_array_failures.fetch_add(1, std::memory_order_relaxed);
        return false;
    }
    g_arrays.fetch_add(1, std::memory_order_relaxed);
    g_array_elems.fetch_add((int64_t)n, std::memory_order_relaxed);
    return true;
}

std::atomic<int64_t> g_int_arrays{0}, g_int_array_fallbacks{0};

// json2pb integer arrays (SURVEY K6 parse half): the array's text and its
// separators go to pinned memory, json_int_array_kernel parses one element
// per lane, one fiber-friendly wait.
bool int_array_offload(const char* base, const uint32_t* seps, size_t nseps, std::vector<int64_t>* out) {
    const int dev = g_device;
    if (dev < 0 || nseps < 2) return false;
    const uint32_t lo = seps[0], hi = seps[nseps - 1];
    const size_t n = nseps - 1;
    PinnedBlock text(hi - lo + 1), sep(nseps * sizeof(uint32_t)), vals(n * sizeof(int64_t) + 64);
    if (!text || !sep || !vals) return false;
    memcpy(text.p, base + lo, hi - lo + 1);
    uint32_t* sp = sep.as<uint32_t>();
    for (size_t i = 0; i < nseps; ++i) sp[i] = seps[i] - lo;
    int32_t* bad = reinterpret_cast<int32_t*>(vals.as<int64_t>() + n);
    *bad = 0;
    const int rc = RunOnPoolStream(dev, [&](hipStream_t s) {
        return LaunchJsonIntArray(text.p, sp, (uint32_t)n, vals.as<int64_t>(), bad, s);
    });
    if (rc != 0 || *bad != 0) {
        g_int_array_fallbacks.fetch_add(1, std::memory_order_relaxed);
        return false;
    }
    out->assign(vals.as<int64_t>(), vals.as<int64_t>() + n);
    g_int_arrays.fetch_add(1, std::memory_order_relaxed);
    return true;
}

std::atomic<int64_t> g_number_arrays{0}, g_number_elems{0}, g_number_array_fallbacks{0}, g_number_redo_elems{0};

// json2pb number arrays that are not all int64 (json::SetNumberArrayOffload).
// The reader's own threshold is 1: the reloadable flag decides here.
bool number_array_offload(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload,
                          uint8_t* classes) {
    const int dev = g_device;
    const int min_elems = FLAGS_gpu_json2pb_float_min_elems;
    if (dev < 0 || nseps < 2 || min_elems <= 0 || nseps - 1 < (size_t)min_elems) return false;
    uint32_t redone = 0;
    if (!ParseNumbersOnDevice(base, seps, nseps, payload, classes, dev, &redone)) {
        g_number_array_fallbacks.fetch_add(1, std::memory_order_relaxed);
        return false;
    }
    g_number_arrays.fetch_add(1, std::memory_order_relaxed);
    g_number_elems.fetch_add((int64_t)(nseps - 1), std::memory_order_relaxed);
    g_number_redo_elems.fetch_add((int64_t)redone, std::memory_order_relaxed);
    return true;
}

}  // namespace

int EnableGpuJsonIndex(int device, size_t min_bytes, std::string* error) {
    if (Init(device, error) != 0 || InitHbmPool(device, error) != 0) return -1;
    g_device = device;
    json2pb::SetJsonIndexOffload(offload, min_bytes);
    json2pb::SetPb2JsonArrayOffload(array_offload, (size_t)std::max(1, FLAGS_gpu_pb2json_min_elems));
    json::SetIntArrayOffload(int_array_offload, (size_t)std::max(1, FLAGS_gpu_pb2json_min_elems));
    json::SetNumberArrayOffload(number_array_offload, 1);
    static var::PassiveStatus<int64_t> v8("gpu_json_number_arrays", [] { return g_number_arrays.load(); });
    static var::PassiveStatus<int64_t> v9("gpu_json_number_elems", [] { return g_number_elems.load(); });
    static var::PassiveStatus<int64_t> v10("gpu_json_number_array_fallbacks",
                                           [] { return g_number_array_fallbacks.load(); });
    static var::PassiveStatus<int64_t> v11("gpu_json_number_redo_elems", [] { return g_number_redo_elems.load(); });
    static var::PassiveStatus<int64_t> v5("gpu_json_int_arrays", [] { return g_int_arrays.load(); });
    static var::PassiveStatus<int64_t> v4("gpu_pb2json_arrays", [] { return g_arrays.load(); });
    static var::PassiveStatus<int64_t> v6("gpu_pb2json_float_arrays", [] { return g_float_arrays.load(); });
    static var::PassiveStatus<int64_t> v7("gpu_pb2json_float_elems", [] { return g_float_elems.load(); });
    static var::PassiveStatus<int64_t> v1("gpu_json_indexed_bodies", [] { return g_bodies.load(); });
    static var::PassiveStatus<int64_t> v2("gpu_json_indexed_bytes", [] { return g_bytes.load(); });
    static var::PassiveStatus<int64_t> v3("gpu_json_index_failures", [] { return g_failures.load(); });
    return 0;
}

void DisableGpuJsonIndex() {
    json2pb::SetJsonIndexOffload(nullptr, (size_t)-1);
    json2pb::SetPb2JsonArrayOffload(nullptr, (size_t)-1);
    json::SetIntArrayOffload(nullptr, (size_t)-1);
    json::SetNumberArrayOffload(nullptr, (size_t)-1);
}

GpuJsonStats GetGpuJsonStats() {
    GpuJsonStats s;
    s.indexed_bodies = g_bodies.load();
    s.indexed_bytes = g_bytes.load();
    s.failures = g_failures.load();
    s.pb2json_arrays = g_arrays.load();
    s.pb2json_elems = g_array_elems.load();
    s.pb2json_failures = g_array_failures.load();
    s.pb2json_float_arrays = g_float_arrays.load();
    s.pb2json_float_elems = g_float_elems.load();
    s.int_arrays = g_int_arrays.load();
    s.int_array_fallbacks = g_int_array_fallbacks.load();
    s.sparse_skips = g_sparse.load();
    s.number_arrays = g_number_arrays.load();
    s.number_elems = g_number_elems.load();
    s.number_array_fallbacks = g_number_array_fallbacks.load();
    s.number_redo_elems = g_number_redo_elems.load();
    s.record_print_jobs = g_record_print_jobs.load();
    s.record_print_rows = g_record_print_rows.load();
    return s;
}

}  // namespace gpu
}  // namespace mrpc
