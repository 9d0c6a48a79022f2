#include "gpu/base64_offload.h"

#include <hip/hip_runtime_api.h>

#include <vector>

#include "base/base64.h"
#include "gpu/kernels.h"
#include "gpu/scoped.h"

namespace mrpc {
namespace gpu {

namespace {

// Refuses what must not reach a kernel and fills the job table of the rest:
// the shared front of both directions. `out_bytes` is the size dst must hold,
// `chunk` the source bytes one workgroup takes.
struct Base64Tables {
    std::vector<int> live;  // the jobs that go to the device, in order
    PinnedBlock tables;     // Base64Job[nlive], then JsonNumberResult[nlive]
    uint32_t nblocks = 0;
    Base64Job* jobs() const { return tables.as<Base64Job>(); }
    JsonNumberResult* results() const { return reinterpret_cast<JsonNumberResult*>(jobs() + live.size()); }
};

// 0: tables ready (maybe with nothing live), -1: too many blocks or no memory
int base64_prepare(DeviceBase64Job* jobs, int n, uint64_t (*out_bytes)(uint64_t), uint32_t chunk, uint64_t max_n,
                   Base64Tables* t) {
    uint64_t nblocks = 0;
    for (int i = 0; i < n; ++i) {
        DeviceBase64Job& j = jobs[i];
        j.len = 0;
        j.first_odd = 0;
        j.err = 0;
        if (j.n == 0) continue;
        const uint64_t need = out_bytes(j.n);
        const uintptr_t s = (uintptr_t)j.src, d = (uintptr_t)j.dst;
        if (!j.src || !j.dst || j.n > max_n || need > 0xFFFFFFFFull || (s < d + need && d < s + j.n)) {
            j.err = 2;
            continue;
        }
        if (j.cap < need) {
            j.err = 3;
            j.len = need;
            continue;
        }
        nblocks += (j.n + chunk - 1) / chunk;
        t->live.push_back(i);
    }
    if (t->live.empty()) return 0;
    if (nblocks > 0x7FFFFFFFull) return -1;  // one grid
    t->tables = PinnedBlock(t->live.size() * (sizeof(Base64Job) + sizeof(JsonNumberResult)));
    if (!t->tables) return -1;
    uint32_t block = 0;
    for (size_t k = 0; k < t->live.size(); ++k) {
        const DeviceBase64Job& j = jobs[t->live[k]];
        t->jobs()[k] = Base64Job{static_cast<const uint8_t*>(j.src), static_cast<uint8_t*>(j.dst), (uint32_t)j.n, block};
        t->results()[k] = JsonNumberResult{0xFFFFFFFFu, 0};
        block += (uint32_t)((j.n + chunk - 1) / chunk);
    }
    t->nblocks = block;
    return 0;
}

uint64_t encoded_bytes(uint64_t n) { return base64::Base64EncodedBytes(n); }
uint64_t decoded_max_bytes(uint64_t n) { return base64::Base64DecodedMaxBytes(n); }

}  // namespace

int DeviceBase64Encode(DeviceBase64Job* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    Base64Tables t;
    if (base64_prepare(jobs, njobs, encoded_bytes, kBase64ChunkBytes, 0xFFFFFFFFull, &t) != 0) return -1;
    if (t.live.empty()) return 0;
    const int nlive = (int)t.live.size();
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchBase64Encode(t.jobs(), nlive, t.nblocks, s); }) != 0)
        return -1;
    for (int i : t.live) jobs[i].len = base64::Base64EncodedBytes(jobs[i].n);
    return 0;
}

int DeviceBase64Decode(DeviceBase64Job* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    Base64Tables t;
    // 2^32 - 1 is the result word's "nothing odd": a text of that size could not report its length rule
    if (base64_prepare(jobs, njobs, decoded_max_bytes, kBase64ChunkSymbols, 0xFFFFFFFEull, &t) != 0) return -1;
    if (t.live.empty()) return 0;
    const int nlive = (int)t.live.size();
    HbmBlock counters(t.live.size() * sizeof(JsonNumberResult), device);
    if (!counters) return -1;
    const int rc = RunOnPoolStream(device, [&](hipStream_t s) {
        return LaunchBase64Decode(t.jobs(), nlive, t.nblocks, counters.as<JsonNumberResult>(), t.results(), s);
    });
    if (rc != 0) return -1;
    for (int k = 0; k < nlive; ++k) {
        DeviceBase64Job& j = jobs[t.live[k]];
        const JsonNumberResult& r = t.results()[k];
        j.len = r.n_redo;
        if (r.bad != 0xFFFFFFFFu) {
            j.err = 1;
            j.first_odd = r.bad;
        }
    }
    return 0;
}

namespace {

constexpr uint64_t kRowsMaxBytes = 0xFFFFFFFEull;  // 2^32 - 1 is the result word's "nothing bad"

bool overlap(const void* a, uint64_t n, const void* b, uint64_t m) {
    const uintptr_t s = (uintptr_t)a, d = (uintptr_t)b;
    return n != 0 && m != 0 && s < d + m && d < s + n;
}

// The live jobs of a rows call, their table and result words in pinned memory
// and their scratch in one block of the arena.
struct RowsTables {
    std::vector<int> live;
    std::vector<Base64RowsJob> table;
    PinnedBlock pinned;  // Base64RowsJob[nlive], then Base64RowsResult[nlive]
    HbmBlock scratch;
    Base64RowsTables t;
    uint64_t chunks64 = 0, rblocks64 = 0, rows64 = 0;

    void add(int index, Base64RowsJob j, uint32_t chunk, bool encode) {
        live.push_back(index);
        j.nchunks = (uint32_t)(((uint64_t)j.n + chunk - 1) / chunk);
        j.first_chunk = (uint32_t)chunks64;
        j.first_rblock = (uint32_t)rblocks64;
        j.first_row = (uint32_t)rows64;
        chunks64 += j.nchunks;
        if (encode) {
            rblocks64 += ((uint64_t)j.rows + kBase64RowsBlockRows - 1) / kBase64RowsBlockRows;
            rows64 += j.rows;
        }
        table.push_back(j);
    }

    // 0: ready, -1: too many blocks for one grid or no memory
    int finish(int device, bool encode) {
        if (chunks64 > 0x3FFFFFFFull || rblocks64 > 0x7FFFFFFEull || rows64 > 0xFFFFFFFFull) return -1;
        const size_t nlive = live.size();
        pinned = PinnedBlock(nlive * (sizeof(Base64RowsJob) + sizeof(Base64RowsResult)));
        if (!pinned) return -1;
        Base64RowsJob* jobs = pinned.as<Base64RowsJob>();
        Base64RowsResult* res = reinterpret_cast<Base64RowsResult*>(jobs + nlive);
        for (size_t k = 0; k < nlive; ++k) {
            jobs[k] = table[k];
            res[k] = Base64RowsResult{0, 0, 0, 0, 0};
        }
        t.nchunks = (uint32_t)chunks64;
        t.nrblocks = (uint32_t)rblocks64;
        t.nrows = (uint32_t)rows64;
        // 16-byte aligned pieces, the job table first
        auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t jobs_b = round16(nlive * sizeof(Base64RowsJob));
        const size_t prefix_b = round16(encode ? ((size_t)t.nrblocks + 1) * 4 : 2 * ((size_t)t.nchunks + 1) * 4);
        const size_t rows_b = encode ? round16((size_t)t.nrows * 4) : 0;
        const size_t info_b = encode ? 0 : round16((size_t)t.nchunks * kBase64RowsInfoWords * 4);
        const size_t bad_b = round16(nlive * 4), ok_b = round16(nlive * 4);
        const size_t state_b = encode ? 0 : round16(nlive * kBase64RowsStateWords * 4);
        scratch = HbmBlock(jobs_b + prefix_b + 2 * rows_b + info_b + bad_b + ok_b + state_b, device);
        if (!scratch) return -1;
        char* p = scratch.as<char>();
        t.jobs = jobs;
        t.njobs = (int)nlive;
        t.res = res;
        t.jobs_dev = reinterpret_cast<Base64RowsJob*>(p);
        p += jobs_b;
        t.prefix = reinterpret_cast<uint32_t*>(p);
        p += prefix_b;
        t.ends = rows_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += rows_b;
        t.rowoff = rows_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += rows_b;
        t.info = info_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += info_b;
        t.bad = reinterpret_cast<uint32_t*>(p);
        p += bad_b;
        t.ok = reinterpret_cast<int32_t*>(p);
        p += ok_b;
        t.state = state_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        return 0;
    }
};

}  // namespace

int DeviceBase64EncodeRows(DeviceBase64RowsEncodeJob* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    RowsTables rt;
    for (int i = 0; i < njobs; ++i) {
        DeviceBase64RowsEncodeJob& j = jobs[i];
        j.len = 0;
        j.first_bad = 0;
        j.err = 0;
        if (j.rows == 0) {
            if (j.n != 0) {  // bytes in no rows
                j.err = 2;
                continue;
            }
            if (!j.brackets) continue;  // nothing to write
        }
        const uint64_t worst = Base64RowsWorstCaseBytes(j.n, j.rows, j.brackets);
        // a cap above the worst case can claim no more of dst than that
        const uint64_t reach = j.cap < worst ? j.cap : worst;
        if ((j.n != 0 && !j.src) || !j.dst || (j.rows != 0 && !j.row_ends) || j.n > kRowsMaxBytes ||
            j.rows > 0xFFFFFFFFull || worst > 0xFFFFFFFFull || ((uintptr_t)j.row_ends & 3) ||
            overlap(j.src, j.n, j.dst, reach) || overlap(j.row_ends, 4 * j.rows, j.dst, reach)) {
            j.err = 2;
            continue;
        }
        Base64RowsJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.dst = static_cast<uint8_t*>(j.dst);
        job.row_ends = static_cast<const uint32_t*>(j.row_ends);
        job.cap = j.cap;
        job.n = (uint32_t)j.n;
        job.rows = (uint32_t)j.rows;
        job.brackets = j.brackets ? 1 : 0;
        rt.add(i, job, kBase64RowsEncodeChunkBytes, true);
    }
    if (rt.live.empty()) return 0;
    if (rt.finish(device, true) != 0) return -1;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchBase64EncodeRows(rt.t, s); }) != 0) return -1;
    for (size_t k = 0; k < rt.live.size(); ++k) {
        DeviceBase64RowsEncodeJob& j = jobs[rt.live[k]];
        const Base64RowsResult& r = rt.t.res[k];
        j.len = r.len;
        j.first_bad = r.first_bad;
        j.err = r.err;
    }
    return 0;
}

int DeviceBase64DecodeRows(DeviceBase64RowsDecodeJob* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    RowsTables rt;
    for (int i = 0; i < njobs; ++i) {
        DeviceBase64RowsDecodeJob& j = jobs[i];
        j.len = j.rows = j.first_bad = 0;
        j.depth = 0;
        j.err = 0;
        if (j.n == 0) continue;
        // a capacity above the worst case can claim no more of its buffer than that
        const uint64_t worst_bytes = Base64RowsMaxBytes(j.n), worst_rows = Base64RowsMaxRows(j.n);
        const uint64_t reach = j.cap < worst_bytes ? j.cap : worst_bytes;
        const uint64_t row_reach = j.row_cap < worst_rows ? j.row_cap : worst_rows;
        if (!j.src || j.n > kRowsMaxBytes || (!j.dst && j.cap != 0) || (!j.row_ends && j.row_cap != 0) ||
            ((uintptr_t)j.row_ends & 3) || overlap(j.src, j.n, j.dst, reach) ||
            overlap(j.src, j.n, j.row_ends, 4 * row_reach) || overlap(j.dst, reach, j.row_ends, 4 * row_reach)) {
            j.err = 2;
            continue;
        }
        Base64RowsJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.dst = static_cast<uint8_t*>(j.dst);
        job.row_ends = static_cast<const uint32_t*>(j.row_ends);  // written by the place pass
        job.cap = reach;
        job.n = (uint32_t)j.n;
        job.rows = (uint32_t)row_reach;  // row_cap
        rt.add(i, job, kBase64RowsDecodeChunkBytes, false);
    }
    if (rt.live.empty()) return 0;
    if (rt.finish(device, false) != 0) return -1;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchBase64DecodeRows(rt.t, s); }) != 0) return -1;
    for (size_t k = 0; k < rt.live.size(); ++k) {
        DeviceBase64RowsDecodeJob& j = jobs[rt.live[k]];
        const Base64RowsResult& r = rt.t.res[k];
        j.len = r.len;
        j.rows = r.rows;
        j.first_bad = r.first_bad;
        j.depth = r.depth;
        j.err = r.err;
    }
    return 0;
}

}  // namespace gpu
}  // namespace mrpc
