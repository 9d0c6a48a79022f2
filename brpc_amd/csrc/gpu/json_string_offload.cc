#include "gpu/json_string_offload.h"

#include <hip/hip_runtime_api.h>

#include <vector>

#include "gpu/scoped.h"

namespace mrpc {
namespace gpu {

namespace {

constexpr uint64_t kMaxBytes = 0xFFFFFFFEull;  // 2^32 - 1 is the result word's "nothing bad"

// The live jobs of a call, their table and result words in pinned memory and
// their scratch in one block of the arena.
struct StringTables {
    std::vector<int> live;
    std::vector<JsonStringJob> table;
    PinnedBlock pinned;  // JsonStringJob[nlive], then JsonStringResult[nlive] (rows: JsonStringRowsResult[nlive])
    HbmBlock scratch;
    JsonStringTables t;

    // row_tables false: row_ends is an output and rows a capacity, no row blocks or groups
    void add(int index, const JsonStringJob& job, bool row_tables = true) {
        live.push_back(index);
        JsonStringJob j = job;
        j.nchunks = (j.n + kJsonStringChunkBytes - 1) / kJsonStringChunkBytes;
        j.first_chunk = t.nchunks;
        j.first_rblock = t.nrblocks;
        j.first_group = t.ngroups;
        chunks64 += j.nchunks;
        rblocks64 += j.row_ends && row_tables ? ((uint64_t)j.rows + kJsonStringBlockRows - 1) / kJsonStringBlockRows : 0;
        t.nchunks = (uint32_t)chunks64;
        t.nrblocks = (uint32_t)rblocks64;
        if (j.row_ends && row_tables) t.ngroups += j.nchunks * (kJsonStringChunkBytes / kJsonStringGroupBytes);
        table.push_back(j);
    }
    uint64_t chunks64 = 0, rblocks64 = 0;

    // prefix_tables size tables of nchunks + 1 entries, info_words per chunk; rows: the result words and the
    // per-job state of the unescape-rows passes. 0: ready, -1: too many blocks for one grid or no memory
    int finish(int device, int prefix_tables, uint32_t info_words, bool rows = false) {
        if (chunks64 > 0x7FFFFFFFull || rblocks64 > 0x7FFFFFFFull) return -1;
        if ((uint64_t)prefix_tables * (chunks64 + 1) > 0x7FFFFFFFull) return -1;  // one prefix scan over all tables
        const size_t nlive = live.size();
        static_assert(sizeof(JsonStringRowsResult) >= sizeof(JsonStringResult), "one block holds either");
        pinned = PinnedBlock(nlive * (sizeof(JsonStringJob) + sizeof(JsonStringRowsResult)));
        if (!pinned) return -1;
        JsonStringJob* jobs = pinned.as<JsonStringJob>();
        JsonStringResult* res = reinterpret_cast<JsonStringResult*>(jobs + nlive);
        JsonStringRowsResult* rows_res = reinterpret_cast<JsonStringRowsResult*>(jobs + nlive);
        for (size_t k = 0; k < nlive; ++k) {
            jobs[k] = table[k];
            if (rows) rows_res[k] = JsonStringRowsResult{0, 0, 0, 0, 0};
            else res[k] = JsonStringResult{0, 0, 0};
        }
        // 16-byte aligned pieces, the job table first
        auto round16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t jobs_b = round16(nlive * sizeof(JsonStringJob));
        const size_t prefix_b = round16((size_t)prefix_tables * ((size_t)t.nchunks + 1) * 4);
        const size_t groups_b = round16((size_t)t.ngroups * 4);
        const size_t info_b = round16((size_t)t.nchunks * info_words * 4);
        const size_t bad_b = round16(nlive * 4), ok_b = round16(nlive * 4);
        const size_t state_b = rows ? round16(nlive * kJsonStringRowsStateWords * 4) : 0;
        scratch = HbmBlock(jobs_b + prefix_b + groups_b + info_b + bad_b + ok_b + state_b, device);
        if (!scratch) return -1;
        char* p = scratch.as<char>();
        t.jobs = jobs;
        t.njobs = (int)nlive;
        t.res = rows ? nullptr : res;
        t.rows_res = rows ? rows_res : nullptr;
        t.jobs_dev = reinterpret_cast<JsonStringJob*>(p);
        p += jobs_b;
        t.prefix = prefix_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += prefix_b;
        t.groups = groups_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += groups_b;
        t.info = info_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        p += info_b;
        t.bad = reinterpret_cast<uint32_t*>(p);
        p += bad_b;
        t.ok = reinterpret_cast<int32_t*>(p);
        p += ok_b;
        t.state = state_b ? reinterpret_cast<uint32_t*>(p) : nullptr;
        return 0;
    }
    const JsonStringResult& result(size_t k) const { return t.res[k]; }
};

bool overlap(const void* src, uint64_t n, const void* dst, uint64_t m) {
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    return s < d + m && d < s + n;
}

}  // namespace

int DeviceEscapeJsonStrings(DeviceJsonEscapeJob* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    StringTables st;
    for (int i = 0; i < njobs; ++i) {
        DeviceJsonEscapeJob& j = jobs[i];
        j.len = 0;
        j.first_bad = 0;
        j.err = 0;
        const bool rows = j.row_ends != nullptr;
        if ((j.rows != 0) != rows) {
            if (!rows || j.n != 0) j.err = 2;  // no bytes in no rows: nothing to write
            continue;
        }
        if (j.n == 0 && !rows && !j.quote) continue;
        const uint64_t worst = JsonEscapeWorstCaseBytes(j.n, j.rows);
        // a cap above the worst case can claim no more of dst than that
        const uint64_t reach = j.cap < worst ? j.cap : worst;
        if ((j.n != 0 && !j.src) || !j.dst || j.n > kMaxBytes || j.rows > 0xFFFFFFFFull || worst > 0xFFFFFFFFull ||
            ((uintptr_t)j.row_ends & 3) || (j.n != 0 && overlap(j.src, j.n, j.dst, reach))) {
            j.err = 2;
            continue;
        }
        JsonStringJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.dst = static_cast<uint8_t*>(j.dst);
        job.row_ends = static_cast<const uint32_t*>(j.row_ends);
        job.cap = j.cap;
        job.n = (uint32_t)j.n;
        job.rows = (uint32_t)j.rows;
        job.quote = j.quote ? 1 : 0;
        st.add(i, job);
    }
    if (st.live.empty()) return 0;
    if (st.finish(device, 1, 0) != 0) return -1;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonStringEscape(st.t, s); }) != 0) return -1;
    for (size_t k = 0; k < st.live.size(); ++k) {
        DeviceJsonEscapeJob& j = jobs[st.live[k]];
        const JsonStringResult& r = st.result(k);
        j.len = r.len;
        j.first_bad = r.first_bad;
        j.err = r.err;
    }
    return 0;
}

int DeviceUnescapeJsonStrings(DeviceJsonUnescapeJob* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    StringTables st;
    for (int i = 0; i < njobs; ++i) {
        DeviceJsonUnescapeJob& j = jobs[i];
        j.len = 0;
        j.first_bad = 0;
        j.err = 0;
        if (j.n == 0) continue;
        if (!j.src || j.n > kMaxBytes || (j.dst && overlap(j.src, j.n, j.dst, j.n))) {
            j.err = 2;
            continue;
        }
        if (j.cap < j.n) {
            j.err = 3;
            j.len = j.n;
            continue;
        }
        if (!j.dst) {
            j.err = 2;
            continue;
        }
        JsonStringJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.dst = static_cast<uint8_t*>(j.dst);
        job.cap = j.cap;
        job.n = (uint32_t)j.n;
        st.add(i, job);
    }
    if (st.live.empty()) return 0;
    if (st.finish(device, 1, kJsonStringInfoWords) != 0) return -1;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonStringUnescape(st.t, s); }) != 0) return -1;
    for (size_t k = 0; k < st.live.size(); ++k) {
        DeviceJsonUnescapeJob& j = jobs[st.live[k]];
        const JsonStringResult& r = st.result(k);
        j.len = r.len;
        j.first_bad = r.first_bad;
        j.err = r.err;
    }
    return 0;
}

int DeviceUnescapeJsonStringRows(DeviceJsonStringRowsJob* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    StringTables st;
    for (int i = 0; i < njobs; ++i) {
        DeviceJsonStringRowsJob& j = jobs[i];
        j.len = j.rows = j.first_bad = 0;
        j.depth = 0;
        j.err = 0;
        if (j.n == 0) continue;
        // a capacity above the worst case can claim no more of its buffer than that
        const uint64_t worst_bytes = JsonStringRowsMaxBytes(j.n), worst_rows = JsonStringRowsMaxRows(j.n);
        const uint64_t reach = j.cap < worst_bytes ? j.cap : worst_bytes;
        const uint64_t row_reach = j.row_cap < worst_rows ? j.row_cap : worst_rows;
        if (!j.src || j.n > kMaxBytes || (!j.dst && j.cap != 0) || (!j.row_ends && j.row_cap != 0) ||
            ((uintptr_t)j.row_ends & 3) || (reach && overlap(j.src, j.n, j.dst, reach)) ||
            (row_reach && overlap(j.src, j.n, j.row_ends, 4 * row_reach)) ||
            (reach && row_reach && overlap(j.dst, reach, j.row_ends, 4 * row_reach))) {
            j.err = 2;
            continue;
        }
        JsonStringJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.dst = static_cast<uint8_t*>(j.dst);
        job.row_ends = static_cast<const uint32_t*>(j.row_ends);  // written by the place pass
        job.cap = j.cap;
        job.n = (uint32_t)j.n;
        job.rows = (uint32_t)row_reach;  // row_cap
        st.add(i, job, false);
    }
    if (st.live.empty()) return 0;
    if (st.finish(device, 2, kJsonStringRowsInfoWords, true) != 0) return -1;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonStringUnescapeRows(st.t, s); }) != 0) return -1;
    for (size_t k = 0; k < st.live.size(); ++k) {
        DeviceJsonStringRowsJob& j = jobs[st.live[k]];
        const JsonStringRowsResult& r = st.t.rows_res[k];
        j.len = r.len;
        j.rows = r.rows;
        j.first_bad = r.first_bad;
        j.depth = r.depth;
        j.err = r.err;
    }
    return 0;
}

int DeviceValidateUtf8(DeviceUtf8Job* jobs, int njobs, int device) {
    if (njobs <= 0) return 0;
    if (!jobs || device < 0) return -1;
    StringTables st;
    for (int i = 0; i < njobs; ++i) {
        DeviceUtf8Job& j = jobs[i];
        j.first_bad = 0;
        j.err = 0;
        if (j.n == 0) continue;
        if (!j.src || j.n > kMaxBytes) {
            j.err = 2;
            continue;
        }
        JsonStringJob job = {};
        job.src = static_cast<const uint8_t*>(j.src);
        job.n = (uint32_t)j.n;
        st.add(i, job);
    }
    if (st.live.empty()) return 0;
    if (st.finish(device, 0, 0) != 0) return -1;
    st.t.ok = nullptr;  // no verdict gates a store here
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchJsonStringValidate(st.t, s); }) != 0) return -1;
    for (size_t k = 0; k < st.live.size(); ++k) {
        DeviceUtf8Job& j = jobs[st.live[k]];
        j.first_bad = st.result(k).first_bad;
        j.err = st.result(k).err;
    }
    return 0;
}

}  // namespace gpu
}  // namespace mrpc
