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

}  // namespace gpu
}  // namespace mrpc
