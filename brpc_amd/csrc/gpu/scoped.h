// Scope guards for the offload entry points in gpu/: the device switch, the
// owners of pooled pinned / HBM blocks (gpu/hbm_pool.h) and the
// launch -> wait -> restore sequence around a pool stream. Header-only, for
// host and device translation units alike.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "gpu/gpu.h"
#include "gpu/hbm_pool.h"

namespace mrpc {
namespace gpu {

// Makes `device` current for the scope: switches only when another device is
// current and restores only what it switched.
class ScopedDevice {
public:
    explicit ScopedDevice(int device) {
        hipGetDevice(&_prev);
        _switched = _prev != device;
        if (_switched) hipSetDevice(device);
    }
    ~ScopedDevice() {
        if (_switched) hipSetDevice(_prev);
    }
    ScopedDevice(const ScopedDevice&) = delete;
    ScopedDevice& operator=(const ScopedDevice&) = delete;

private:
    int _prev = 0;
    bool _switched = false;
};

inline void pinned_block_deleter(void* p, void* arg) { PinnedFree(p, (size_t)reinterpret_cast<uintptr_t>(arg)); }

// Owner of one PinnedAlloc block. A request for 0 bytes holds nothing and
// allocates nothing (p == nullptr without being a failure).
struct PinnedBlock {
    char* p = nullptr;  // host memory: addressed by byte
    size_t n = 0;
    PinnedBlock() = default;
    explicit PinnedBlock(size_t bytes) : p(bytes ? static_cast<char*>(PinnedAlloc(bytes)) : nullptr), n(bytes) {}
    ~PinnedBlock() { PinnedFree(p, n); }
    PinnedBlock(PinnedBlock&& o) noexcept : p(o.p), n(o.n) { o.release(); }
    PinnedBlock& operator=(PinnedBlock&& o) noexcept {
        if (this != &o) {
            PinnedFree(p, n);
            p = o.p;
            n = o.n;
            o.release();
        }
        return *this;
    }
    explicit operator bool() const { return p != nullptr; }
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
    // the caller owns the returned block from here on
    char* release() {
        char* r = p;
        p = nullptr;
        n = 0;
        return r;
    }
    // hand the block to *b as one PINNED block, freed with its last reference
    void give_to(Buf* b) {
        b->append_user_data(p, n, pinned_block_deleter, reinterpret_cast<void*>((uintptr_t)n), MemKind::PINNED);
        release();
    }
};

// Owner of one HbmAlloc block of `dev`; 0 bytes as for PinnedBlock.
struct HbmBlock {
    void* p = nullptr;
    size_t n = 0;
    int dev = -1;
    HbmBlock() = default;
    HbmBlock(size_t bytes, int d) : p(bytes ? HbmAlloc(bytes, d) : nullptr), n(bytes), dev(d) {}
    ~HbmBlock() { HbmFree(p, n, dev); }
    HbmBlock(HbmBlock&& o) noexcept : p(o.p), n(o.n), dev(o.dev) { o.release(); }
    HbmBlock& operator=(HbmBlock&& o) noexcept {
        if (this != &o) {
            HbmFree(p, n, dev);
            p = o.p;
            n = o.n;
            dev = o.dev;
            o.release();
        }
        return *this;
    }
    explicit operator bool() const { return p != nullptr; }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
    void* release() {
        void* r = p;
        p = nullptr;
        n = 0;
        return r;
    }
};

// A pinned host array the kernels read (job tables) or write (results);
// grows, never shrinks, lives as long as its (recycled) owner.
template <typename T>
struct PinnedArray {
    T* p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n, size_t floor = 64) {
        if (n <= cap) return true;
        if (p) PinnedFree(p, cap * sizeof(T));
        cap = std::max(n, floor);
        p = static_cast<T*>(PinnedAlloc(cap * sizeof(T)));
        if (!p) cap = 0;
        return p != nullptr;
    }
};

// The same in the HBM of one device (always the same one for one array).
template <typename T>
struct HbmArray {
    T* p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n, size_t floor, int device) {
        if (n <= cap) return true;
        if (p) HbmFree(p, cap * sizeof(T), device);
        cap = std::max(n, floor);
        p = static_cast<T*>(HbmAlloc(cap * sizeof(T), device));
        if (!p) cap = 0;
        return p != nullptr;
    }
};

// Runs launch(stream) on a pool stream of `device` with that device current
// and waits for the stream (fiber-friendly) before the device is restored.
// It waits even when the launch failed: never free buffers a launched kernel
// may still use, and the callers free theirs as soon as this returns.
// 0 only when both the launch and the wait succeeded.
// (Whether a fiber may resume on another worker thread across the wait, and
// what the restore then means, is not settled here: the order launch, wait,
// restore is the one every caller had.)
template <typename F>
int RunOnPoolStream(int device, F&& launch) {
    ScopedDevice on(device);
    hipStream_t s = PoolStream(device);
    if (!s) return -1;
    const int rc = launch(s);
    const int wrc = SyncStream(s);
    return rc == 0 && wrc == 0 ? 0 : -1;
}

}  // namespace gpu
}  // namespace mrpc
