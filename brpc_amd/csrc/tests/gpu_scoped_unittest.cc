// The holders of gpu/scoped.h. Without a device every allocation fails, and
// the suite checks that a failed or empty holder is inert; with one it checks
// ownership: each block goes back to its pool exactly once. Nothing is
// launched. Every check that needs memory is conditional on having got it.
#include <cstring>
#include <string>
#include <utility>

#include "base/buf.h"
#include "gpu/scoped.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

// A block freed twice sits twice in its pool's free list: the next two
// allocations of its size class would then return the same address.
void expect_pinned_not_doubly_freed(size_t n) {
    gpu::PinnedBlock a(n), b(n);
    if (a && b) EXPECT_TRUE(a.p != b.p);
}
void expect_hbm_not_doubly_freed(size_t n) {
    gpu::HbmBlock a(n, 0), b(n, 0);
    if (a && b) EXPECT_TRUE(a.p != b.p);
}

}  // namespace

TEST(GpuScoped, zero_bytes_hold_nothing) {
    const int64_t live = gpu::GetHbmPoolStats(0).live_blocks;
    {
        gpu::PinnedBlock p(0);
        gpu::HbmBlock h(0, 0);
        EXPECT_FALSE((bool)p);
        EXPECT_FALSE((bool)h);
        EXPECT_TRUE(p.p == nullptr && p.n == 0);
        EXPECT_TRUE(h.p == nullptr && h.n == 0);
        EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live);  // nothing was allocated
        gpu::PinnedBlock d;
        gpu::HbmBlock e;
        EXPECT_FALSE((bool)d);
        EXPECT_FALSE((bool)e);
    }
    EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live);
}

TEST(GpuScoped, failed_allocation_is_false_and_inert) {
    // reached only where there is no device (there every allocation fails)
    gpu::PinnedBlock p(4096);
    gpu::HbmBlock h(4096, 0);
    if (!p) {
        EXPECT_TRUE(p.p == nullptr);
        EXPECT_TRUE(p.as<uint32_t>() == nullptr);
        EXPECT_TRUE(p.release() == nullptr);
        gpu::PinnedBlock q(std::move(p));
        EXPECT_FALSE((bool)q);
    }
    if (!h) {
        EXPECT_TRUE(h.p == nullptr);
        EXPECT_TRUE(h.release() == nullptr);
        gpu::HbmBlock g(std::move(h));
        EXPECT_FALSE((bool)g);
    }
}

TEST(GpuScoped, moves_leave_the_source_empty_and_free_once) {
    {
        gpu::PinnedBlock a(4096);
        char* ap = a.p;
        gpu::PinnedBlock b(std::move(a));
        EXPECT_TRUE(a.p == nullptr && a.n == 0);
        EXPECT_TRUE(b.p == ap);
        if (b) EXPECT_EQ(b.n, (size_t)4096);
        gpu::PinnedBlock c(4096);  // freed by the assignment below
        c = std::move(b);
        EXPECT_TRUE(b.p == nullptr && b.n == 0);
        EXPECT_TRUE(c.p == ap);
    }
    expect_pinned_not_doubly_freed(4096);

    const int64_t live = gpu::GetHbmPoolStats(0).live_blocks;
    {
        gpu::HbmBlock a(4096, 0);
        void* ap = a.p;
        gpu::HbmBlock b(std::move(a));
        EXPECT_TRUE(a.p == nullptr && a.n == 0);
        EXPECT_TRUE(b.p == ap);
        EXPECT_EQ(b.dev, 0);
        gpu::HbmBlock c(4096, 0);
        if (b && c) EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live + 2);
        c = std::move(b);
        EXPECT_TRUE(b.p == nullptr && b.n == 0);
        EXPECT_TRUE(c.p == ap);
        if (c) EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live + 1);  // c's old block went back
    }
    EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live);
    expect_hbm_not_doubly_freed(4096);
}

TEST(GpuScoped, release_empties_the_holder) {
    char* raw = nullptr;
    {
        gpu::PinnedBlock a(512);
        raw = a.release();
        EXPECT_FALSE((bool)a);
        EXPECT_TRUE(a.p == nullptr && a.n == 0);
    }
    if (raw) {
        memset(raw, 0x5a, 512);  // still ours: the holder did not free it
        gpu::PinnedFree(raw, 512);
    }
    expect_pinned_not_doubly_freed(512);

    const int64_t live = gpu::GetHbmPoolStats(0).live_blocks;
    void* dev = nullptr;
    {
        gpu::HbmBlock h(512, 0);
        dev = h.release();
        EXPECT_FALSE((bool)h);
    }
    if (dev) {
        EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live + 1);
        gpu::HbmFree(dev, 512, 0);
    }
    EXPECT_EQ(gpu::GetHbmPoolStats(0).live_blocks, live);
}

TEST(GpuScoped, give_to_hands_the_block_to_the_buf) {
    Buf buf;
    {
        gpu::PinnedBlock a(300);
        if (!a) return;
        for (int i = 0; i < 300; ++i) a.p[i] = (char)i;
        a.give_to(&buf);
        EXPECT_FALSE((bool)a);
        EXPECT_TRUE(a.p == nullptr && a.n == 0);
    }
    ASSERT_EQ(buf.size(), (size_t)300);
    ASSERT_EQ(buf.backing_block_num(), (size_t)1);
    EXPECT_TRUE(buf.ref_at(0).block->kind == MemKind::PINNED);
    std::string back = buf.to_string();
    for (int i = 0; i < 300; ++i) ASSERT_EQ(back[i], (char)i);
    buf.clear();  // the last reference: the block goes back to the pool, once
    expect_pinned_not_doubly_freed(300);
}

TEST(GpuScoped, arrays_grow_only_and_fail_empty) {
    gpu::PinnedArray<uint32_t> pa;
    if (pa.reserve(10)) {
        EXPECT_EQ(pa.cap, (size_t)64);  // the default floor
        uint32_t* first = pa.p;
        EXPECT_TRUE(pa.reserve(64));
        EXPECT_TRUE(pa.p == first);
        EXPECT_TRUE(pa.reserve(1));
        EXPECT_TRUE(pa.p == first && pa.cap == 64);
        if (pa.reserve(65, 256)) EXPECT_EQ(pa.cap, (size_t)256);
    }
    if (!pa.p) EXPECT_EQ(pa.cap, (size_t)0);
    gpu::PinnedFree(pa.p, pa.cap * sizeof(uint32_t));

    gpu::HbmArray<uint64_t> ha;
    if (ha.reserve(10, 256, 0)) {
        EXPECT_EQ(ha.cap, (size_t)256);
        uint64_t* first = ha.p;
        EXPECT_TRUE(ha.reserve(256, 256, 0));
        EXPECT_TRUE(ha.p == first);
        if (ha.reserve(1000, 256, 0)) EXPECT_EQ(ha.cap, (size_t)1000);
    }
    if (!ha.p) EXPECT_EQ(ha.cap, (size_t)0);
    gpu::HbmFree(ha.p, ha.cap * sizeof(uint64_t), 0);
    // reserving nothing allocates nothing
    gpu::HbmArray<char> none;
    EXPECT_TRUE(none.reserve(0, 1, 0));
    EXPECT_TRUE(none.p == nullptr && none.cap == 0);
}
