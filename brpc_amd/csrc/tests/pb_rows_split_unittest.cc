// pb_rows::SpecField and pb::SplitRows (base/pb_rows.h, pb/rows.h), the wire
// rules and the host twin of gpu::DeviceSplitRows, and the host half of that
// entry: the two invariants the device's parallel walk rests on (a parse at
// ANY offset of ANY bytes reads inside the message and moves forward), the
// twin as the inverse of pb::SerializeRows, its codes, and the checks that
// refuse a job before anything is launched. The device half runs in
// tests/test_gpu_pb_rows_split.py on the GPU box.
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/pb_rows.h"
#include "gpu/device_codec.h"
#include "pb/rows.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

struct Split {
    int err = 0;
    uint64_t count = 0, rows = 0, others = 0, first_bad = 0;
    std::vector<uint64_t> values;  // the memory image
    std::vector<uint32_t> ends;
};

Split split(uint32_t number, uint32_t inner, uint32_t kind, const std::string& msg, uint64_t cap, uint64_t row_cap) {
    Split s;
    s.values.assign((size_t)cap + 1, 0xA5A5A5A5A5A5A5A5ull);
    s.ends.assign((size_t)row_cap + 1, 0xA5A5A5A5u);
    s.err = pb::SplitRows(number, inner, kind, msg.data(), msg.size(), s.values.data(), cap, s.ends.data(), row_cap,
                          &s.count, &s.rows, &s.others, &s.first_bad);
    return s;
}

bool untouched(const Split& s) {
    for (uint64_t v : s.values) {
        if (v != 0xA5A5A5A5A5A5A5A5ull) return false;
    }
    for (uint32_t e : s.ends) {
        if (e != 0xA5A5A5A5u) return false;
    }
    return true;
}

char g_mem[64] __attribute__((aligned(16)));  // never dereferenced: every device job here is refused

}  // namespace

TEST(PbRowsSplit, a_parse_at_any_offset_of_any_bytes_moves_forward_inside_the_message) {
    std::mt19937_64 rng(11);
    // bytes that often are tags, lengths and continuation runs
    const uint8_t likely[] = {0x00, 0x01, 0x02, 0x08, 0x0a, 0x0d, 0x09, 0x22, 0x12, 0x80, 0xff, 0x7f, 0x0b, 0x0c};
    size_t valid = 0;
    for (int round = 0; round < 100000; ++round) {
        const size_t n = 1 + rng() % 48;
        std::vector<uint8_t> b(n);
        for (uint8_t& c : b) c = rng() % 3 ? likely[rng() % sizeof(likely)] : (uint8_t)rng();
        for (size_t p = 0; p <= n; ++p) {
            const pb_rows::Field f = pb_rows::SpecField(b.data(), p, n);
            if (!f.valid) continue;
            ++valid;
            ASSERT_TRUE(f.next > p && f.next <= n);
            if ((f.tag & 7) == 2) ASSERT_TRUE(f.vpos > p && f.vpos + f.vlen == f.next);
            // what lies beyond the bytes it may read does not change the verdict
            if (p + pb_rows::kSpecReadBytes < n) {
                std::vector<uint8_t> c(b);
                for (size_t i = p + pb_rows::kSpecReadBytes; i < n; ++i) c[i] = (uint8_t)~c[i];
                const pb_rows::Field g = pb_rows::SpecField(c.data(), p, n);
                ASSERT_TRUE(g.valid && g.next == f.next && g.tag == f.tag);
            }
        }
    }
    EXPECT_TRUE(valid > 100000);
}

TEST(PbRowsSplit, verdicts_on_single_fields) {
    const struct {
        const char* bytes;
        size_t n;
        bool valid;
        uint64_t next;
    } cases[] = {
        {"\x08\x01", 2, true, 2},                       // varint
        {"\x08\x81", 2, false, 0},                      // cut inside the value
        {"\x09\x01\x02\x03\x04\x05\x06\x07\x08", 9, true, 9},
        {"\x09\x01\x02\x03\x04\x05\x06\x07", 8, false, 0},
        {"\x0d\x01\x02\x03\x04", 5, true, 5},
        {"\x0a\x00", 2, true, 2},
        {"\x0a\x03\x01\x02", 4, false, 0},              // a length past the end
        {"\x0b\x00", 2, false, 0},                      // wire types 3, 4, 6, 7
        {"\x0c\x00", 2, false, 0},
        {"\x0e\x00", 2, false, 0},
        {"\x0f\x00", 2, false, 0},
        {"\x02\x00", 2, false, 0},                      // field number 0
        {"\x88\x80\x80\x80\x00\x01", 6, true, 6},       // an over-long tag of five bytes
        {"\x88\x80\x80\x80\x10\x01", 6, false, 0},      // a tag above 2^32-1
        {"\x08\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01", 11, true, 11},
        {"\x08\xff\xff\xff\xff\xff\xff\xff\xff\xff\x02", 11, false, 0},
        {"\x08\x80\x80\x80\x80\x80\x80\x80\x80\x80\x80\x00", 12, false, 0},  // eleven bytes
        {"\x0a\x80\x80\x80\x80\x10", 6, false, 0},      // a length above 2^32-1
    };
    for (const auto& c : cases) {
        const pb_rows::Field f = pb_rows::SpecField(reinterpret_cast<const uint8_t*>(c.bytes), 0, c.n);
        EXPECT_EQ(f.valid, c.valid);
        if (f.valid) EXPECT_EQ(f.next, c.next);
    }
}

TEST(PbRowsSplit, the_twin_inverts_the_serializer_for_every_kind) {
    std::mt19937_64 rng(5);
    const uint32_t numbers[] = {1, 15, 16, 2047, 2048, (1u << 29) - 1};
    for (uint32_t kind = 0; kind <= 9; ++kind) {
        const uint32_t eb = pb_rows::SourceBytes(kind);
        for (int round = 0; round < 60; ++round) {
            const size_t count = round < 3 ? (size_t)round : rng() % 600, rows = 1 + rng() % 20;
            std::vector<uint64_t> mem(count * eb / 8 + 1);
            char* p = reinterpret_cast<char*>(mem.data());
            for (size_t i = 0; i < count; ++i) {
                uint64_t v = rng() >> (rng() % 64);
                if (rng() % 4 == 0) v = ~v;
                if (kind == 6) v &= 1;  // bools come back as 0 / 1
                memcpy(p + i * eb, &v, eb);
            }
            std::vector<uint32_t> ends(rows);
            uint32_t at = 0;
            for (size_t r = 0; r < rows; ++r) {
                if (rng() % 3) at += (uint32_t)(rng() % (count - at + 1));
                ends[r] = r + 1 == rows ? (uint32_t)count : at;
            }
            const uint32_t number = numbers[rng() % 6], inner = kind == 7 && round % 2 ? 0 : numbers[rng() % 6];
            std::string msg;
            ASSERT_EQ(pb::SerializeRows(number, inner, kind, mem.data(), count, ends.data(), rows, &msg), 0);
            const Split s = split(number, inner, kind, msg, count, rows);
            ASSERT_EQ(s.err, 0);
            EXPECT_EQ(s.count, count);
            EXPECT_EQ(s.rows, rows);
            EXPECT_EQ(s.others, 0u);
            EXPECT_TRUE(memcmp(s.values.data(), mem.data(), count * eb) == 0);
            EXPECT_TRUE(std::vector<uint32_t>(s.ends.begin(), s.ends.begin() + rows) == ends);
            std::string again;
            ASSERT_EQ(pb::SerializeRows(number, inner, kind, s.values.data(), s.count, s.ends.data(), s.rows, &again), 0);
            EXPECT_TRUE(again == msg);
            // a capacity one short: the needs, and nothing written
            if (count > 0) {
                const Split few = split(number, inner, kind, msg, count - 1, rows);
                EXPECT_EQ(few.err, 5);
                EXPECT_TRUE(few.count == count && few.rows == rows && untouched(few));
            }
            const Split short_rows = split(number, inner, kind, msg, count, rows - 1);
            EXPECT_EQ(short_rows.err, 5);
            EXPECT_TRUE(short_rows.count == count && short_rows.rows == rows && untouched(short_rows));
        }
    }
}

TEST(PbRowsSplit, codes_and_the_lowest_offender) {
    const std::string good("\x22\x03\x12\x01\x07\x0a\x02hi\x22\x00", 11);  // a row, a foreign string, an empty row
    Split s = split(4, 2, 1, good, 8, 8);
    EXPECT_EQ(s.err, 0);
    EXPECT_TRUE(s.count == 1 && s.rows == 2 && s.others == 1 && s.ends[0] == 1 && s.ends[1] == 1);
    const std::string two_fields("\x22\x05\x12\x01\x07\x18\x01", 7), no_wire("\x4b", 1);
    s = split(4, 2, 1, good + two_fields + good + no_wire, 64, 64);
    EXPECT_TRUE(s.err == 6 && s.first_bad == 11 && untouched(s));
    s = split(4, 2, 1, good + no_wire + good + two_fields, 64, 64);
    EXPECT_TRUE(s.err == 1 && s.first_bad == 11 && untouched(s));
    s = split(4, 2, 1, good + std::string("\x20\x07", 2), 64, 64);  // the rows field as a scalar
    EXPECT_TRUE(s.err == 6 && s.first_bad == 11);
    s = split(4, 2, 8, std::string("\x22\x07\x12\x05\x01\x02\x03\x04\x05", 9), 64, 64);  // five bytes of floats
    EXPECT_TRUE(s.err == 1 && s.first_bad == 0);
    s = split(4, 2, 3, std::string("\x22\x04\x12\x02\x01\x81", 6), 64, 64);  // ends inside a varint
    EXPECT_TRUE(s.err == 1 && s.first_bad == 0);
    s = split(4, 2, 3, "\x22\x0d\x12\x0b" + std::string(10, '\x80') + std::string("\x01", 1), 64, 64);
    EXPECT_TRUE(s.err == 1 && s.first_bad == 0);  // an element of eleven bytes
    s = split(4, 0, 7, std::string("\x22\x02\x22\x00", 4), 64, 64);  // a blob that looks like a row
    EXPECT_TRUE(s.err == 0 && s.rows == 1 && s.count == 2);
    EXPECT_EQ(split(0, 2, 1, good, 8, 8).err, 2);
    EXPECT_EQ(split(4, 0, 1, good, 8, 8).err, 2);
    EXPECT_EQ(split(4, 2, 10, good, 8, 8).err, 2);
    uint64_t a, b, c, d;
    EXPECT_EQ(pb::SplitRows(4, 2, 1, nullptr, 3, g_mem, 1, reinterpret_cast<uint32_t*>(g_mem), 1, &a, &b, &c, &d), 2);
    EXPECT_EQ(pb::SplitRows(4, 2, 1, nullptr, 0, nullptr, 0, nullptr, 0, &a, &b, &c, &d), 0);
}

TEST(PbRowsSplit, the_device_entry_refuses_before_any_launch) {
    auto code = [](gpu::DeviceRowsSplitJob j) {
        j.err = -1;
        EXPECT_EQ(gpu::DeviceSplitRows(&j, 1, 0), 0);
        return j.err;
    };
    gpu::DeviceRowsSplitJob good;
    good.number = 4;
    good.inner = 2;
    good.kind = 3;
    good.msg = g_mem;
    good.n = 16;
    good.values = g_mem;
    good.cap = 4;
    good.row_ends = reinterpret_cast<uint32_t*>(g_mem);
    good.row_cap = 4;
    gpu::DeviceRowsSplitJob j = good;
    j.number = 0;
    EXPECT_EQ(code(j), 2);
    j = good;
    j.inner = 1u << 29;
    EXPECT_EQ(code(j), 2);
    j = good;
    j.kind = 10;
    EXPECT_EQ(code(j), 2);
    j = good;
    j.inner = 0;  // only bytes go without a wrapper
    EXPECT_EQ(code(j), 2);
    j = good;
    j.msg = nullptr;
    EXPECT_EQ(code(j), 2);
    j = good;
    j.values = nullptr;
    EXPECT_EQ(code(j), 2);
    j = good;
    j.values = g_mem + 4;  // 8-byte elements
    EXPECT_EQ(code(j), 2);
    j = good;
    j.row_ends = reinterpret_cast<uint32_t*>(g_mem + 2);
    EXPECT_EQ(code(j), 2);
    j = good;
    j.n = gpu::kDeviceSplitMaxBytes + 1;
    EXPECT_EQ(code(j), 2);
    j = good;  // an empty message has no row, and needs no device
    j.n = 0;
    j.msg = nullptr;
    EXPECT_EQ(code(j), 0);
}
