// json::FormatNumberRows, the host twin of gpu::DevicePrintNumbers, against a
// naive printer (std::to_string per element, AppendShortestDouble's text for
// floats, the punctuation put together row by row): every kind in the three
// forms on random arrays, the digit boundaries, the extremes, each clause of
// the first_bad rule, and what the twin and the device entry refuse before
// any launch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "base/number_print.h"
#include "gpu/json_offload.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;
namespace np = mrpc::number_print;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
const uint32_t kKinds[] = {0, 1, 2, 3, 4, 5, 6, 8, 9};

// Element i of a memory image, printed without the code under test.
std::string naive_elem(const std::vector<uint64_t>& image, size_t i, uint32_t kind) {
    const char* p = reinterpret_cast<const char*>(image.data());
    switch (kind) {
    case 0:
    case 2: {
        int32_t v;
        memcpy(&v, p + 4 * i, 4);
        return std::to_string(v);
    }
    case 1: {
        uint32_t v;
        memcpy(&v, p + 4 * i, 4);
        return std::to_string(v);
    }
    case 3:
    case 5: {
        int64_t v;
        memcpy(&v, p + 8 * i, 8);
        return std::to_string(v);
    }
    case 4: {
        uint64_t v;
        memcpy(&v, p + 8 * i, 8);
        return std::to_string(v);
    }
    case 6: return p[i] ? "true" : "false";
    case 8: {
        float v;
        memcpy(&v, p + 4 * i, 4);
        return json::Value((double)v).ToString();
    }
    default: {
        double v;
        memcpy(&v, p + 8 * i, 8);
        return json::Value(v).ToString();
    }
    }
}

std::string naive(const std::vector<uint64_t>& image, size_t count, uint32_t kind, const std::vector<uint32_t>* ends,
                  bool brackets) {
    std::string s;
    if (ends) {
        s = "[";
        size_t i = 0;
        for (size_t r = 0; r < ends->size(); ++r) {
            s += r ? ",[" : "[";
            for (size_t first = i; i < (*ends)[r]; ++i) s += (i > first ? "," : "") + naive_elem(image, i, kind);
            s += "]";
        }
        return s + "]";
    }
    for (size_t i = 0; i < count; ++i) s += (i ? "," : "") + naive_elem(image, i, kind);
    return brackets ? "[" + s + "]" : s;
}

// `count` random elements of `kind`: all magnitudes, both signs.
std::vector<uint64_t> random_image(std::mt19937_64& rng, size_t count, uint32_t kind) {
    std::vector<uint64_t> image(count + 1);
    char* p = reinterpret_cast<char*>(image.data());
    for (size_t i = 0; i < count; ++i) {
        const uint64_t bits = rng() >> (rng() % 64);  // every width
        const uint64_t v = (rng() & 1) ? bits : 0 - bits;
        switch (np::ElemBytes(kind)) {
        case 1: p[i] = (char)((rng() & 1) ? (v | 1) : 0); break;
        case 4: memcpy(p + 4 * i, &v, 4); break;
        default: memcpy(p + 8 * i, &v, 8); break;
        }
    }
    return image;
}

std::vector<uint32_t> random_rows(std::mt19937_64& rng, size_t count) {
    std::vector<uint32_t> ends;
    for (uint32_t at = 0; at < count;) {
        at += 1 + (uint32_t)(rng() % 5);
        ends.push_back(at < count ? at : (uint32_t)count);
    }
    return ends;
}

struct Got {
    int err;
    uint32_t first_bad;
    std::string text;
};

Got format(const void* values, uint64_t count, uint32_t kind, const uint32_t* row_ends, uint64_t rows, bool brackets) {
    Got g;
    g.text = "kept";
    g.first_bad = 77;
    g.err = json::FormatNumberRows(values, count, kind, row_ends, rows, brackets, &g.text, &g.first_bad);
    EXPECT_TRUE(g.text.compare(0, 4, "kept") == 0);  // appended, never assigned
    if (g.err != 0) EXPECT_EQ(g.text, std::string("kept"));
    g.text.erase(0, 4);
    return g;
}

template <class T>
std::vector<uint64_t> image_of(const std::vector<T>& v) {
    std::vector<uint64_t> image(v.size() * sizeof(T) / 8 + 1);
    memcpy(image.data(), v.data(), v.size() * sizeof(T));
    return image;
}

}  // namespace

TEST(NumberPrint, every_kind_in_the_three_forms_equals_the_naive_printer) {
    std::mt19937_64 rng(20250131);
    for (uint32_t kind : kKinds) {
        for (size_t count : {(size_t)1, (size_t)2, (size_t)7, (size_t)64, (size_t)257, (size_t)1000}) {
            const std::vector<uint64_t> image = random_image(rng, count, kind);
            const std::vector<uint32_t> ends = random_rows(rng, count);
            Got g = format(image.data(), count, kind, nullptr, 0, false);
            EXPECT_EQ(g.err, 0);
            EXPECT_EQ(g.first_bad, kNone);
            EXPECT_EQ(g.text, naive(image, count, kind, nullptr, false));
            g = format(image.data(), count, kind, nullptr, 0, true);
            EXPECT_EQ(g.err, 0);
            EXPECT_EQ(g.text, naive(image, count, kind, nullptr, true));
            for (bool brackets : {false, true}) {  // ignored with rows
                g = format(image.data(), count, kind, ends.data(), ends.size(), brackets);
                EXPECT_EQ(g.err, 0);
                EXPECT_EQ(g.first_bad, kNone);
                EXPECT_EQ(g.text, naive(image, count, kind, &ends, true));
            }
            EXPECT_LE(g.text.size(), np::WorstCaseBytes(kind, count, ends.size()));
            // the text is what the number-text parser takes, with the same rows
            if (kind != 6 && g.text.find('"') == std::string::npos) {
                json::NumberText back;
                EXPECT_TRUE(json::ParseNumberText(g.text.data(), g.text.size(), 0, &back));
                EXPECT_EQ(back.depth, 2u);
                EXPECT_EQ((size_t)back.count, count);
                EXPECT_TRUE(back.row_ends == ends);
            }
        }
        // nothing to print
        Got g = format(nullptr, 0, kind, nullptr, 0, false);
        EXPECT_EQ(g.err, 0);
        EXPECT_EQ(g.text, std::string());
        g = format(nullptr, 0, kind, nullptr, 0, true);
        EXPECT_EQ(g.err, 0);
        EXPECT_EQ(g.text, std::string("[]"));
    }
}

TEST(NumberPrint, digit_boundaries_and_extremes) {
    // 10^k - 1 and 10^k for every k an unsigned 64-bit number has
    std::vector<uint64_t> u64 = {0};
    std::string want = "[0";
    uint64_t p = 1;
    for (int k = 1; k <= 19; ++k) {
        p *= 10;
        u64.push_back(p - 1);
        u64.push_back(p);
        want += "," + std::string((size_t)k, '9') + ",1" + std::string((size_t)k, '0');
        EXPECT_EQ(np::DecimalLength(p - 1), (uint32_t)k);
        EXPECT_EQ(np::DecimalLength(p), (uint32_t)k + 1);
    }
    u64.push_back(std::numeric_limits<uint64_t>::max());
    want += ",18446744073709551615]";
    EXPECT_EQ(np::DecimalLength(std::numeric_limits<uint64_t>::max()), 20u);
    Got g = format(u64.data(), u64.size(), 4, nullptr, 0, true);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text, want);

    // the same boundaries with both signs as int64 (up to 10^18), then the extremes
    std::vector<int64_t> i64;
    want = "";
    int64_t q = 1;
    for (int k = 1; k <= 18; ++k) {
        q *= 10;
        for (int64_t v : {q - 1, q, -(q - 1), -q}) {
            i64.push_back(v);
            want += std::to_string(v) + ",";
        }
    }
    i64.push_back(std::numeric_limits<int64_t>::min());
    i64.push_back(std::numeric_limits<int64_t>::max());
    want += "-9223372036854775808,9223372036854775807";
    for (uint32_t kind : {3u, 5u}) {  // sint64 prints the number, not its wire form
        g = format(i64.data(), i64.size(), kind, nullptr, 0, false);
        EXPECT_EQ(g.err, 0);
        EXPECT_EQ(g.text, want);
    }

    const std::vector<int32_t> i32 = {std::numeric_limits<int32_t>::min(), -1000000000, -999999999, -10, -9, -1, 0, 9,
                                      10,  99, 100, 999999999, 1000000000, std::numeric_limits<int32_t>::max()};
    const std::vector<uint64_t> img32 = image_of(i32);
    for (uint32_t kind : {0u, 2u}) {
        g = format(img32.data(), i32.size(), kind, nullptr, 0, false);
        EXPECT_EQ(g.err, 0);
        EXPECT_EQ(g.text, std::string("-2147483648,-1000000000,-999999999,-10,-9,-1,0,9,10,99,100,999999999,"
                                      "1000000000,2147483647"));
    }
    // the same bits as uint32
    g = format(img32.data(), 2, 1, nullptr, 0, false);
    EXPECT_EQ(g.text, std::string("2147483648,3294967296"));
    const std::vector<uint32_t> u32 = {0, 9, 10, 4294967295u};
    g = format(image_of(u32).data(), u32.size(), 1, nullptr, 0, true);
    EXPECT_EQ(g.text, std::string("[0,9,10,4294967295]"));

    const uint8_t bools[] = {0, 1, 2, 255};
    const uint32_t ends[] = {1, 4};
    g = format(bools, 4, 6, ends, 2, false);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text, std::string("[[false],[true,true,true]]"));

    // every kind's widest element is its MaxElemChars
    EXPECT_EQ(np::MaxElemChars(0), 11u);
    EXPECT_EQ(np::MaxElemChars(1), 10u);
    EXPECT_EQ(np::MaxElemChars(3), 20u);
    EXPECT_EQ(np::MaxElemChars(4), 20u);
    EXPECT_EQ(np::MaxElemChars(6), 5u);
    EXPECT_EQ(np::MaxElemChars(9), 25u);
}

TEST(NumberPrint, first_bad_is_the_lowest_row_that_breaks_a_clause) {
    const std::vector<int32_t> v(10, 7);
    auto bad = [&](std::vector<uint32_t> ends) {
        const Got g = format(v.data(), v.size(), 0, ends.data(), ends.size(), true);
        EXPECT_EQ(g.err, g.first_bad == kNone ? 0 : 1);
        return g.first_bad;
    };
    EXPECT_EQ(bad({3, 5, 10}), kNone);
    EXPECT_EQ(bad({10}), kNone);
    EXPECT_EQ(bad({1, 2, 3, 4, 5, 6, 7, 8, 9, 10}), kNone);
    EXPECT_EQ(bad({3, 2, 10}), 1u);       // a decrease
    EXPECT_EQ(bad({3, 3, 10}), 1u);       // two equal neighbours: an empty row
    EXPECT_EQ(bad({0, 5, 10}), 0u);       // row_ends[0] == 0: an empty first row
    EXPECT_EQ(bad({3, 11, 12}), 1u);      // an end above count
    EXPECT_EQ(bad({3, 5, 9}), 2u);        // a last end below count
    EXPECT_EQ(bad({3, 5, 11}), 2u);       // a last end above count
    EXPECT_EQ(bad({11}), 0u);
    EXPECT_EQ(bad({3, 5, 4, 4, 10}), 2u);  // the lowest of several
    EXPECT_EQ(bad({4294967295u, 10}), 0u);
    // rows over no elements: whatever the first end is, row 0 is bad
    uint32_t first_bad = 9;
    std::string out;
    const uint32_t one[] = {1}, zero[] = {0};
    EXPECT_EQ(json::FormatNumberRows(nullptr, 0, 0, one, 1, true, &out, &first_bad), 1);
    EXPECT_EQ(first_bad, 0u);
    EXPECT_EQ(json::FormatNumberRows(nullptr, 0, 0, zero, 1, true, &out, &first_bad), 1);
    EXPECT_EQ(first_bad, 0u);
    EXPECT_TRUE(out.empty());
    EXPECT_EQ(json::FormatNumberRows(v.data(), 10, 0, one, 1, true, &out, nullptr), 1);  // first_bad is optional
}

TEST(NumberPrint, the_twin_refuses_what_the_device_entry_refuses) {
    alignas(8) static char mem[64];
    const uint32_t ends[] = {4};
    std::string out;
    EXPECT_EQ(json::FormatNumberRows(mem, 4, 7, nullptr, 0, true, &out), 2);    // kind 7
    EXPECT_EQ(json::FormatNumberRows(mem, 4, 10, nullptr, 0, true, &out), 2);   // above 9
    EXPECT_EQ(json::FormatNumberRows(nullptr, 4, 0, nullptr, 0, true, &out), 2);  // null values
    EXPECT_EQ(json::FormatNumberRows(mem + 2, 4, 0, nullptr, 0, true, &out), 2);  // an int32 at 2 (mod 4)
    EXPECT_EQ(json::FormatNumberRows(mem + 4, 4, 3, nullptr, 0, true, &out), 2);  // an int64 at 4 (mod 8)
    EXPECT_EQ(json::FormatNumberRows(mem + 1, 4, 6, nullptr, 0, true, &out), 0);  // a bool anywhere
    out.clear();
    EXPECT_EQ(json::FormatNumberRows(mem, 4, 0, nullptr, 1, true, &out), 2);  // rows without row_ends
    EXPECT_EQ(json::FormatNumberRows(mem, 4, 0, ends, 0, true, &out), 2);     // row_ends without rows
    EXPECT_EQ(json::FormatNumberRows(mem, 1ull << 32, 6, nullptr, 0, true, &out), 2);  // a worst case above 2^32 - 1
    EXPECT_TRUE(out.empty());
    EXPECT_EQ(np::WorstCaseBytes(7, 1, 0), 0u);
    EXPECT_EQ(np::WorstCaseBytes(0, 0, 0), 2u);                // "[]"
    EXPECT_EQ(np::WorstCaseBytes(0, 3, 0), 3u * 11 + 4);       // "[" 3 elements, 2 commas "]"
    EXPECT_EQ(np::WorstCaseBytes(9, 3, 2), 3u * 25 + 3 + 5);   // "[[" "],[" "]]" and one comma
    EXPECT_GT(np::WorstCaseBytes(6, 1ull << 40, 0), 0xFFFFFFFFull);
}

// Host half of gpu::DevicePrintNumbers: a refused or empty job reaches no
// kernel, so these run without a GPU.
TEST(NumberPrint, device_entry_refuses_before_any_launch) {
    alignas(16) static char mem[256];
    auto code = [](const void* src, uint64_t count, uint32_t kind, const void* row_ends, uint64_t rows, bool brackets,
                   void* dst, uint64_t cap) {
        gpu::DeviceNumberPrintJob j;
        j.src = src;
        j.count = count;
        j.kind = kind;
        j.row_ends = static_cast<const uint32_t*>(row_ends);
        j.rows = rows;
        j.brackets = brackets;
        j.dst = dst;
        j.cap = cap;
        j.err = -7;
        j.len = 99;
        EXPECT_EQ(gpu::DevicePrintNumbers(&j, 1, 0), 0);
        EXPECT_EQ(j.len, 0u);
        EXPECT_EQ(j.first_bad, kNone);
        return j.err;
    };
    char* dst = mem + 128;
    EXPECT_EQ(code(nullptr, 0, 0, nullptr, 0, false, nullptr, 0), 0);  // bare and empty: nothing to do
    EXPECT_EQ(code(mem, 0, 9, nullptr, 0, false, dst, 64), 0);
    EXPECT_EQ(code(mem, 0, 7, nullptr, 0, false, dst, 64), 2);           // a bad kind even then
    EXPECT_EQ(code(mem, 4, 10, nullptr, 0, true, dst, 64), 2);
    EXPECT_EQ(code(nullptr, 4, 0, nullptr, 0, true, dst, 64), 2);        // null src
    EXPECT_EQ(code(mem, 4, 0, nullptr, 0, true, nullptr, 64), 2);        // null dst
    EXPECT_EQ(code(nullptr, 0, 0, nullptr, 0, true, nullptr, 64), 2);    // "[]" has to go somewhere
    EXPECT_EQ(code(mem + 2, 4, 0, nullptr, 0, true, dst, 64), 2);        // an int32 at 2 (mod 4)
    EXPECT_EQ(code(mem + 4, 4, 4, nullptr, 0, true, dst, 64), 2);        // a uint64 at 4 (mod 8)
    EXPECT_EQ(code(mem + 4, 4, 9, nullptr, 0, true, dst, 64), 2);        // a double at 4 (mod 8)
    EXPECT_EQ(code(mem, 4, 0, mem + 66, 1, true, dst, 64), 2);           // row_ends at 2 (mod 4)
    EXPECT_EQ(code(mem, 4, 0, nullptr, 1, true, dst, 64), 2);            // rows without row_ends
    EXPECT_EQ(code(mem, 4, 0, mem + 64, 0, true, dst, 64), 2);           // row_ends without rows
    EXPECT_EQ(code(mem, 4, 0, nullptr, 0, true, mem + 15, 64), 2);       // dst overlaps src
    EXPECT_EQ(code(mem + 32, 4, 0, nullptr, 0, true, mem, 33), 2);       // dst runs into src
    EXPECT_EQ(code(mem, 4, 0, mem + 64, 1, true, mem + 60, 64), 2);      // dst overlaps row_ends
    EXPECT_EQ(code(mem, 1ull << 32, 6, nullptr, 0, true, dst, 64), 2);   // a worst case above 2^32 - 1
    EXPECT_EQ(code(mem, 4, 0, mem + 64, 1ull << 31, true, dst, 64), 2);  // by its rows alone
    EXPECT_EQ(gpu::NumberPrintWorstCaseBytes(0, 3, 0), 3u * 11 + 4);
    EXPECT_EQ(gpu::NumberPrintWorstCaseBytes(7, 3, 0), 0u);
    EXPECT_EQ(gpu::JsonNumberPrintChunkElems(), 256u);
}
