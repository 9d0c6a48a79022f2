// json::ParseNumberText, the host twin of gpu::DeviceParseNumberText: the
// shapes it takes, what it refuses and where (first_bad), the row ends of
// ragged rows, and the redo list a device lane would leave (exact = false).
// The host half of the device entry: what it refuses before any launch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "base/decimal_to_double.h"
#include "gpu/json_offload.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

json::NumberText parse(const std::string& t, uint32_t mode = 1, bool exact = true, bool nested_ok = true) {
    json::NumberText r;
    const bool ok = json::ParseNumberText(t.data(), t.size(), mode, &r, exact, nested_ok);
    EXPECT_EQ(ok, r.err == 0);
    return r;
}

std::vector<double> doubles(const json::NumberText& r) {
    std::vector<double> v(r.out.size() / 8);
    memcpy(v.data(), r.out.data(), v.size() * 8);
    return v;
}

}  // namespace

TEST(NumberText, the_three_depths_and_the_empty_texts) {
    for (const char* t : {"", " \t\r\n", "[]", " [ ] "}) {
        const json::NumberText r = parse(t);
        EXPECT_EQ(r.err, 0);
        EXPECT_EQ(r.count, 0u);
        EXPECT_EQ(r.rows, 0u);
        EXPECT_EQ(r.first_bad, kNone);
        EXPECT_EQ(r.depth, strchr(t, '[') ? 1u : 0u);
        EXPECT_TRUE(r.out.empty());
    }
    json::NumberText r = parse("1.5,-2,3e2");
    EXPECT_EQ(r.err, 0);
    EXPECT_EQ(r.depth, 0u);
    EXPECT_EQ(r.count, 3u);
    EXPECT_TRUE(doubles(r) == (std::vector<double>{1.5, -2.0, 300.0}));
    r = parse(" [ 1.5\t,\n-2 ,\r\n 3e2 ] ");
    EXPECT_EQ(r.err, 0);
    EXPECT_EQ(r.depth, 1u);
    EXPECT_EQ(r.count, 3u);
    EXPECT_EQ(r.rows, 0u);
    EXPECT_TRUE(doubles(r) == (std::vector<double>{1.5, -2.0, 300.0}));
    r = parse("[[1,2]]");
    EXPECT_EQ(r.err, 0);
    EXPECT_EQ(r.depth, 2u);
    EXPECT_EQ(r.count, 2u);
    EXPECT_EQ(r.rows, 1u);
    EXPECT_TRUE(r.row_ends == (std::vector<uint32_t>{2}));
    r = parse("7");
    EXPECT_EQ(r.count, 1u);
    EXPECT_EQ(r.depth, 0u);
    r = parse("[[7]]");
    EXPECT_EQ(r.count, 1u);
    EXPECT_EQ(r.rows, 1u);
}

TEST(NumberText, ragged_rows_and_their_ends) {
    const json::NumberText r = parse(" [ [1, 2,3] ,[4],\n[5,6] , [ 7 ] ] ");
    EXPECT_EQ(r.err, 0);
    EXPECT_EQ(r.depth, 2u);
    EXPECT_EQ(r.count, 7u);
    EXPECT_EQ(r.rows, 4u);
    EXPECT_TRUE(r.row_ends == (std::vector<uint32_t>{3, 4, 6, 7}));
    EXPECT_TRUE(doubles(r) == (std::vector<double>{1, 2, 3, 4, 5, 6, 7}));
    // without somewhere to put row ends the same text is refused at piece 0
    const json::NumberText flat = parse("[[1,2],[3]]", 1, true, false);
    EXPECT_EQ(flat.err, 1);
    EXPECT_EQ(flat.first_bad, 0u);
}

TEST(NumberText, modes_mean_what_the_separator_twin_makes_of_them) {
    const std::string bare = "1,-0,-0.0,18446744073709551615,0.5,1e400,3.4028235677973366e38";
    std::vector<uint32_t> seps;
    json::NumberArraySeparators(bare.data(), bare.size(), &seps);
    std::vector<uint64_t> payload(seps.size() - 1);
    std::vector<uint8_t> classes(seps.size() - 1);
    ASSERT_TRUE(json::ParseNumberArray(bare.data(), seps.data(), seps.size(), payload.data(), classes.data()));
    const json::NumberText n = parse("[" + bare + "]", 0);
    ASSERT_EQ(n.err, 0);
    ASSERT_EQ(n.out.size(), payload.size() * 8);
    EXPECT_EQ(memcmp(n.out.data(), payload.data(), n.out.size()), 0);
    EXPECT_EQ(memcmp(n.classes.data(), classes.data(), classes.size()), 0);
    const json::NumberText d = parse(bare, 1), f = parse(bare, 2);
    ASSERT_EQ(d.out.size(), payload.size() * 8);
    ASSERT_EQ(f.out.size(), payload.size() * 4);
    EXPECT_TRUE(d.classes.empty());
    for (size_t i = 0; i < payload.size(); ++i) {
        const uint64_t want = decimal_to_double::NumberToDoubleBits(decimal_to_double::NumberResult{payload[i], classes[i]});
        uint64_t got;
        uint32_t got32;
        memcpy(&got, d.out.data() + 8 * i, 8);
        memcpy(&got32, f.out.data() + 4 * i, 4);
        EXPECT_EQ(got, want);
        EXPECT_EQ(got32, decimal_to_double::NarrowDoubleBits(want));
    }
    EXPECT_EQ(doubles(d)[1], 0.0);
    EXPECT_FALSE(std::signbit(doubles(d)[1]));  // "-0" the integer is +0.0
    EXPECT_TRUE(std::signbit(doubles(d)[2]));
    EXPECT_EQ(parse("1", 3).err, 2);
}

TEST(NumberText, refusals_and_first_bad) {
    struct Case {
        const char* text;
        uint32_t first_bad;
    };
    const Case cases[] = {
        {"[[],[1]]", 0},       // an empty inner row
        {"[[1],[]]", 1},
        {"[[]]", 0},
        {"[[[1]]]", 0},        // depth 3
        {"[1,2", 1},           // a missing bracket
        {"[1", 0},
        {"1,2]", 1},           // surplus brackets
        {"[1,2]]", 1},
        {"[[1,2],[3]", 2},
        {"[[1,2]],[3]]", 1},
        {"[1,[2]]", 1},
        {"[[1],2]", 1},
        {"[1],[2]", 0},
        {"[[1][2]]", 0},
        {"[\"NaN\"]", 0},
        {"1,\"NaN\",3", 1},
        {"1,2,", 2},           // a trailing comma
        {"[1,2,]", 2},
        {",1", 0},
        {",,,,", 0},
        {"1,,2", 1},
        {"1.", 0},
        {"1,2,01", 2},
        {"1 2", 0},
        {"[1,2] x", 1},
        {"x[1,2]", 0},
        {"[1,]2]", 1},
        {"1,1.,\"NaN\"", 1},  // two bad pieces: the lower index
    };
    for (const Case& c : cases) {
        const json::NumberText r = parse(c.text, 0);
        EXPECT_EQ(r.err, 1);
        if (r.first_bad != c.first_bad) fprintf(stderr, "text %s: first_bad %u, want %u\n", c.text, r.first_bad, c.first_bad);
        EXPECT_EQ(r.first_bad, c.first_bad);
        EXPECT_TRUE(r.out.empty() && r.classes.empty() && r.row_ends.empty());
    }
}

TEST(NumberText, redo_pairs_point_at_the_piece) {
    const std::string longer = "0." + std::string(decimal_to_double::kMaxDeviceNumberChars, '3');
    const std::string text = "[[1.5, " + longer + "],\n[ " + longer + ",2]]";
    json::NumberText r = parse(text, 0, false);
    ASSERT_EQ(r.err, 0);
    EXPECT_EQ(r.count, 4u);
    ASSERT_EQ(r.redo.size(), 4u);
    EXPECT_EQ(r.redo[0], 1u);
    EXPECT_EQ(r.redo[1], (uint32_t)text.find(',') + 1);
    EXPECT_EQ(r.redo[2], 2u);
    EXPECT_EQ(r.redo[3], (uint32_t)text.find("],") + 2);
    EXPECT_EQ(r.classes[1], (char)decimal_to_double::kNeedsExact);
    EXPECT_EQ(r.classes[2], (char)decimal_to_double::kNeedsExact);
    for (size_t k = 0; k < r.redo.size(); k += 2) {  // the number stands in the piece that starts there
        const size_t at = text.find_first_not_of(" \t\r\n[", r.redo[k + 1]);
        EXPECT_EQ(text.compare(at, longer.size(), longer), 0);
    }
    // the first element's piece starts at 0
    r = parse(longer + ",1", 1, false);
    ASSERT_EQ(r.redo.size(), 2u);
    EXPECT_EQ(r.redo[0], 0u);
    EXPECT_EQ(r.redo[1], 0u);
    // exact: converted, nothing listed
    r = parse(text, 1, true);
    EXPECT_TRUE(r.redo.empty());
    EXPECT_EQ(doubles(r)[1], strtod(longer.c_str(), nullptr));
    EXPECT_EQ(doubles(r)[2], strtod(longer.c_str(), nullptr));
}

// Host half of gpu::DeviceParseNumberText: a refused or empty job reaches no
// kernel, so these run without a GPU.
TEST(NumberText, device_entry_refuses_before_any_launch) {
    alignas(8) static char mem[64];
    auto code = [](const char* text, uint64_t n, uint32_t mode, void* out, uint8_t* classes, uint64_t cap,
                   uint32_t* row_ends, uint64_t row_cap, uint32_t* redo, uint32_t redo_cap) {
        gpu::DeviceNumberTextJob j;
        j.text = text;
        j.n = n;
        j.mode = mode;
        j.out = out;
        j.classes = classes;
        j.cap = cap;
        j.row_ends = row_ends;
        j.row_cap = row_cap;
        j.redo = redo;
        j.redo_cap = redo_cap;
        j.err = -7;
        EXPECT_EQ(gpu::DeviceParseNumberText(&j, 1, 0), 0);
        EXPECT_EQ(j.first_bad, kNone);
        EXPECT_EQ(j.count, 0u);
        return j.err;
    };
    uint8_t* m8 = reinterpret_cast<uint8_t*>(mem);
    uint32_t* m32 = reinterpret_cast<uint32_t*>(mem);
    EXPECT_EQ(code(nullptr, 0, gpu::kJsonParseFloat64, nullptr, nullptr, 0, nullptr, 0, nullptr, 0), 0);  // empty
    EXPECT_EQ(code(mem, 0, gpu::kJsonParseFloat64, mem, nullptr, 4, nullptr, 0, nullptr, 0), 0);
    EXPECT_EQ(code(nullptr, 4, gpu::kJsonParseFloat64, mem, nullptr, 4, nullptr, 0, nullptr, 0), 2);  // null text
    EXPECT_EQ(code(mem, 4, 3, mem, m8, 4, nullptr, 0, nullptr, 0), 2);                                // bad mode
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, nullptr, nullptr, 4, nullptr, 0, nullptr, 0), 2);  // null out
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, mem + 4, nullptr, 4, nullptr, 0, nullptr, 0), 2);  // a double at 4 (mod 8)
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat32, mem + 2, nullptr, 4, nullptr, 0, nullptr, 0), 2);  // a float at 2 (mod 4)
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseNumbers, mem, nullptr, 4, nullptr, 0, nullptr, 0), 2);      // numbers without classes
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, mem, nullptr, 4, nullptr, 0, nullptr, 8), 2);      // redo_cap without redo
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, mem, nullptr, 4, nullptr, 8, nullptr, 0), 2);      // row_cap without row_ends
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, mem, nullptr, 4, reinterpret_cast<uint32_t*>(mem + 2), 8, nullptr, 0), 2);
    EXPECT_EQ(code(mem, 4, gpu::kJsonParseFloat64, mem, nullptr, 4, nullptr, 0, reinterpret_cast<uint32_t*>(mem + 2), 8), 2);
    EXPECT_EQ(code(mem, 0xFFFFFFFFull, gpu::kJsonParseFloat64, mem, nullptr, 4, m32, 4, nullptr, 0), 2);  // above 2^32 - 2
    EXPECT_GE(gpu::JsonTextChunkBytes(), 256u);
}
