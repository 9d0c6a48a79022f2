// json::EncodeBase64Rows / DecodeBase64Rows (base/base64_rows.h) against a
// straightforward loop over base64_encode / base64_decode row by row, the
// local rule of the header against its sequential walk on every short text,
// every refusal with its offset, and the bounds on texts that attain them.
//
// The suite also runs under AddressSanitizer and UBSan as a program of its
// own, on the CPU only, from this file, tests/test_main.cc, json/json.cc and
// base/*.cc alone (inputs come from heap buffers of exactly their size):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -march=x86-64-v2 -mpclmul -Ibrpc_amd/csrc
//       brpc_amd/csrc/tests/base64_rows_unittest.cc brpc_amd/csrc/tests/test_main.cc
//       brpc_amd/csrc/json/json.cc brpc_amd/csrc/base/*.cc -lcrypto -lz -lpthread
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/base64_rows.h"
#include "base/util.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;
namespace br = mrpc::base64_rows;
namespace jr = mrpc::json_string_rows;

namespace {

// n bytes in a heap buffer of exactly n: one byte read too many is a report under ASan
struct Exact {
    char* p;
    size_t n;
    explicit Exact(const std::string& s) : p(static_cast<char*>(malloc(s.size() ? s.size() : 1))), n(s.size()) {
        if (n) memcpy(p, s.data(), n);
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
};

int decode(const std::string& text, json::StringRows* out) {
    const Exact in(text);
    return json::DecodeBase64Rows(in.p, in.n, out);
}

// The lowest offset at which a local rule of the header fails, n when only the
// end fails, -1 when none does: every byte judged from its state alone.
int64_t lowest_local_fault(const std::string& t) {
    uint32_t pred = jr::kStart, depth = 0;
    bool inside = false;
    uint64_t j = 0;
    for (size_t i = 0; i < t.size(); ++i) {
        const uint8_t c = (uint8_t)t[i];
        if (inside) {
            if (br::BodyByteBad(c, (uint8_t)t[i - 1], j)) return (int64_t)i;
            if (c == '"') {
                inside = false;
                pred = jr::kCloseQuote;
            }
            ++j;
            continue;
        }
        if (number_text::IsSpace((char)c)) continue;
        const uint32_t tok = jr::OutsideKind(c);
        if (tok == 0 || !jr::Follows(pred, tok) || (tok == jr::kCloseBracket && depth == 0)) return (int64_t)i;
        if (tok == jr::kOpenBracket) depth = 1;
        pred = tok;
        if (tok == jr::kOpenQuote) inside = true, j = 0;
    }
    if (inside || !jr::EndsWell(pred, depth)) return (int64_t)t.size();
    return -1;
}

// The rows of an accepted text the slow way: cut at the quotes, base64_decode each body.
bool naive_rows(const std::string& t, std::string* bytes, std::vector<uint32_t>* ends) {
    size_t p = 0;
    while ((p = t.find('"', p)) != std::string::npos) {
        const size_t q = t.find('"', p + 1);
        if (q == std::string::npos) return false;
        std::string row;
        if (!base64_decode(t.data() + p + 1, q - p - 1, &row)) return false;
        bytes->append(row);
        ends->push_back((uint32_t)bytes->size());
        p = q + 1;
    }
    return true;
}

}  // namespace

TEST(Base64Rows, twin_against_a_loop_over_the_flat_coder) {
    std::mt19937 rng(20240611);
    for (int it = 0; it < 100000; ++it) {
        const size_t rows = rng() % 6;
        std::string bytes, want;
        std::vector<uint32_t> ends;
        const bool brackets = rng() & 1;
        if (brackets) want.push_back('[');
        for (size_t r = 0; r < rows; ++r) {
            const size_t len = (rng() % 4 == 0) ? 0 : rng() % 14;
            std::string row(len, 0);
            for (char& c : row) c = (char)rng();
            bytes += row;
            ends.push_back((uint32_t)bytes.size());
            if (r) want.push_back(',');
            want += '"' + base64_encode(row.data(), row.size()) + '"';
        }
        if (brackets) want.push_back(']');
        std::string text = "x";
        const Exact data(bytes);
        ASSERT_TRUE(json::EncodeBase64Rows(data.p, ends.data(), rows, brackets, &text));
        ASSERT_TRUE_M(text == "x" + want, want);
        ASSERT_LE(want.size(), br::Base64RowsWorstCaseBytes(bytes.size(), rows, brackets));
        json::StringRows got;
        ASSERT_EQ(decode(want, &got), 0);
        ASSERT_TRUE_M(got.bytes == bytes && got.row_ends == ends && got.depth == (brackets ? 1u : 0u), want);
        std::string nbytes;
        std::vector<uint32_t> nends;
        ASSERT_TRUE(naive_rows(want, &nbytes, &nends));
        ASSERT_TRUE_M(nbytes == got.bytes && nends == got.row_ends, want);
        ASSERT_LE(got.bytes.size(), br::Base64RowsMaxBytes(want.size()));
        ASSERT_LE(got.row_ends.size(), br::Base64RowsMaxRows(want.size()));
    }
}

TEST(Base64Rows, decreasing_row_ends_append_nothing) {
    const uint32_t ends[3] = {2, 1, 3};
    std::string out = "keep";
    EXPECT_FALSE(json::EncodeBase64Rows("abc", ends, 3, true, &out));
    EXPECT_EQ(out, std::string("keep"));
}

TEST(Base64Rows, local_rule_agrees_with_the_walk_on_every_short_text) {
    const char alphabet[] = {'A', 'z', '=', '"', ' ', '\\'};
    uint64_t texts = 0, accepted = 0;
    for (size_t n = 0; n <= 8; ++n) {
        std::vector<uint32_t> digit(n, 0);
        std::string t(n, 'A');
        for (;;) {
            for (size_t i = 0; i < n; ++i) t[i] = alphabet[digit[i]];
            ++texts;
            json::StringRows got;
            const int rc = decode(t, &got);
            const int64_t want = lowest_local_fault(t);
            ASSERT_TRUE_M((rc == 0) == (want < 0), t);
            if (rc != 0) {
                ASSERT_TRUE_M(got.first_bad == (uint64_t)want, t);
                ASSERT_TRUE_M(got.bytes.empty() && got.row_ends.empty() && got.depth == 0, t);
            } else {
                ++accepted;
                std::string nbytes;
                std::vector<uint32_t> nends;
                ASSERT_TRUE_M(naive_rows(t, &nbytes, &nends), t);
                ASSERT_TRUE_M(nbytes == got.bytes && nends == got.row_ends, t);
            }
            size_t k = 0;
            while (k < n && ++digit[k] == sizeof(alphabet)) digit[k++] = 0;
            if (k == n) break;
        }
    }
    EXPECT_EQ(texts, 2015539u);
    EXPECT_GT(accepted, 0u);
}

TEST(Base64Rows, refusals_and_their_offsets) {
    struct Case {
        const char* text;
        uint64_t first_bad;
    };
    const Case cases[] = {
        {"\"Q\"", 2},            // a lone symbol: the closing quote at body offset 1
        {"\"QUJDR\"", 6},        // the same behind a whole group
        {"\"=\"", 1},            // '=' at body offset 0
        {"\"Q=\"", 2},           // '=' at body offset 1
        {"\"QQ=\"", 4},          // padded, but not to four: the closing quote
        {"\"QQ=Q\"", 4},         // a symbol behind '='
        {"\"QQ===\"", 5},        // a third '='
        {"\"QUI==\"", 5},        // '=' at body offset 0 of the next group
        {"\"QUJD=\"", 5},        // the same behind a whole group
        {"\"QU\\/D\"", 3},       // a backslash, even in an escape JSON would read
        {"\"QU JD\"", 3},        // whitespace inside a string
        {"\"QU\nJD\"", 3},       // a line break inside a string
        {"\"QU-_\"", 3},         // URL-safe symbols
        {"\"QUJD", 5},           // never closed
        {"\"QUJD\",", 7},        // a trailing comma
        {"[\"QUJD\",]", 8},      // and in brackets
        {"[[\"QQ==\"]]", 1},     // depth 2
        {"[1,2]", 1},            // numbers
        {"\"QQ==\"]", 6},        // ']' without '['
        {"[\"QQ==\"", 7},        // '[' without ']'
        {"\"QQ==\" \"QQ==\"", 7},  // no comma
        {"[\"QQ==\"] x", 9},     // something behind the end
    };
    for (const Case& c : cases) {
        json::StringRows got;
        ASSERT_TRUE_M(decode(c.text, &got) == 1, c.text);
        EXPECT_TRUE_M(got.first_bad == c.first_bad, c.text);
        EXPECT_TRUE(got.bytes.empty() && got.row_ends.empty() && got.depth == 0);
        EXPECT_EQ(lowest_local_fault(c.text), (int64_t)c.first_bad);
    }
}

TEST(Base64Rows, accepted_shapes) {
    struct Case {
        const char* text;
        const char* bytes;
        std::vector<uint32_t> ends;
        uint32_t depth;
    };
    const Case cases[] = {
        {"", "", {}, 0},
        {" \t\r\n", "", {}, 0},
        {"[ ]", "", {}, 1},
        {"\"\"", "", {0}, 0},
        {"[\"QUJD\",\"\",\"3q2+7w==\"]", "ABC\xde\xad\xbe\xef", {3, 3, 7}, 1},
        {" \"QQ\" ,\n\"QUI\" ", "AAB", {1, 3}, 0},  // unpadded
        {"\"QR==\"", "A", {1}, 0},                   // trailing bits that are not zero are dropped
        {"[\"QUJDQUJD\"]", "ABCABC", {6}, 1},
    };
    for (const Case& c : cases) {
        json::StringRows got;
        ASSERT_TRUE_M(decode(c.text, &got) == 0, c.text);
        EXPECT_EQ(got.bytes, std::string(c.bytes));
        EXPECT_TRUE(got.row_ends == c.ends);
        EXPECT_EQ(got.depth, c.depth);
    }
}

TEST(Base64Rows, bounds_are_attained) {
    EXPECT_EQ(br::Base64RowsMaxBytes(0), 0u);
    EXPECT_EQ(br::Base64RowsMaxBytes(1), 0u);
    EXPECT_EQ(br::Base64RowsMaxRows(0), 0u);
    EXPECT_EQ(br::Base64RowsWorstCaseBytes(0, 0, false), 0u);
    EXPECT_EQ(br::Base64RowsWorstCaseBytes(0, 0, true), 2u);
    for (size_t n = 2; n <= 200; ++n) {
        // one string of n - 2 symbols, one fewer where a lone symbol would trail (then a blank makes up the length)
        const size_t m = (n - 2) % 4 == 1 ? n - 3 : n - 2;
        const std::string text = '"' + std::string(m, 'Q') + '"' + std::string(n - 2 - m, ' ');
        json::StringRows got;
        ASSERT_EQ(decode(text, &got), 0);
        EXPECT_EQ(got.bytes.size(), br::Base64RowsMaxBytes(n));
    }
    for (size_t rows = 1; rows <= 50; ++rows) {
        std::string text;
        for (size_t r = 0; r < rows; ++r) text += r ? ",\"\"" : "\"\"";
        json::StringRows got;
        ASSERT_EQ(decode(text, &got), 0);
        EXPECT_EQ(got.row_ends.size(), rows);
        EXPECT_EQ(br::Base64RowsMaxRows(text.size()), rows);
        // rows of one byte each take the most text
        const std::string bytes(rows, 'x');
        std::vector<uint32_t> ends(rows);
        for (size_t r = 0; r < rows; ++r) ends[r] = (uint32_t)r + 1;
        for (int brackets = 0; brackets < 2; ++brackets) {
            std::string out;
            ASSERT_TRUE(json::EncodeBase64Rows(bytes.data(), ends.data(), rows, brackets != 0, &out));
            EXPECT_EQ(out.size(), br::Base64RowsWorstCaseBytes(rows, rows, brackets != 0));
        }
    }
}
