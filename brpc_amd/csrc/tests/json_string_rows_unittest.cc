// json::UnescapeStringRows (base/json_string_rows.h) against a naive reference
// written here: a byte-by-byte state machine cuts the text at the quotes no
// backslash escapes, json::UnescapeStringBody decodes each body, and a walk
// from token to token over that cut gives first_bad. Every accepted shape,
// every refusal class with its offset, and EscapeStringRows ->
// UnescapeStringRows on seeded random row sets.
#include <cstdint>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/json_string_rows.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

struct Naive {
    int rc = 0;
    std::string bytes;
    std::vector<uint32_t> ends;
    uint32_t depth = 0;
    uint64_t first_bad = 0;
};

bool naive_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// One token of the text outside strings: a byte, or a whole string [at, end).
struct NaiveToken {
    char kind;  // '[' ']' ',' 's' (a closed string) 'o' (a string the text ends in) '?' (any other byte)
    size_t at, end;
};

std::vector<NaiveToken> naive_tokens(const std::string& t) {
    std::vector<NaiveToken> out;
    size_t p = 0;
    while (p < t.size()) {
        const char c = t[p];
        if (naive_space(c)) {
            ++p;
            continue;
        }
        if (c != '"') {
            out.push_back({c == '[' || c == ']' || c == ',' ? c : '?', p, p + 1});
            ++p;
            continue;
        }
        size_t q = p + 1;
        bool escaped = false, closed = false;
        for (; q < t.size(); ++q) {
            if (escaped) escaped = false;
            else if (t[q] == '\\') escaped = true;
            else if (t[q] == '"') {
                closed = true;
                break;
            }
        }
        out.push_back({closed ? 's' : 'o', p, closed ? q + 1 : t.size()});
        p = closed ? q + 1 : t.size();
    }
    return out;
}

Naive naive_rows(const std::string& t) {
    Naive r;
    auto fail = [&](uint64_t at) {
        r = Naive();
        r.rc = 1;
        r.first_bad = at;
        return r;
    };
    const std::vector<NaiveToken> tok = naive_tokens(t);
    size_t k = 0;
    // a string token: its body decodes, or the text sticks inside it
    auto string_at = [&](const NaiveToken& s, uint64_t* bad) {
        const size_t body = s.at + 1, len = (s.kind == 's' ? s.end - 1 : s.end) - body;
        std::string got;
        uint64_t where = 0;
        // the body with what follows it in the text: an escape cut off by the closing quote reads the quote
        // and fails on it, one cut off by the end of the text fails there
        if (json::UnescapeStringBody(t.data() + body, len, &got, &where) != 0) {
            *bad = body + where;
            return false;
        }
        if (s.kind == 'o') {
            *bad = t.size();
            return false;
        }
        r.bytes += got;
        r.ends.push_back((uint32_t)r.bytes.size());
        return true;
    };
    if (k < tok.size() && tok[k].kind == '[') {
        r.depth = 1;
        ++k;
        if (k < tok.size() && tok[k].kind == ']') {
            ++k;
            return k == tok.size() ? r : fail(tok[k].at);
        }
    } else if (tok.empty()) {
        return r;
    }
    for (;;) {
        if (k == tok.size()) return fail(t.size());
        if (tok[k].kind != 's' && tok[k].kind != 'o') return fail(tok[k].at);
        uint64_t bad = 0;
        if (!string_at(tok[k], &bad)) return fail(bad);
        ++k;
        if (k < tok.size() && tok[k].kind == ',') {
            ++k;
            continue;
        }
        break;
    }
    if (r.depth == 1) {
        if (k == tok.size()) return fail(t.size());
        if (tok[k].kind != ']') return fail(tok[k].at);
        ++k;
    }
    return k == tok.size() ? r : fail(tok[k].at);
}

void expect_same(const std::string& t) {
    const Naive want = naive_rows(t);
    json::StringRows got;
    const int rc = json::UnescapeStringRows(t.data(), t.size(), &got);
    ASSERT_TRUE_M(rc == want.rc, t);
    ASSERT_TRUE_M(got.first_bad == want.first_bad, t);
    ASSERT_TRUE_M(got.bytes == want.bytes && got.row_ends == want.ends && got.depth == want.depth, t);
}

}  // namespace

TEST(JsonStringRows, accepted_shapes) {
    struct Case {
        const char* text;
        const char* bytes;
        std::vector<uint32_t> ends;
        uint32_t depth;
    };
    const Case cases[] = {
        {"", "", {}, 0},
        {" \t\n\r", "", {}, 0},
        {"[]", "", {}, 1},
        {" [ \n] ", "", {}, 1},
        {"\"\"", "", {0}, 0},
        {"[\"\"]", "", {0}, 1},
        {"\"a\"", "a", {1}, 0},
        {" \"a\" , \"b\"\t", "ab", {1, 2}, 0},
        {"[\"a\",\"b\"]", "ab", {1, 2}, 1},
        {"[ \"a\" ,\n\"\" , \"c,[]\\\"\" ] ", "ac,[]\"", {1, 1, 6}, 1},
        {"\"\",\"\",\"\"", "", {0, 0, 0}, 0},
        {"\"\\ud83d\\ude00\\u00e9\"", "\xf0\x9f\x98\x80\xc3\xa9", {6}, 0},
        {"[\"\x01\xff raw\"]", "\x01\xff raw", {6}, 1},
        {"\"\\\\\",\"\\\\\\\"\"", "\\\\\"", {1, 3}, 0},
    };
    for (const Case& c : cases) {
        json::StringRows got;
        ASSERT_EQ(json::UnescapeStringRows(c.text, strlen(c.text), &got), 0);
        EXPECT_EQ(got.bytes, std::string(c.bytes));
        EXPECT_TRUE(got.row_ends == c.ends);
        EXPECT_EQ(got.depth, c.depth);
        expect_same(c.text);
    }
}

TEST(JsonStringRows, refusals_and_their_offsets) {
    struct Case {
        const char* text;
        uint64_t first_bad;
    };
    const Case cases[] = {
        // the text ends too soon: an open string, a trailing comma, a '[' without its ']'
        {"\"abc", 4}, {"\"", 1}, {"\"a\",", 4}, {"\"a\", ", 5}, {"[", 1}, {"[\"a\"", 4}, {"[\"a\" ", 5}, {"[\"a\",", 5},
        // what is no string: nested arrays, numbers, null, objects
        {"[[\"a\"]]", 1}, {"[1]", 1}, {"null", 0}, {"{\"a\":\"b\"}", 0}, {"\"a\"x", 3}, {"x\"a\"", 0},
        // tokens out of place
        {"[\"a\" \"b\"]", 5}, {"\"a\" \"b\"", 4}, {"\"a\"]", 3}, {"]", 0}, {",", 0}, {"[,\"a\"]", 1}, {"[\"a\",]", 5},
        {"[\"a\",,\"b\"]", 5}, {"[]\"a\"", 2}, {"[] ]", 3}, {"[][", 2}, {"[\"a\"],", 5},
        // bad escapes, at their backslash
        {"\"a\\q\"", 2}, {"[\"\\u12\"]", 2}, {"\"\\ud83d\"", 1}, {"\"\\ude00\"", 1}, {"\"\\ud83d\",\"\\ude00\"", 1},
        {"\"abc\\", 4}, {"\\\"a\"", 0}, {"\"a\"\\", 3},
    };
    for (const Case& c : cases) {
        json::StringRows got;
        got.bytes = "stale";
        got.row_ends.push_back(7);
        ASSERT_EQ(json::UnescapeStringRows(c.text, strlen(c.text), &got), 1);
        EXPECT_EQ(got.first_bad, c.first_bad);
        EXPECT_TRUE(got.bytes.empty() && got.row_ends.empty() && got.depth == 0);
        expect_same(c.text);
    }
}

TEST(JsonStringRows, local_rules_agree_with_the_walk) {
    // every text over a small alphabet up to 7 bytes: the twin and the naive reference
    const char alphabet[] = {'"', '\\', ',', '[', ']', ' ', 'a'};
    for (int len = 0; len <= 7; ++len) {
        uint64_t total = 1;
        for (int i = 0; i < len; ++i) total *= sizeof(alphabet);
        for (uint64_t code = 0; code < total; ++code) {
            std::string t;
            uint64_t c = code;
            for (int i = 0; i < len; ++i, c /= sizeof(alphabet)) t.push_back(alphabet[c % sizeof(alphabet)]);
            expect_same(t);
        }
    }
}

TEST(JsonStringRows, worst_cases) {
    namespace jr = json_string_rows;
    EXPECT_EQ(jr::JsonStringRowsMaxBytes(0), 0u);
    EXPECT_EQ(jr::JsonStringRowsMaxBytes(1), 0u);
    EXPECT_EQ(jr::JsonStringRowsMaxBytes(2), 0u);
    EXPECT_EQ(jr::JsonStringRowsMaxBytes(10), 8u);
    EXPECT_EQ(jr::JsonStringRowsMaxRows(0), 0u);
    EXPECT_EQ(jr::JsonStringRowsMaxRows(2), 1u);   // ""
    EXPECT_EQ(jr::JsonStringRowsMaxRows(5), 2u);   // "",""
    EXPECT_EQ(jr::JsonStringRowsMaxRows(7), 2u);
    EXPECT_EQ(jr::JsonStringRowsMaxRows(8), 3u);
}

TEST(JsonStringRows, inverse_of_escape_rows_on_random_row_sets) {
    std::mt19937 rng(20240607);
    for (int round = 0; round < 100000; ++round) {
        const size_t rows = rng() % 7;
        std::string bytes;
        std::vector<uint32_t> ends;
        for (size_t r = 0; r < rows; ++r) {
            const size_t len = rng() % 4 == 0 ? 0 : rng() % 24;  // empty rows included
            for (size_t i = 0; i < len; ++i) bytes.push_back((char)(rng() & 0xFF));  // all 256 values
            ends.push_back((uint32_t)bytes.size());
        }
        std::string text;
        ASSERT_TRUE(json::EscapeStringRows(bytes.data(), ends.data(), rows, &text));
        json::StringRows got;
        ASSERT_EQ(json::UnescapeStringRows(text.data(), text.size(), &got), 0);
        ASSERT_TRUE(got.bytes == bytes && got.row_ends == ends && got.depth == 0);
        if (round % 16 == 0) {
            const std::string bracketed = " [ " + text + "\n]";
            ASSERT_EQ(json::UnescapeStringRows(bracketed.data(), bracketed.size(), &got), 0);
            ASSERT_TRUE(got.bytes == bytes && got.row_ends == ends && got.depth == 1);
            expect_same(bracketed);
        }
    }
}
