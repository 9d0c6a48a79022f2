// base/json_string.h and the host twins on top of it (json::EscapeStringBody,
// EscapeStringRows, UnescapeStringBody, Utf8FirstBad): EscapeString against
// the loop it had before it moved onto the shared header, kept here as the
// oracle; the unescaper against json::Reader; every refused form with its
// offset; UTF-8 on every pair of boundary bytes against a validator written
// from Unicode's table.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/json_string.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;
namespace js = mrpc::json_string;

namespace {

// json::EscapeString as it was: word-wise plain runs, a switch, snprintf
bool old_word_is_plain(uint64_t w) {
    const uint64_t ones = 0x0101010101010101ull, highs = 0x8080808080808080ull;
    const uint64_t lt20 = (w - ones * 0x20) & ~w & highs;
    const uint64_t q = w ^ (ones * '"'), b = w ^ (ones * '\\');
    const uint64_t zq = (q - ones) & ~q & highs, zb = (b - ones) & ~b & highs;
    return (lt20 | zq | zb) == 0;
}
bool old_byte_is_plain(unsigned char c) { return c >= 0x20 && c != '"' && c != '\\'; }
void old_escape_string(const std::string& s, std::string* out) {
    out->push_back('"');
    const char* p = s.data();
    const char* const end = p + s.size();
    while (p < end) {
        const char* run = p;
        while (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            if (!old_word_is_plain(w)) break;
            p += 8;
        }
        while (p < end && old_byte_is_plain((unsigned char)*p)) ++p;
        out->append(run, (size_t)(p - run));
        if (p >= end) break;
        const unsigned char c = (unsigned char)*p++;
        switch (c) {
        case '"': *out += "\\\""; break;
        case '\\': *out += "\\\\"; break;
        case '\n': *out += "\\n"; break;
        case '\r': *out += "\\r"; break;
        case '\t': *out += "\\t"; break;
        case '\b': *out += "\\b"; break;
        case '\f': *out += "\\f"; break;
        default: {
            char b[8];
            snprintf(b, sizeof(b), "\\u%04x", c);
            *out += b;
        }
        }
    }
    out->push_back('"');
}

// Unicode Table 3-7, written out on its own
size_t oracle_utf8_first_bad(const std::string& s) {
    const uint8_t* u = (const uint8_t*)s.data();
    const size_t n = s.size();
    size_t p = 0;
    auto cont = [&](size_t i, uint8_t lo, uint8_t hi) { return i < n && u[i] >= lo && u[i] <= hi; };
    while (p < n) {
        const uint8_t c = u[p];
        if (c <= 0x7F) p += 1;
        else if (c >= 0xC2 && c <= 0xDF && cont(p + 1, 0x80, 0xBF)) p += 2;
        else if (c == 0xE0 && cont(p + 1, 0xA0, 0xBF) && cont(p + 2, 0x80, 0xBF)) p += 3;
        else if (((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) && cont(p + 1, 0x80, 0xBF) && cont(p + 2, 0x80, 0xBF)) p += 3;
        else if (c == 0xED && cont(p + 1, 0x80, 0x9F) && cont(p + 2, 0x80, 0xBF)) p += 3;
        else if (c == 0xF0 && cont(p + 1, 0x90, 0xBF) && cont(p + 2, 0x80, 0xBF) && cont(p + 3, 0x80, 0xBF)) p += 4;
        else if (c >= 0xF1 && c <= 0xF3 && cont(p + 1, 0x80, 0xBF) && cont(p + 2, 0x80, 0xBF) && cont(p + 3, 0x80, 0xBF)) p += 4;
        else if (c == 0xF4 && cont(p + 1, 0x80, 0x8F) && cont(p + 2, 0x80, 0xBF) && cont(p + 3, 0x80, 0xBF)) p += 4;
        else return p;
    }
    return n;
}

bool reader_string(const std::string& body, std::string* out) {
    json::Value v;
    if (!json::Parse("\"" + body + "\"", &v) || !v.is_string()) return false;
    *out = v.as_string();
    return true;
}

const uint8_t kBoundary[] = {0x00, 0x41, 0x7f, 0x80, 0x8f, 0x90, 0x9f, 0xa0, 0xbf, 0xc0, 0xc1, 0xc2, 0xdf,
                             0xe0, 0xe1, 0xec, 0xed, 0xee, 0xef, 0xf0, 0xf1, 0xf3, 0xf4, 0xf5, 0xff};

}  // namespace

TEST(JsonString, header_sizes_every_byte_and_every_word) {
    for (int c = 0; c < 256; ++c) {
        char b[8];
        const uint32_t n = js::EscapeByte((uint8_t)c, b);
        EXPECT_EQ(n, js::EscapedSize((uint8_t)c));
        std::string want;
        old_escape_string(std::string(1, (char)c), &want);
        EXPECT_EQ(std::string(b, n), want.substr(1, want.size() - 2));
    }
    std::mt19937_64 rng(7);
    const uint8_t pool[] = {'"', '\\', '\n', 0, 1, 0x1f, 0x20, 0x7f, 0x80, 0xff, 'a', '/', '\t', '\r', '\b', '\f', 0x21, 0x5b, 0x5d, 0x23};
    for (int it = 0; it < 20000; ++it) {
        uint8_t b[8];
        uint32_t want = 0;
        bool plain = true;
        for (int k = 0; k < 8; ++k) {
            b[k] = (it & 1) ? pool[rng() % sizeof(pool)] : (uint8_t)rng();
            want += js::EscapedSize(b[k]);
            plain = plain && js::EscapedSize(b[k]) == 1;
        }
        uint64_t w;
        uint32_t w4;
        memcpy(&w, b, 8);
        memcpy(&w4, b, 4);
        EXPECT_EQ(js::EscapedSize8(w), want);
        EXPECT_EQ(js::PlainWord8(w), plain);
        EXPECT_EQ(js::EscapedSize4(w4), js::EscapedSize(b[0]) + js::EscapedSize(b[1]) + js::EscapedSize(b[2]) + js::EscapedSize(b[3]));
    }
}

TEST(JsonString, escape_string_equals_the_loop_it_replaced) {
    std::mt19937 rng(11);
    const uint8_t pool[] = {'"', '\\', '\n', '\r', '\t', '\b', '\f', 0, 1, 0x0b, 0x1f, 0x20, 0x7f, 0x80, 0xc3, 0xa9, 0xff, '/',
                            'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', 'j', 'k', 'l', 'm', 'n', 'o', 'p', 'q', 'r', 's', 't'};
    for (int it = 0; it < 100000; ++it) {
        std::string s(rng() % 70, '\0');
        const int mode = it % 3;  // all from the pool, mostly letters, any byte
        for (char& c : s) {
            if (mode == 0) c = (char)pool[rng() % sizeof(pool)];
            else if (mode == 1) c = rng() % 24 == 0 ? (char)pool[rng() % 18] : (char)('a' + rng() % 26);
            else c = (char)rng();
        }
        std::string want = "x", got = "x", body;
        old_escape_string(s, &want);
        json::EscapeString(s, &got);
        ASSERT_EQ(got, want);
        json::EscapeStringBody(s.data(), s.size(), &body);
        ASSERT_EQ("x\"" + body + "\"", want);
    }
}

TEST(JsonString, rows_are_quoted_and_joined) {
    const std::string bytes = "ab\"c\n";
    const uint32_t ends[] = {0, 2, 2, 4, 5, 5};
    std::string out = ">";
    EXPECT_TRUE(json::EscapeStringRows(bytes.data(), ends, 6, &out));
    EXPECT_EQ(out, ">\"\",\"ab\",\"\",\"\\\"c\",\"\\n\",\"\"");
    const uint32_t down[] = {2, 1, 5};
    out = ">";
    EXPECT_FALSE(json::EscapeStringRows(bytes.data(), down, 3, &out));
    EXPECT_EQ(out, ">");
    EXPECT_TRUE(json::EscapeStringRows(nullptr, nullptr, 0, &out));
    EXPECT_EQ(out, ">");
}

TEST(JsonString, unescape_equals_the_reader_on_well_formed_bodies) {
    std::mt19937 rng(13);
    const char* pieces[] = {"\\\"", "\\\\", "\\/", "\\b", "\\f", "\\n", "\\r", "\\t", "\\u0041", "\\u00e9", "\\u00E9",
                            "\\u20ac", "\\u20AC", "\\ud83d\\ude00", "\\uD83D\\uDE00", "\\udbff\\udfff", "\\ud800\\udc00",
                            "\\u0000", "\\uffff", "\\ue000", "\\ud7ff", "a", "z", " ", "/", "\x01", "\n", "\xc3\xa9", "\x80",
                            "\xff", "u", "uD83D", "0", "f"};
    const size_t npieces = sizeof(pieces) / sizeof(pieces[0]);
    for (int it = 0; it < 30000; ++it) {
        std::string body;
        const int parts = rng() % 12;
        for (int k = 0; k < parts; ++k) {
            if (rng() % 3 == 0) body += std::string(rng() % 11, (char)('a' + rng() % 26));
            body += pieces[rng() % npieces];
        }
        std::string want, got = "kept";
        ASSERT_TRUE(reader_string(body, &want));
        uint64_t bad = 99;
        ASSERT_EQ(json::UnescapeStringBody(body.data(), body.size(), &got, &bad), 0);
        ASSERT_EQ(got, "kept" + want);
    }
}

TEST(JsonString, unescape_leaves_the_loose_forms_to_the_reader) {
    struct Case {
        const char* body;
        uint64_t first_bad;
    };
    const Case cases[] = {
        {"ab\"cd", 2},                        // an unescaped quote
        {"\"", 0},
        {"abcdefgh\\", 8},                    // a backslash as the last byte
        {"\\\\\\", 2},
        {"ab\\x41", 2},                       // an unknown letter
        {"\\U0041", 0},
        {"ab\\u12", 2},                       // fewer than four hex digits
        {"ab\\u", 2},
        {"\\u12g4 and more text", 0},         // a digit that is none
        {"abc\\u00\\n12", 3},
        {"\\ud83d", 0},                       // a high surrogate alone
        {"x\\ud83dabcdef", 1},
        {"x\\ud83d\\n", 1},
        {"\\ud83d\\u0041", 0},                // ... followed by another escape
        {"\\ud83d\\ud83d\\ude00", 0},
        {"\\ud83d\\ude0", 0},                 // ... by a low one cut short
        {"\\ude00", 0},                       // a low surrogate alone
        {"abcdefghij\\udc00", 10},
        {"\\ud83d\\ude00\\ude00", 12},        // a pair, then a low one
        {"\\\\ud83d\\ude00", 7},              // the high half is text: its backslash is escaped
        {"fine\\n\\u0041 then \\q", 18},
    };
    for (const Case& c : cases) {
        std::string out = "kept";
        uint64_t bad = 999;
        EXPECT_EQ(json::UnescapeStringBody(c.body, strlen(c.body), &out, &bad), 1);
        EXPECT_EQ(bad, c.first_bad);
        EXPECT_EQ(out, "kept");
    }
    // the same offsets when plain text of every length stands in front (the word-wise run finder)
    for (size_t lead = 0; lead < 40; ++lead) {
        const std::string body = std::string(lead, 'p') + "\\ude00";
        uint64_t bad = 999;
        std::string out;
        EXPECT_EQ(json::UnescapeStringBody(body.data(), body.size(), &out, &bad), 1);
        EXPECT_EQ(bad, lead);
    }
}

TEST(JsonString, every_byte_judged_alone_gives_the_walk_s_answer) {
    // the device rule: a backslash starts an escape when an even number of backslashes stands right before
    // it; a byte is the letter of the escape one place before it, a hex digit of a \u escape two to five
    // places before it, or judged by itself. Summed counts and the lowest offender are the walk's.
    std::mt19937 rng(23);
    const char* pieces[] = {"\\", "\\", "\\\\", "\"", "u", "n", "x", "\\u", "\\u00e9", "\\ud83d", "\\ude00", "\\ud83d\\ude00",
                            "d83d", "0", "g", "ab", "\\n", "\\uD", "\\u12", "/"};
    const char* good[] = {"\\\\", "\\u00e9", "\\ud83d\\ude00", "ab", "\\n", "/", "u", "0", "d83d", "\\\"", "\\u20AC"};
    const size_t npieces = sizeof(pieces) / sizeof(pieces[0]), ngood = sizeof(good) / sizeof(good[0]);
    int refused = 0, done = 0;
    for (int it = 0; it < 200000; ++it) {
        std::string body;
        const int parts = rng() % 10;
        const int mood = rng() % 4;  // anything; well-formed but for one piece; well-formed
        for (int k = 0; k < parts; ++k) {
            body += mood == 0 ? pieces[rng() % npieces] : good[rng() % ngood];
            if (mood == 1 && k == parts / 2) body += pieces[rng() % npieces];
        }
        const size_t n = body.size();
        std::vector<bool> starts(n, false);
        size_t run = 0;
        for (size_t i = 0; i < n; ++i) {
            if (body[i] == '\\') {
                starts[i] = run % 2 == 0;
                ++run;
            } else {
                run = 0;
            }
        }
        auto started = [&](size_t i, size_t k) { return i >= k && starts[i - k]; };
        uint64_t lowest = n;
        std::string out;
        for (size_t i = 0; i < n; ++i) {
            if (started(i, 1)) continue;
            bool hex = false;
            for (size_t k = 2; k <= 5; ++k) hex = hex || (started(i, k) && body[i - k + 1] == 'u');
            if (hex) continue;
            if (body[i] == '\\') {
                char b[4];
                uint32_t span;
                const int got = js::DecodeEscape([&](int d) { return (uint8_t)body[(ptrdiff_t)i + d]; }, i, n - i,
                                                 [&] { return started(i, 6); }, b, &span);
                if (got < 0) lowest = std::min<uint64_t>(lowest, i);
                else out.append(b, (size_t)got);
            } else if (body[i] == '"') {
                lowest = std::min<uint64_t>(lowest, i);
            } else {
                out.push_back(body[i]);
            }
        }
        std::string want;
        uint64_t bad = n;
        const int rc = json::UnescapeStringBody(body.data(), n, &want, &bad);
        ASSERT_EQ(rc, lowest == n ? 0 : 1);
        if (rc == 0) {
            ASSERT_EQ(out, want);
            ++done;
        } else {
            ASSERT_EQ(bad, lowest);
            ++refused;
        }
    }
    EXPECT_TRUE(done > 20000 && refused > 20000);
}

TEST(JsonString, utf8_first_bad_on_every_boundary_byte_pair) {
    const size_t nb = sizeof(kBoundary);
    // every pair, alone, after ASCII of each length up to a word and a half, and in front of a tail
    const std::string tails[] = {"", "\x80", "\x80\x80", "\xbf\xbf\xbf", "A"};
    for (size_t a = 0; a < nb; ++a) {
        for (size_t b = 0; b < nb; ++b) {
            for (const std::string& tail : tails) {
                for (size_t lead = 0; lead < 13; ++lead) {
                    std::string s(lead, 'a');
                    s.push_back((char)kBoundary[a]);
                    s.push_back((char)kBoundary[b]);
                    s += tail;
                    ASSERT_EQ(json::Utf8FirstBad(s.data(), s.size()), oracle_utf8_first_bad(s));
                }
            }
        }
    }
    std::mt19937 rng(17);
    for (int it = 0; it < 100000; ++it) {
        std::string s(rng() % 24, '\0');
        for (char& c : s) c = (char)kBoundary[rng() % nb];
        ASSERT_EQ(json::Utf8FirstBad(s.data(), s.size()), oracle_utf8_first_bad(s));
    }
    EXPECT_EQ(json::Utf8FirstBad(nullptr, 0), 0u);
    const std::string good = "a\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80z";
    EXPECT_EQ(json::Utf8FirstBad(good.data(), good.size()), good.size());
    EXPECT_EQ(json::Utf8FirstBad(good.data(), good.size() - 2), 6u);  // the last character cut short
}

TEST(JsonString, a_continuation_is_judged_from_the_bytes_before_it) {
    // the device rule: the lowest offender over all bytes, each judged alone, is the walk's answer
    std::mt19937 rng(19);
    const size_t nb = sizeof(kBoundary);
    for (int it = 0; it < 100000; ++it) {
        std::string s(rng() % 20, '\0');
        for (char& c : s) c = (char)kBoundary[rng() % nb];
        const uint8_t* u = (const uint8_t*)s.data();
        const size_t n = s.size();
        size_t lowest = n;
        auto at = [&](size_t i) { return i < n ? u[i] : (uint8_t)0; };
        for (size_t i = n; i-- > 0;) {
            bool fine;
            if (js::Utf8IsCont(u[i])) {
                fine = js::Utf8ContCovered(i >= 1 ? u[i - 1] : 0, i >= 2 ? u[i - 2] : 0, i >= 3 ? u[i - 3] : 0, i);
            } else {
                fine = js::Utf8SequenceLen(u[i], at(i + 1), at(i + 2), at(i + 3), n - i) != 0;
            }
            if (!fine) lowest = i;
        }
        ASSERT_EQ(lowest, oracle_utf8_first_bad(s));
    }
}
