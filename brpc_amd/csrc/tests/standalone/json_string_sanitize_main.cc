// The host string twins under AddressSanitizer and UBSan, as a program of its
// own: the fast loops of json::EscapeStringBody, UnescapeStringBody and
// Utf8FirstBad read whole words, so every length 0..64 goes through them from
// heap buffers of exactly its size, where one byte too many is a report.
// Built by hand, on the CPU only, from this file and json/json.cc alone
// (build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/json_string_sanitize_main.cc
//       brpc_amd/csrc/json/json.cc -lpthread
// Prints "ok" and returns 0 when every result is right.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "base/json_string.h"
#include "json/json.h"

namespace js = mrpc::json_string;

namespace {

// n bytes in a heap buffer of exactly n
struct Exact {
    char* p;
    size_t n;
    explicit Exact(const std::string& s) : p(static_cast<char*>(malloc(s.size()))), n(s.size()) {
        if (n) memcpy(p, s.data(), n);
    }
    ~Exact() { free(p); }
};

std::string slow_escape(const std::string& s) {
    std::string out;
    for (char c : s) {
        char b[8];
        out.append(b, js::EscapeByte((uint8_t)c, b));
    }
    return out;
}

}  // namespace

int main() {
    int failures = 0;
    for (size_t n = 0; n <= 64; ++n) {
        // plain text, text with an escape at each place, all escapes
        for (size_t special = 0; special <= n + 1; ++special) {
            std::string s(n, 'a');
            for (size_t i = 0; i < n; ++i) s[i] = (char)('a' + (i * 7 + n) % 26);
            if (special < n) s[special] = special % 3 == 0 ? '"' : special % 3 == 1 ? '\n' : '\x01';
            if (special == n + 1) s.assign(n, '\\');
            const Exact in(s);
            std::string esc;
            mrpc::json::EscapeStringBody(in.p, in.n, &esc);
            if (esc != slow_escape(s)) ++failures;
            std::string quoted;
            mrpc::json::EscapeString(s, &quoted);
            if (quoted != "\"" + esc + "\"") ++failures;
            // two rows cut at `special`
            const uint32_t ends[2] = {(uint32_t)(special < n ? special : n), (uint32_t)n};
            std::string rows;
            if (!mrpc::json::EscapeStringRows(in.p, ends, 2, &rows)) ++failures;
            if (rows != "\"" + slow_escape(s.substr(0, ends[0])) + "\",\"" + slow_escape(s.substr(ends[0])) + "\"") ++failures;
            // back again, and every prefix of the escaped text (escapes cut short are refused, never overread)
            const Exact text(esc);
            std::string back;
            uint64_t bad = 0;
            if (mrpc::json::UnescapeStringBody(text.p, text.n, &back, &bad) != 0 || back != s) ++failures;
            for (size_t cut = 0; cut < esc.size(); ++cut) {
                const Exact part(esc.substr(0, cut));
                std::string out;
                const int rc = mrpc::json::UnescapeStringBody(part.p, part.n, &out, &bad);
                if (rc != 0 && (bad >= cut || !out.empty())) ++failures;
            }
        }
        // \u escapes and pairs ending exactly at the buffer's end, and cut short by 1..11 bytes
        const std::string tail = "\\u00e9\\u20ac\\ud83d\\ude00";
        for (size_t cut = 0; cut <= 12; ++cut) {
            const std::string body = std::string(n, 'x') + tail.substr(0, tail.size() - cut);
            const Exact part(body);
            std::string out;
            uint64_t bad = 0;
            const int rc = mrpc::json::UnescapeStringBody(part.p, part.n, &out, &bad);
            if ((cut == 0 || cut == 12) != (rc == 0)) ++failures;
        }
        // UTF-8: ASCII, one character of each width at each place, cut short at the end
        const char* chars[] = {"\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80"};
        for (const char* ch : chars) {
            const size_t w = strlen(ch);
            for (size_t at = 0; at + w <= n; ++at) {
                std::string s(n, 'a');
                s.replace(at, w, ch);
                const Exact in(s);
                if (mrpc::json::Utf8FirstBad(in.p, in.n) != n) ++failures;
                const Exact shorter(s.substr(0, at + w - 1));
                if (mrpc::json::Utf8FirstBad(shorter.p, shorter.n) != at) ++failures;
            }
        }
        const Exact ascii(std::string(n, 'a'));
        if (mrpc::json::Utf8FirstBad(ascii.p, ascii.n) != n) ++failures;
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
