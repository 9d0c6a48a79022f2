// json::UnescapeStringRows under AddressSanitizer and UBSan, as a program of
// its own: the walk looks up to 11 bytes ahead of a backslash and 6 behind it,
// so every length 0..64 goes through it from heap buffers of exactly its size,
// where one byte too many is a report. Built by hand, on the CPU only, from
// this file and json/json.cc alone (build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/json_string_rows_sanitize_main.cc
//       brpc_amd/csrc/json/json.cc -lpthread
// Prints "ok" and returns 0 when every result is right.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "json/json.h"

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

}  // namespace

int main() {
    int failures = 0;
    // pieces an escape can be cut in, a pair among them, and the tokens
    const char* const units[] = {"\"a\\n\\u00e9\\ud83d\\ude00\\\\\",", "\"\",", "\"\\\"q\", ", "[\"x\",\"\\uD83D\\uDE00\"]",
                                 "\"\\ude00\",", "\\\\\\\\\\\\", " \t\n\r"};
    for (const char* unit : units) {
        const size_t ulen = strlen(unit);
        for (size_t n = 0; n <= 64; ++n) {
            std::string s;
            while (s.size() < n) s.append(unit, ulen);
            s.resize(n);
            for (int bracket = 0; bracket < 2; ++bracket) {
                if (bracket && n) s[0] = '[';
                const Exact in(s);
                mrpc::json::StringRows got;
                const int rc = mrpc::json::UnescapeStringRows(in.p, in.n, &got);
                if (rc == 0) {
                    // accepted: the row ends ascend to the bytes, and the text escapes back to the same rows
                    uint32_t prev = 0;
                    for (uint32_t e : got.row_ends) {
                        if (e < prev) ++failures;
                        prev = e;
                    }
                    if (prev != (got.row_ends.empty() ? 0 : got.bytes.size())) ++failures;
                    std::string again;
                    if (!mrpc::json::EscapeStringRows(got.bytes.data(), got.row_ends.data(), got.row_ends.size(), &again))
                        ++failures;
                    const Exact twice(again);
                    mrpc::json::StringRows back;
                    if (mrpc::json::UnescapeStringRows(twice.p, twice.n, &back) != 0 || back.bytes != got.bytes ||
                        back.row_ends != got.row_ends)
                        ++failures;
                } else if (rc != 1 || got.first_bad > n || !got.bytes.empty() || !got.row_ends.empty()) {
                    ++failures;
                }
            }
        }
    }
    // whole escaped row sets of every total length 0..64
    for (size_t n = 0; n <= 64; ++n) {
        std::string bytes(n, 'a');
        for (size_t i = 0; i < n; ++i) bytes[i] = (char)(i * 37 + n);
        const uint32_t ends[3] = {(uint32_t)(n / 3), (uint32_t)(n / 3), (uint32_t)n};
        std::string text;
        if (!mrpc::json::EscapeStringRows(bytes.data(), ends, 3, &text)) ++failures;
        const Exact in(text);
        mrpc::json::StringRows got;
        if (mrpc::json::UnescapeStringRows(in.p, in.n, &got) != 0 || got.bytes != bytes ||
            got.row_ends != std::vector<uint32_t>(ends, ends + 3))
            ++failures;
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
