// json::FormatNumberRows under AddressSanitizer and UBSan, as a program of
// its own: the twin formats into the tail of a growing string and negates
// INT64_MIN's magnitude, so every count 0..64 of every kind goes through it
// from heap buffers of exactly its size (values and row ends), where one byte
// too many is a report, with the widest elements of each kind among them.
// Built by hand, on the CPU only, from this file and json/json.cc alone
// (build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/number_print_sanitize_main.cc
//       brpc_amd/csrc/json/json.cc -lpthread
// Prints "ok" and returns 0 when every result is right.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "base/number_print.h"
#include "json/json.h"

namespace {

namespace np = mrpc::number_print;

// n bytes in a heap buffer of exactly n (malloc aligns it for any element)
struct Exact {
    char* p;
    explicit Exact(const std::string& s) : p(static_cast<char*>(malloc(s.size() ? s.size() : 1))) {
        if (!s.empty()) memcpy(p, s.data(), s.size());
    }
    ~Exact() { free(p); }
};

// Bit patterns that print widest, and some that print short.
const uint64_t kPatterns[] = {0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, 0x7FFFFFFFFFFFFFFFull, 0x80000000ull,
                              0xFFFFFFFF80000000ull, 0,                     1,                     0x8010000000000001ull,
                              0xFFF0000000000000ull, 0x7FF8000000000000ull, 0xFF800000FF800000ull, 0x80000001807FFFFFull,
                              0xC1E0000000000000ull, 0x3FB999999999999Aull};

}  // namespace

int main() {
    int failures = 0;
    const uint32_t kinds[] = {0, 1, 2, 3, 4, 5, 6, 8, 9};
    for (uint32_t kind : kinds) {
        const size_t eb = np::ElemBytes(kind);
        for (size_t n = 0; n <= 64; ++n) {
            std::string image(n * eb, '\0');
            for (size_t i = 0; i < n; ++i) {
                const uint64_t v = kPatterns[(i + n) % (sizeof(kPatterns) / sizeof(kPatterns[0]))];
                memcpy(&image[i * eb], &v, eb);
            }
            const Exact values(image);
            // rows of 1, 2, 3, 1, 2, 3, ... elements
            std::vector<uint32_t> ends;
            for (uint32_t at = 0, k = 0; at < n; ++k) {
                at += 1 + k % 3;
                ends.push_back(at < n ? at : (uint32_t)n);
            }
            const Exact table(std::string(reinterpret_cast<const char*>(ends.data()), ends.size() * 4));
            const uint32_t* row_ends = reinterpret_cast<const uint32_t*>(table.p);
            std::string flat, bracketed, nested;
            uint32_t first_bad = 0;
            if (mrpc::json::FormatNumberRows(values.p, n, kind, nullptr, 0, false, &flat, &first_bad) != 0) ++failures;
            if (mrpc::json::FormatNumberRows(values.p, n, kind, nullptr, 0, true, &bracketed, &first_bad) != 0) ++failures;
            if (bracketed != "[" + flat + "]") ++failures;
            if (flat.size() + 2 > np::WorstCaseBytes(kind, n, 0)) ++failures;
            if (n == 0) continue;
            if (mrpc::json::FormatNumberRows(values.p, n, kind, row_ends, ends.size(), false, &nested, &first_bad) != 0 ||
                first_bad != np::kNone)
                ++failures;
            if (nested.size() != flat.size() + 2 * ends.size() + 2 || nested.size() > np::WorstCaseBytes(kind, n, ends.size()))
                ++failures;
            // without its row punctuation the nested text is the bracketed one
            std::string joined;
            for (size_t i = 1; i + 1 < nested.size(); ++i) {
                if (nested.compare(i, 3, "],[") == 0) {
                    joined += ',';
                    i += 2;
                } else if (nested[i] != '[' && nested[i] != ']') {
                    joined += nested[i];
                }
            }
            if (joined != flat) ++failures;
            // a table cut short, and one whose last end is off by one: refused where they break
            if (ends.size() > 1) {
                std::string kept = "kept";
                if (mrpc::json::FormatNumberRows(values.p, n, kind, row_ends, ends.size() - 1, true, &kept, &first_bad) != 1 ||
                    first_bad != ends.size() - 2 || kept != "kept")
                    ++failures;
            }
            if (mrpc::json::FormatNumberRows(values.p, n - 1, kind, row_ends, ends.size(), true, &nested, &first_bad) != 1 ||
                first_bad != ends.size() - 1)
                ++failures;
        }
    }
    // the extremes by name
    const int64_t i64[] = {INT64_MIN, INT64_MAX};
    const int32_t i32[] = {INT32_MIN, INT32_MAX};
    const uint64_t u64[] = {UINT64_MAX, 10000000000000000000ull, 9999999999999999999ull};
    std::string s;
    if (mrpc::json::FormatNumberRows(i64, 2, 5, nullptr, 0, false, &s) != 0 || s != "-9223372036854775808,9223372036854775807")
        ++failures;
    s.clear();
    if (mrpc::json::FormatNumberRows(i32, 2, 2, nullptr, 0, false, &s) != 0 || s != "-2147483648,2147483647") ++failures;
    s.clear();
    if (mrpc::json::FormatNumberRows(u64, 3, 4, nullptr, 0, true, &s) != 0 ||
        s != "[18446744073709551615,10000000000000000000,9999999999999999999]")
        ++failures;
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
