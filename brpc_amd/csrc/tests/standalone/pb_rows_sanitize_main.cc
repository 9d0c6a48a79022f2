// pb::SerializeRows (pb/rows.h over base/pb_rows.h) under AddressSanitizer
// and UBSan, as a program of its own: every kind, sources and row tables in
// heap buffers of exactly their size, where one element too many is a report,
// and the output checked against the sizes the header rules promise. Built by
// hand, on the CPU only, from this file alone (the twin is header-only;
// build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/pb_rows_sanitize_main.cc
// Prints "ok" and returns 0 when every job is right.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pb/rows.h"

namespace rows = mrpc::pb_rows;

int main() {
    int failures = 0;
    uint64_t seed = 88172645463325252ull;
    auto next = [&seed]() {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return seed;
    };
    const uint32_t numbers[] = {1, 15, 16, 2047, 2048, (1u << 29) - 1};
    for (uint32_t kind = 0; kind <= 9; ++kind) {
        const uint32_t eb = rows::SourceBytes(kind);
        for (int round = 0; round < 200; ++round) {
            const size_t count = round < 4 ? (size_t)round / 2 : next() % 700;
            const size_t nrows = 1 + next() % 24;
            // exact-size heap buffers: malloc(0) may be null, which is fine for count 0
            unsigned char* src = static_cast<unsigned char*>(malloc(count * eb));
            for (size_t i = 0; i < count; ++i) {
                uint64_t v = next() >> (next() % 64);
                if (next() % 4 == 0) v = ~v;
                memcpy(src + i * eb, &v, eb);
            }
            uint32_t* ends = static_cast<uint32_t*>(malloc(nrows * sizeof(uint32_t)));
            uint32_t at = 0;
            for (size_t r = 0; r < nrows; ++r) {
                if (next() % 3) at += (uint32_t)(next() % (count - at + 1));
                ends[r] = r + 1 == nrows ? (uint32_t)count : at;
            }
            const uint32_t number = numbers[next() % 6];
            const uint32_t inner = kind == 7 && round % 2 ? 0 : numbers[next() % 6];
            std::string out;
            uint32_t first_bad = 0;
            const int err = mrpc::pb::SerializeRows(number, inner, kind, src, count, ends, nrows, &out, &first_bad);
            if (err != 0 || first_bad != 0xFFFFFFFFu) ++failures;
            if (out.size() > rows::WorstCaseBytes(number, inner, kind, count, nrows)) ++failures;
            if (out.size() < 2 * nrows || (uint8_t)out[0] != (uint8_t)(((number << 3) | 2) & 0x7f) +
                                                                 (number >= 16 ? 0x80 : 0)) {
                ++failures;
            }
            // a table that decreases, and one that ends elsewhere: reported, nothing appended
            if (nrows >= 2 && ends[nrows - 2] > 0) {
                ends[nrows - 1] = ends[nrows - 2] - 1;
                const size_t before = out.size();
                if (mrpc::pb::SerializeRows(number, inner, kind, src, count, ends, nrows, &out, &first_bad) != 1 ||
                    first_bad != nrows - 1 || out.size() != before) {
                    ++failures;
                }
            }
            ends[nrows - 1] = (uint32_t)count + 1;
            if (mrpc::pb::SerializeRows(number, inner, kind, src, count, ends, nrows, &out, &first_bad) != 1) ++failures;
            free(ends);
            free(src);
        }
    }
    // the largest header, into a buffer of exactly its size
    uint8_t* head = static_cast<uint8_t*>(malloc(rows::kMaxHeaderBytes));
    if (rows::PutHeader(head, (1u << 29) - 1, (1u << 29) - 1, 7, 1, 0xFFFFFF00ull) != rows::kMaxHeaderBytes) ++failures;
    free(head);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
