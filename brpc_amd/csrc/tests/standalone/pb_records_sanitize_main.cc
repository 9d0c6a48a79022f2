// pb::SerializeRecords (pb/records.h over base/pb_records.h) under
// AddressSanitizer and UBSan, as a program of its own: columns of every kind
// and form, sources and row tables in heap buffers of exactly their size,
// where one element too many is a report, the output checked against the
// worst-case size the header rules promise, and bad tables walked to their
// verdict. Built by hand, on the CPU only, from this file alone (the twin is
// header-only; build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/pb_records_sanitize_main.cc
// Prints "ok" and returns 0 when every job is right.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pb/records.h"

namespace rows = mrpc::pb_rows;
namespace records = mrpc::pb_records;

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
    for (int round = 0; round < 2000; ++round) {
        const size_t nrows = 1 + next() % 24;
        const uint32_t ncols = 1 + (uint32_t)(next() % records::kRecordMaxColumns);
        records::Column cols[records::kRecordMaxColumns];
        void* owned[2 * records::kRecordMaxColumns];
        size_t nowned = 0;
        for (uint32_t c = 0; c < ncols; ++c) {
            const uint32_t kind = (uint32_t)((round + c) % 10);
            const bool scalar = kind != rows::kKindBytes && next() % 3 == 0;
            const uint32_t eb = rows::SourceBytes(kind);
            const size_t count = scalar ? nrows : (next() % 5 == 0 ? 0 : next() % 300);
            // exact-size heap buffers: malloc(0) may be null, which is fine for count 0
            unsigned char* src = static_cast<unsigned char*>(malloc(count * eb));
            for (size_t i = 0; i < count; ++i) {
                uint64_t v = next() >> (next() % 64);
                if (next() % 4 == 0) v = ~v;
                memcpy(src + i * eb, &v, eb);
            }
            owned[nowned++] = src;
            uint32_t* ends = nullptr;
            if (!scalar) {
                ends = static_cast<uint32_t*>(malloc(nrows * sizeof(uint32_t)));
                uint64_t at = 0;
                for (size_t r = 0; r + 1 < nrows; ++r) {
                    if (next() % 3) at += next() % (count - at + 1);
                    ends[r] = (uint32_t)at;
                }
                ends[nrows - 1] = (uint32_t)count;
                owned[nowned++] = ends;
            }
            cols[c].inner = numbers[next() % 6];
            cols[c].kind = kind;
            cols[c].src = src;
            cols[c].count = count;
            cols[c].row_ends = ends;
        }
        records::Job job;
        job.number = numbers[next() % 6];
        job.columns = cols;
        job.ncols = ncols;
        job.rows = nrows;
        std::string out;
        uint32_t bad = 0, col = 0;
        const int rc = mrpc::pb::SerializeRecords(job, &out, &bad, &col);
        const uint64_t worst = records::WorstCaseBytes(job);
        if (rc != 0 || worst == 0 || out.size() > worst || out.size() < 2 * nrows) {
            fprintf(stderr, "round %d: rc %d, %zu bytes, worst case %llu\n", round, rc, out.size(),
                    (unsigned long long)worst);
            ++failures;
        }
        // the same job with one table broken: the verdict names that row and column, nothing is appended
        uint32_t victim = ncols;
        for (uint32_t c = 0; c < ncols; ++c) {
            if (cols[c].row_ends && nrows >= 2 && cols[c].count > 0) victim = c;
        }
        if (victim < ncols) {
            uint32_t* ends = const_cast<uint32_t*>(cols[victim].row_ends);
            const size_t r = 1 + next() % (nrows - 1);
            // the first row at which a table that ends at count > 0 is above 0 exists; break at or after it
            size_t first = 0;
            while (ends[first] == 0) ++first;
            const size_t at = r > first ? r : first + (first + 1 < nrows ? 1 : 0);
            if (at > first) {
                ends[at] = ends[at - 1] - 1;
                std::string none;
                const int rc2 = mrpc::pb::SerializeRecords(job, &none, &bad, &col);
                if (rc2 != 1 || bad != at || col != victim || !none.empty()) {
                    fprintf(stderr, "round %d: broken table: rc %d, row %u (want %zu), column %u (want %u)\n", round, rc2,
                            bad, at, col, victim);
                    ++failures;
                }
            }
        }
        for (size_t i = 0; i < nowned; ++i) free(owned[i]);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
