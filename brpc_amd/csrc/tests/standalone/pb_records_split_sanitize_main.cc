// pb::SplitRecords and pb_records::RecordShape (pb/records.h over
// base/pb_records.h) under AddressSanitizer and UBSan, as a program of its
// own: records of every kind and form serialized by pb::SerializeRecords,
// then split from a heap buffer of exactly the message's size into values and
// row ends in heap buffers of exactly their counts, where one byte read or
// one element written too many is a report. The same message is split again
// with every capacity short by one (nothing may be written), from every
// prefix of it, and from copies with one byte changed (any code, no report).
// Built by hand, on the CPU only, from this file alone (the twin is
// header-only; build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/pb_records_split_sanitize_main.cc
// Prints "ok" and returns 0 when every job is right.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pb/records.h"

namespace rows = mrpc::pb_rows;
namespace records = mrpc::pb_records;

namespace {

struct Outputs {
    mrpc::pb::SplitRecordsColumn cols[records::kRecordMaxColumns];
    void* owned[2 * records::kRecordMaxColumns + 1];
    size_t nowned = 0;
    mrpc::pb::SplitRecordsJob job;
    ~Outputs() {
        for (size_t i = 0; i < nowned; ++i) free(owned[i]);
    }
};

// The job with its message and every output in a heap buffer of exactly its size.
void make(Outputs* o, uint32_t number, const records::Column* src, uint32_t ncols, const std::string& msg, uint64_t row_cap,
          const uint64_t* caps) {
    void* m = malloc(msg.size());
    if (!msg.empty()) memcpy(m, msg.data(), msg.size());
    o->owned[o->nowned++] = m;
    for (uint32_t c = 0; c < ncols; ++c) {
        mrpc::pb::SplitRecordsColumn& col = o->cols[c];
        col.inner = src[c].inner;
        col.kind = src[c].kind;
        col.scalar = src[c].row_ends == nullptr;
        col.cap = caps[c];
        col.values = malloc((size_t)caps[c] * rows::SourceBytes(col.kind));
        o->owned[o->nowned++] = col.values;
        if (!col.scalar) {
            col.row_ends = static_cast<uint32_t*>(malloc((size_t)row_cap * sizeof(uint32_t)));
            o->owned[o->nowned++] = col.row_ends;
        }
    }
    o->job.number = number;
    o->job.columns = o->cols;
    o->job.ncols = ncols;
    o->job.msg = msg.empty() ? nullptr : m;
    o->job.n = msg.size();
    o->job.row_cap = row_cap;
}

}  // namespace

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
    for (int round = 0; round < 600; ++round) {
        const size_t nrows = 1 + next() % 12;
        const uint32_t ncols = 1 + (uint32_t)(next() % records::kRecordMaxColumns);
        records::Column cols[records::kRecordMaxColumns];
        void* owned[2 * records::kRecordMaxColumns];
        size_t nowned = 0;
        for (uint32_t c = 0; c < ncols; ++c) {
            const uint32_t kind = (uint32_t)((round + c) % 10);
            const bool scalar = kind != rows::kKindBytes && next() % 3 == 0;
            const uint32_t eb = rows::SourceBytes(kind);
            const size_t count = scalar ? nrows : (next() % 5 == 0 ? 0 : next() % 60);
            unsigned char* src = static_cast<unsigned char*>(malloc(count * eb + 1));
            for (size_t i = 0; i < count; ++i) {
                uint64_t v = next() >> (next() % 64);
                if (next() % 4 == 0) v = ~v;
                if (kind == rows::kKindBool) v &= 1;
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
            cols[c].inner = c < 6 ? numbers[c] : 100 + c;  // distinct
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
        std::string msg;
        if (mrpc::pb::SerializeRecords(job, &msg) != 0) {
            fprintf(stderr, "round %d: the serializer refused the job\n", round);
            return 1;
        }
        uint64_t caps[records::kRecordMaxColumns];
        for (uint32_t c = 0; c < ncols; ++c) caps[c] = cols[c].count;
        {
            Outputs o;  // exact sizes: the columns come back
            make(&o, job.number, cols, ncols, msg, nrows, caps);
            const int rc = mrpc::pb::SplitRecords(&o.job);
            bool same = rc == 0 && o.job.rows == nrows;
            for (uint32_t c = 0; c < ncols && same; ++c) {
                same = o.cols[c].count == cols[c].count &&
                       memcmp(o.cols[c].values, cols[c].src, (size_t)cols[c].count * rows::SourceBytes(cols[c].kind)) == 0 &&
                       (!cols[c].row_ends || memcmp(o.cols[c].row_ends, cols[c].row_ends, nrows * sizeof(uint32_t)) == 0);
            }
            if (!same) {
                fprintf(stderr, "round %d: rc %d, the columns did not come back\n", round, rc);
                ++failures;
            }
        }
        for (uint32_t c = 0; c <= ncols; ++c) {  // one capacity short by one: code 5, and no store (the buffers are exact)
            uint64_t less[records::kRecordMaxColumns];
            memcpy(less, caps, sizeof(caps));
            if (c < ncols && less[c] == 0) continue;
            if (c < ncols) --less[c];
            Outputs o;
            make(&o, job.number, cols, ncols, msg, c < ncols ? nrows : nrows - 1, less);
            const int rc = mrpc::pb::SplitRecords(&o.job);
            if (rc != rows::kSplitShort || o.job.rows != nrows) {
                fprintf(stderr, "round %d: short capacity %u: rc %d\n", round, c, rc);
                ++failures;
            }
        }
        for (size_t cut = 0; cut < msg.size(); cut += 1 + next() % 3) {  // every few prefixes
            Outputs o;
            make(&o, job.number, cols, ncols, msg.substr(0, cut), nrows, caps);
            const int rc = mrpc::pb::SplitRecords(&o.job);
            if (rc != 0 && rc != rows::kSplitMalformed) {
                fprintf(stderr, "round %d: prefix %zu: rc %d\n", round, cut, rc);
                ++failures;
            }
        }
        for (int k = 0; k < 40 && !msg.empty(); ++k) {  // one byte changed: any verdict, outputs of the same exact sizes
            std::string bent = msg;
            bent[next() % bent.size()] = (char)next();
            Outputs o;
            make(&o, job.number, cols, ncols, bent, nrows, caps);
            const int rc = mrpc::pb::SplitRecords(&o.job);
            if (rc != 0 && rc != rows::kSplitMalformed && rc != rows::kSplitShort && rc != rows::kSplitUnsupported) {
                fprintf(stderr, "round %d: changed byte: rc %d\n", round, rc);
                ++failures;
            }
        }
        for (size_t i = 0; i < nowned; ++i) free(owned[i]);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
