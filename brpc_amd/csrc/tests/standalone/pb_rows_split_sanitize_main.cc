// pb::SplitRows and pb_rows::SpecField (pb/rows.h over base/pb_rows.h) under
// AddressSanitizer and UBSan, as a program of its own: every message sits in a
// heap buffer of exactly its size, where one byte read beyond it is a report,
// and so do the outputs, sized to the element and row counts the message
// holds. SpecField runs at EVERY offset of every message (the device calls it
// so), SplitRows on the whole message, on every prefix of it and on copies
// with one byte changed. Built by hand, on the CPU only, from this file alone
// (the twin is header-only; build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/pb_rows_split_sanitize_main.cc
// Prints "ok" and returns 0 when every job is right.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pb/rows.h"

namespace rows = mrpc::pb_rows;

namespace {

int failures = 0;

// The message in an exact-size heap buffer; outputs of exactly cap elements
// and row_cap rows. Returns the code.
int run(uint32_t number, uint32_t inner, uint32_t kind, const std::string& msg, uint64_t cap, uint64_t row_cap,
        uint64_t* count, uint64_t* nrows) {
    unsigned char* m = static_cast<unsigned char*>(malloc(msg.size()));
    if (!msg.empty()) memcpy(m, msg.data(), msg.size());
    for (size_t p = 0; p <= msg.size(); ++p) {
        const rows::Field f = rows::SpecField(m, p, msg.size());
        if (f.valid && (f.next <= p || f.next > msg.size())) ++failures;
    }
    void* values = malloc((size_t)cap * rows::SourceBytes(kind));
    uint32_t* ends = static_cast<uint32_t*>(malloc((size_t)row_cap * sizeof(uint32_t)));
    uint64_t others = 0, first_bad = 0;
    const int err = mrpc::pb::SplitRows(number, inner, kind, msg.empty() ? nullptr : m, msg.size(), cap ? values : nullptr,
                                        cap, row_cap ? ends : nullptr, row_cap, count, nrows, &others, &first_bad);
    if ((err == 1 || err == 6) != (first_bad < msg.size())) ++failures;
    if (err == 0 && *nrows > 0 && ends[*nrows - 1] != *count) ++failures;
    free(ends);
    free(values);
    free(m);
    return err;
}

}  // namespace

int main() {
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
        for (int round = 0; round < 40; ++round) {
            const size_t count = round < 4 ? (size_t)round / 2 : next() % 120;
            const size_t nrows = 1 + next() % 8;
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
            std::string rows_only, msg;
            if (mrpc::pb::SerializeRows(number, inner, kind, src, count, ends, nrows, &rows_only) != 0) ++failures;
            free(ends);
            free(src);
            // foreign fields in front and behind (another number: number + 1 wraps to 1 at the top)
            const uint32_t other = number == (1u << 29) - 1 ? 1 : number + 1;
            uint8_t head[16];
            uint32_t hn = rows::PutVarint(head, ((uint64_t)other << 3) | 2);
            head[hn++] = 3;
            msg.assign(reinterpret_cast<char*>(head), hn);
            msg += "abc" + rows_only;
            hn = rows::PutVarint(head, ((uint64_t)other << 3) | 5);
            msg.append(reinterpret_cast<char*>(head), hn);
            msg += "wxyz";
            uint64_t c = 0, r = 0;
            if (run(number, inner, kind, msg, count, nrows, &c, &r) != 0 || c != count || r != nrows) ++failures;
            // capacities one short: outputs of exactly that size stay untouched (ASan sees a store beyond them)
            if (count > 0 && run(number, inner, kind, msg, count - 1, nrows, &c, &r) != 5) ++failures;
            if (run(number, inner, kind, msg, count, nrows - 1, &c, &r) != 5) ++failures;
            // every prefix, and one changed byte at a time: any code, no report
            for (size_t cut = 0; cut < msg.size(); ++cut) run(number, inner, kind, msg.substr(0, cut), count, nrows, &c, &r);
            for (size_t i = 0; i < msg.size(); ++i) {
                std::string bad(msg);
                bad[i] = (char)(bad[i] ^ (1u << (next() % 8)));
                run(number, inner, kind, bad, count, nrows, &c, &r);
                bad[i] = (char)next();
                run(number, inner, kind, bad, count, nrows, &c, &r);
            }
        }
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
