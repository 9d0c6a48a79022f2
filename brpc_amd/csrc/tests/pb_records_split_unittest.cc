// pb_records::RecordShape and pb::SplitRecords (base/pb_records.h,
// pb/records.h), the rules and the host twin of gpu::DeviceSplitRecords, and
// the host half of that entry: every rule of a record's walk on hand-built
// records, the twin's codes and their precedence, the code-5 count rule, the
// twin as the inverse of pb::SerializeRecords (also with the fields of every
// record reversed and foreign top-level fields in between), and the checks
// that refuse a job before anything is launched. The device half runs in
// tests/test_gpu_pb_records_split.py on the GPU box.
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/pb_records.h"
#include "gpu/device_codec.h"
#include "pb/records.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

constexpr uint64_t kFill = 0xA5A5A5A5A5A5A5A5ull;

std::string varint(uint64_t v) {
    uint8_t b[10];
    return std::string(reinterpret_cast<char*>(b), pb_rows::PutVarint(b, v));
}
std::string fld(uint32_t number, uint32_t wire, const std::string& payload) {
    return varint(((uint64_t)number << 3) | wire) + (wire == 2 ? varint(payload.size()) : std::string()) + payload;
}
std::string rec(const std::string& sub, uint32_t number = 4) { return fld(number, 2, sub); }

// ids (packed int64, 1), weights (packed float, 2), label (int32, 3), blob (bytes, 4)
const pb_records::SplitColumn kExample[4] = {{1, 3, 0}, {2, pb_rows::kKindFixed32, 0}, {3, 0, 1}, {4, pb_rows::kKindBytes, 0}};

struct Shape {
    int code = 0;
    uint32_t taken = 0;
    uint64_t off[8] = {0}, len[8] = {0};
};
Shape shape(const std::string& sub, const pb_records::SplitColumn* cols = kExample, uint32_t ncols = 4) {
    Shape s;
    // the record alone in a buffer of its size: a read outside it is one outside the buffer
    std::vector<uint8_t> b(sub.begin(), sub.end());
    s.code = pb_records::RecordShape(b.data(), 0, b.size(), cols, ncols, [&](uint32_t c, uint64_t o, uint64_t l) {
        EXPECT_TRUE(!(s.taken >> c & 1));
        s.taken |= 1u << c;
        s.off[c] = o;
        s.len[c] = l;
    });
    return s;
}

struct Split {
    int err = 0;
    pb::SplitRecordsJob job;
    std::vector<pb::SplitRecordsColumn> cols;
    std::vector<std::vector<uint64_t>> values;  // the memory images
    std::vector<std::vector<uint32_t>> ends;
    bool untouched() const {
        for (const auto& v : values) {
            for (uint64_t x : v) {
                if (x != kFill) return false;
            }
        }
        for (const auto& e : ends) {
            for (uint32_t x : e) {
                if (x != (uint32_t)kFill) return false;
            }
        }
        return true;
    }
};

void split(Split* s, uint32_t number, const std::vector<pb_records::SplitColumn>& cols, const std::string& msg,
           uint64_t row_cap, const std::vector<uint64_t>& caps) {
    s->cols.resize(cols.size());
    s->values.resize(cols.size());
    s->ends.resize(cols.size());
    for (size_t c = 0; c < cols.size(); ++c) {
        s->values[c].assign((size_t)caps[c] + 1, kFill);
        s->ends[c].assign((size_t)row_cap + 1, (uint32_t)kFill);
        s->cols[c].inner = cols[c].inner;
        s->cols[c].kind = cols[c].kind;
        s->cols[c].scalar = cols[c].scalar != 0;
        s->cols[c].values = s->values[c].data();
        s->cols[c].cap = caps[c];
        s->cols[c].row_ends = cols[c].scalar ? nullptr : s->ends[c].data();
    }
    s->job.number = number;
    s->job.columns = s->cols.data();
    s->job.ncols = (uint32_t)cols.size();
    s->job.msg = msg.data();
    s->job.n = msg.size();
    s->job.row_cap = row_cap;
    s->err = pb::SplitRecords(&s->job);
}

const std::vector<pb_records::SplitColumn> kExampleCols(kExample, kExample + 4);

void split_example(Split* s, const std::string& msg, uint64_t row_cap = 64, std::vector<uint64_t> caps = {64, 64, 64, 64}) {
    split(s, 4, kExampleCols, msg, row_cap, caps);
}

const std::string kFloat = std::string("\x00\x00\x80\x3f", 4);  // 1.0f
// a good record: ids {7, 300}, weights {1.0}, label 5, blob "ab"
const std::string kGood = rec(fld(1, 2, varint(7) + varint(300)) + fld(2, 2, kFloat) + fld(3, 0, varint(5)) + fld(4, 2, "ab"));
const std::string kLongElem = std::string(10, '\x80') + "\x01";  // a varint of eleven bytes

char g_mem[64] __attribute__((aligned(16)));  // never dereferenced: every device job here is refused

}  // namespace

TEST(PbRecordsSplit, wire_type_of_a_column) {
    for (uint32_t k = 0; k <= 9; ++k) EXPECT_EQ(pb_records::WireType(k, false), 2u);
    for (uint32_t k = 0; k <= 6; ++k) EXPECT_EQ(pb_records::WireType(k, true), 0u);
    EXPECT_EQ(pb_records::WireType(pb_rows::kKindFixed32, true), 5u);
    EXPECT_EQ(pb_records::WireType(pb_rows::kKindFixed64, true), 1u);
}

TEST(PbRecordsSplit, taken_fields_in_any_order) {
    const std::string ids = fld(1, 2, varint(7) + varint(300)), w = fld(2, 2, kFloat), label = fld(3, 0, varint(5)),
                      blob = fld(4, 2, "ab");
    Shape s = shape(ids + w + label + blob);
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 15u);
    EXPECT_EQ(s.off[0], 2u);
    EXPECT_EQ(s.len[0], 3u);
    EXPECT_EQ(s.off[1], ids.size() + 2);
    EXPECT_EQ(s.len[1], 4u);
    EXPECT_EQ(s.off[2], ids.size() + w.size() + 1);  // a scalar: the value's place
    EXPECT_EQ(s.len[2], 1u);
    EXPECT_EQ(s.off[3], ids.size() + w.size() + label.size() + 2);
    EXPECT_EQ(s.len[3], 2u);
    s = shape(blob + label + w + ids);
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 15u);
    EXPECT_EQ(s.off[3], 2u);
    EXPECT_EQ(s.off[2], blob.size() + 1);
    EXPECT_EQ(s.off[0], blob.size() + label.size() + w.size() + 2);
}

TEST(PbRecordsSplit, absent_fields_and_the_empty_record) {
    Shape s = shape("");
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 0u);
    s = shape(fld(3, 0, varint(5)));
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 4u);
    s = shape(fld(4, 2, ""));  // an empty bytes field is taken, with no byte
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 8u);
    EXPECT_EQ(s.len[3], 0u);
}

TEST(PbRecordsSplit, scalar_values_of_every_wire_type) {
    const pb_records::SplitColumn cols[3] = {{1, 5, 1}, {2, pb_rows::kKindFixed32, 1}, {3, pb_rows::kKindFixed64, 1}};
    // the varint's tag is over-long (two bytes): the value's place follows the tag as it is written
    const std::string sub = std::string("\x88\x00", 2) + varint(300) + fld(2, 5, kFloat) + fld(3, 1, std::string(8, '\x11'));
    const Shape s = shape(sub, cols, 3);
    EXPECT_EQ(s.code, 0);
    EXPECT_EQ(s.taken, 7u);
    EXPECT_EQ(s.off[0], 2u);
    EXPECT_EQ(s.len[0], 2u);
    EXPECT_EQ(s.off[1], 5u);
    EXPECT_EQ(s.len[1], 4u);
    EXPECT_EQ(s.off[2], 10u);
    EXPECT_EQ(s.len[2], 8u);
}

TEST(PbRecordsSplit, malformed_records) {
    EXPECT_EQ(shape(fld(3, 0, varint(5)) + varint((9 << 3) | 3)).code, 1);             // wire type 3
    EXPECT_EQ(shape(fld(3, 0, varint(5)) + std::string("\x0a\x05\x01", 3)).code, 1);   // a length past the record
    EXPECT_EQ(shape(std::string("\x18", 1) + kLongElem).code, 1);                      // a scalar of eleven bytes
    EXPECT_EQ(shape(fld(2, 2, std::string(5, '\x01'))).code, 1);                       // 5 bytes of floats
    EXPECT_EQ(shape(fld(1, 2, std::string("\x01\x81", 2))).code, 1);                   // ends inside a varint
    const pb_records::SplitColumn doubles[1] = {{1, pb_rows::kKindFixed64, 0}};
    EXPECT_EQ(shape(fld(1, 2, std::string(12, '\x01')), doubles, 1).code, 1);
    EXPECT_EQ(shape(fld(1, 2, std::string(16, '\x01')), doubles, 1).code, 0);
    // a breach in a taken field is 1 also behind a field that is 6
    EXPECT_EQ(shape(fld(9, 0, varint(1)) + fld(2, 2, std::string(5, '\x01'))).code, 1);
    // RecordShape does not look inside a varint payload: VarintsOk does
    const Shape s = shape(fld(1, 2, kLongElem));
    EXPECT_EQ(s.code, 0);
    uint64_t ne = 0;
    EXPECT_TRUE(!pb_rows::VarintsOk(reinterpret_cast<const uint8_t*>(kLongElem.data()), kLongElem.size(), &ne));
}

TEST(PbRecordsSplit, unsupported_records_keep_their_taken_fields) {
    Shape s = shape(fld(1, 2, varint(7)) + fld(9, 0, varint(1)) + fld(4, 2, "ab"));  // an unknown number
    EXPECT_EQ(s.code, 6);
    EXPECT_EQ(s.taken, 9u);  // the device's table holds both payloads
    s = shape(fld(1, 0, varint(7)));  // the packed field unpacked
    EXPECT_EQ(s.code, 6);
    EXPECT_EQ(s.taken, 0u);
    s = shape(fld(3, 2, "ab"));  // a packed field where the scalar is expected
    EXPECT_EQ(s.code, 6);
    s = shape(fld(3, 5, kFloat));  // another scalar wire type
    EXPECT_EQ(s.code, 6);
    s = shape(fld(1, 2, varint(7)) + fld(1, 2, varint(8)));  // a column twice: the first occurrence is the taken one
    EXPECT_EQ(s.code, 6);
    EXPECT_EQ(s.taken, 1u);
    EXPECT_EQ(s.off[0], 2u);
    s = shape(fld(3, 0, varint(5)) + fld(3, 0, varint(6)));
    EXPECT_EQ(s.code, 6);
    // 6, then something that is no wire: 1
    EXPECT_EQ(shape(fld(9, 0, varint(1)) + varint((9 << 3) | 4)).code, 1);
}

TEST(PbRecordsSplit, the_walk_stays_inside_the_record_and_moves_forward) {
    std::mt19937_64 rng(5);
    const uint8_t likely[] = {0x00, 0x01, 0x02, 0x08, 0x0a, 0x12, 0x18, 0x22, 0x1d, 0x80, 0xff, 0x7f, 0x0b, 0x04};
    int codes[7] = {0};
    for (int round = 0; round < 200000; ++round) {
        const size_t n = rng() % 40;
        std::vector<uint8_t> b(n);  // exactly the record: AddressSanitizer builds see a read beyond it
        for (uint8_t& c : b) c = rng() % 4 ? likely[rng() % sizeof(likely)] : (uint8_t)rng();
        size_t steps = 0;
        const int code = pb_records::RecordShape(b.data(), 0, n, kExample, 4, [&](uint32_t c, uint64_t off, uint64_t len) {
            ++steps;
            ASSERT_TRUE(c < 4 && off <= n && len <= n - off);
        });
        ASSERT_TRUE(code == 0 || code == 1 || code == 6);
        ASSERT_TRUE(steps <= n / 2 && steps <= 4);
        ++codes[code];
    }
    EXPECT_TRUE(codes[0] > 1000 && codes[1] > 1000 && codes[6] > 1000);
}

TEST(PbRecordsSplit, the_example_splits_into_its_columns) {
    const std::string msg = fld(1, 2, "model") + kGood + rec("") + fld(7, 0, varint(3)) + rec(fld(4, 2, "xyz") + fld(1, 2, varint(1)));
    Split s;
    split_example(&s, msg);
    EXPECT_EQ(s.err, 0);
    EXPECT_EQ(s.job.rows, 3u);
    EXPECT_EQ(s.job.others, 2u);
    EXPECT_EQ(s.job.first_bad, ~0ull);
    EXPECT_EQ(s.cols[0].count, 3u);
    EXPECT_EQ(s.cols[1].count, 1u);
    EXPECT_EQ(s.cols[2].count, 3u);
    EXPECT_EQ(s.cols[2].absent, 2u);
    EXPECT_EQ(s.cols[3].count, 5u);
    const uint64_t* ids = s.values[0].data();
    EXPECT_TRUE(ids[0] == 7 && ids[1] == 300 && ids[2] == 1 && ids[3] == kFill);
    const uint32_t* labels = reinterpret_cast<const uint32_t*>(s.values[2].data());
    EXPECT_TRUE(labels[0] == 5 && labels[1] == 0 && labels[2] == 0 && labels[3] == (uint32_t)kFill);
    EXPECT_EQ(memcmp(s.values[3].data(), "abxyz", 5), 0);
    EXPECT_TRUE(s.ends[0][0] == 2 && s.ends[0][1] == 2 && s.ends[0][2] == 3 && s.ends[0][3] == (uint32_t)kFill);
    EXPECT_TRUE(s.ends[1][0] == 1 && s.ends[1][1] == 1 && s.ends[1][2] == 1);
    EXPECT_TRUE(s.ends[3][0] == 2 && s.ends[3][1] == 2 && s.ends[3][2] == 5);
    Split e;
    split_example(&e, "");
    EXPECT_EQ(e.err, 0);
    EXPECT_EQ(e.job.rows, 0u);
    EXPECT_TRUE(e.untouched());
}

TEST(PbRecordsSplit, codes_1_and_6_name_the_lowest_offender_and_write_nothing) {
    const std::string unknown = rec(fld(9, 0, varint(1))), long_elem = rec(fld(1, 2, kLongElem));
    const std::string both = rec(fld(9, 0, varint(1)) + fld(1, 2, kLongElem));
    const struct {
        std::string msg;
        int err;
        uint64_t first_bad;
    } cases[] = {
        {kGood + unknown + kGood, 6, kGood.size()},
        {kGood + long_elem + kGood, 1, kGood.size()},
        {kGood + both + kGood, 1, kGood.size()},  // both 6 and 1 is 1
        {kGood + unknown + kGood + long_elem, 6, kGood.size()},
        {kGood + long_elem + kGood + unknown, 1, kGood.size()},
        {kGood + fld(4, 0, varint(7)) + kGood, 6, kGood.size()},  // `number` with wire type 0
        {kGood + kGood.substr(0, kGood.size() - 1), 1, kGood.size()},  // truncated
        {kGood + unknown + std::string("\x0b", 1), 6, kGood.size()},
        {kGood + std::string("\x0b", 1) + unknown, 1, kGood.size()},
    };
    for (const auto& c : cases) {
        Split s;
        split_example(&s, c.msg);
        EXPECT_EQ(s.err, c.err);
        EXPECT_EQ(s.job.first_bad, c.first_bad);
        EXPECT_TRUE(s.untouched());
        // 1 and 6 win over 5
        Split t;
        split_example(&t, c.msg, 1, {0, 0, 0, 0});
        EXPECT_EQ(t.err, c.err);
        EXPECT_EQ(t.job.first_bad, c.first_bad);
    }
}

TEST(PbRecordsSplit, code_5_and_its_counts) {
    const std::string msg = kGood + kGood + rec("");
    Split s;
    split_example(&s, msg, 3, {4, 2, 3, 4});
    EXPECT_EQ(s.err, 0);
    const uint64_t exact[4] = {4, 2, 3, 4};
    for (int short_col = 0; short_col < 4; ++short_col) {
        std::vector<uint64_t> caps(exact, exact + 4);
        --caps[short_col];
        Split t;
        split_example(&t, msg, 3, caps);
        EXPECT_EQ(t.err, 5);
        EXPECT_EQ(t.job.rows, 3u);
        for (int c = 0; c < 4; ++c) EXPECT_EQ(t.cols[c].count, exact[c]);
        EXPECT_EQ(t.cols[2].absent, 1u);
        EXPECT_TRUE(t.untouched());
    }
    // rows above row_cap: rows is exact, every count is 0
    Split t;
    split_example(&t, msg, 2, {4, 2, 3, 4});
    EXPECT_EQ(t.err, 5);
    EXPECT_EQ(t.job.rows, 3u);
    for (int c = 0; c < 4; ++c) EXPECT_EQ(t.cols[c].count, 0u);
    EXPECT_EQ(t.cols[2].absent, 0u);
    EXPECT_TRUE(t.untouched());
}

TEST(PbRecordsSplit, refusals) {
    const auto code = [](uint32_t number, std::vector<pb_records::SplitColumn> cols) {
        Split s;
        split(&s, number, cols, kGood, 8, std::vector<uint64_t>(cols.size(), 8));
        EXPECT_TRUE(s.err == 0 || s.untouched());
        return s.err;
    };
    EXPECT_EQ(code(4, kExampleCols), 0);
    EXPECT_EQ(code(0, kExampleCols), 2);
    EXPECT_EQ(code(1u << 29, kExampleCols), 2);
    EXPECT_EQ(code(4, {{0, 3, 0}}), 2);
    EXPECT_EQ(code(4, {{1u << 29, 3, 0}}), 2);
    EXPECT_EQ(code(4, {{1, 10, 0}}), 2);
    EXPECT_EQ(code(4, {{1, pb_rows::kKindBytes, 1}}), 2);
    EXPECT_EQ(code(4, {}), 2);
    EXPECT_EQ(code(4, std::vector<pb_records::SplitColumn>(9, pb_records::SplitColumn{1, 0, 1})), 2);
    EXPECT_EQ(code(4, {{1, 3, 0}, {2, 0, 1}, {1, pb_rows::kKindFixed32, 0}}), 2);  // a duplicate inner
    EXPECT_EQ(code(4, {{3, 0, 1}, {3, 0, 0}}), 2);                                   // one number, two wire forms
    Split s;
    split_example(&s, kGood);
    s.job.msg = nullptr;
    EXPECT_EQ(pb::SplitRecords(&s.job), 2);
    s.job.msg = kGood.data();
    s.cols[0].values = nullptr;
    EXPECT_EQ(pb::SplitRecords(&s.job), 2);
    s.cols[0].values = s.values[0].data();
    s.cols[3].row_ends = nullptr;
    EXPECT_EQ(pb::SplitRecords(&s.job), 2);
    s.cols[3].row_ends = s.ends[3].data();
    s.job.n = 1ull << 32;
    EXPECT_EQ(pb::SplitRecords(&s.job), 2);
    s.job.n = kGood.size();
    EXPECT_EQ(pb::SplitRecords(&s.job), 0);
}

namespace {

// The records of a canonical message with the fields of every record in
// reverse order, and foreign top-level fields of every wire type in between.
std::string reversed_and_interleaved(const std::string& msg, uint32_t number, uint64_t* foreign) {
    // numbers no job here uses for its records
    const std::string others[4] = {fld(3000, 0, varint(300)), fld(3001, 1, std::string(8, '\x01')), fld(3002, 2, "model-7"),
                                   fld(3003, 5, std::string(4, '\xff'))};
    const uint8_t* b = reinterpret_cast<const uint8_t*>(msg.data());
    std::string out;
    *foreign = 0;
    for (uint64_t p = 0, r = 0; p < msg.size(); ++r) {
        const pb_rows::Field f = pb_rows::SpecField(b, p, msg.size());
        std::string sub;
        for (uint64_t q = f.vpos; q < f.vpos + f.vlen;) {
            const pb_rows::Field g = pb_rows::SpecField(b, q, f.vpos + f.vlen);
            sub.insert(0, msg.substr(q, g.next - q));
            q = g.next;
        }
        if (r % 3 != 1) {
            out += others[r % 4];
            ++*foreign;
        }
        out += rec(sub, number);
        p = f.next;
    }
    out += others[2];
    ++*foreign;
    return out;
}

}  // namespace

TEST(PbRecordsSplit, round_trip_with_the_serializer_for_every_kind_and_column_count) {
    std::mt19937_64 rng(29);
    const uint32_t numbers[] = {1, 15, 16, 2047, 2048, (1u << 29) - 1};
    bool ragged_seen[10] = {false}, scalar_seen[10] = {false};
    for (int round = 0; round < 400; ++round) {
        const uint32_t ncols = 1 + round % 8;
        const uint64_t rows = 1 + rng() % 20;
        std::vector<std::vector<uint64_t>> src(ncols);
        std::vector<std::vector<uint32_t>> ends(ncols);
        std::vector<pb_records::Column> cols(ncols);
        std::vector<pb_records::SplitColumn> specs(ncols);
        for (uint32_t c = 0; c < ncols; ++c) {
            const uint32_t kind = (uint32_t)((round / 8 + c * 3) % 10);
            const bool scalar = kind != pb_rows::kKindBytes && rng() % 3 == 0;
            (scalar ? scalar_seen : ragged_seen)[kind] = true;
            const uint32_t eb = pb_rows::SourceBytes(kind);
            const uint64_t count = scalar ? rows : rng() % 200;
            src[c].assign((size_t)(count * eb + 7) / 8 + 1, 0);
            uint8_t* bytes = reinterpret_cast<uint8_t*>(src[c].data());
            for (uint64_t i = 0; i < count; ++i) {
                uint64_t v = rng() >> (rng() % 64);
                if (rng() % 4 == 0) v = ~v;
                if (kind == pb_rows::kKindBool) v &= 1;  // what a split gives back
                memcpy(bytes + i * eb, &v, eb);
            }
            if (!scalar) {
                uint64_t at = 0;
                for (uint64_t r = 0; r + 1 < rows; ++r) {
                    if (rng() % 3) at += rng() % (count - at + 1);
                    ends[c].push_back((uint32_t)at);
                }
                ends[c].push_back((uint32_t)count);
            }
            cols[c].inner = specs[c].inner = c + 1 + (c % 2 ? 2000 : 0);  // distinct; tags of one and two bytes
            cols[c].kind = specs[c].kind = kind;
            cols[c].src = src[c].data();
            cols[c].count = count;
            cols[c].row_ends = scalar ? nullptr : ends[c].data();
            specs[c].scalar = scalar;
        }
        pb_records::Job job;
        job.number = numbers[rng() % 6];
        job.columns = cols.data();
        job.ncols = ncols;
        job.rows = rows;
        std::string wire;
        ASSERT_TRUE(pb::SerializeRecords(job, &wire) == 0);
        uint64_t foreign = 0;
        const std::string shuffled = reversed_and_interleaved(wire, job.number, &foreign);
        for (int form = 0; form < 2; ++form) {
            std::vector<uint64_t> caps(ncols);
            for (uint32_t c = 0; c < ncols; ++c) caps[c] = cols[c].count;
            Split s;
            split(&s, job.number, specs, form ? shuffled : wire, rows, caps);  // exact capacities
            ASSERT_EQ(s.err, 0);
            EXPECT_EQ(s.job.rows, rows);
            EXPECT_EQ(s.job.others, form ? foreign : 0);
            std::vector<pb_records::Column> back(cols);
            for (uint32_t c = 0; c < ncols; ++c) {
                EXPECT_EQ(s.cols[c].count, cols[c].count);
                EXPECT_EQ(s.cols[c].absent, 0u);
                EXPECT_EQ(memcmp(s.values[c].data(), src[c].data(), (size_t)cols[c].count * pb_rows::SourceBytes(cols[c].kind)), 0);
                EXPECT_EQ(s.values[c][(size_t)(cols[c].count * pb_rows::SourceBytes(cols[c].kind) + 7) / 8], kFill);
                back[c].src = s.values[c].data();
                if (cols[c].row_ends) {
                    EXPECT_EQ(memcmp(s.ends[c].data(), ends[c].data(), (size_t)rows * 4), 0);
                    EXPECT_EQ(s.ends[c][(size_t)rows], (uint32_t)kFill);
                    back[c].row_ends = s.ends[c].data();
                }
            }
            job.columns = back.data();
            std::string again;
            ASSERT_TRUE(pb::SerializeRecords(job, &again) == 0);
            EXPECT_TRUE(again == wire);
            job.columns = cols.data();
        }
    }
    for (uint32_t k = 0; k <= 9; ++k) {
        EXPECT_TRUE(ragged_seen[k]);
        EXPECT_TRUE(scalar_seen[k] || k == pb_rows::kKindBytes);
    }
}

TEST(PbRecordsSplit, device_entry_refuses_before_any_launch) {
    gpu::DeviceRecordSplitColumn cols[9];
    for (int c = 0; c < 9; ++c) {
        cols[c].inner = (uint32_t)c + 1;
        cols[c].kind = 3;
        cols[c].values = g_mem;
        cols[c].cap = 4;
        cols[c].row_ends = reinterpret_cast<uint32_t*>(g_mem);
    }
    const auto code = [&](void (*change)(gpu::DeviceRecordsSplitJob*)) {
        gpu::DeviceRecordsSplitJob j;
        j.number = 4;
        j.columns = cols;
        j.ncols = 2;
        j.msg = g_mem;
        j.n = 8;
        j.row_cap = 4;
        change(&j);
        EXPECT_EQ(gpu::DeviceSplitRecords(&j, 1, 0), 0);
        return j.err;
    };
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->number = 0; }), 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->ncols = 0; }), 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->ncols = 9; }), 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->columns = nullptr; }), 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->msg = nullptr; }), 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) { j->n = gpu::kDeviceSplitMaxBytes + 1; }), 2);
    // min(row_cap, n / 2) * ncols entries of 8 bytes above 256 MiB
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) {
                  j->ncols = 8;
                  j->n = 16 << 20;
                  j->row_cap = 8 << 20;
              }),
              2);
    cols[1].inner = 1;  // a duplicate
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob*) {}), 2);
    cols[1].inner = 2;
    cols[1].values = g_mem + 4;  // misaligned for int64
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob*) {}), 2);
    cols[1].values = g_mem;
    cols[1].row_ends = reinterpret_cast<uint32_t*>(g_mem + 2);
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob*) {}), 2);
    cols[1].row_ends = nullptr;
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob*) {}), 2);
    cols[1].kind = pb_rows::kKindBytes;
    cols[1].scalar = true;
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob*) {}), 2);
    // an empty message is code 0 without a launch
    cols[1].kind = 0;
    EXPECT_EQ(code([](gpu::DeviceRecordsSplitJob* j) {
                  j->n = 0;
                  j->msg = nullptr;
              }),
              0);
}
