// pb::SerializeRecords (pb/records.h), the host twin of
// gpu::DeviceBuildRecords, and the host half of that entry: the twin against
// a serializer written byte by byte here, against pb::SerializeRows for a job
// of one column and against pb::Message's own serialization of a .proto
// parsed at run time; the offender it names in a bad table, the worst-case
// size a caller allocates from, and the checks that refuse a job before
// anything is launched. The device half runs in tests/test_gpu_pb_records.py
// on the GPU box.
#include <algorithm>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "base/buf.h"
#include "base/pb_records.h"
#include "gpu/device_codec.h"
#include "gpu/kernels.h"
#include "pb/dynamic.h"
#include "pb/parser.h"
#include "pb/records.h"
#include "pb/rows.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

void put_varint(std::string* o, uint64_t v) {
    while (v >= 0x80) {
        o->push_back((char)(v | 0x80));
        v >>= 7;
    }
    o->push_back((char)v);
}

uint32_t source_bytes(uint32_t kind) { return kind == 6 || kind == 7 ? 1 : (kind <= 2 || kind == 8 ? 4 : 8); }

// One element on the wire, by the protobuf encoding rules alone.
void put_element(std::string* o, uint32_t kind, const char* src, uint64_t i) {
    uint64_t v = 0;
    memcpy(&v, src + source_bytes(kind) * i, source_bytes(kind));
    switch (kind) {
    case 0: put_varint(o, (uint64_t)(int64_t)(int32_t)v); break;
    case 1: put_varint(o, (uint32_t)v); break;
    case 2: put_varint(o, ((uint32_t)v << 1) ^ (uint32_t)((int32_t)v >> 31)); break;
    case 3:
    case 4: put_varint(o, v); break;
    case 5: put_varint(o, (v << 1) ^ (uint64_t)((int64_t)v >> 63)); break;
    case 6: o->push_back(v ? 1 : 0); break;
    default: o->append(src + source_bytes(kind) * i, source_bytes(kind)); break;
    }
}

struct TestColumn {
    uint32_t inner = 0, kind = 0;
    std::vector<uint64_t> mem;  // the elements, aligned
    uint64_t count = 0;
    std::vector<uint32_t> ends;  // empty: scalar
    bool scalar = false;
};

std::string by_hand(uint32_t number, const std::vector<TestColumn>& cols, uint64_t rows) {
    std::string out;
    for (uint64_t r = 0; r < rows; ++r) {
        std::string sub;
        for (const TestColumn& c : cols) {
            const char* src = reinterpret_cast<const char*>(c.mem.data());
            if (c.scalar) {
                put_varint(&sub, ((uint64_t)c.inner << 3) | (c.kind <= 6 ? 0 : (c.kind == 8 ? 5 : 1)));
                put_element(&sub, c.kind, src, r);
                continue;
            }
            std::string p;
            for (uint64_t i = r ? c.ends[r - 1] : 0; i < c.ends[r]; ++i) put_element(&p, c.kind, src, i);
            if (p.empty() && c.kind != 7) continue;
            put_varint(&sub, ((uint64_t)c.inner << 3) | 2);
            put_varint(&sub, p.size());
            sub += p;
        }
        put_varint(&out, ((uint64_t)number << 3) | 2);
        put_varint(&out, sub.size());
        out += sub;
    }
    return out;
}

std::vector<uint64_t> random_source(std::mt19937_64& rng, uint32_t kind, size_t count) {
    std::vector<uint64_t> mem(count * source_bytes(kind) / 8 + 1);
    char* p = reinterpret_cast<char*>(mem.data());
    for (size_t i = 0; i < count; ++i) {
        uint64_t v = rng() >> (rng() % 64);
        if (rng() % 4 == 0) v = ~v;  // negative ones
        memcpy(p + i * source_bytes(kind), &v, source_bytes(kind));
    }
    return mem;
}

std::vector<uint32_t> random_ends(std::mt19937_64& rng, size_t count, size_t rows) {
    std::vector<uint32_t> ends(rows);
    for (size_t r = 0; r + 1 < rows; ++r) ends[r] = (uint32_t)(rng() % (count + 1));
    ends[rows - 1] = (uint32_t)count;
    std::sort(ends.begin(), ends.end());
    return ends;
}

TestColumn random_column(std::mt19937_64& rng, uint32_t inner, uint32_t kind, bool scalar, size_t rows) {
    TestColumn c;
    c.inner = inner;
    c.kind = kind;
    c.scalar = scalar;
    c.count = scalar ? rows : (rng() % 5 == 0 ? 0 : rng() % 600);
    c.mem = random_source(rng, kind, c.count);
    if (!scalar) c.ends = random_ends(rng, c.count, rows);
    return c;
}

struct View {
    std::vector<pb_records::Column> cols;
    pb_records::Job job;
};
void make_view(uint32_t number, const std::vector<TestColumn>& cols, uint64_t rows, View* v) {
    v->cols.resize(cols.size());
    for (size_t i = 0; i < cols.size(); ++i) {
        v->cols[i].inner = cols[i].inner;
        v->cols[i].kind = cols[i].kind;
        v->cols[i].src = cols[i].mem.data();
        v->cols[i].count = cols[i].count;
        v->cols[i].row_ends = cols[i].scalar ? nullptr : cols[i].ends.data();
    }
    v->job.number = number;
    v->job.columns = v->cols.data();
    v->job.ncols = (uint32_t)cols.size();
    v->job.rows = rows;
}

char g_mem[64] __attribute__((aligned(16)));  // never dereferenced: every device job here is refused

struct DeviceJob {
    gpu::DeviceRecordColumn cols[9];
    gpu::DeviceRecordsJob job;
};
// Two packed float columns and a scalar int32 one over 4 records: accepted.
void good_job(DeviceJob* d) {
    for (int c = 0; c < 9; ++c) {
        d->cols[c].inner = (uint32_t)c + 1;
        d->cols[c].kind = 8;
        d->cols[c].src = g_mem;
        d->cols[c].count = 4;
        d->cols[c].row_ends = reinterpret_cast<const uint32_t*>(g_mem);
    }
    d->cols[2].kind = 0;
    d->cols[2].row_ends = nullptr;
    d->job = gpu::DeviceRecordsJob();
    d->job.number = 4;
    d->job.columns = d->cols;
    d->job.ncols = 3;
    d->job.rows = 4;
    d->job.dst = g_mem;
    d->job.cap = 1 << 20;
}

int build_code(DeviceJob* d) {
    d->job.err = -1;
    EXPECT_EQ(gpu::DeviceBuildRecords(&d->job, 1, 0), 0);
    return d->job.err;
}

}  // namespace

TEST(PbRecords, twin_equals_a_byte_by_byte_serializer_for_every_kind_and_shape) {
    std::mt19937_64 rng(20240917);
    const uint32_t numbers[] = {1, 15, 16, 2047, 2048, (1u << 29) - 1};
    for (int round = 0; round < 300; ++round) {
        const size_t rows = 1 + rng() % 40;
        const size_t ncols = 1 + rng() % pb_records::kRecordMaxColumns;
        std::vector<TestColumn> cols;
        for (size_t c = 0; c < ncols; ++c) {
            const uint32_t kind = (uint32_t)((round + c) % 10);  // every kind in every position
            const bool scalar = kind != 7 && rng() % 3 == 0;
            cols.push_back(random_column(rng, numbers[rng() % 6], kind, scalar, rows));
        }
        const uint32_t number = numbers[rng() % 6];
        View v;
        make_view(number, cols, rows, &v);
        std::string out = "x";  // appended to, not replaced
        uint32_t first_bad = 0, bad_column = 0;
        ASSERT_EQ(pb::SerializeRecords(v.job, &out, &first_bad, &bad_column), 0);
        EXPECT_EQ(first_bad, 0xFFFFFFFFu);
        EXPECT_EQ(bad_column, 0xFFFFFFFFu);
        const std::string want = by_hand(number, cols, rows);
        ASSERT_TRUE(out == "x" + want);
        EXPECT_TRUE(pb_records::WorstCaseBytes(v.job) >= want.size());
    }
}

TEST(PbRecords, one_column_equals_the_row_twin) {
    std::mt19937_64 rng(7);
    for (uint32_t kind = 0; kind <= 9; ++kind) {
        for (int round = 0; round < 10; ++round) {
            const size_t rows = 1 + rng() % 30;
            std::vector<TestColumn> cols = {random_column(rng, 1 + (uint32_t)(rng() % 3000), kind, false, rows)};
            View v;
            make_view(9, cols, rows, &v);
            std::string got, want;
            ASSERT_EQ(pb::SerializeRecords(v.job, &got), 0);
            ASSERT_EQ(pb::SerializeRows(9, cols[0].inner, kind, cols[0].mem.data(), cols[0].count, cols[0].ends.data(), rows,
                                        &want),
                      0);
            ASSERT_TRUE(got == want);
        }
    }
}

TEST(PbRecords, headers_follow_the_sizes) {
    uint8_t head[pb_records::kMaxFieldHeaderBytes];
    for (uint64_t p : {1ull, 127ull, 128ull, 16383ull, 16384ull, 0xFFFFFF00ull}) {
        std::string want;
        put_varint(&want, 0x12);
        put_varint(&want, p);
        const uint32_t n = pb_records::PutFieldHeader(head, 2, 8, false, p);
        EXPECT_EQ(n, pb_records::FieldHeaderBytes(2, 8, false, p));
        EXPECT_TRUE(std::string(reinterpret_cast<char*>(head), n) == want);
        want.clear();
        put_varint(&want, 0x22);
        put_varint(&want, p);
        const uint32_t rn = pb_records::PutRowHeader(head, 4, p);
        EXPECT_EQ(rn, pb_records::RowHeaderBytes(4, p));
        EXPECT_TRUE(std::string(reinterpret_cast<char*>(head), rn) == want);
    }
    EXPECT_EQ(pb_records::PutFieldHeader(head, 2, 8, false, 0), 0u);  // an empty packed field is omitted
    EXPECT_EQ(pb_records::PutFieldHeader(head, 2, 7, false, 0), 2u);  // an empty bytes field is present
    EXPECT_EQ(head[0], 0x12);
    EXPECT_EQ(head[1], 0);
    EXPECT_EQ(pb_records::PutFieldHeader(head, 3, 0, true, 1), 1u);  // scalars: the tag alone
    EXPECT_EQ(head[0], 0x18);
    EXPECT_EQ(pb_records::PutFieldHeader(head, 3, 6, true, 1), 1u);
    EXPECT_EQ(head[0], 0x18);
    EXPECT_EQ(pb_records::PutFieldHeader(head, 3, 8, true, 4), 1u);
    EXPECT_EQ(head[0], 0x1d);
    EXPECT_EQ(pb_records::PutFieldHeader(head, 3, 9, true, 8), 1u);
    EXPECT_EQ(head[0], 0x19);
    EXPECT_EQ(pb_records::PutFieldHeader(head, (1u << 29) - 1, 7, false, 0xFFFFFF00ull), pb_records::kMaxFieldHeaderBytes);
    EXPECT_EQ(pb_records::PutRowHeader(head, (1u << 29) - 1, 0xFFFFFF00ull), pb_records::kMaxRowHeaderBytes);
    EXPECT_EQ(pb_records::PutRowHeader(head, 4, 0), 2u);  // a record without fields: tag 0x00
    EXPECT_EQ(head[1], 0);
}

TEST(PbRecords, twin_equals_the_message_serializer) {
    static const char kProto[] = R"(
syntax = "proto2";
package r;
message Example {
  repeated int64 input_ids = 1 [packed = true];
  repeated float weights = 2 [packed = true];
  optional int32 label = 3;
  optional bytes blob = 4;
  optional double score = 5;
}
message Batch {
  optional string model = 1;
  repeated Example examples = 4;
}
)";
    pb::Importer imp({});
    std::string err;
    ASSERT_TRUE(imp.ImportFromString("r.proto", kProto, &err) != nullptr);
    const pb::Descriptor* d = imp.FindMessageTypeByName("r.Batch");
    ASSERT_TRUE(d != nullptr);
    std::unique_ptr<pb::Message> m(d->prototype->New());
    const int64_t ids[] = {-1, 300, 1ll << 40, -(1ll << 62), 0};
    const uint32_t id_ends[] = {2, 2, 5, 5};
    const float weights[] = {1.5f, 2.25f, 0.1f};
    const uint32_t weight_ends[] = {0, 1, 3, 3};
    const int32_t labels[] = {7, 0, -3, 1 << 30};
    const char blobs[] = "abcde";
    const uint32_t blob_ends[] = {1, 1, 5, 5};
    const double scores[] = {0.0, -1.25, 1e300, 3.0};
    size_t ia = 0, wa = 0, ba = 0;
    for (int r = 0; r < 4; ++r) {
        pb::Message* e = pb::Reflection::AddMessage(m.get(), d->FindFieldByName("examples"));
        const pb::Descriptor* ed = e->GetDescriptor();
        for (; ia < id_ends[r]; ++ia) pb::Reflection::AddInt64(e, ed->FindFieldByName("input_ids"), ids[ia]);
        for (; wa < weight_ends[r]; ++wa) pb::Reflection::AddFloat(e, ed->FindFieldByName("weights"), weights[wa]);
        pb::Reflection::SetInt32(e, ed->FindFieldByName("label"), labels[r]);
        pb::Reflection::SetString(e, ed->FindFieldByName("blob"), std::string(blobs + ba, blob_ends[r] - ba));
        ba = blob_ends[r];
        pb::Reflection::SetDouble(e, ed->FindFieldByName("score"), scores[r]);
    }
    std::string want;
    ASSERT_TRUE(m->SerializeToString(&want));
    pb_records::Column cols[5];
    cols[0] = {1, 3, ids, 5, id_ends};
    cols[1] = {2, 8, weights, 3, weight_ends};
    cols[2] = {3, 0, labels, 4, nullptr};
    cols[3] = {4, 7, blobs, 5, blob_ends};
    cols[4] = {5, 9, scores, 4, nullptr};
    pb_records::Job job;
    job.number = 4;
    job.columns = cols;
    job.ncols = 5;
    job.rows = 4;
    std::string got;
    ASSERT_EQ(pb::SerializeRecords(job, &got), 0);
    EXPECT_TRUE(got == want);
    std::unique_ptr<pb::Message> back(d->prototype->New());
    ASSERT_TRUE(back->ParseFromString(got));
    EXPECT_EQ(pb::Reflection::FieldSize(*back, d->FindFieldByName("examples")), 4);
    std::string again;
    ASSERT_TRUE(back->SerializeToString(&again));
    EXPECT_TRUE(again == want);
}

TEST(PbRecords, twin_names_the_lowest_row_then_the_lowest_column) {
    const int32_t vals[10] = {0};
    const uint32_t fine[] = {3, 5, 10};
    const uint32_t down1[] = {3, 2, 10};   // row 1
    const uint32_t down2[] = {3, 5, 4};    // row 2 (decreases, and does not end at count)
    const uint32_t shorter[] = {3, 5, 9};  // row 2
    pb_records::Column cols[4];
    cols[0] = {1, 0, vals, 10, fine};
    cols[1] = {2, 0, vals, 10, down2};
    cols[2] = {3, 0, vals, 10, down1};
    cols[3] = {4, 0, vals, 10, down1};
    pb_records::Job job;
    job.number = 1;
    job.columns = cols;
    job.ncols = 4;
    job.rows = 3;
    std::string out;
    uint32_t bad = 0, col = 0;
    EXPECT_EQ(pb::SerializeRecords(job, &out, &bad, &col), 1);
    EXPECT_EQ(bad, 1u);  // the lowest row over all columns
    EXPECT_EQ(col, 2u);  // the lowest column that offends there
    cols[2].row_ends = cols[3].row_ends = shorter;
    EXPECT_EQ(pb::SerializeRecords(job, &out, &bad, &col), 1);
    EXPECT_EQ(bad, 2u);
    EXPECT_EQ(col, 1u);
    cols[1].row_ends = fine;
    EXPECT_EQ(pb::SerializeRecords(job, &out, &bad, &col), 1);
    EXPECT_EQ(bad, 2u);
    EXPECT_EQ(col, 2u);
    EXPECT_TRUE(out.empty());
}

TEST(PbRecords, twin_refuses_what_the_rules_refuse) {
    const int32_t vals[10] = {0};
    const uint32_t ends[] = {3, 10};
    pb_records::Column cols[9];
    for (int c = 0; c < 9; ++c) cols[c] = {(uint32_t)c + 1, 0, vals, 10, ends};
    pb_records::Job good;
    good.number = 1;
    good.columns = cols;
    good.ncols = 8;
    good.rows = 2;
    std::string out;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 0);
    EXPECT_TRUE(!out.empty());
    out.clear();
    pb_records::Job j = good;
    j.ncols = 9;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    j.ncols = 0;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    j = good;
    j.columns = nullptr;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    j = good;
    j.number = 0;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    j.number = 1u << 29;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    j = good;
    j.rows = 0;
    EXPECT_EQ(pb::SerializeRecords(j, &out), 2);
    EXPECT_EQ(pb::SerializeRecords(good, nullptr), 2);
    const pb_records::Column keep = cols[3];
    cols[3].inner = 0;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3].inner = 1u << 29;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].kind = 10;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].kind = 7;
    cols[3].row_ends = nullptr;  // bytes have no scalar form
    cols[3].count = 2;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].row_ends = nullptr;  // a scalar column of 10 elements over 2 records
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].src = nullptr;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].count = 1ull << 32;
    EXPECT_EQ(pb::SerializeRecords(good, &out), 2);
    cols[3] = keep;
    cols[3].inner = cols[2].inner;  // the wire allows a number twice
    EXPECT_EQ(pb::SerializeRecords(good, &out), 0);
    EXPECT_TRUE(pb_records::FieldsOk(good));
}

TEST(PbRecords, worst_case_sizes) {
    DeviceJob d;
    good_job(&d);
    // 4 records: two float columns of 4 elements (16 payload bytes, tag +
    // length each a record), a scalar int32 (10 bytes and a tag), tag + length
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 16u + 16u + 40u + 4u * (2u + 2u + 1u + 2u));
    d.job.ncols = 8;
    EXPECT_TRUE(gpu::DeviceRecordsWorstCaseBytes(d.job) > 0u);
    d.job.ncols = 9;
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    d.job.ncols = 0;
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    good_job(&d);
    d.job.rows = 0;
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    good_job(&d);
    d.job.rows = 5;  // the scalar column holds 4
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    good_job(&d);
    d.cols[0].kind = 3;
    d.cols[0].count = 0xFFFFFFFFull / 10 + 1;  // the total above 2^32-1
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    d.cols[0].kind = 7;
    d.cols[0].count = 1ull << 32;
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
    good_job(&d);
    d.job.rows = 1ull << 32;
    d.cols[2].count = 1ull << 32;
    EXPECT_EQ(gpu::DeviceRecordsWorstCaseBytes(d.job), 0u);
}

TEST(PbRecords, bad_jobs_are_refused_before_any_launch) {
    const gpu::DeviceCodecStats s0 = gpu::GetDeviceCodecStats();
    DeviceJob d;
    int refused = 0;
#define REFUSED(change)                   \
    do {                                  \
        good_job(&d);                     \
        change;                           \
        EXPECT_EQ(build_code(&d), 2);     \
        ++refused;                        \
    } while (0)
    REFUSED(d.job.number = 0);
    REFUSED(d.job.number = 1u << 29);
    REFUSED(d.cols[1].inner = 0);
    REFUSED(d.cols[1].inner = 1u << 29);
    REFUSED(d.cols[1].kind = 10);
    REFUSED(d.cols[2].kind = 7);  // bytes without row_ends
    REFUSED(d.job.ncols = 0);
    REFUSED(d.job.ncols = 9);
    REFUSED(d.job.columns = nullptr);
    REFUSED(d.cols[0].src = nullptr);
    REFUSED(d.cols[0].src = g_mem + 2);  // misaligned floats
    REFUSED(d.cols[2].src = g_mem + 2);  // a misaligned scalar column
    REFUSED(d.cols[1].row_ends = reinterpret_cast<const uint32_t*>(g_mem + 2));
    REFUSED(d.cols[2].count = 5);  // a scalar column whose count is not rows
    REFUSED(d.job.rows = 0);
    REFUSED(d.job.dst = nullptr);
    REFUSED(d.cols[0].count = 1ull << 32);
    REFUSED(d.cols[0].kind = 3; d.cols[0].count = 0xFFFFFFFFull / 10 + 1);  // worst case above 2^32-1
#undef REFUSED
    const gpu::DeviceCodecStats s1 = gpu::GetDeviceCodecStats();
    EXPECT_EQ(s1.build_errors - s0.build_errors, refused);
    EXPECT_EQ(s1.built_record_jobs, s0.built_record_jobs);
    EXPECT_EQ(gpu::DeviceBuildRecords(nullptr, 0, 0), 0);
    Buf out;
    good_job(&d);
    d.job.ncols = 9;
    EXPECT_EQ(gpu::BuildDeviceRecords(d.job, &out, 0), 2);
    EXPECT_EQ(out.size(), 0u);
}

// DeviceBuildRows runs a rows job as a record job of one column: the record
// header rules must give pb_rows' row header for every kind, number, inner
// and payload size at which a varint grows, the headerless column (inner 0,
// bytes) and the empty rows included.
TEST(PbRecords, one_column_headers_are_the_row_headers) {
    const uint32_t numbers[] = {1, 15, 16, (1u << 29) - 1};
    const uint64_t pays[] = {0, 1, 127, 128, 16383, 16384, (1u << 21) - 1, 1u << 21, 1u << 28, 0xFFFFFFFFull - 20};
    int checked = 0;
    for (uint32_t kind = 0; kind <= 9; ++kind) {
        for (int ii = 0; ii < 5; ++ii) {
            if (ii == 4 && kind != pb_rows::kKindBytes) continue;
            const uint32_t inner = ii == 4 ? 0 : numbers[ii];
            for (uint32_t number : numbers) {
                for (uint64_t p : pays) {
                    // a packed row has no element exactly when it has no byte;
                    // an empty bytes row is one empty element or none
                    const int ncounts = kind == pb_rows::kKindBytes && p == 0 ? 2 : 1;
                    for (int k = 0; k < ncounts; ++k) {
                        const uint64_t nelems = p == 0 ? (uint64_t)k : (kind == pb_rows::kKindBytes ? p : 1);
                        const uint32_t fh = pb_records::FieldHeaderBytes(inner, kind, false, p);
                        const uint32_t want = pb_rows::HeaderBytes(number, inner, kind, nelems, p);
                        ASSERT_EQ(want, fh + pb_records::RowHeaderBytes(number, fh + p));
                        uint8_t a[pb_rows::kMaxHeaderBytes + 1], b[pb_rows::kMaxHeaderBytes + 1];
                        memset(a, 0xEE, sizeof(a));
                        memset(b, 0xEE, sizeof(b));
                        ASSERT_EQ(pb_rows::PutHeader(a, number, inner, kind, nelems, p), want);
                        uint32_t n = pb_records::PutRowHeader(b, number, fh + p);
                        n += pb_records::PutFieldHeader(b + n, inner, kind, false, p);
                        ASSERT_EQ(n, want);
                        ASSERT_EQ(memcmp(a, b, sizeof(a)), 0);
                        ++checked;
                    }
                }
            }
        }
    }
    // 10 kinds x 4 inners x 4 numbers x 10 sizes, bytes with a fifth inner and
    // two empty rows per (inner, number)
    EXPECT_EQ(checked, 10 * 4 * 4 * 10 + 4 * 10 + 5 * 4);
}

TEST(PbRecords, table_rows_have_the_layout_the_kernels_read) {
    EXPECT_EQ(sizeof(gpu::PbRecordsJob), 40u);
    EXPECT_EQ(sizeof(gpu::PbRecordsResult), 24u);
    EXPECT_EQ(sizeof(gpu::PbRowsJob) % 8, 0u);  // the column table sits between 8-byte tables
    EXPECT_EQ(gpu::kDeviceRecordMaxColumns, pb_records::kRecordMaxColumns);
}
