// pb::SerializeRows (pb/rows.h), the host twin of gpu::DeviceBuildRows, and
// the host half of that entry: the twin against a serializer written byte by
// byte here and against pb::Message's own serialization of a .proto parsed at
// run time, the worst-case size a caller allocates from, and the checks that
// refuse a job before anything is launched. The device half runs in
// tests/test_gpu_pb_rows.py on the GPU box.
#include <algorithm>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "base/buf.h"
#include "base/pb_rows.h"
#include "gpu/device_codec.h"
#include "gpu/kernels.h"
#include "pb/dynamic.h"
#include "pb/parser.h"
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

// One element on the wire, by the protobuf encoding rules alone.
void put_element(std::string* o, uint32_t kind, const char* src, uint64_t i) {
    switch (kind) {
    case 0: {
        int32_t v;
        memcpy(&v, src + 4 * i, 4);
        put_varint(o, (uint64_t)(int64_t)v);
        break;
    }
    case 1: {
        uint32_t v;
        memcpy(&v, src + 4 * i, 4);
        put_varint(o, v);
        break;
    }
    case 2: {
        int32_t v;
        memcpy(&v, src + 4 * i, 4);
        put_varint(o, ((uint32_t)v << 1) ^ (uint32_t)(v >> 31));
        break;
    }
    case 3:
    case 4: {
        uint64_t v;
        memcpy(&v, src + 8 * i, 8);
        put_varint(o, v);
        break;
    }
    case 5: {
        int64_t v;
        memcpy(&v, src + 8 * i, 8);
        put_varint(o, ((uint64_t)v << 1) ^ (uint64_t)(v >> 63));
        break;
    }
    case 6: o->push_back(src[i] ? 1 : 0); break;
    case 7: o->push_back(src[i]); break;
    case 8: o->append(src + 4 * i, 4); break;
    default: o->append(src + 8 * i, 8); break;
    }
}

std::string by_hand(uint32_t number, uint32_t inner, uint32_t kind, const char* src,
                    const std::vector<uint32_t>& ends) {
    std::string out;
    uint64_t at = 0;
    for (uint32_t end : ends) {
        std::string p;
        for (uint64_t i = at; i < end; ++i) put_element(&p, kind, src, i);
        put_varint(&out, ((uint64_t)number << 3) | 2);
        if (inner == 0) {
            put_varint(&out, p.size());
            out += p;
        } else if (end == at && kind != 7) {
            out.push_back(0);
        } else {
            std::string sub;
            put_varint(&sub, ((uint64_t)inner << 3) | 2);
            put_varint(&sub, p.size());
            sub += p;
            put_varint(&out, sub.size());
            out += sub;
        }
        at = end;
    }
    return out;
}

uint32_t source_bytes(uint32_t kind) { return kind == 6 || kind == 7 ? 1 : (kind <= 2 || kind == 8 ? 4 : 8); }

// Random elements whose varints take every length: the top bits of each are
// cut off at a random position.
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

char g_mem[64] __attribute__((aligned(16)));  // never dereferenced: every device job here is refused

gpu::DeviceRowsJob rows_job(uint32_t number, uint32_t inner, uint32_t kind, uint64_t count, uint64_t rows) {
    gpu::DeviceRowsJob j;
    j.number = number;
    j.inner = inner;
    j.kind = kind;
    j.src = g_mem;
    j.count = count;
    j.row_ends = reinterpret_cast<const uint32_t*>(g_mem);
    j.rows = rows;
    j.dst = g_mem;
    j.cap = 1 << 20;
    return j;
}

int build_code(gpu::DeviceRowsJob j) {
    j.err = -1;
    EXPECT_EQ(gpu::DeviceBuildRows(&j, 1, 0), 0);
    return j.err;
}

}  // namespace

TEST(PbRows, twin_equals_a_byte_by_byte_serializer_for_every_kind) {
    std::mt19937_64 rng(20240607);
    const uint32_t numbers[] = {1, 15, 16, 2047, 2048, (1u << 29) - 1};
    for (uint32_t kind = 0; kind <= 9; ++kind) {
        for (int round = 0; round < 40; ++round) {
            const size_t count = round == 0 ? 0 : rng() % 3000;
            const size_t rows = 1 + rng() % 40;
            const std::vector<uint64_t> mem = random_source(rng, kind, count);
            const std::vector<uint32_t> ends = random_ends(rng, count, rows);
            const uint32_t number = numbers[rng() % 6];
            uint32_t inner = numbers[rng() % 6];
            if (kind == 7 && round % 2) inner = 0;
            std::string out = "x";  // appended to, not replaced
            uint32_t first_bad = 0;
            ASSERT_EQ(pb::SerializeRows(number, inner, kind, mem.data(), count, ends.data(), rows, &out, &first_bad), 0);
            EXPECT_EQ(first_bad, 0xFFFFFFFFu);
            const std::string want = by_hand(number, inner, kind, reinterpret_cast<const char*>(mem.data()), ends);
            ASSERT_TRUE(out == "x" + want);
            gpu::DeviceRowsJob j = rows_job(number, inner, kind, count, rows);
            EXPECT_TRUE(gpu::DeviceRowsWorstCaseBytes(j) >= want.size());
        }
    }
}

TEST(PbRows, header_bytes_follow_the_payload_size) {
    // both lengths step at 127 / 128 and 16383 / 16384, the inner one first
    for (uint64_t p : {0ull, 1ull, 125ull, 126ull, 127ull, 128ull, 129ull, 16381ull, 16382ull, 16383ull, 16384ull,
                       16385ull, 0xFFFFFF00ull}) {
        uint8_t head[pb_rows::kMaxHeaderBytes];
        const uint32_t n = pb_rows::PutHeader(head, 4, 2, 7, p, p);
        EXPECT_EQ(n, pb_rows::HeaderBytes(4, 2, 7, p, p));
        std::string want;
        put_varint(&want, 0x22);
        put_varint(&want, 1 + pb_rows::VarintLen(p) + p);
        put_varint(&want, 0x12);
        put_varint(&want, p);
        EXPECT_TRUE(std::string(reinterpret_cast<char*>(head), n) == want);
    }
    uint8_t head[pb_rows::kMaxHeaderBytes];
    EXPECT_EQ(pb_rows::PutHeader(head, 4, 2, 8, 0, 0), 2u);  // an empty packed row: tag 0x00
    EXPECT_EQ(head[1], 0);
    EXPECT_EQ(pb_rows::PutHeader(head, 4, 2, 7, 0, 0), 4u);  // an empty bytes row keeps its inner field
    EXPECT_EQ(pb_rows::PutHeader(head, 4, 0, 7, 0, 0), 2u);  // an empty blob
    EXPECT_EQ(pb_rows::PutHeader(head, (1u << 29) - 1, (1u << 29) - 1, 7, 1, 0xFFFFFF00ull), pb_rows::kMaxHeaderBytes);
}

TEST(PbRows, twin_equals_the_message_serializer) {
    static const char kProto[] = R"(
syntax = "proto2";
package r;
message Row { repeated float v = 2 [packed = true]; }
message Ids { repeated sint64 v = 3 [packed = true]; }
message Batch {
  optional string model = 1;
  repeated Row rows = 4;
  repeated bytes blobs = 5;
  repeated Ids ids = 6;
}
)";
    pb::Importer imp({});
    std::string err;
    ASSERT_TRUE(imp.ImportFromString("r.proto", kProto, &err) != nullptr);
    const pb::Descriptor* d = imp.FindMessageTypeByName("r.Batch");
    ASSERT_TRUE(d != nullptr);
    std::unique_ptr<pb::Message> m(d->prototype->New());
    const float vals[] = {1.5f, 2.25f, 0.1f, -3.0f};
    const std::vector<uint32_t> row_ends = {2, 2, 3, 4, 4};
    const int64_t ids[] = {-1, 300, 1ll << 40, -(1ll << 62)};
    const std::vector<uint32_t> id_ends = {0, 2, 4};
    const char blobs[] = "abcde";
    const std::vector<uint32_t> blob_ends = {1, 1, 5};
    size_t at = 0;
    for (uint32_t end : row_ends) {
        pb::Message* row = pb::Reflection::AddMessage(m.get(), d->FindFieldByName("rows"));
        for (; at < end; ++at) pb::Reflection::AddFloat(row, row->GetDescriptor()->FindFieldByName("v"), vals[at]);
    }
    at = 0;
    for (uint32_t end : blob_ends) {
        pb::Reflection::AddString(m.get(), d->FindFieldByName("blobs"), std::string(blobs + at, end - at));
        at = end;
    }
    at = 0;
    for (uint32_t end : id_ends) {
        pb::Message* row = pb::Reflection::AddMessage(m.get(), d->FindFieldByName("ids"));
        for (; at < end; ++at) pb::Reflection::AddInt64(row, row->GetDescriptor()->FindFieldByName("v"), ids[at]);
    }
    std::string want;
    ASSERT_TRUE(m->SerializeToString(&want));
    std::string got;
    EXPECT_EQ(pb::SerializeRows(4, 2, 8, vals, 4, row_ends.data(), row_ends.size(), &got), 0);
    EXPECT_EQ(pb::SerializeRows(5, 0, 7, blobs, 5, blob_ends.data(), blob_ends.size(), &got), 0);
    EXPECT_EQ(pb::SerializeRows(6, 3, 5, ids, 4, id_ends.data(), id_ends.size(), &got), 0);
    EXPECT_TRUE(got == want);
    // and the parts parse back as one message (concatenation is merge)
    std::unique_ptr<pb::Message> back(d->prototype->New());
    ASSERT_TRUE(back->ParseFromString(got));
    EXPECT_EQ(pb::Reflection::FieldSize(*back, d->FindFieldByName("rows")), 5);
    EXPECT_EQ(pb::Reflection::FieldSize(*back, d->FindFieldByName("blobs")), 3);
}

TEST(PbRows, twin_reports_bad_tables) {
    const int32_t vals[10] = {0};
    std::string out;
    uint32_t bad = 0;
    const uint32_t down[] = {3, 2, 10};
    EXPECT_EQ(pb::SerializeRows(1, 2, 0, vals, 10, down, 3, &out, &bad), 1);
    EXPECT_EQ(bad, 1u);
    const uint32_t shorter[] = {3, 9};
    EXPECT_EQ(pb::SerializeRows(1, 2, 0, vals, 10, shorter, 2, &out, &bad), 1);
    EXPECT_EQ(bad, 1u);
    EXPECT_EQ(pb::SerializeRows(0, 2, 0, vals, 10, shorter, 2, &out, &bad), 2);
    EXPECT_EQ(pb::SerializeRows(1, 0, 0, vals, 10, shorter, 2, &out, &bad), 2);  // no wrapper, not bytes
    EXPECT_EQ(pb::SerializeRows(1, 2, 0, vals, 10, shorter, 0, &out, &bad), 2);  // no row
    EXPECT_TRUE(out.empty());
}

TEST(PbRows, worst_case_sizes) {
    // 3 rows over 7 floats in field 4 / 2: 28 payload bytes, 4 header bytes a row
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 2, 8, 7, 3)), 28u + 3u * 4u);
    // bare blobs: tag + length
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(5, 0, 7, 100, 4)), 100u + 4u * 2u);
    // refused jobs have no size
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(0, 2, 8, 7, 3)), 0u);
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 0, 8, 7, 3)), 0u);
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 2, 10, 7, 3)), 0u);
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 2, 8, 7, 0)), 0u);
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 2, 3, 0xFFFFFFFFull / 10 + 1, 1)), 0u);
    EXPECT_EQ(gpu::DeviceRowsWorstCaseBytes(rows_job(4, 2, 7, 1ull << 32, 1)), 0u);
}

TEST(PbRows, bad_jobs_are_refused_before_any_launch) {
    const gpu::DeviceCodecStats s0 = gpu::GetDeviceCodecStats();
    gpu::DeviceRowsJob good = rows_job(4, 2, 8, 4, 2);
    gpu::DeviceRowsJob j = good;
    j.number = 0;
    EXPECT_EQ(build_code(j), 2);
    j.number = 1u << 29;
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.inner = 1u << 29;
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.kind = 10;
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.inner = 0;  // only bytes go without a wrapper
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.src = nullptr;
    EXPECT_EQ(build_code(j), 2);
    j.src = g_mem + 2;  // misaligned floats
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.row_ends = nullptr;
    EXPECT_EQ(build_code(j), 2);
    j.row_ends = reinterpret_cast<const uint32_t*>(g_mem + 2);
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.rows = 0;
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.dst = nullptr;
    EXPECT_EQ(build_code(j), 2);
    j = good;
    j.count = 1ull << 32;
    EXPECT_EQ(build_code(j), 2);
    j = rows_job(4, 2, 3, 0xFFFFFFFFull / 10 + 1, 1);  // worst case above 2^32-1
    EXPECT_EQ(build_code(j), 2);
    const gpu::DeviceCodecStats s1 = gpu::GetDeviceCodecStats();
    EXPECT_EQ(s1.build_errors - s0.build_errors, 13);
    EXPECT_EQ(s1.built_row_jobs, s0.built_row_jobs);
    EXPECT_EQ(gpu::DeviceBuildRows(nullptr, 0, 0), 0);
    Buf out;
    j = good;
    j.kind = 10;
    EXPECT_EQ(gpu::BuildDeviceRows(j, &out, 0), 2);
    EXPECT_EQ(out.size(), 0u);
}

TEST(PbRows, table_rows_have_the_layout_the_kernels_read) {
    EXPECT_EQ(sizeof(gpu::PbRowsJob), 72u);
    EXPECT_EQ(gpu::kDeviceFieldFixed32, pb_rows::kKindFixed32);
    EXPECT_EQ(gpu::kDeviceFieldFixed64, pb_rows::kKindFixed64);
    EXPECT_EQ(gpu::kDeviceFieldBytes, pb_rows::kKindBytes);
}
