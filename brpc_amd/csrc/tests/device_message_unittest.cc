// Host half of the device message builder (gpu/device_codec.h): the
// worst-case sizes a caller allocates from, and the checks that refuse a job
// before anything is launched (a refused job must never reach the kernels,
// and no pointer of it is dereferenced). The device half runs in
// tests/test_gpu_device_message.py on the GPU box.
#include <vector>

#include "base/buf.h"
#include "gpu/codec_batch.h"
#include "gpu/device_codec.h"
#include "gpu/kernels.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

char g_mem[64] __attribute__((aligned(16)));  // never dereferenced: every job here is refused or empty

gpu::DeviceMessageField field(uint32_t number, uint32_t kind, uint64_t count, const void* src = g_mem) {
    gpu::DeviceMessageField f;
    f.number = number;
    f.kind = kind;
    f.src = src;
    f.count = count;
    return f;
}

int build_code(std::vector<gpu::DeviceMessageField> fields, void* dst = g_mem) {
    gpu::DeviceMessageJob j;
    j.fields = fields.data();
    j.nfields = (int)fields.size();
    j.dst = dst;
    j.cap = 1 << 20;
    j.err = -1;
    EXPECT_EQ(gpu::DeviceBuildMessages(&j, 1, 0), 0);
    return j.err;
}

}  // namespace

TEST(DeviceMessage, worst_case_sizes_are_exact) {
    // 3 int64 in field 8: tag 0x42, length 30, 3 x 10 bytes
    gpu::DeviceMessageField a = field(8, gpu::PB_RUN_INT64, 3);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&a, 1), 1u + 1u + 30u);
    // int32 takes 10 too (a negative value is sign-extended)
    gpu::DeviceMessageField i32 = field(8, gpu::PB_RUN_INT32, 3);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&i32, 1), 32u);
    // uint32 / sint32: 5 per element
    gpu::DeviceMessageField u = field(2, gpu::PB_RUN_UINT32, 7);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&u, 1), 1u + 1u + 35u);
    gpu::DeviceMessageField s = field(2, gpu::PB_RUN_SINT32, 7);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&s, 1), 37u);
    // bool: 1 per element
    gpu::DeviceMessageField b = field(1, gpu::PB_RUN_BOOL, 100);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&b, 1), 1u + 1u + 100u);
    // bytes: verbatim; field 16 needs a 2-byte tag
    gpu::DeviceMessageField y = field(16, gpu::kDeviceFieldBytes, 100);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&y, 1), 2u + 1u + 100u);
    // the length varint follows the WORST payload across 127 / 128:
    // 25 uint32 -> 125 (1-byte length), 26 -> 130 (2-byte length)
    gpu::DeviceMessageField p = field(1, gpu::PB_RUN_UINT32, 25);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&p, 1), 1u + 1u + 125u);
    p.count = 26;
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&p, 1), 1u + 2u + 130u);
    gpu::DeviceMessageField q = field(1, gpu::PB_RUN_BOOL, 127);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&q, 1), 1u + 1u + 127u);
    q.count = 128;
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&q, 1), 1u + 2u + 128u);
    // a 5-byte tag, and fields add up
    gpu::DeviceMessageField two[2] = {field((1u << 29) - 1, gpu::PB_RUN_BOOL, 1), field(8, gpu::PB_RUN_INT64, 3)};
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(two, 2), (5u + 1u + 1u) + 32u);
    // an empty packed field is omitted, an empty bytes field is tag + 0x00
    gpu::DeviceMessageField e[2] = {field(3, gpu::PB_RUN_INT64, 0), field(4, gpu::kDeviceFieldBytes, 0)};
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(e, 2), 2u);
    // refused fields have no size
    gpu::DeviceMessageField bad = field(0, gpu::PB_RUN_INT64, 3);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&bad, 1), 0u);
    bad = field(1, 9, 3);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&bad, 1), 0u);
    bad = field(1, gpu::PB_RUN_INT64, (0xFFFFFFFFull / 10) + 1);
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&bad, 1), 0u);
    bad.count = 0xFFFFFFFFull / 10;  // the largest int64 field
    EXPECT_EQ(gpu::DeviceMessageWorstCaseBytes(&bad, 1), 1u + 5u + bad.count * 10);
}

TEST(DeviceMessage, bad_jobs_are_refused_before_any_launch) {
    const gpu::DeviceCodecStats s0 = gpu::GetDeviceCodecStats();
    const gpu::CodecBatchStats b0 = gpu::GetCodecBatchStats();
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_INT64, 4, nullptr)}), 2);            // null src with count > 0
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_INT64, 4)}, nullptr), 2);            // null dst
    EXPECT_EQ(build_code({field(1, 9, 4)}), 2);                                     // bad kind
    EXPECT_EQ(build_code({field(0, gpu::PB_RUN_INT64, 4)}), 2);                     // field number 0
    EXPECT_EQ(build_code({field(1u << 29, gpu::PB_RUN_INT64, 4)}), 2);              // field number above 2^29-1
    EXPECT_EQ(build_code(std::vector<gpu::DeviceMessageField>(gpu::kCodecScanFields + 1,
                                                              field(1, gpu::PB_RUN_BOOL, 1))), 2);  // 129 fields
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_INT64, 4, g_mem + 4)}), 2);          // misaligned int64
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_UINT32, 4, g_mem + 2)}), 2);         // misaligned uint32
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_INT64, 0xFFFFFFFFull / 10 + 1)}), 2);  // worst case above 2^32-1
    EXPECT_EQ(build_code({field(1, gpu::kDeviceFieldBytes, 1ull << 32)}), 2);
    // one bad field refuses the whole message
    EXPECT_EQ(build_code({field(1, gpu::PB_RUN_BOOL, 0), field(0, gpu::PB_RUN_BOOL, 0)}), 2);
    const gpu::DeviceCodecStats s1 = gpu::GetDeviceCodecStats();
    EXPECT_EQ(s1.build_errors - s0.build_errors, 11);
    EXPECT_EQ(s1.built_messages, s0.built_messages);
    EXPECT_EQ(gpu::GetCodecBatchStats().requests, b0.requests);  // nothing reached the batch

    // the helpers refuse the same way
    Buf out;
    gpu::DeviceMessageField bad = field(0, gpu::PB_RUN_INT64, 4);
    EXPECT_EQ(gpu::BuildDeviceMessage(&bad, 1, &out, 0), 2);
    EXPECT_EQ(out.size(), 0u);
    gpu::DevicePackedEncodeRun runs[4];
    runs[0].count = 4;  // no source
    runs[0].dst = g_mem;
    runs[1].src = g_mem;  // no destination
    runs[1].count = 4;
    runs[2].src = g_mem;  // a bare run has no bytes kind
    runs[2].dst = g_mem;
    runs[2].count = 4;
    runs[2].kind = gpu::kDeviceFieldBytes;
    runs[3].src = g_mem;  // empty: nothing to encode, not an error
    runs[3].dst = g_mem;
    EXPECT_EQ(gpu::DeviceEncodePackedRuns(runs, 4, 0), 0);
    EXPECT_EQ(runs[0].err, 2);
    EXPECT_EQ(runs[1].err, 2);
    EXPECT_EQ(runs[2].err, 2);
    EXPECT_EQ(runs[3].err, 0);
    EXPECT_EQ(runs[3].bytes, 0u);
    EXPECT_EQ(gpu::GetCodecBatchStats().requests, b0.requests);
}

TEST(DeviceMessage, trivial_calls_launch_nothing) {
    const gpu::CodecBatchStats b0 = gpu::GetCodecBatchStats();
    EXPECT_EQ(gpu::DeviceBuildMessages(nullptr, 0, 0), 0);
    EXPECT_EQ(gpu::DeviceEncodePackedRuns(nullptr, 0, 0), 0);
    // every job refused: the request is never submitted
    gpu::DeviceMessageField f0 = field(0, gpu::PB_RUN_INT64, 4), f1 = field(1, 9, 4);
    gpu::DeviceMessageJob jobs[2];
    jobs[0].fields = &f0;
    jobs[0].nfields = 1;
    jobs[0].dst = g_mem;
    jobs[0].cap = 64;
    jobs[1].fields = &f1;
    jobs[1].nfields = 1;
    jobs[1].dst = g_mem;
    jobs[1].cap = 64;
    EXPECT_EQ(gpu::DeviceBuildMessages(jobs, 2, 0), 0);
    EXPECT_EQ(jobs[0].err, 2);
    EXPECT_EQ(jobs[1].err, 2);
    // a message without an emitted field is empty: built, zero bytes, no launch
    gpu::DeviceMessageField none = field(5, gpu::PB_RUN_SINT64, 0, nullptr);
    gpu::DeviceMessageJob empty;
    empty.fields = &none;
    empty.nfields = 1;
    empty.dst = g_mem;
    empty.len = 99;
    EXPECT_EQ(gpu::DeviceBuildMessages(&empty, 1, 0), 0);
    EXPECT_EQ(empty.err, 0);
    EXPECT_EQ(empty.len, 0u);
    EXPECT_EQ(gpu::GetCodecBatchStats().requests, b0.requests);
}

TEST(DeviceMessage, pooled_request_reset_empties_the_message_tables) {
    gpu::CodecRequest r;
    r.msgs.resize(2);
    r.msg_fields.resize(3);
    r.msg_chunks.resize(5);
    r.msg_res.resize(2);
    r.msg_field_res.resize(3);
    r.Reset();
    EXPECT_TRUE(r.msgs.empty());
    EXPECT_TRUE(r.msg_fields.empty());
    EXPECT_TRUE(r.msg_chunks.empty());
    EXPECT_TRUE(r.msg_res.empty());
    EXPECT_TRUE(r.msg_field_res.empty());
}

TEST(DeviceMessage, table_rows_have_the_layout_the_kernels_read) {
    // the tables cross to the device as raw pinned arrays
    EXPECT_EQ(sizeof(gpu::PbMsgJob), 24u);
    EXPECT_EQ(sizeof(gpu::PbMsgField), 24u);
    EXPECT_EQ(sizeof(gpu::PbMsgChunk), 24u);
    EXPECT_EQ(sizeof(gpu::PbMsgResult), 16u);
    EXPECT_EQ(sizeof(gpu::PbMsgFieldResult), 16u);
    EXPECT_EQ(gpu::kDeviceFieldBytes, gpu::PB_MSG_BYTES);
    EXPECT_EQ(gpu::kDeviceFieldBytes, (uint32_t)gpu::PB_RUN_BOOL + 1);
}
