// Device-payload codec: snappy for HBM-resident attachments, end to end in
// HBM (MI355X-native; reference analog: the body codec of
// src/brpc/compress.cpp:79-92 and src/brpc/policy/snappy_compress.cpp:28-64,
// which runs on the host over IOBuf bytes).
//
// The sender encodes the payload in HBM into independent raw snappy blocks
// (one wave each, gpu/snappy_kernels.hip snappy_compress_kernel) laid out at
// a fixed stride inside one lendable arena block, and lends that block. Only
// the block table (compressed size per block) goes into the meta. The
// receiver decodes every block straight out of the lent region — local HBM,
// or the peer's HBM across xGMI — into its own HBM with the piece decoder
// (snappy_decompress_pieces_par_kernel), optionally pb_scan-indexing the
// result, and only then releases the lend. No byte of the payload crosses
// PCIe or touches a host cache, and both sides join the cross-RPC codec
// batch (gpu/codec_batch.h): one launch sequence and one event for every
// RPC's codec work that arrived meanwhile.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mrpc {
struct DevicePayloadIndex;
class Buf;
namespace gpu {

struct DeviceSnappyLayout {
    uint32_t block_ulen = 0;  // uncompressed bytes per block (the last: the rest)
    uint32_t stride = 0;      // bytes between block starts (>= worst-case block)
    uint32_t nblocks = 0;
    uint64_t region() const { return (uint64_t)stride * nblocks; }
};
// -device_payload_block_kb blocks for a payload of `len` bytes.
DeviceSnappyLayout DeviceSnappyLayoutFor(size_t len);

// Encode [src, +len) (device memory) into `dst` (device, >= lay.region()
// bytes). clen[i] receives block i's size, its varint header included.
// Blocks the calling fiber on the codec batch; 0 on success.
int DeviceSnappyEncode(const void* src, size_t len, void* dst, const DeviceSnappyLayout& lay, uint32_t* clen,
                       int device);

// One received payload: blocks at region + i*stride of clen[i] bytes each
// (header included), decoded into dst (len bytes, device memory).
struct DeviceSnappyBlocks {
    const char* region = nullptr;
    uint64_t region_len = 0;
    DeviceSnappyLayout lay;
    const uint32_t* clen = nullptr;
    void* dst = nullptr;
    uint64_t len = 0;
    bool scan = false;  // pb_scan the decoded message into index[i]
};
// Validates every block table against its region (a bad table fails that
// job without launching anything for it), then decodes all jobs in one codec
// request. err[i] = 0, or nonzero when job i was malformed. `index` (may be
// null) gets job i's field table when jobs[i].scan. Returns -1 only on a
// device error.
int DeviceSnappyDecode(const DeviceSnappyBlocks* jobs, int n, int* err, DevicePayloadIndex* index, int device);

// Index already-decoded device messages (one codec request). 0 on success.
int DevicePbScan(const void* const* bufs, const uint64_t* lens, int n, DevicePayloadIndex* index, int device);

// The field table entry of length-delimited field `number` (the first one
// when repeated): its bytes are [*off, *off + *len) of the scanned payload.
// False when the index holds no such field.
bool DevicePayloadField(const DevicePayloadIndex& index, uint32_t number, uint64_t* off, uint64_t* len);

// A packed repeated numeric field whose bytes are already in device memory
// (a device payload located by its DevicePayloadIndex), decoded into a device
// array in the field's vector layout (kind: gpu::PbRunKind; 4 bytes per
// element for the 32-bit kinds, 8 for the 64-bit ones, 1 for bool). dst needs
// room for every element of the run (never more than `len`). The reference
// parses such fields element by element on the host
// (src/brpc/protocol.cpp:349-360 ParsePbFromIOBuf); here the bytes never
// leave HBM.
struct DevicePackedRun {
    const void* src = nullptr;
    uint64_t len = 0;
    uint32_t kind = 0;
    void* dst = nullptr;
    uint64_t count = 0;  // out: elements written
    int err = 0;         // out: 0 ok, 1 malformed or truncated varint, 2 refused (bad arguments)
};
// All runs in one codec request (two launches: count, then place). Returns
// -1 only on a device error; per-run codes in runs[i].err.
int DeviceDecodePackedRuns(DevicePackedRun* runs, int n, int device);

// ---- the encode side: arrays in device memory -> one serialized message in
// device memory, ready to lend as a device attachment. The host never sees a
// value and learns only lengths (the reference serializes every message on
// the host: SerializeToString / SerializeAsCompressedData,
// src/brpc/compress.cpp:92).
// Field kind of raw bytes, next to the gpu::PbRunKind values 0..6: a
// length-delimited field copied verbatim (string / bytes / embedded message,
// and packed float / double / fixed32 / fixed64, whose wire form is their
// memory image). The packed-run decoder keeps refusing it.
constexpr uint32_t kDeviceFieldBytes = 7;
struct DeviceMessageField {
    uint32_t number = 0;        // 1 .. 2^29-1
    uint32_t kind = 0;          // gpu::PbRunKind (a packed field) or kDeviceFieldBytes
    const void* src = nullptr;  // device; vector layout of the kind, naturally aligned
    uint64_t count = 0;         // elements (bytes for kDeviceFieldBytes)
    uint64_t off = 0, len = 0;  // out: the payload's position in the message
};
// Most bytes the message can take (10 per element for int32 and the 64-bit
// kinds, 5 for uint32 / sint32, 1 for bool and bytes; a header is its tag plus
// the varint of the worst payload). Host only. 0 when the fields would be
// refused (or when they make an empty message).
uint64_t DeviceMessageWorstCaseBytes(const DeviceMessageField* fields, int n);
struct DeviceMessageJob {
    DeviceMessageField* fields = nullptr;
    int nfields = 0;
    void* dst = nullptr;  // device, cap bytes
    uint64_t cap = 0;
    uint64_t len = 0;  // out: serialized size (with err 3: the size it needs)
    // out: 0 built; 2 refused before any launch (null src with count > 0, null
    // dst, bad kind, field number 0 or above 2^29-1, more than
    // kCodecScanFields fields, misaligned src, a field whose worst case
    // exceeds 2^32-1 bytes); 3 longer than cap (dst untouched); 4 a source
    // array changed while the message was built
    int err = 0;
};
// Fields are emitted in the order given; a packed field of count 0 is
// omitted (as the host serializer does), a bytes field of length 0 is tag +
// 0x00. All jobs form one codec request. Returns -1 only on a device error.
int DeviceBuildMessages(DeviceMessageJob* jobs, int n, int device);
// Builds into a fresh arena block of the worst-case size and appends exactly
// the message's bytes to *out as one DEVICE block (its deleter frees the whole
// allocation). 0, a DeviceMessageJob::err code, or -1 on a device error.
int BuildDeviceMessage(DeviceMessageField* fields, int n, Buf* out, int device);
// The mirror of DeviceDecodePackedRuns: a bare packed run (no tag, no
// length) per array, through the same kernels.
struct DevicePackedEncodeRun {
    const void* src = nullptr;
    uint64_t count = 0;
    uint32_t kind = 0;  // gpu::PbRunKind
    void* dst = nullptr;
    uint64_t cap = 0;
    uint64_t bytes = 0;  // out
    int err = 0;         // out: as DeviceMessageJob::err
};
int DeviceEncodePackedRuns(DevicePackedEncodeRun* runs, int n, int device);

// ---- rows: a ragged batch in device memory (all rows' elements back to back
// plus the table of row ends that gpu::DeviceParseNumberText writes) -> the
// occurrences of one repeated field, one per row:
//   message Row   { repeated float v = 2 [packed = true]; }
//   message Batch { repeated Row rows = 4; repeated bytes blobs = 5; }
// `rows` is number 4, inner 2, kind 8; `blobs` is number 5, inner 0, kind
// bytes. The wire rules (and the empty-row rules) are base/pb_rows.h;
// pb::SerializeRows (pb/rows.h) is the host twin. Sub-messages with several
// fields are DeviceBuildRecords below; rows of rows are not built.
//
// The output is a sequence of occurrences of one field, which is a valid
// message by itself; protobuf concatenation is merge, so a caller composes
// Batch by appending a BuildDeviceMessage block (the scalar and flat fields)
// and a BuildDeviceRows block to the same Buf.
constexpr uint32_t kDeviceFieldFixed32 = 8;  // 4-byte elements: packed float / fixed32 / sfixed32
constexpr uint32_t kDeviceFieldFixed64 = 9;  // 8-byte elements: packed double / fixed64 / sfixed64
struct DeviceRowsJob {
    uint32_t number = 0;  // the repeated field, 1 .. 2^29-1
    uint32_t inner = 0;   // the packed field inside each row's sub-message; 0: no wrapper (kind bytes only)
    uint32_t kind = 0;    // gpu::PbRunKind, kDeviceFieldBytes, kDeviceFieldFixed32 / 64
    const void* src = nullptr;           // device; all rows' elements, naturally aligned for the kind
    uint64_t count = 0;                  // elements at src
    const uint32_t* row_ends = nullptr;  // device, 4-byte aligned: row_ends[r] = elements in rows 0..r
    uint64_t rows = 0;                   // >= 1; equal neighbours in row_ends are an empty row
    void* dst = nullptr;                 // device, any alignment
    uint64_t cap = 0;
    uint64_t len = 0;  // out: serialized size (with err 3: the size it needs)
    uint32_t first_bad = 0xFFFFFFFFu;  // out, with err 1
    // out: 0 built; 1 row_ends decreases at row first_bad, or its last entry
    // is not count (first_bad = rows - 1): found on the device, the host never
    // reads row_ends; 2 refused before any launch (a null pointer with a
    // nonzero size, bad number / inner / kind, inner 0 with a kind other than
    // bytes, misaligned src or row_ends, rows 0, count or the worst case above
    // 2^32-1); 3 longer than cap; 4 a source changed while the rows were
    // built. With 1 and 3 dst is untouched; no store ever goes beyond cap.
    int err = 0;
};
// Host only: the bytes a destination needs for any values; 0 when the job
// would be refused for its fields, rows or sizes.
uint64_t DeviceRowsWorstCaseBytes(const DeviceRowsJob& job);
// All jobs share one sequence of launches on a pool stream and one wait.
// Returns -1 only on a device error; per-job codes in jobs[i].err.
int DeviceBuildRows(DeviceRowsJob* jobs, int n, int device);
// Builds job's rows (its dst / cap are ignored) into a fresh arena block of
// the worst-case size and appends exactly their bytes to *out as one DEVICE
// block, as BuildDeviceMessage does. 0, a DeviceRowsJob::err code, or -1.
int BuildDeviceRows(const DeviceRowsJob& job, Buf* out, int device);

// ---- records: a batch whose elements are sub-messages with several fields,
// each field a column in device memory:
//   message Example { repeated int64 input_ids = 1 [packed = true];
//                     repeated float weights   = 2 [packed = true];
//                     optional int32 label     = 3;
//                     optional bytes blob      = 4; }
//   message Batch   { optional string model = 1; repeated Example examples = 4; }
// `examples` is number 4 with four columns: two packed ones and a bytes one,
// each a flat array plus row ends as in DeviceRowsJob, and a scalar one (no
// row ends, one element per record, always written). The wire rules are
// base/pb_records.h; pb::SerializeRecords (pb/records.h) is the host twin. A
// job of one packed or one bytes column is DeviceBuildRows' output byte for
// byte. As there, the output is a valid message by itself and composes with
// a BuildDeviceMessage block by concatenation. DeviceSplitRecords below is
// the way back; DeviceSplitRows answers 6 for such records (with inner 0 and
// kind bytes it returns each record's sub-message).
constexpr uint32_t kDeviceRecordMaxColumns = 8;
struct DeviceRecordColumn {
    uint32_t inner = 0;  // the field inside the record, 1 .. 2^29-1; numbers may repeat
    uint32_t kind = 0;   // as DeviceRowsJob; bytes needs row_ends
    const void* src = nullptr;           // device; count elements, naturally aligned for the kind
    uint64_t count = 0;
    const uint32_t* row_ends = nullptr;  // device, 4-byte aligned, rows entries; null: a scalar column, count == rows
};
struct DeviceRecordsJob {
    uint32_t number = 0;  // the repeated field, 1 .. 2^29-1
    const DeviceRecordColumn* columns = nullptr;  // host; written into every record in this order
    uint32_t ncols = 0;                           // 1 .. kDeviceRecordMaxColumns
    uint64_t rows = 0;                            // >= 1
    void* dst = nullptr;                          // device, any alignment
    uint64_t cap = 0;
    uint64_t len = 0;  // out: serialized size (with err 3: the size it needs)
    // out, with err 1: the lowest row at which a column's row_ends decreases
    // (or, at rows - 1, does not end at that column's count), and the lowest
    // column that offends there
    uint32_t first_bad = 0xFFFFFFFFu, bad_column = 0xFFFFFFFFu;
    // out: 0 built; 1 bad table, found on the device (the host never reads a
    // table); 2 refused before any launch (a null pointer with a nonzero
    // size, a misaligned src or row_ends, a bad number / inner / kind, bytes
    // without row_ends, ncols 0 or above 8, a scalar column whose count is
    // not rows, a worst case of 0); 3 longer than cap; 4 a source or table
    // changed between passes. With 1 and 3 dst is untouched; no store ever
    // goes beyond cap.
    int err = 0;
};
// Host only: the bytes a destination needs for any values; 0 when the job
// would be refused for its fields, columns, rows or sizes.
uint64_t DeviceRecordsWorstCaseBytes(const DeviceRecordsJob& job);
// All jobs share one sequence of launches on a pool stream and one wait.
// Returns -1 only on a device error; per-job codes in jobs[i].err.
int DeviceBuildRecords(DeviceRecordsJob* jobs, int n, int device);
// Builds job's records (its dst / cap are ignored) into a fresh arena block
// of the worst-case size and appends exactly their bytes to *out as one
// DEVICE block, as BuildDeviceRows does. 0, a DeviceRecordsJob::err code, or
// -1.
int BuildDeviceRecords(const DeviceRecordsJob& job, Buf* out, int device);

// ---- and back: a message in device memory that holds such rows (what
// DeviceBuildRows wrote, or any sender's `repeated Row rows = N`, other
// top-level fields around and between the rows included) -> the flat array
// and the row ends, without a copy of the message to the host. DevicePbScan
// walks a message with one lane and stops at its field table's size; here
// the top-level field starts are found in parallel (gpu/kernels.h
// LaunchPbRowsSplit), with one serial hop per 4 KiB. pb::SplitRows
// (pb/rows.h) is the host twin: same codes, same outputs.
// The scratch is 10.5 bytes per byte of message in three blocks (6.5 in two
// with -device_split_skip 1), the largest of 4 bytes per byte: the arena's
// largest block (256 MiB) bounds a message.
constexpr uint64_t kDeviceSplitMaxBytes = 64ull << 20;
struct DeviceRowsSplitJob {
    uint32_t number = 0;  // the repeated field, 1 .. 2^29-1
    uint32_t inner = 0;   // the packed field inside each row; 0: the row is the payload (kind bytes only)
    uint32_t kind = 0;    // as DeviceRowsJob
    const void* msg = nullptr;  // device, any byte alignment
    uint64_t n = 0;
    void* values = nullptr;  // device, cap elements, naturally aligned for the kind
    uint64_t cap = 0;
    uint32_t* row_ends = nullptr;  // device, 4-byte aligned, row_cap entries
    uint64_t row_cap = 0;
    // out
    uint64_t count = 0, rows = 0;  // elements and rows (with err 5: what the outputs need)
    uint64_t others = 0;           // top-level fields other than `number`, skipped
    uint64_t first_bad = ~0ull;    // with err 1 and 6: the offset of the top-level field that offends
    // 0 split; 1 malformed wire; 2 refused before any launch (bad number /
    // inner / kind, a null pointer with a nonzero size, misaligned values or
    // row_ends, n above kDeviceSplitMaxBytes); 5 more than cap elements or
    // row_cap rows; 6 well-formed wire of a shape that is not split (see
    // pb_rows::RowShape): the host parser takes it. With 1, 5 and 6 values
    // and row_ends are untouched; no store ever goes beyond cap or row_cap.
    int err = 0;
};
// All jobs share one sequence of launches on a pool stream and one wait; the
// host reads nothing but the result words. Returns -1 only on a device error
// (a failed scratch allocation is one); per-job codes in jobs[i].err.
int DeviceSplitRows(DeviceRowsSplitJob* jobs, int n, int device);

// ---- records back into columns: a message in device memory that holds
// records of several fields (what DeviceBuildRecords wrote, or any sender's
// `repeated Example examples = N`, fields in any order, other top-level
// fields around and between the records) -> every column's flat array, its
// row ends, and one element per record for a scalar column, without a copy of
// the message to the host. The rules are base/pb_records.h (RecordShape);
// pb::SplitRecords (pb/records.h) is the host twin: same codes, same outputs.
// A ragged column absent from a record is a row of no element, a scalar
// absent from one reads as 0 and is counted in `absent`. The top-level walk
// is the row splitter's (gpu/kernels.h LaunchPbRecordsSplit), so the scratch
// is that of DeviceSplitRows plus a record table of 12 bytes and a tag of 4
// per (record, column) and record, sized by min(row_cap, n / 2) records.
struct DeviceRecordSplitColumn {
    uint32_t inner = 0;   // the field inside the record, 1 .. 2^29-1, distinct among the job's columns
    uint32_t kind = 0;    // as DeviceRowsJob
    bool scalar = false;  // one element per record, no row ends (not for bytes)
    void* values = nullptr;  // device, cap elements, naturally aligned for the kind
    uint64_t cap = 0;
    uint32_t* row_ends = nullptr;  // device, 4-byte aligned, the job's row_cap entries; ragged columns only
    // out
    uint64_t count = 0;   // elements; a scalar column: the records
    uint64_t absent = 0;  // scalar columns: records without the field
};
struct DeviceRecordsSplitJob {
    uint32_t number = 0;  // the repeated field, 1 .. 2^29-1
    DeviceRecordSplitColumn* columns = nullptr;  // host
    uint32_t ncols = 0;                          // 1 .. kDeviceRecordMaxColumns
    const void* msg = nullptr;                   // device, any byte alignment
    uint64_t n = 0;
    uint64_t row_cap = 0;  // entries of every ragged column's row_ends
    // out
    uint64_t rows = 0;           // records: always exact
    uint64_t others = 0;         // top-level fields other than `number`, skipped
    uint64_t first_bad = ~0ull;  // with err 1 and 6: the offset of the top-level field that offends
    // 0 split; 1 malformed wire; 2 refused before any launch (bad number /
    // inner / kind, a scalar bytes column, ncols 0 or above 8, a duplicate
    // inner, a null pointer with a nonzero size, misaligned values or
    // row_ends, n above kDeviceSplitMaxBytes, a record table of min(row_cap,
    // n / 2) * ncols entries of 8 bytes above the arena's largest block of
    // 256 MiB); 5 rows > row_cap or a column's count above its cap: the
    // counts are exact when rows <= row_cap and all 0 otherwise, as the record
    // table is sized by row_cap; 6 well-formed wire of a shape that is not
    // split (pb_records::RecordShape): the host parser takes it. 1 and 6 name
    // the lowest offender and win over 5. With 1, 5 and 6 every output is
    // untouched; no store ever goes beyond a cap or row_cap.
    int err = 0;
};
// All jobs share one sequence of launches on a pool stream and one wait; the
// host reads nothing but the result words. Returns -1 only on a device error
// (a failed scratch allocation is one); per-job codes in jobs[i].err.
int DeviceSplitRecords(DeviceRecordsSplitJob* jobs, int n, int device);

struct DeviceCodecStats {
    int64_t encodes = 0, encoded_bytes = 0, encoded_out_bytes = 0;
    int64_t decodes = 0, decoded_bytes = 0, bad_tables = 0, decode_errors = 0;
    int64_t scans = 0;
    int64_t packed_runs = 0, packed_bytes = 0, packed_elems = 0, packed_errors = 0;
    int64_t built_messages = 0, built_fields = 0, built_bytes = 0, build_errors = 0;
    int64_t built_row_jobs = 0, built_rows = 0, built_row_bytes = 0;  // failed row jobs count in build_errors
    int64_t split_row_jobs = 0, split_rows = 0;                       // DeviceSplitRows jobs that ended with code 0
    int64_t built_record_jobs = 0, built_records = 0, built_record_bytes = 0;  // failed ones count in build_errors
    int64_t split_record_jobs = 0, split_records = 0;  // DeviceSplitRecords jobs that ended with code 0
};
DeviceCodecStats GetDeviceCodecStats();

}  // namespace gpu
}  // namespace mrpc
