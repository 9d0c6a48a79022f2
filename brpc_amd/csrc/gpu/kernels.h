// Host-side launch API of the hand-written CDNA4 kernels in kernels.hip.
// All launches are stream-ordered and asynchronous; pointers are device (or
// device-accessible pinned) addresses.
#pragma once

#include <cstddef>
#include <cstdint>

#include "base/pb_records.h"
#include "gpu/gpu.h"

namespace mrpc {
namespace gpu {

struct Segment {
    const void* src;
    void* dst;   // used by copies; ignored by crc
    uint64_t len;
};

// Maximum number of segments one launch carries inline in its kernel
// arguments (no descriptor upload); launchers split larger batches.
constexpr int kInlineSegments = 32;
// Bytes covered by one workgroup (256 lanes x 64 bytes).
constexpr uint64_t kChunkBytes = 16384;

// Standard (finalized) CRC32C of every segment into out_dev[i] — the
// MFMA (GF(2) matmul on v_mfma_i32_32x32x32_i8) kernel. Segment table lives
// in device memory: starts_dev[i] = address, lens_dev[i] = bytes.
// total_bytes bounds the sum of lengths (sizes the grid); max_seg_len
// bounds any one length. scratch: Crc32cScratchBytes(nseg) of device memory.
size_t Crc32cScratchBytes(int64_t nseg);
int LaunchCrc32cSegments(const uint64_t* starts_dev, const uint64_t* lens_dev, int64_t nseg, uint64_t total_bytes,
                         uint64_t max_seg_len, uint32_t* out_dev, void* scratch, hipStream_t s);
// Same result from the LDS slicing-by-8 kernel (segments passed inline;
// kept as an independent implementation for cross-checks and A/B timing).
// `out` needs no initialisation and may be pinned host memory (the kernel
// stores each finished CRC; read it after the stream's event).
int LaunchCrc32c(const Segment* segs, int nseg, uint32_t* out, hipStream_t s);
// One lane stores the GPU wall clock (100 MHz) into *out_pinned (pinned host
// memory, system scope): clock correlation for diagnostics.
int LaunchClockProbe(uint64_t* out_pinned, hipStream_t s);
// One wave that sleeps `us` microseconds of GPU wall clock (capped at 10 s).
int LaunchSleepKernel(uint64_t us, hipStream_t s);
// Completion word of a launch: the kernel's last workgroup to finish
// stores `seq` into *word (pinned host memory, system-scope release, after
// every workgroup's stores were released at agent scope), so the host sees
// the batch done by reading one word — no hipEvent in the completion path.
// `counter` (device memory, zero between launches) counts finished
// workgroups; the last one resets it. Launchers that split a batch into
// several launches on one stream pass the word to the last launch only.
// word[1] / word[2] receive the GPU wall clock (hipDeviceAttributeWallClockRate)
// when workgroup 0 started and when the last workgroup finished.
struct DoneWord {
    uint32_t* counter = nullptr;
    uint64_t* word = nullptr;
    uint64_t seq = 0;
};
// Copy every segment src -> dst (one launch for many small copies).
int LaunchBatchedCopy(const Segment* segs, int nseg, hipStream_t s, const DoneWord* done = nullptr);
// Fused: copy every segment AND write its standard CRC32C to out[i]
// (one read of the bytes; sources may be local/peer HBM or pinned host).
// One launch per 32 segments and nothing else: no memset of `out`, which
// may be pinned host memory read after the stream's event.
// mfma: the CRC runs on the matrix cores (copy_crc32c_mfma_kernel, the
// default), else on the byte-table kernel.
int LaunchBatchedCopyCrc32c(const Segment* segs, int nseg, uint32_t* out, hipStream_t s, bool mfma = true);
// Same copy, but consecutive segments with equal msg_of[] (non-decreasing,
// starting anywhere) form a MESSAGE and out[msg_of[i]] receives the CRC32C
// of the message's bytes (its segments concatenated), folded on the device.
// A message may have at most kInlineSegments segments (else -2, nothing
// launched for it).
int LaunchBatchedCopyCrc32cMessages(const Segment* segs, const int* msg_of, int nseg, uint32_t* out, hipStream_t s,
                                    const DoneWord* done = nullptr, bool mfma = true);

// Packed-varint decode (protobuf wire type 0, packed repeated field):
// `in` holds n bytes of concatenated varints; out receives the values
// (uint64, zigzag-decoded to int64 when zigzag). count_dev receives the
// number of values; err_dev gets 1 if the stream is malformed (value longer
// than 10 bytes or truncated). scratch must hold VarintScratchBytes(n).
size_t VarintScratchBytes(uint64_t n);
int LaunchVarintDecode(const uint8_t* in, uint64_t n, uint64_t* out, uint64_t max_out, bool zigzag,
                       uint64_t* count_dev, int* err_dev, void* scratch, hipStream_t s);
// Packed-varint encode: values -> bytes. out must hold 10*n bytes; bytes_dev
// receives the encoded size. scratch must hold VarintScratchBytes(n).
int LaunchVarintEncode(const uint64_t* in, uint64_t n, bool zigzag, uint8_t* out, uint64_t* bytes_dev,
                       void* scratch, hipStream_t s);

// Batched snappy decompression (gpu/snappy_kernels.hip): every job is an
// independent raw snappy stream of at most kSnappyMaxBlock uncompressed
// bytes. jobs_dev is a device array; out_len_dev[i] / err_dev[i] receive
// the decoded size and 0 (or a nonzero malformed-input code) per job.
constexpr uint32_t kSnappyMaxBlock = 65536;
struct SnappyJob {
    const void* src;    // compressed stream (device)
    void* dst;          // output (device), dst_cap bytes
    uint64_t src_len;
    uint64_t dst_cap;
};
// max_ulen (>= every job's uncompressed size) sizes the LDS per wave: 32 KiB
// blocks run 5 waves per CU, 64 KiB blocks 2.
int LaunchSnappyDecompress(const SnappyJob* jobs_dev, int n, uint32_t max_ulen, uint32_t* out_len_dev, int* err_dev,
                           hipStream_t s);
// Whole raw streams of any length, cut on the device (no host tag walk):
// one wave per stream walks its element headers and cuts it into pieces of
// at most piece_limit uncompressed bytes whose copies stay inside the piece
// (every fragmenting encoder's output: ours cuts at -gpu_snappy_block_kb,
// CPU encoders at 64 KiB; a stream that does not cut at piece_limit is
// retried at kSnappyMaxBlock). Pieces land in pieces[first, first +
// max_pieces) (unused slots get ulen 0); stream_err[i] = 0 or a code
// (malformed, longer than dst_cap, not cuttable). A piece is headerless: its
// ulen is known, its src points into the stream.
struct SnappyStream {
    const void* src;  // whole compressed stream (device)
    void* dst;        // output, dst_cap bytes (device-accessible)
    uint32_t src_len, dst_cap;
    uint32_t first, max_pieces;
};
struct SnappyPiece {
    const void* src;
    void* dst;
    uint32_t src_len, ulen;
};
// Slots a stream of ulen bytes can need: consecutive pieces sum to more
// than the limit, so there are at most 2*ceil(ulen/limit) of them.
constexpr uint32_t SnappyMaxPieces(uint64_t ulen, uint32_t limit) {
    return (uint32_t)(2 * ((ulen + limit - 1) / limit) + 1);
}
int LaunchSnappySplit(const SnappyStream* streams_dev, int n, uint32_t piece_limit, SnappyPiece* pieces_dev,
                      int* stream_err_dev, hipStream_t s);
// Decodes the pieces with lo < ulen <= hi (LDS per wave = hi, so small
// pieces run many waves per CU; a second launch takes the large ones) and
// writes their err (0 or a code); the launch with lo == 0 also writes 0 for
// empty slots.
int LaunchSnappyDecompressPieces(const SnappyPiece* pieces_dev, int n, uint32_t lo, uint32_t hi, int* err_dev,
                                 hipStream_t s);
// The serial decoder (one element per wave step) for every size: A/B and
// tests; LaunchSnappyDecompressPieces takes the parallel decoder (source map
// + pointer jumping) for pieces up to 8 KiB.
int LaunchSnappyDecompressPiecesSerial(const SnappyPiece* pieces_dev, int n, uint32_t lo, uint32_t hi, int* err_dev,
                                       hipStream_t s);
// With phase stamps (shader clock, block 0) written to stamps[0..4].
int LaunchSnappyDecompressPiecesStamped(const SnappyPiece* pieces_dev, int n, uint32_t lo, uint32_t hi, int* err_dev,
                                        uint64_t* stamps, hipStream_t s);
// Batched snappy compression: job.src = raw block (<= kSnappyMaxBlock),
// job.dst = output with job.dst_cap >= SnappyMaxCompressedLength(src_len),
// which is enough for every src_len and content (blocks under 449 bytes are
// cut into segments of 8 bytes, not 64 shorter ones, to stay within it).
// scratch: n * SnappyCompressScratchPerBlock() bytes of device memory.
// out_len_dev[i] = compressed size, err_dev[i] = 0 or an error code.
constexpr uint32_t SnappyCompressSlot() { return ((kSnappyMaxBlock / 64) + 32 + 63) & ~63u; }
constexpr uint64_t SnappyCompressScratchPerBlock() { return 64ull * SnappyCompressSlot(); }
constexpr uint64_t SnappyMaxCompressedLength(uint64_t n) { return 32 + n + n / 6; }
// max_ulen (>= every job's src_len) sizes the LDS: the block is staged in
// LDS, and blocks up to 16 KiB keep their output slots there too (scratch
// is then unused).
int LaunchSnappyCompress(const SnappyJob* jobs_dev, int n, uint32_t max_ulen, void* scratch, uint32_t* out_len_dev,
                         int* err_dev, hipStream_t s);
// Same, stamping block 0's phases (shader clock) into stamps[0..4]: start,
// staged, earliest-position table built, matched, written.
int LaunchSnappyCompressStamped(const SnappyJob* jobs_dev, int n, uint32_t max_ulen, void* scratch,
                                uint32_t* out_len_dev, int* err_dev, uint64_t* stamps, hipStream_t s);
// Whether a launch with this max_ulen writes the global scratch (blocks
// above 16 KiB); otherwise scratch may be null.
constexpr bool SnappyCompressUsesScratch(uint32_t max_ulen) { return max_ulen > 16384; }

// Batched protobuf wire scan (gpu/pb_kernels.hip): message i is
// buf[offsets[i], offsets[i+1]); its top-level fields land in
// fields[i * max_fields * 2 + 2k] = tag, [.. + 1] = value (varint / fixed /
// (offset << 32) | length); nfields[i] = count or a negative error code
// (-5: the offsets of message i leave [0, buf_len) or descend).
int LaunchPbScan(const uint8_t* buf, uint64_t buf_len, const int64_t* offsets_dev, int64_t n, uint32_t max_fields,
                 uint64_t* fields, int32_t* nfields, hipStream_t s);
// Same scan for messages in separate buffers: job i is buf[0, len) (device
// or device-readable pinned table).
struct PbScanJob {
    const uint8_t* buf;
    uint64_t len;
};
int LaunchPbScanPtrs(const PbScanJob* jobs, int64_t n, uint32_t max_fields, uint64_t* fields, int32_t* nfields,
                     hipStream_t s);

// Fused device-body codec launch (codec_waves_kernel, snappy_kernels.hip):
// ONE launch runs a codec batch's compress blocks and headerless decode
// pieces, each at most kFusedMaxBlock uncompressed bytes, one wave per block
// or piece (the per-lane-segment compressor and the wave decoder); a
// message's field table follows as a pb-scan launch, or (opt-in) the wave
// that finished its last piece scans it.
constexpr uint32_t kFusedMaxBlock = 8192;
constexpr uint32_t kFusedNoGroup = 0xFFFFFFFFu;
struct FusedCodecArgs {
    const SnappyJob* comp = nullptr;  // compress jobs (device-readable table)
    int ncomp = 0;
    uint32_t* comp_len = nullptr;
    int* comp_err = nullptr;          // 0, 1 (block too large), 2 (output exceeds dst_cap)
    const SnappyPiece* pieces = nullptr;
    int npieces = 0;
    int* piece_err = nullptr;         // 0, 1 (too large), 3 (element chain leaves the piece), 4 (size), 6 (offset)
    const uint32_t* piece_group = nullptr;  // per piece: scan group, or kFusedNoGroup
    const PbScanJob* scans = nullptr;       // per group: the message its pieces form
    const uint32_t* group_pieces = nullptr; // per group: how many pieces decode into it
    uint32_t* group_done = nullptr;         // per group: HBM counter, zero between launches
    uint64_t* scan_fields = nullptr;        // per group: max_fields {tag, value} rows
    int32_t* scan_n = nullptr;
    uint32_t max_fields = 0;
    uint32_t max_ulen = 0;                  // >= every block's and piece's size
};
int LaunchCodecWaves(const FusedCodecArgs& a, hipStream_t s);


// Batched encoder of repeated numeric runs (SURVEY K2, and the number
// arrays of pb2json, K6): one workgroup per chunk of <= kPbRunChunkElems
// elements, read in the std::vector layout of the field (1/4/8 bytes per
// element), written as protobuf varints (the payload of a packed field) or
// as comma-separated JSON numbers. The host knows every chunk's output size
// (its size pass) and so its destination: chunks of many runs of many
// messages go into one launch with no device-side scan across chunks.
constexpr uint32_t kPbRunChunkElems = 2048;
enum PbRunKind : uint32_t {
    PB_RUN_INT32 = 0,   // int32/enum: sign-extended to 64 bits (negative -> 10 bytes)
    PB_RUN_UINT32 = 1,
    PB_RUN_SINT32 = 2,  // zigzag32
    PB_RUN_INT64 = 3,
    PB_RUN_UINT64 = 4,
    PB_RUN_SINT64 = 5,  // zigzag64
    PB_RUN_BOOL = 6,    // one byte per element
};
enum PbRunFormat : uint32_t {
    PB_RUN_VARINT = 0,
    PB_RUN_DECIMAL = 1,  // JSON: "v,v,...,v" (true/false for bools); no trailing comma on a run's last chunk
};
struct PbRunChunk {
    const void* src;  // this chunk's first element (device-readable)
    uint8_t* dst;     // this chunk's first output byte (device-writable)
    uint32_t count;   // elements, 1..kPbRunChunkElems
    uint32_t kind;    // PbRunKind
    uint32_t format;  // PbRunFormat
    uint32_t last;    // 1: the run's last chunk (decimal: no trailing comma)
    uint32_t bytes;   // output size the host computed; a mismatch is reported and nothing is written
    uint32_t pad;
};
// err[i] is set to 0 (ok) or 1 (size mismatch) for every chunk.
int LaunchPbRunEncode(const PbRunChunk* chunks, int n, int32_t* err, hipStream_t s);

// Batched decoder of packed varint runs (the parse half of K2: large packed
// fields of a body the device already decoded): a run is cut into chunks of
// <= kPbRunDecodeChunkBytes; pass 1 counts the varints ending in each chunk
// (into counts, and into `prefix`, device memory of n entries, which one
// workgroup then scans), pass 2 gives every chunk its first element index
// (prefix[chunk] - prefix[run's first chunk]) and writes each varint ending in it,
// converted to the field's vector layout, at dst[index]. A varint belongs
// to the chunk its last byte is in, so one may start up to 9 bytes into the
// previous chunk (read from there). Codes in err: 0 ok, 1 a varint longer
// than 10 bytes (or a 10th byte above 1).
constexpr uint32_t kPbRunDecodeChunkBytes = 4096;
struct PbRunDecodeChunk {
    const uint8_t* run;  // the run's first byte (device-readable)
    void* dst;           // the run's output array (kind's vector layout)
    uint32_t offset;     // this chunk's first byte within the run
    uint32_t len;        // bytes in the chunk, 1..kPbRunDecodeChunkBytes
    uint32_t first;      // table index of the run's first chunk
    uint32_t kind;       // PbRunKind
};
int LaunchPbRunDecode(const PbRunDecodeChunk* chunks, int n, uint32_t* counts, uint32_t* prefix, int32_t* err,
                      hipStream_t s);

// Message builder (the encode mirror of the packed-run decoder): arrays in
// device memory become whole serialized protobuf messages in device memory,
// the host knowing no value and learning only lengths. A message is a list
// of length-delimited fields; a field's payload is the concatenation of its
// chunks, each <= kPbRunChunkElems numeric elements encoded as varints (a
// packed field) or <= kPbMsgBytesChunk raw bytes copied verbatim (a bytes
// field, and so a packed float/double/fixed field: its wire form is its
// memory image). Four launches on one stream, ordered by the launches alone
// (no workgroup waits on another):
//   size   a wave per chunk writes its encoded size into prefix[chunk]
//          (prefix: device memory, nchunks + 1 entries; the last gets 0)
//   prefix pb_run_prefix_kernel scans them (exclusive, mod 2^32)
//   layout a wave per message scans header + payload lengths of its fields in
//          64 bits; a message longer than its cap is marked (err 3) and gets
//          nothing written, else every header is written and base[field]
//          (device memory, nfields entries) gets the payload's address
//   place  a workgroup per chunk encodes it into LDS and copies it to
//          base[field] + (prefix[chunk] - prefix[field's first chunk])
// The three tables are device-readable (pinned host) arrays; res / fres are
// device-writable (pinned host) results.
constexpr uint32_t PB_MSG_BYTES = 7;  // chunk kind next to the PbRunKind values: raw bytes
constexpr uint32_t kPbMsgBytesChunk = 16384;
struct PbMsgJob {
    uint8_t* dst;  // the message's first byte (device-writable), never null
    uint64_t cap;  // bytes available at dst
    uint32_t first_field, nfields;  // its fields, in wire order
};
struct PbMsgField {
    uint32_t msg;          // owning message
    uint32_t tag;          // (number << 3) | 2
    uint32_t first_chunk;  // its chunks, in order (a valid index even when nchunks == 0)
    uint32_t nchunks;
    uint32_t headerless;   // 1: a bare run, neither tag nor length is written
    uint32_t pad;
};
struct PbMsgChunk {
    const void* src;  // this chunk's first element / byte (device-readable, naturally aligned)
    uint32_t count;   // elements, 1..kPbRunChunkElems (bytes, 1..kPbMsgBytesChunk, for PB_MSG_BYTES)
    uint32_t kind;    // PbRunKind or PB_MSG_BYTES
    uint32_t field;   // owning field
    uint32_t first;   // the owning field's first chunk
};
struct PbMsgResult {
    uint64_t len;  // serialized size (also when it did not fit)
    int32_t err;   // 0, 3 (longer than cap; nothing written), 4 (a source changed between size and place)
    int32_t pad;
};
struct PbMsgFieldResult {
    uint64_t off, len;  // the payload's position in the message (0, 0 when the message failed)
};
struct PbMsgTables {
    const PbMsgJob* msgs = nullptr;
    int nmsgs = 0;
    const PbMsgField* fields = nullptr;
    int nfields = 0;
    const PbMsgChunk* chunks = nullptr;
    int nchunks = 0;
    uint32_t* prefix = nullptr;  // device memory, nchunks + 1 entries
    uint64_t* base = nullptr;    // device memory, nfields entries
    PbMsgResult* res = nullptr;          // nmsgs
    PbMsgFieldResult* fres = nullptr;    // nfields
};
int LaunchPbMsgEncode(const PbMsgTables& t, hipStream_t s);
// The one-workgroup exclusive prefix sum (mod 2^32) those passes use, over
// prefix[0, n) in place (device memory), for other kernels' size tables.
int LaunchPbRunPrefix(uint32_t* prefix, int n, hipStream_t s);

// Record builder: several columns in device memory become the occurrences of
// one repeated sub-message with several fields (base/pb_records.h has the
// wire rules; pb::SerializeRecords is the host twin). A column is one flat
// array plus a table of row ends; a scalar column has no table and element r
// belongs to record r. A rows job (one flat array plus row ends -> the
// occurrences of one repeated field; base/pb_rows.h, host twin
// pb::SerializeRows) is a record job of one column. Its `repeated bytes`
// form, inner == 0, is the headerless column of base/pb_records.h: the
// record header is followed by the payload, with no field header in between.
// A header depends on the encoded size behind it, so on every value: nothing
// here takes a size from the host. A column is cut into chunks of
// kPbRowsChunkElems elements and, for the kinds encoded as varints, into
// groups of 64 elements; records are taken 256 to a workgroup. All jobs share
// seven launches on one stream, ordered by the launches alone (no count or
// size is read back in between):
//   init     copies the job and column tables to device memory, resets each
//            job's offender word and zeroes the tail groups of each varint
//            column
//   size     varint kinds only: a workgroup per chunk, one grid over the
//            chunks of every column of every job, writes the encoded bytes of
//            each of its groups into groups[] (fixed-width kinds need none:
//            the bytes before element e are e times the width)
//   prefix   LaunchPbRunPrefix over groups[]
//   measure  a lane per record: the bytes before an element are its group's
//            prefix plus at most 63 element sizes recomputed from the source;
//            a column's payload in the row is the difference of two of them,
//            into col_pay[], and the bytes before the row's first element go
//            into col_delta[]. The record's size, header and field headers
//            included, goes into row_size[] and the workgroup's sum into
//            block_off[]. A column whose row end lies before its start, or
//            whose last end is not its count, goes into bad[] through one
//            atomic min on row << 4 | column: the lowest row, then the lowest
//            column
//   prefix   LaunchPbRunPrefix over block_off[]: one entry per 256 rows (the
//            one-workgroup scan over an entry per row took 600 us of the 750 us
//            of 2^20 one-element rows)
//   heads    a lane per record: row 0's lane writes the job's result; a job
//            that is malformed (err 1) or longer than its cap (err 3) gets
//            nothing written here or later. Else the record's offset is its
//            block's plus a scan of the sizes inside the workgroup; its header
//            and every field's header (for a scalar column: its tag) are
//            written there (a record without payload is complete with them)
//            and col_delta[] becomes the distance from "bytes before element
//            e" to "offset of element e in dst"
//   place    a workgroup per chunk of every column finds the rows that meet
//            it by binary search in row_ends. A chunk that meets few rows is
//            encoded into LDS and leaves per row segment with 16-byte stores;
//            one that meets many marks the row starts in LDS, spreads the row
//            index over the elements with a max-scan, and every lane stores
//            its own element, each at its column's delta. A chunk whose bytes
//            are not what the size pass measured, or a store that would leave
//            the message, writes nothing and marks err 4
// The job and column tables are device-readable (pinned host) arrays, res a
// device-writable one; everything else is device memory.
constexpr uint32_t kPbRowsChunkElems = kPbRunChunkElems;
constexpr uint32_t kPbRowsGroupElems = 64;
constexpr uint32_t kPbRowsBlockRows = 256;
// A column. dst / cap / number / rows are its job's; first_chunk and
// first_group count over all columns of all jobs.
struct PbRowsJob {
    const void* src;           // count elements, the kind's vector layout, naturally aligned
    const uint32_t* row_ends;  // rows entries; null for a scalar column (count == rows)
    uint8_t* dst;              // any alignment, never null
    uint64_t cap;
    uint32_t count, rows;      // rows >= 1
    uint32_t number, inner, kind;   // inner 0: the headerless column
    uint32_t first_chunk, nchunks;  // nchunks = ceil(count / kPbRowsChunkElems)
    uint32_t first_rblock;          // the index of its record job
    uint32_t first_row;             // in col_pay and col_delta: rows entries each
    uint32_t first_group;           // in groups: count / 64 + 2 entries (varint kinds only)
};
struct PbRecordsJob {
    uint8_t* dst;  // any alignment, never null
    uint64_t cap;
    uint32_t rows;  // >= 1
    uint32_t number;
    uint32_t ncols, first_col;  // its columns in the column table, 1 .. pb_records::kRecordMaxColumns
    uint32_t first_rblock;      // ceil(rows / kPbRowsBlockRows) row blocks; job k's entries of block_off start
                                // at first_rblock + k (its blocks, then one entry for its total)
    uint32_t first_row;         // in row_size: rows entries
};
struct PbRecordsResult {
    uint64_t len;         // serialized size (also when it did not fit)
    uint32_t first_bad;   // with err 1
    uint32_t bad_column;  // with err 1
    int32_t err;          // 0, 1, 3, 4
};
struct PbRecordsTables {
    const PbRecordsJob* jobs = nullptr;
    int njobs = 0;
    const PbRowsJob* cols = nullptr;
    int ncols = 0;                       // of all jobs
    PbRecordsJob* jobs_dev = nullptr;    // njobs
    PbRowsJob* cols_dev = nullptr;       // ncols
    uint32_t nchunks = 0, nrblocks = 0, ngroups = 0, nrows = 0, ncolrows = 0;  // of all jobs
    uint32_t* groups = nullptr;          // ngroups
    uint32_t* row_size = nullptr;        // nrows
    uint32_t* col_pay = nullptr;         // ncolrows: rows entries per column
    uint32_t* col_delta = nullptr;       // ncolrows
    uint32_t* block_off = nullptr;       // nrblocks + njobs
    unsigned long long* bad = nullptr;   // njobs
    PbRecordsResult* res = nullptr;      // njobs
};
int LaunchPbRecordsBuild(const PbRecordsTables& t, hipStream_t s);

// Row splitter, the inverse: a message in device memory whose field `number`
// repeats once per row becomes the flat array and the row ends again
// (base/pb_rows.h has the rules, pb::SplitRows is the host twin). Finding the
// top-level fields of a message is a walk of length-prefixed fields; here
// only one hop per chunk of kPbSplitChunk bytes of it stays serial. All jobs
// share one sequence of launches on one stream, ordered by the launches alone:
// no workgroup waits for another, and every loop is bounded by n or by the
// two invariants of pb_rows::SpecField (it never reads beyond n, and `next`
// grows strictly).
//   spec    a workgroup per chunk parses a field at EVERY byte offset of the
//           chunk (staged in LDS with the bytes a parse may read behind it)
//           and resolves, by pointer doubling in LDS, exit[p]: the first
//           offset at or beyond the chunk's end on p's chain of `next`, or
//           invalid. Also the chunk's terminator mask (bytes without a
//           continuation bit, a bit per byte), the terminators before each of
//           its 64-byte groups and their total, and entry[chunk] = none
//   prefix  LaunchPbRunPrefix over the chunks' terminator totals
//   skip    skip[p] = exit applied skip_hops times to p, for every offset:
//           a pass of gathers that mostly meet (chains merge within a few
//           fields), which makes every serial hop below skip_hops chunks long
//   chase   a lane per job hops pos = skip[pos] from 0 and writes land[c],
//           the first true field start of every chunk it lands in: one
//           dependent load per skip_hops chunks, the serial remainder (260 ns
//           a hop on MI355X: the table was written by other XCDs a moment ago)
//   fill    a lane per landing writes entry[] of the chunks up to the next
//           landing, skip_hops - 1 hops of exit[] further. With skip_hops 1
//           there is neither skip nor fill: the chase follows exit[] and
//           writes entry[] itself
//   mark    a workgroup per chunk parses every offset again and finds the
//           true starts from entry[c] in two levels: exits of the 64-byte
//           sub-chunks by doubling, one lane across the 64 sub-chunks, then a
//           lane per sub-chunk walks its own. A true start that is no field
//           reports its offset (code 1), field `number` with another wire
//           type too (code 6); rows are marked in the row mask and counted
//           per chunk, other fields counted per job
//   prefix  over the chunks' row counts: every row has its rank
//   table   the lane that owns a row's tag applies pb_rows::RowShape (from
//           device memory: a row's sub-header may lie in the next chunk) and
//           writes {tag offset, header bytes, payload bytes} into the row
//           table, which takes the place of exit[] (two bytes of message at
//           least per row, eight bytes per entry)
//   check   varint kinds: a workgroup per chunk looks for varints of more
//           than ten bytes (or ten with a last byte above 1) and reports those
//           inside a row's payload (code 1). The byte in front of a payload
//           ends a length, so a varint's extent needs no row bounds
//   count   a lane per row: elements of the row (payload bytes over the
//           element size, or the difference of two terminator counts), summed
//           per 256 rows
//   prefix  over those sums
//   publish a lane per job combines the lowest offender, the counts and the
//           capacities into the result; everything below runs only for jobs
//           whose code is 0, read from device memory
//   ends    a lane per row: row_ends, by a scan inside each block of 256 rows,
//           and for varint kinds the row's first element index less the
//           terminators in front of its payload
//   place   fixed-width kinds and bytes: a workgroup per 2048 elements of the
//           output; every element finds its row in row_ends by binary search
//           between the rows of the chunk's first and last element. Varint
//           kinds: a workgroup per message chunk; every terminator inside a
//           payload is the end of one element, whose row is found in the
//           slice of the row table that meets the chunk
// The offender word of a job is (offset << 3 | code), lowered with atomicMin.
constexpr uint32_t kPbSplitChunk = 4096;
constexpr uint32_t kPbSplitBlockRows = 256;
constexpr uint32_t kPbSplitOutChunk = 2048;  // elements
constexpr uint32_t kPbSplitNone = 0xFFFFFFFFu;
struct PbSplitJob {
    const uint8_t* msg;  // n bytes, any alignment
    void* values;        // cap elements, naturally aligned
    uint32_t* row_ends;  // row_cap entries
    uint64_t cap, row_cap;
    uint32_t n;  // 1 .. kDeviceSplitMaxBytes
    uint32_t number, inner, kind;
    // the job's part of the tables: chunk c of the job is entry first_chunk + c of entry, term_chunk and
    // row_chunk, its 64 groups those from there times 64 of the masks and term_group, its bytes those from
    // there times kPbSplitChunk of exit
    uint32_t first_chunk, nchunks;    // ceil(n / kPbSplitChunk)
    uint32_t first_rblock, nrblocks;  // blocks of 256 rows in block_sum: ceil((n / 2) / 256), at least 1
    uint32_t first_ochunk, nochunks;  // fixed-width kinds and bytes: ceil(min(cap, n / width) / 2048) output chunks
    uint32_t first_row;               // in row_bias: min(row_cap, n / 2) entries (varint kinds)
};
struct PbSplitResult {
    uint64_t count, rows, others;
    uint32_t first_bad;
    int32_t err;  // 0, 1, 5, 6
};
struct PbSplitTables {
    const PbSplitJob* jobs = nullptr;  // pinned host
    int njobs = 0;
    PbSplitJob* jobs_dev = nullptr;
    uint32_t nchunks = 0, nrblocks = 0, nochunks = 0, nrows = 0;
    bool any_varint = false;
    uint32_t* exit = nullptr;       // nchunks * kPbSplitChunk; later the row table (uint64 per row)
    uint32_t skip_hops = 1;         // chunks a serial hop of the chase spans at least; above 1 with skip and land
    uint32_t* skip = nullptr;       // nchunks * kPbSplitChunk
    uint32_t* land = nullptr;       // nchunks
    uint64_t* term_mask = nullptr;  // nchunks * 64
    uint64_t* row_mask = nullptr;   // nchunks * 64
    uint32_t* term_group = nullptr; // nchunks * 64
    uint32_t* term_chunk = nullptr; // nchunks + 1, scanned
    uint32_t* row_chunk = nullptr;  // nchunks + 1, scanned
    uint32_t* entry = nullptr;      // nchunks
    uint32_t* block_sum = nullptr;  // nrblocks + 1, scanned
    uint32_t* row_bias = nullptr;   // nrows
    uint32_t* bad = nullptr;        // njobs
    uint32_t* others = nullptr;     // njobs
    int32_t* ok = nullptr;          // njobs
    PbSplitResult* res = nullptr;   // njobs, pinned host
};
int LaunchPbRowsSplit(const PbSplitTables& t, hipStream_t s);

// Record splitter: the same message walk, but every occurrence of `number` is
// a record of up to 8 columns (base/pb_records.h has the rules,
// pb::SplitRecords is the host twin). The passes up to and including mark and
// the prefix over the row counts are the row splitter's own kernels, launched
// on a PbSplitJob that carries the record job's {msg, n, number}: they find
// and rank every occurrence of `number` whatever it holds, and neither they
// nor LaunchPbRowsSplit change. What follows is new: six kernels in eight
// launches (the check kernel is also the varint place pass, the count kernel
// also the ends pass) and one prefix. With the row splitter's eight a call is
// 17 launches, 15 when the message is short enough to be chased without the
// skip table; 3 fewer when no column is a ragged varint one (the prefix over
// the terminators, check and the varint place pass), 1 fewer when no column is
// a ragged fixed-width or bytes one:
//   init    a lane per job copies the record job, a lane per column the
//           column, and zeroes the absent counters
//   table   the lane that owns a record's tag applies
//           pb_records::RecordShape from device memory. Record `rank` gets its
//           tag offset in rec_tag and, per column, a 64-bit entry {payload
//           offset (28 bits), payload bytes (28 bits), taken (1 bit)}; for a
//           scalar that is the value's place. The table holds min(row_cap,
//           n / 2) records: a record beyond it (the job then ends with 5
//           unless something is 1 or 6) is judged all the same, and its taken
//           varint payloads are checked by its lane with pb_rows::VarintsOk,
//           as the check pass cannot find it in the table
//   check   a workgroup per message chunk looks for varints of more than ten
//           bytes (or ten with a last byte above 1). Such a terminator finds
//           its record by binary search of rec_tag among the records that
//           meet the chunk, then its column among the record's at most 8
//           payloads, linearly, as field order inside a record is free.
//           Terminators inside bytes, fixed-width or scalar payloads are not
//           elements. A payload is preceded by the last byte of a length, so
//           a varint's extent needs no bounds
//   count   a workgroup per 256 records, column after column: the elements of
//           (record, column) are payload bytes over the width or the
//           difference of two terminator counts from the spec pass's tables,
//           summed per block per column; absent scalars are counted per job
//   prefix  over those sums: a column's are nrblocks consecutive entries
//   publish a lane per job: the lowest offender, else rows against row_cap
//           (then every count is 0), else every column's count against its
//           cap; everything below runs only for jobs whose code is 0
//   ends    the count kernel again: row_ends of every ragged column, the bias
//           of varint ones (the row's first element index less the
//           terminators in front of its payload), and the scalar values,
//           decoded here (an absent one is 0)
//   place   varint columns: the check kernel again, a workgroup per message
//           chunk; every terminator inside a taken varint payload ends one
//           element. Fixed-width and bytes columns: a workgroup per 2048
//           output elements per column, every element finds its record in that
//           column's row_ends by binary search
// As in the row splitter no workgroup waits for another, every loop is
// bounded by n, by 8 or by SpecField's invariants, and every table store is
// guarded by its capacity.
constexpr uint32_t kPbRecSplitMaxColumns = 8;
struct PbRecSplitCol {
    void* values;        // cap elements, naturally aligned
    uint32_t* row_ends;  // row_cap entries (ragged columns)
    uint64_t cap;
    uint32_t inner, kind, scalar;
    uint32_t job, index;              // its record job and its place among that job's columns
    uint32_t first_ochunk, nochunks;  // ragged fixed-width and bytes columns: output chunks of 2048 elements
    uint32_t first_bsum;              // in block_sum: the job's nrblocks entries of this column
};
struct PbRecSplitJob {
    uint64_t row_cap;
    uint64_t first_entry;             // in entry / bias: rec_cap * ncols entries, record-major
    uint32_t first_tag, rec_cap;      // in rec_tag: min(row_cap, n / 2) records
    uint32_t first_col, ncols;
    uint32_t first_rblock, nrblocks;  // blocks of 256 records: ceil(rec_cap / 256), at least 1
    uint32_t any_varint;              // some column is a ragged varint one
};
struct PbRecSplitResult {
    uint64_t rows, others;
    uint64_t count[kPbRecSplitMaxColumns], absent[kPbRecSplitMaxColumns];
    uint32_t first_bad;
    int32_t err;  // 0, 1, 5, 6
};
struct PbRecSplitTables {
    PbSplitTables front;  // the row splitter's passes up to the row ranks: nrblocks 1, nochunks 0, nrows 0
    const PbRecSplitJob* jobs = nullptr;  // pinned host, front.njobs of them
    const PbRecSplitCol* cols = nullptr;  // pinned host
    int ncols = 0;
    PbRecSplitJob* jobs_dev = nullptr;
    PbRecSplitCol* cols_dev = nullptr;
    pb_records::SplitColumn* specs = nullptr;  // ncols: what RecordShape reads
    uint32_t nrblocks = 0, nbsums = 0, nochunks = 0;
    bool any_varint = false;
    uint64_t* entry = nullptr;      // sum of rec_cap * ncols
    uint32_t* bias = nullptr;       // as entry
    uint32_t* rec_tag = nullptr;    // sum of rec_cap
    uint32_t* block_sum = nullptr;  // nbsums + 1, scanned
    uint32_t* absent = nullptr;     // ncols
    PbRecSplitResult* res = nullptr;  // front.njobs, pinned host
};
int LaunchPbRecordsSplit(const PbRecSplitTables& t, hipStream_t s);

// JSON float / double arrays (gpu/json_kernels.hip): arrays in device (or
// pinned host) memory become "v,v,...,v" in device memory, every element
// exactly as json::Value prints a double (base/shortest_double.h; a float is
// widened first; "NaN" / "Infinity" / "-Infinity" quoted). An element's size
// is known only once it is formatted, so the host sizes nothing. An array is
// cut into chunks of <= kJsonFloatChunkElems elements, one lane per element;
// three launches on one stream, ordered by the launches alone:
//   size   a workgroup per chunk finds each element's digits, keeps them as a
//          16-byte Decimal in digits[chunk * 256 + lane] and writes the
//          chunk's text size into prefix[chunk] (prefix: device memory,
//          nchunks + 1 entries; the last gets 0)
//   prefix LaunchPbRunPrefix scans the sizes
//   place  a workgroup per chunk: an array longer than its cap is marked
//          (err 3) and gets nothing written; else the chunk's text is laid
//          out in LDS from `digits` and leaves with 16-byte stores at
//          dst + (prefix[chunk] - prefix[first]). A chunk whose text is not
//          the size the size pass measured writes nothing and marks err 4.
// Keeping the digits beat formatting the source a second time in the place
// pass at every size measured (profiles/json_float_print.txt), and a pinned
// host source is read once.
constexpr uint32_t kJsonFloatChunkElems = 256;
constexpr uint32_t JSON_FLOAT32 = 8, JSON_FLOAT64 = 9;  // json2pb::kArrayKindFloat / kArrayKindDouble
struct JsonFloatJob {
    uint8_t* dst;  // device-writable, never null
    uint64_t cap;
    uint32_t first_chunk, nchunks;  // nchunks >= 1
};
struct JsonFloatChunk {
    const void* src;  // this chunk's first element (device-readable, naturally aligned)
    uint32_t count;   // 1..kJsonFloatChunkElems
    uint32_t kind;    // JSON_FLOAT32 or JSON_FLOAT64
    uint32_t job;
    uint32_t last;    // 1: the array's last chunk (no comma after its last element)
};
struct JsonFloatResult {
    uint64_t len;  // text size (also when it did not fit)
    int32_t err;   // zero before the launch; 3 or 4 afterwards when the array failed
    int32_t pad;
};
struct JsonFloatTables {
    const JsonFloatJob* jobs = nullptr;      // device-readable (pinned host)
    int njobs = 0;
    const JsonFloatChunk* chunks = nullptr;  // device-readable (pinned host)
    int nchunks = 0;
    uint32_t* prefix = nullptr;  // device memory, nchunks + 1 entries
    void* digits = nullptr;      // device memory, nchunks * kJsonFloatChunkElems * 16 bytes
    JsonFloatResult* res = nullptr;  // device-writable (pinned host), njobs
};
int LaunchJsonFloatPrint(const JsonFloatTables& t, hipStream_t s);

// JSON number arrays and nested number rows
// (gpu/json_number_print_kernels.hip): `count` elements of one kind in device
// (or pinned host) memory, PbRunKind 0..6 or JSON_FLOAT32 / JSON_FLOAT64,
// become "v,v,...,v", "[v,v,...,v]" or, with a table of row ends (row_ends[r]
// = the elements in rows 0..r, no row empty), "[[v,..],[v,..],..]" in device
// memory: the inverse of LaunchJsonNumberText. The rules, the punctuation
// among them, are base/number_print.h, the code json::FormatNumberRows runs.
// The elements are cut into chunks of kJsonNumberPrintChunkElems, a lane per
// element, and the row ends into blocks of as many rows, a lane per row; a
// chunk's text holds the punctuation in front of each of its elements ("[[",
// "," or "],[") and, behind the job's last element, its "]]". All jobs share
// four launches on one stream, ordered by the launches alone:
//   size    a workgroup per chunk: each element's text size (a float's digits
//           are kept as a 16-byte Decimal in digits[chunk * 256 + lane], as
//           the float printer keeps them; integers and bools keep nothing)
//           plus its punctuation; the chunk's sum goes to prefix[chunk]
//           (prefix: device memory, nchunks + 1 entries; the last gets 0).
//           The row starts inside a chunk are found by one lower-bound search
//           of row_ends for the chunk's first element, the same in every
//           lane, and a look at the <= 256 entries from there on, which are
//           all that can fall into the chunk when the table ascends. The
//           first chunk of a job also sets bad[job] to 0xFFFFFFFF.
//   rows    a workgroup per row block: row r is bad when row_ends[r] <=
//           row_ends[r - 1], row_ends[r] > count, or r is the last row and
//           row_ends[r] != count; atomicMin of r into bad[job]. Not launched
//           when no job has rows.
//   prefix  LaunchPbRunPrefix scans the sizes
//   place   a workgroup per chunk: a job with a bad row (err 1, first_bad) or
//           longer than its cap (err 3, len the size needed) is marked by its
//           first chunk and gets nothing written; else the chunk's text is
//           laid out in LDS and leaves with 16-byte stores at dst +
//           (prefix[chunk] - prefix[first]). A chunk whose text is not the
//           size the size pass measured writes nothing and marks err 4.
// A job has at least one chunk: "[]" is a chunk of no elements. Nothing is
// quadratic: a lane reads its element, at most one row end in the chunk
// passes and two in the rows pass, and the search is logarithmic in rows.
constexpr uint32_t kJsonNumberPrintChunkElems = 256;
struct JsonNumberPrintJob {
    const void* src;           // device-readable, naturally aligned; null only with count 0
    const uint32_t* row_ends;  // device-readable; null unless form 2
    uint8_t* dst;              // device-writable, never null
    uint64_t cap;
    uint32_t count, rows;
    uint32_t kind;
    uint32_t form;  // number_print::Form: 0 bare, 1 bracketed, 2 nested
    uint32_t first_chunk, nchunks;        // nchunks = max(1, ceil(count / 256))
    uint32_t first_row_block, nrow_blocks;  // nrow_blocks = ceil(rows / 256)
};
struct JsonNumberPrintResult {
    uint64_t len;        // text size (also with err 3); 0 with err 1
    uint32_t first_bad;  // 0xFFFFFFFF before the launch; with err 1 the lowest bad row
    int32_t err;         // zero before the launch; 1, 3 or 4 afterwards when the job failed
};
struct JsonNumberPrintTables {
    const JsonNumberPrintJob* jobs = nullptr;  // device-readable (pinned host)
    int njobs = 0;
    uint32_t nchunks = 0, nrow_blocks = 0;
    uint32_t* prefix = nullptr;  // device memory, nchunks + 1 entries
    uint32_t* bad = nullptr;     // device memory, njobs entries
    void* digits = nullptr;      // device memory, nchunks * 256 * 16 bytes; null when no job prints floats
    JsonNumberPrintResult* res = nullptr;  // device-writable (pinned host), njobs
};
int LaunchJsonNumberPrint(const JsonNumberPrintTables& t, hipStream_t s);

// Records as JSON objects (gpu/json_records_kernels.hip): the columns of the
// record builder, each with a key, become [{"k0":cell,"k1":cell,...},...] in
// device memory (base/json_records.h has the rules, json::FormatRecordObjects
// is the host twin). The shape is the record builder's and easier: a key
// prefix does not depend on what follows it. A column is cut into chunks of
// kJsonRecordsChunkElems elements (a string column's element is a byte) and
// into groups of 64, a wave each; records are taken 256 to a workgroup. All
// jobs share seven launches on one stream, ordered by the launches alone:
//   init     copies the job and column tables and the key prefixes to device
//            memory, resets each job's offender word and zeroes the group
//            behind each column's last element
//   size     number and string columns (a base64 cell follows from the row
//            length alone): a lane per element, a grid over the chunks of
//            every column of every job. A wave scans the text lengths of its
//            group: elem_incl[e] becomes the text bytes of the group's
//            elements up to and including e (two bytes: a group holds at most
//            64 * 25), groups[] the group's sum, and a float's digits are kept
//            as a 16-byte Decimal so that no later pass formats it again
//   prefix   LaunchPbRunPrefix over groups[]. The text before element e is
//            then its group's prefix plus elem_incl[e - 1] inside the group:
//            two loads, no walk
//   measure  a lane per record: a cell's inner bytes are the difference of two
//            such texts plus the commas between a number row's elements (a
//            base64 cell: 4 * ceil(len / 3)), into col_cell[]; the text before
//            the row's first element goes into col_delta[]. The record's size
//            with the punctuation in front of and behind it goes into
//            row_size[], the workgroup's sum into block_off[]. A bad table
//            goes into bad[] through one atomic min on row << 4 | column
//   prefix   LaunchPbRunPrefix over block_off[]: an entry per 256 records and
//            one per job for its total
//   heads    a lane per record: row 0's lane writes the job's result; a job
//            with a bad table (err 1) or longer than its cap (err 3) gets
//            nothing written here or later. Else the record's offset is its
//            block's plus a scan inside the workgroup; the lane writes the ','
//            or '[' in front, every key prefix, every cell's opening and
//            closing [ ] or " ", the '}' and the outer ']' (an empty cell is
//            complete with that), and col_delta[] becomes the distance from
//            "text before element e" to "offset of element e in dst"
//   place    a lane per element, a workgroup per chunk of every column. The
//            rows that meet the chunk lie between two lower-bound searches of
//            row_ends that are the same in every lane; a lane finds its own
//            row between them. It stores its element's text at the column's
//            delta, and the ',' in front of an element that does not start a
//            row; a base64 column stores the four symbols of the group that
//            begins at each row offset divisible by 3. A chunk with an
//            element whose text is not the size measured, or with a store
//            that would leave the text, writes nothing and marks err 4
// No workgroup waits for another; a record's lane does work bounded by the
// column count and the longest prefix, an element's lane by the logarithm of
// the rows; every store is compared with the job's size, which is at most
// its cap. The job and column tables and the prefixes are device-readable
// (pinned host) arrays, res a device-writable one; the rest is device memory.
constexpr uint32_t kJsonRecordsChunkElems = 256;
constexpr uint32_t kJsonRecordsGroupElems = 64;
constexpr uint32_t kJsonRecordsBlockRows = 256;
constexpr uint32_t kJsonRecordsPrefixStride = 260;  // json_records::kMaxPrefixBytes, in whole words
struct JsonRecordsColumn {
    const void* src;           // count elements, naturally aligned
    const uint32_t* row_ends;  // rows entries; null for a scalar column (count == rows)
    uint32_t count;
    uint32_t kind, text;       // number_print::Kind or 7; json_records::Text
    uint32_t job;              // its record job
    uint32_t first_chunk, nchunks;  // nchunks = ceil(count / kJsonRecordsChunkElems); over all columns of all jobs
    uint32_t first_row;        // in col_cell and col_delta: rows entries
    uint32_t first_group;      // in groups: count / 64 + 1 entries (not for base64)
    uint32_t first_elem;       // in elem_incl: count entries (not for base64)
    uint32_t first_digit;      // in digits: count entries (float kinds only)
    uint32_t prefix_len;       // of its kJsonRecordsPrefixStride bytes in the prefix table
    uint32_t pad;
};
struct JsonRecordsJob {
    uint8_t* dst;  // any alignment; null only with cap 0
    uint64_t cap;
    uint32_t rows;  // >= 1
    uint32_t brackets;
    uint32_t ncols, first_col;
    uint32_t first_rblock;  // ceil(rows / kJsonRecordsBlockRows) row blocks; job k's entries of block_off start at
                            // first_rblock + k (its blocks, then one entry for its total)
    uint32_t first_row;     // in row_size
    uint32_t fixed;         // per record: the prefixes and '}'
    uint32_t pad;
};
struct JsonRecordsResult {
    uint64_t len;         // text size (also when it did not fit)
    uint32_t first_bad;   // with err 1
    uint32_t bad_column;  // with err 1
    int32_t err;          // 0, 1, 3, 4
};
struct JsonRecordsTables {
    const JsonRecordsJob* jobs = nullptr;
    int njobs = 0;
    const JsonRecordsColumn* cols = nullptr;
    int ncols = 0;                           // of all jobs
    const uint8_t* prefixes = nullptr;       // ncols * kJsonRecordsPrefixStride, 4-byte aligned
    JsonRecordsJob* jobs_dev = nullptr;      // njobs
    JsonRecordsColumn* cols_dev = nullptr;   // ncols
    uint8_t* prefixes_dev = nullptr;         // ncols * kJsonRecordsPrefixStride, 4-byte aligned
    uint32_t nchunks = 0, nrblocks = 0, ngroups = 0, nrows = 0, ncolrows = 0, nelems = 0, ndigits = 0;  // of all jobs
    uint32_t* groups = nullptr;          // ngroups
    uint16_t* elem_incl = nullptr;       // nelems
    void* digits = nullptr;              // ndigits * 16 bytes, 16-byte aligned
    uint32_t* row_size = nullptr;        // nrows
    uint32_t* col_cell = nullptr;        // ncolrows
    uint32_t* col_delta = nullptr;       // ncolrows
    uint32_t* block_off = nullptr;       // nrblocks + njobs
    unsigned long long* bad = nullptr;   // njobs
    JsonRecordsResult* res = nullptr;    // njobs
};
int LaunchJsonRecordsPrint(const JsonRecordsTables& t, hipStream_t s);

// JSON structural index (gpu/json_kernels.hip): out_pos receives, in order,
// the byte offsets of every unescaped '"' and of every { } [ ] : , outside
// strings; count_dev the number found (positions past max_out are dropped
// and err |= 2); err |= 1 when a string is left open at the end. n < 4 GiB.
// JSON integer arrays (K6 parse half): element i of an array is the text
// between separators seps[i] and seps[i+1] (the '[' / ',' / ']' positions of
// the structural index); one lane per element trims whitespace and parses
// -?[0-9]+ into out[i] as int64. Any element that is not such an integer
// (a float, a literal, out of int64 range) sets *bad = 1: the host then
// parses the array itself. *bad must be 0 before the launch.
int LaunchJsonIntArray(const char* text, const uint32_t* seps, uint32_t n, int64_t* out, int32_t* bad,
                       hipStream_t s);
// JSON number arrays (floats among them): json_number_array_kernel, in the
// shape of the integer kernel above (a lane per element, 256 per workgroup,
// the workgroup's text span staged in LDS, memory read directly when the
// span exceeds the window), converts each trimmed element with
// base/decimal_to_double.h, the code the host reader runs. All jobs share
// one launch: job j owns the blocks [first_block, first_block +
// ceil(count / 256)). Output by mode:
//   JSON_PARSE_NUMBERS  out: 8 bytes of payload per element, classes: a byte
//                       per element (0 int64, 1 uint64, 2 double bits)
//   JSON_PARSE_FLOAT64  out: the double per element (an integer class is
//                       converted to the double of its value, so "-0" is +0.0)
//   JSON_PARSE_FLOAT32  out: (float) of that double, rounded in integers
// res[j].bad: the lowest index of an element outside the RFC 8259 number
// grammar (atomicMin), 0xFFFFFFFF when there is none; when it is set nothing
// of the job's output may be trusted. An element that needs exact arithmetic
// (more than 19 significant digits that do not decide the rounding, or more
// than kMaxDeviceNumberChars characters) gets nothing written to out; its
// index goes to redo[slot] with slot taken from the atomic counter
// res[j].n_redo, which keeps counting past redo_cap (slots >= redo_cap are
// dropped). The counters live in device memory (res_dev, njobs entries,
// initialised by the launch) and are copied to res_out (device-writable,
// pinned host or device) by a last small kernel, so the host needs no atomics
// across the bus.
constexpr uint32_t JSON_PARSE_NUMBERS = 0, JSON_PARSE_FLOAT64 = 1, JSON_PARSE_FLOAT32 = 2;
struct JsonNumberJob {
    const char* text;      // device-readable (pinned host or device)
    const uint32_t* seps;  // count + 1 separator offsets into text; element i is (seps[i], seps[i+1])
    void* out;             // device-writable, naturally aligned for the mode
    uint8_t* classes;      // JSON_PARSE_NUMBERS only
    uint32_t* redo;        // redo_cap entries, may be null when redo_cap is 0
    uint32_t count;        // 1 .. 2^32 - 2
    uint32_t mode;
    uint32_t redo_cap;
    uint32_t first_block;
};
struct JsonNumberResult {
    uint32_t bad;
    uint32_t n_redo;
};
int LaunchJsonNumberArrays(const JsonNumberJob* jobs, int njobs, uint32_t nblocks, JsonNumberResult* res_dev,
                           JsonNumberResult* res_out, hipStream_t s);
// The two small kernels around it, for other job kernels that keep a pair of
// counters per job in device memory: res_dev[0, njobs) = {0xFFFFFFFF, 0}, and
// res_out[0, njobs) = res_dev[0, njobs).
int LaunchJsonNumberResultInit(JsonNumberResult* res_dev, int njobs, hipStream_t s);
int LaunchJsonNumberResultPublish(const JsonNumberResult* res_dev, JsonNumberResult* res_out, int njobs,
                                  hipStream_t s);

// JSON number text with no separator table: bare "v,v,...,v", "[v,...,v]" or
// "[[v,..],[v,..],..]" in device (or pinned) memory -> the outputs of
// JSON_PARSE_* above. The device finds the elements and the rows itself; the
// shape rules are base/number_text.h, the code json::ParseNumberText runs.
// A text is cut into chunks of kJsonTextChunkBytes; all jobs share the
// launches, ordered by the stream alone (no count is read back between them):
//   count   a workgroup per chunk counts its ',' and ']' bytes into prefix
//           (and resets the job's state, and copies the job to device memory
//           for the passes that follow)
//   prefix  LaunchPbRunPrefix scans both tables
//   parse   a workgroup per chunk stages it with 16 bytes before and 112
//           after in LDS, ranks its commas, and lanes take the pieces that
//           follow them in rounds (a chunk holds 0 to kJsonTextChunkBytes
//           pieces; the text's first chunk also takes the piece before any
//           comma): piece index = commas before the chunk + rank + 1. A piece
//           that leaves the staged window is read from memory directly. The
//           lane that holds the k-th ']' of the text writes row_ends[k] (the
//           last ']' closes the outer array and ends no row).
//   publish a lane per job combines depth, brackets and counts into res
// Stores go below cap (out, classes), row_cap and redo_cap only. An element a
// lane does not decide takes a slot of redo as the pair {index, offset of the
// byte after the comma before it}; n_redo keeps counting past redo_cap.
constexpr uint32_t kJsonTextChunkBytes = 4096;
struct JsonTextJob {
    const char* text;    // device-readable, any alignment
    void* out;           // device-writable, naturally aligned for the mode; may be null when cap is 0
    uint8_t* classes;    // JSON_PARSE_NUMBERS only
    uint32_t* row_ends;  // null: depth 2 is malformed
    uint32_t* redo;      // 2 * redo_cap entries, may be null when redo_cap is 0
    uint32_t n;          // 1 .. 2^32 - 2 bytes
    uint32_t mode;
    uint32_t cap, row_cap, redo_cap;
    uint32_t first_chunk, nchunks;  // nchunks = ceil(n / kJsonTextChunkBytes)
};
struct JsonTextResult {
    uint32_t first_bad;  // lowest index of a piece that does not fit, 0xFFFFFFFF when all do
    uint32_t n_redo;
    uint32_t depth, count, rows;  // count / rows: what the text holds, also beyond cap / row_cap
    uint32_t pad;
};
constexpr size_t kJsonTextStateBytes = 20;  // number_text::TextState, per job
struct JsonTextTables {
    const JsonTextJob* jobs = nullptr;  // device-readable (pinned host)
    int njobs = 0;
    JsonTextJob* jobs_dev = nullptr;    // device memory, njobs: the count pass copies the table there
    uint32_t nchunks = 0;        // of all jobs
    uint32_t* prefix = nullptr;  // device memory, 2 * nchunks + 2 entries
    void* state = nullptr;       // device memory, njobs * kJsonTextStateBytes
    uint32_t* n_redo = nullptr;  // device memory, njobs entries
    JsonTextResult* res = nullptr;  // device-writable (pinned host), njobs
};
int LaunchJsonNumberText(const JsonTextTables& t, hipStream_t s);

// Base64 of bytes in device memory (gpu/base64_kernels.hip; the arithmetic is
// base/base64.h, the code base64_encode / base64_decode run on the host).
// All jobs share one launch: job j owns the blocks [first_block, first_block
// + chunks), a workgroup takes one chunk of kBase64ChunkBytes data bytes <->
// kBase64ChunkSymbols symbols, a lane 12 bytes <-> 16 symbols. src and dst
// may have any byte alignment and must not overlap.
//   encode  n data bytes at src -> (n + 2) / 3 * 4 symbols at dst, '=' padded;
//           chunks = ceil(n / kBase64ChunkBytes)
//   decode  n bytes of canonical text at src (a body of alphabet symbols and
//           p = 0..2 trailing '=') -> the data at dst, which must hold
//           n / 4 * 3 + (n % 4) * 3 / 4 bytes; chunks = ceil(n /
//           kBase64ChunkSymbols). res[j].bad: the lowest offset of a body
//           byte outside the alphabet (atomicMin), n when the body length
//           m = n - p breaks a rule (m % 4 == 1, or p > 0 and n % 4 != 0),
//           0xFFFFFFFF for canonical text; when it is set nothing of dst may
//           be trusted. res[j].n_redo: the decoded length m / 4 * 3 +
//           (m % 4) * 3 / 4. The counters live in device memory (res_dev,
//           initialised by the launch) and a last small kernel copies them to
//           res_out (device-writable, pinned host or device).
constexpr uint32_t kBase64ChunkBytes = 3072, kBase64ChunkSymbols = 4096;
struct Base64Job {
    const uint8_t* src;  // device-readable, never null
    uint8_t* dst;        // device-writable, never null
    uint32_t n;          // 1 .. 2^32 - 1: data bytes (encode), text bytes (decode)
    uint32_t first_block;
};
int LaunchBase64Encode(const Base64Job* jobs, int njobs, uint32_t nblocks, hipStream_t s);
int LaunchBase64Decode(const Base64Job* jobs, int njobs, uint32_t nblocks, JsonNumberResult* res_dev,
                       JsonNumberResult* res_out, hipStream_t s);

// Base64 rows in device memory (gpu/base64_kernels.hip; the rules are
// base/base64_rows.h, the code json::EncodeBase64Rows / DecodeBase64Rows run
// on the host): (bytes, row_ends) <-> the text "b0","b1",.. or ["b0",..] of a
// JSON array of base64 strings. All jobs of a call share the launches, ordered
// by the stream alone; the job table is copied to device memory first, and
// nothing is written to a dst before the job's verdict (ok[job]) is known.
// Workgroups of 256 lanes; no workgroup waits for another.
//   encode  rows    a lane per row reads row_ends once and keeps what it read
//                   in ends[] (the later passes read only that copy, so a table
//                   that changes under the call cannot move a store): a
//                   decrease, an end above n or a last end other than n goes
//                   into bad[job] (atomicMin); the symbols of the row,
//                   (len + 2) / 3 * 4, are summed over the block of 256 rows
//                   by a workgroup scan: the symbols in front of the row
//                   within its block into rowoff[], the block's sum into
//                   prefix[]
//           prefix  LaunchPbRunPrefix over the row blocks
//           verdict a lane per job: len, err 1 / 3, ok[job], the brackets
//           punct   a lane per row writes its two quotes and its comma at
//                   symbols before the row + 3 * row (+ 1 with brackets), so
//                   empty rows cost the place pass nothing
//           place   a workgroup per kBase64RowsEncodeChunkBytes of source,
//                   staged in LDS with two bytes beyond. The rows that meet
//                   the chunk are found by two lower-bound searches of ends[].
//                   A 3-byte group is counted from its row's start and belongs
//                   to the chunk that holds its first byte. Up to
//                   kBase64RowsSegmentRows rows: per row a lane takes four
//                   groups of the row's part of the chunk, the symbols go
//                   through an LDS image and leave with 16-byte stores
//                   (wg::copy_out_shifted). More rows: a lane takes the groups
//                   that start in its 12 bytes, finds its row by a lower-bound
//                   search (again at every row end it crosses, so a run of
//                   empty rows is skipped in one search) and stores four bytes
//                   per group. Every store is compared with cap.
//   decode  a chunk is kBase64RowsDecodeChunkBytes of text, a lane 16 bytes.
//           The in-string mask is the prefix-xor of all quotes (no escape can
//           hide one: a backslash is refused). What crosses a chunk's edge is
//           one of nine states: outside a string after token kind k
//           (json_string_rows::Kind, 5 states) or inside at body offset mod 4
//           (4 states); the byte before a chunk is read from the text.
//           scan    a workgroup per chunk: a bit per byte for symbols, '=',
//                   quotes and the tokens outside; the quote parity in front of
//                   each lane by ballot, the last quote in front of it by a
//                   max-scan (its distance gives the body offset). For the two
//                   ways the mask can start: decoded bytes (a group belongs to
//                   the lane and chunk of its first symbol and reads up to 3
//                   bytes on, never past n), closing quotes, the lowest byte
//                   that breaks a local rule, first token, first ']', exit.
//                   The lanes in front of the chunk's first quote also compute
//                   size and lowest fault for each of the four phases
//           carry   a workgroup per job composes the chunks' maps over the nine
//                   states (4 bits per image in a 64-bit word), picks every
//                   chunk's entry, judges its first token against the true
//                   predecessor, writes the two size tables and the job's
//                   lowest offender, first ']', depth and final state
//           prefix  LaunchPbRunPrefix over both tables at once
//           verdict a lane per job: a ']' at depth 0, the end rule, cap and
//                   row_cap (err 3), ok[job], the result words
//           place   a workgroup per chunk with its entry: groups decoded with
//                   Decode4 into an LDS image that leaves with 16-byte stores;
//                   the lane that holds the k-th closing quote writes
//                   row_ends[k]. Sizes that differ from the scan's: err 4
// res is device-writable pinned host memory; everything else device memory.
constexpr uint32_t kBase64RowsEncodeChunkBytes = kBase64ChunkBytes;
constexpr uint32_t kBase64RowsDecodeChunkBytes = 4096;
constexpr uint32_t kBase64RowsBlockRows = 256;
constexpr uint32_t kBase64RowsSegmentRows = 8;
// decode, per chunk: for the entries outside / inside size, closing quotes,
// lowest offender, first token, first ']', exit; then size and lowest offender
// of the leading in-string run for the four phases; then the chosen entry
constexpr uint32_t kBase64RowsInfoWords = 24;
constexpr uint32_t kBase64RowsStateWords = 4;  // per job: lowest offender, final state, depth, first ']'
struct Base64RowsJob {
    const uint8_t* src;
    uint8_t* dst;
    const uint32_t* row_ends;  // encode: the table to read. decode: the row ends to write
    uint64_t cap;
    uint32_t n, rows;          // decode: rows is row_cap
    uint32_t brackets;         // encode
    uint32_t first_chunk, nchunks;  // encode: ceil(n / encode chunk); decode: ceil(n / decode chunk); may be 0
    uint32_t first_rblock;          // encode: ceil(rows / kBase64RowsBlockRows) row blocks
    uint32_t first_row;             // encode: the job's rows in ends[] and rowoff[]
    uint32_t pad;
};
struct Base64RowsResult {
    uint64_t len;  // bytes written (with err 3: the size needed)
    uint32_t rows, first_bad, depth;
    int32_t err;  // 0, 1, 3, 4
};
struct Base64RowsTables {
    const Base64RowsJob* jobs = nullptr;  // pinned host
    int njobs = 0;
    Base64RowsJob* jobs_dev = nullptr;
    uint32_t nchunks = 0, nrblocks = 0, nrows = 0;  // of all jobs
    uint32_t* prefix = nullptr;  // encode: nrblocks + 1. decode: 2 * (nchunks + 1)
    uint32_t* ends = nullptr;    // encode: nrows
    uint32_t* rowoff = nullptr;  // encode: nrows
    uint32_t* info = nullptr;    // decode: nchunks * kBase64RowsInfoWords
    uint32_t* bad = nullptr;     // njobs
    int32_t* ok = nullptr;       // njobs
    uint32_t* state = nullptr;   // decode: njobs * kBase64RowsStateWords
    Base64RowsResult* res = nullptr;  // njobs, pinned host
};
int LaunchBase64EncodeRows(const Base64RowsTables& t, hipStream_t s);
int LaunchBase64DecodeRows(const Base64RowsTables& t, hipStream_t s);

// JSON string bodies and UTF-8 in device memory (gpu/json_string_kernels.hip;
// the rules are base/json_string.h, the code json::EscapeStringBody,
// UnescapeStringBody and Utf8FirstBad run on the host). A job's n bytes are
// cut into chunks of kJsonStringChunkBytes, a workgroup of 256 lanes takes one
// chunk, a lane 16 bytes. src and dst may have any byte alignment. All jobs of
// a call share the launches, ordered by the stream alone; the job table is
// copied to device memory first, and nothing is written to a dst before the
// job's verdict (ok[job], device memory) is known.
//   escape    size    a workgroup per chunk: the escaped size of the chunk into
//                     prefix[], and for jobs with rows the escaped bytes in
//                     front of each 64-byte group of the chunk into groups[]
//             rows    a lane per row: a row end below its predecessor, or a
//                     last end other than n, goes into bad[job] (atomicMin)
//             prefix  LaunchPbRunPrefix over the chunk sizes
//             verdict a lane per job: len, err 1 / 3, ok[job], the quotes of a
//                     single string
//             punct   a lane per row writes its two quotes and its comma: the
//                     escaped bytes in front of a row end are its group's
//                     prefix plus at most 63 sizes recomputed from the source
//             place   a workgroup per chunk escapes it into an LDS image sized
//                     for the worst case (6 x chunk; there is no direct-store
//                     path for a chunk that expands) and copies it out with
//                     16-byte stores; a chunk that needs no escape leaves
//                     straight from the staged source. With rows, a chunk that
//                     meets at most 8 rows copies one segment per row, one that
//                     meets more lets every lane store its own bytes, each
//                     finding its row in row_ends by binary search
//   unescape  scan    a workgroup per chunk: whether a backslash starts an
//                     escape depends on the parity of the backslashes before
//                     it, so the chunk computes output size, lowest bad offset
//                     and carry-out for carry-in 0 and 1. The parity span of
//                     chunk k is [kC - 16, (k + 1)C - 16): with it a chunk
//                     knows which of the 16 bytes before it start an escape,
//                     which is all an escape's tail (at most 11 bytes) and the
//                     low half of a surrogate pair need to know
//             carry   a workgroup per job composes the chunks' two-state maps,
//                     picks each chunk's result and lowers bad[job]
//             prefix, verdict as above
//             place   a workgroup per chunk, with its carry-in: an escape
//                     belongs to the chunk that holds its backslash (it reads
//                     up to 11 bytes beyond its end); bytes are compacted into
//                     an LDS image by a scan of the lanes' counts and leave
//                     with 16-byte stores
//   validate          one launch: a lead byte is judged by the lane that holds
//                     it (up to 3 bytes beyond), a continuation byte from up to
//                     3 bytes before; lowest offender by atomicMin; then a
//                     lane per job publishes
//   rows      the text of a JSON array of strings ("r0","r1",.. or ["r0",..],
//             base/json_string_rows.h) -> the decoded bytes and row ends. Two
//             facts cross a chunk's edge: the backslash parity, as above, and
//             whether the edge lies inside a string. A chunk is entered
//             outside a string, inside one after an even backslash run, or
//             inside after an odd one.
//             scan    a workgroup per chunk, for each of the three entries: the
//                     quotes no escape covers from the starter masks, the
//                     in-string mask as their prefix-xor (within a lane's 16
//                     bits, by ballot parity across the wave, then across the
//                     four waves), and from it the decoded size, the closing
//                     quotes, the lowest offender a chunk can decide alone (a
//                     bad escape inside, a byte outside that is no token, a
//                     token its predecessor inside the chunk does not allow),
//                     the kind and offset of the first token outside (only the
//                     chunk before knows its predecessor), the first ']'
//                     outside, and the exit: inside (even / odd), or outside
//                     with the kind of the last token, "none" when all of the
//                     chunk outside strings is whitespace. A chunk with neither
//                     quote nor backslash (nor a backslash in the 16 bytes
//                     before) is all copy when entered inside and all
//                     punctuation when entered outside
//             carry   a workgroup per job composes the chunks' maps over seven
//                     states (outside after START [ "close , ], inside even /
//                     odd), picks every chunk's entry, judges its first token
//                     against the true predecessor, writes the two size tables
//                     (bytes, closing quotes) and the job's lowest offender,
//                     first ']', depth and final state. No lane reads
//                     backwards through the text: the predecessor travels in
//                     the state
//             prefix  LaunchPbRunPrefix over both tables at once
//             verdict a lane per job: a ']' at depth 0, the end rule, cap and
//                     row_cap (err 3), ok[job], the result words
//             place   a workgroup per chunk with its entry: the bytes inside
//                     strings are compacted into an LDS image and leave with
//                     16-byte stores; the lane that holds the k-th closing
//                     quote writes row_ends[k] = the bytes before the chunk +
//                     the decoded bytes before that quote in the chunk
// res is device-writable pinned host memory; everything else device memory.
constexpr uint32_t kJsonStringChunkBytes = 4096;
constexpr uint32_t kJsonStringNone = 0xFFFFFFFFu;
constexpr uint32_t kJsonStringBlockRows = 256;
constexpr uint32_t kJsonStringGroupBytes = 64;
constexpr uint32_t kJsonStringInfoWords = 6;  // per chunk: size, bad for carry-in 0 / 1, the map, the carry-in
// rows, per chunk: for each of the three entries size, closing quotes, lowest
// offender, first token, first ']', exit; then the entry state the carry chose
constexpr uint32_t kJsonStringRowsEntryWords = 6;
constexpr uint32_t kJsonStringRowsInfoWords = 3 * kJsonStringRowsEntryWords + 2;
constexpr uint32_t kJsonStringRowsStateWords = 4;  // per job: lowest offender, final state, depth, first ']'
struct JsonStringJob {
    const uint8_t* src;
    uint8_t* dst;              // null for validate
    const uint32_t* row_ends;  // escape: null for a single string. unescape rows: the row ends to write
    uint64_t cap;
    uint32_t n, rows;          // unescape rows: rows is row_cap
    uint32_t quote;                 // escape without rows: 1 = surrounding quotes
    uint32_t first_chunk, nchunks;  // nchunks = ceil(n / kJsonStringChunkBytes), may be 0
    uint32_t first_rblock;          // ceil(rows / kJsonStringBlockRows) row blocks
    uint32_t first_group;           // in groups: nchunks * 64 entries (jobs with rows)
    uint32_t pad;
};
struct JsonStringResult {
    uint64_t len;        // bytes written (with err 3: the size needed)
    uint32_t first_bad;  // with err 1
    int32_t err;         // 0, 1, 3, 4 (the source changed between two passes; dst may be partly written)
};
struct JsonStringRowsResult {
    uint64_t len;  // decoded bytes (with err 3: what the text holds)
    uint32_t rows, first_bad, depth;
    int32_t err;  // 0, 1, 3, 4
};
struct JsonStringTables {
    const JsonStringJob* jobs = nullptr;  // pinned host
    int njobs = 0;
    JsonStringJob* jobs_dev = nullptr;    // njobs
    uint32_t nchunks = 0, nrblocks = 0, ngroups = 0;  // of all jobs
    uint32_t* prefix = nullptr;  // nchunks + 1 (escape, unescape), 2 * (nchunks + 1) (unescape rows)
    uint32_t* groups = nullptr;  // ngroups (escape with rows)
    uint32_t* info = nullptr;    // nchunks * kJsonStringInfoWords (unescape), * kJsonStringRowsInfoWords (rows)
    uint32_t* bad = nullptr;     // njobs
    int32_t* ok = nullptr;       // njobs (escape, unescape)
    uint32_t* state = nullptr;   // njobs * kJsonStringRowsStateWords (unescape rows)
    JsonStringResult* res = nullptr;  // njobs, pinned host
    JsonStringRowsResult* rows_res = nullptr;  // njobs, pinned host (unescape rows, in place of res)
};
int LaunchJsonStringEscape(const JsonStringTables& t, hipStream_t s);
int LaunchJsonStringUnescape(const JsonStringTables& t, hipStream_t s);
int LaunchJsonStringValidate(const JsonStringTables& t, hipStream_t s);
int LaunchJsonStringUnescapeRows(const JsonStringTables& t, hipStream_t s);

// scratch must hold JsonIndexScratchBytes(n).
size_t JsonIndexScratchBytes(uint64_t n);
int LaunchJsonIndex(const uint8_t* in, uint64_t n, uint32_t* out_pos, uint64_t max_out, uint64_t* count_dev,
                    int* err_dev, void* scratch, hipStream_t s);

// ---- resident copy worker (persistent kernel fed from a pinned ring;
// kernels.hip explains the protocol). Created on first use per device
// (nullptr: unavailable); instances exit after idle_us without work or
// max_us of life and are relaunched on demand.
struct ResidentRing;
ResidentRing* ResidentRingFor(int device, uint32_t idle_us, uint32_t max_us, uint32_t groups);
// Publish segs as ring batches (groups of <= kInlineSegments segments that
// never split a message; msg_of as in LaunchBatchedCopyCrc32cMessages, null:
// one message per segment). crc_out (pinned host, null: copy only) receives
// one CRC32C per message; a null segment dst only checksums. [first, last]
// are the batches' sequence numbers. 0 on success.
int ResidentSubmit(ResidentRing* r, const Segment* segs, const int* msg_of, int nseg, uint32_t* crc_out,
                   uint64_t* first_seq, uint64_t* last_seq);
// Whether every batch of [first, last] is complete (reads pinned memory).
bool ResidentDone(ResidentRing* r, uint64_t first_seq, uint64_t last_seq);
// Watchdog: relaunch when no instance is on the device but a batch waits.
void ResidentKick(ResidentRing* r);
// Stop every instance and wait for them (process exit).
void ResidentShutdown();
struct ResidentStats {
    int64_t launches = 0, batches = 0, ring_full_waits = 0;
};
ResidentStats GetResidentStats();

// ---- synchronous helpers (fiber-friendly waits)
// CRC32C of device buffers; results to host.
int Crc32cDevice(const void* const* ptrs, const uint64_t* lens, int n, uint32_t* out_host, int device);
int Crc32cOfBuf(const Buf& b, uint32_t* out, int device);  // any block kinds

}  // namespace gpu
}  // namespace mrpc
