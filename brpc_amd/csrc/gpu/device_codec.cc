#include "gpu/device_codec.h"

#include <algorithm>
#include <atomic>
#include <vector>

#include "base/buf.h"
#include "base/flags.h"
#include "base/pb_records.h"
#include "base/pb_rows.h"
#include "base/pool.h"
#include "gpu/codec_batch.h"
#include "gpu/gpu.h"
#include "gpu/hbm_pool.h"
#include "gpu/kernels.h"
#include "gpu/scoped.h"
#include "policy/device_payload.h"

DEFINE_int32(device_payload_block_kb, 2,
             "uncompressed KiB per device snappy block of a compressed device payload (one wave each); 1..64. "
             "Smaller blocks spread a payload over more waves: on MI355X the 64 KiB text leg runs 121k QPS at 2 KiB "
             "(ratio 1.96) against 80k at 4 KiB (ratio 2.24)");

DEFINE_int32(device_split_skip, 8,
             "chunks of 4 KiB a serial hop of DeviceSplitRows' chase spans at least (1..64; 1: no skip table, one hop "
             "per chunk). A hop costs 260 ns on MI355X whatever it spans; the skip table costs a pass of gathers and "
             "4 bytes of scratch per byte of message");

namespace mrpc {
namespace gpu {

namespace {

std::atomic<int64_t> g_encodes{0}, g_enc_bytes{0}, g_enc_out{0}, g_decodes{0}, g_dec_bytes{0}, g_bad_tables{0},
    g_dec_err{0}, g_scans{0}, g_runs{0}, g_run_bytes{0}, g_run_elems{0}, g_run_err{0};
std::atomic<int64_t> g_built{0}, g_built_fields{0}, g_built_bytes{0}, g_build_err{0};
std::atomic<int64_t> g_built_row_jobs{0}, g_built_rows{0}, g_built_row_bytes{0};
std::atomic<int64_t> g_split_row_jobs{0}, g_split_rows{0};
std::atomic<int64_t> g_split_record_jobs{0}, g_split_records{0};
std::atomic<int64_t> g_built_record_jobs{0}, g_built_records{0}, g_built_record_bytes{0};

uint32_t varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) {
        v >>= 7;
        ++n;
    }
    return n;
}

uint32_t block_len(const DeviceSnappyLayout& lay, uint64_t len, uint32_t i) {
    const uint64_t off = (uint64_t)i * lay.block_ulen;
    return (uint32_t)std::min<uint64_t>(lay.block_ulen, len - off);
}

// A table that cannot describe `len` bytes inside the region is refused
// before anything runs on the device: every block lies inside the region,
// holds at least its header, and the blocks cover the payload exactly.
bool table_ok(const DeviceSnappyBlocks& j) {
    const DeviceSnappyLayout& l = j.lay;
    if (!j.region || !j.dst || !j.clen || j.len == 0 || l.block_ulen == 0 || l.block_ulen > kSnappyMaxBlock ||
        l.nblocks == 0 || l.stride == 0) {
        return false;
    }
    if ((uint64_t)l.nblocks != (j.len + l.block_ulen - 1) / l.block_ulen) return false;
    for (uint32_t i = 0; i < l.nblocks; ++i) {
        const uint64_t c = j.clen[i];
        const uint32_t ul = block_len(l, j.len, i);
        if (c <= varint_len(ul) || c > l.stride || (uint64_t)i * l.stride + c > j.region_len) return false;
    }
    return true;
}

void fill_index(const CodecRequest& req, size_t row, DevicePayloadIndex* out) {
    out->nfields = req.scan_nfields[row];
    const uint64_t* f = req.scan_fields.data() + row * 2 * kCodecScanFields;
    const int n = std::max(0, std::min<int>(out->nfields, (int)kCodecScanFields));
    out->fields.assign(f, f + 2 * n);
}

// A CodecRequest from the object pool, emptied but with its vectors'
// capacity (the encode and decode of every device-body RPC build one).
struct PooledRequest {
    CodecRequest* r;
    PooledRequest() : r(get_object<CodecRequest>()) { r->Reset(); }
    ~PooledRequest() { return_object(r); }
    PooledRequest(const PooledRequest&) = delete;
    PooledRequest& operator=(const PooledRequest&) = delete;
};

}  // namespace

DeviceSnappyLayout DeviceSnappyLayoutFor(size_t len) {
    DeviceSnappyLayout l;
    l.block_ulen = (uint32_t)std::max(1, std::min(64, FLAGS_device_payload_block_kb)) << 10;
    l.stride = (uint32_t)((SnappyMaxCompressedLength(l.block_ulen) + 15) & ~15ull);
    l.nblocks = (uint32_t)((len + l.block_ulen - 1) / l.block_ulen);
    return l;
}

int DeviceSnappyEncode(const void* src, size_t len, void* dst, const DeviceSnappyLayout& lay, uint32_t* clen,
                       int device) {
    if (!src || !dst || len == 0 || lay.nblocks == 0) return -1;
    const char* s = static_cast<const char*>(src);
    char* d = static_cast<char*>(dst);
    PooledRequest pooled;
    CodecRequest& req = *pooled.r;
    req.comp.resize(lay.nblocks);
    for (uint32_t i = 0; i < lay.nblocks; ++i) {
        req.comp[i] = SnappyJob{s + (size_t)i * lay.block_ulen, d + (size_t)i * lay.stride, block_len(lay, len, i),
                                lay.stride};
    }
    req.comp_max_ulen = (uint32_t)std::min<uint64_t>(lay.block_ulen, len);
    if (RunCodecRequest(&req, device) != 0) return -1;
    uint64_t out = 0;
    for (uint32_t i = 0; i < lay.nblocks; ++i) {
        if (req.comp_err[i] || req.comp_len[i] > lay.stride || req.comp_len[i] == 0) return -1;
        clen[i] = req.comp_len[i];
        out += clen[i];
    }
    g_encodes.fetch_add(1, std::memory_order_relaxed);
    g_enc_bytes.fetch_add((int64_t)len, std::memory_order_relaxed);
    g_enc_out.fetch_add((int64_t)out, std::memory_order_relaxed);
    return 0;
}

int DeviceSnappyDecode(const DeviceSnappyBlocks* jobs, int n, int* err, DevicePayloadIndex* index, int device) {
    PooledRequest pooled;
    CodecRequest& req = *pooled.r;
    std::vector<size_t> first(n, 0), count(n, 0), scan_row(n, (size_t)-1);
    for (int k = 0; k < n; ++k) {
        const DeviceSnappyBlocks& j = jobs[k];
        err[k] = 0;
        if (!table_ok(j)) {
            err[k] = 1;
            g_bad_tables.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        first[k] = req.pieces.size();
        count[k] = j.lay.nblocks;
        char* d = static_cast<char*>(j.dst);
        for (uint32_t i = 0; i < j.lay.nblocks; ++i) {
            const uint32_t ul = block_len(j.lay, j.len, i);
            const uint32_t h = varint_len(ul);
            // headerless pieces: the block's varint length is known from the
            // table, the decoder starts at its first element
            req.pieces.push_back(SnappyPiece{j.region + (size_t)i * j.lay.stride + h, d + (size_t)i * j.lay.block_ulen,
                                             j.clen[i] - h, ul});
        }
        req.pieces_max_ulen = std::max(req.pieces_max_ulen, std::min<uint32_t>(j.lay.block_ulen, (uint32_t)j.len));
        if (j.scan && index) {
            scan_row[k] = req.scans.size();
            req.scans.push_back(PbScanJob{static_cast<const uint8_t*>(j.dst), j.len});
            req.scan_piece_first.push_back((uint32_t)first[k]);
            req.scan_piece_count.push_back(j.lay.nblocks);
        }
    }
    if (req.pieces.empty()) return 0;
    if (RunCodecRequest(&req, device) != 0) return -1;
    for (int k = 0; k < n; ++k) {
        if (err[k]) continue;
        for (size_t p = first[k]; p < first[k] + count[k]; ++p) {
            if (req.piece_err[p]) {
                err[k] = 2;
                g_dec_err.fetch_add(1, std::memory_order_relaxed);
                break;
            }
        }
        if (err[k]) continue;
        g_decodes.fetch_add(1, std::memory_order_relaxed);
        g_dec_bytes.fetch_add((int64_t)jobs[k].len, std::memory_order_relaxed);
        if (scan_row[k] != (size_t)-1) {
            fill_index(req, scan_row[k], &index[k]);
            g_scans.fetch_add(1, std::memory_order_relaxed);
        }
    }
    return 0;
}

int DevicePbScan(const void* const* bufs, const uint64_t* lens, int n, DevicePayloadIndex* index, int device) {
    if (n <= 0) return 0;
    CodecRequest req;
    for (int k = 0; k < n; ++k) req.scans.push_back(PbScanJob{static_cast<const uint8_t*>(bufs[k]), lens[k]});
    if (RunCodecRequest(&req, device) != 0) return -1;
    for (int k = 0; k < n; ++k) fill_index(req, (size_t)k, &index[k]);
    g_scans.fetch_add(n, std::memory_order_relaxed);
    return 0;
}

bool DevicePayloadField(const DevicePayloadIndex& index, uint32_t number, uint64_t* off, uint64_t* len) {
    const int n = std::min<int>(index.nfields, (int)(index.fields.size() / 2));
    for (int k = 0; k < n; ++k) {
        const uint64_t key = index.fields[2 * k];
        if ((key >> 3) != number || (key & 7) != 2) continue;
        const uint64_t v = index.fields[2 * k + 1];
        *off = v >> 32;
        *len = v & 0xFFFFFFFFull;
        return true;
    }
    return false;
}

int DeviceDecodePackedRuns(DevicePackedRun* runs, int n, int device) {
    if (n <= 0) return 0;
    CodecRequest req;
    std::vector<size_t> first(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        DevicePackedRun& r = runs[i];
        first[i] = req.dec_runs.size();
        r.count = 0;
        r.err = 0;
        if (!r.src || !r.dst || r.kind > PB_RUN_BOOL || r.len > 0xFFFFFFFFull) {
            r.err = 2;
            continue;
        }
        if (r.len == 0) continue;
        const uint32_t head = (uint32_t)req.dec_runs.size();
        for (uint64_t o = 0; o < r.len; o += kPbRunDecodeChunkBytes) {
            PbRunDecodeChunk c;
            c.run = static_cast<const uint8_t*>(r.src);
            c.dst = r.dst;
            c.offset = (uint32_t)o;
            c.len = (uint32_t)std::min<uint64_t>(kPbRunDecodeChunkBytes, r.len - o);
            c.first = head;
            c.kind = r.kind;
            req.dec_runs.push_back(c);
        }
    }
    first[n] = req.dec_runs.size();
    if (req.dec_runs.empty()) return 0;
    // every run's final byte comes back with the batch (the host cannot read
    // HBM): one still carrying a continuation bit ends inside a varint
    PinnedBlock tail_block((size_t)n);
    if (!tail_block) return -1;
    uint8_t* tail = tail_block.as<uint8_t>();
    for (int i = 0; i < n; ++i) {
        tail[i] = 0;
        if (first[i + 1] > first[i]) {
            req.d2h.push_back(Segment{static_cast<const uint8_t*>(runs[i].src) + runs[i].len - 1, tail + i, 1});
        }
    }
    if (RunCodecRequest(&req, device) != 0) return -1;
    for (int i = 0; i < n; ++i) {
        DevicePackedRun& r = runs[i];
        if (r.err || r.len == 0) continue;
        uint64_t count = 0;
        for (size_t k = first[i]; k < first[i + 1]; ++k) {
            count += req.dec_counts[k];
            if (req.dec_err[k]) r.err = 1;
        }
        if (tail[i] & 0x80) r.err = 1;
        if (r.err) {
            g_run_err.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        r.count = count;
        g_runs.fetch_add(1, std::memory_order_relaxed);
        g_run_bytes.fetch_add((int64_t)r.len, std::memory_order_relaxed);
        g_run_elems.fetch_add((int64_t)count, std::memory_order_relaxed);
    }
    return 0;
}

namespace {

constexpr uint32_t kMaxFieldNumber = (1u << 29) - 1;

uint32_t elem_bytes(uint32_t kind) {
    return kind == PB_RUN_BOOL || kind == kDeviceFieldBytes ? 1 : (kind <= PB_RUN_SINT32 ? 4 : 8);
}

// Worst-case payload of a field, or false when the field is refused by what
// the host can check without its pointers.
bool field_worst(const DeviceMessageField& f, bool headerless, uint64_t* worst) {
    if (f.kind > kDeviceFieldBytes) return false;
    if (!headerless && (f.number == 0 || f.number > kMaxFieldNumber)) return false;
    const uint64_t per = f.kind == PB_RUN_BOOL || f.kind == kDeviceFieldBytes
                             ? 1
                             : (f.kind == PB_RUN_UINT32 || f.kind == PB_RUN_SINT32 ? 5 : 10);
    if (f.count > 0xFFFFFFFFull / per) return false;
    *worst = f.count * per;
    return true;
}

bool field_emitted(const DeviceMessageField& f) { return f.count > 0 || f.kind == kDeviceFieldBytes; }

// Worst-case size of the whole message; false when refused.
bool message_worst(const DeviceMessageField* fields, int n, bool headerless, uint64_t* total) {
    *total = 0;
    if (n < 0 || n > (int)kCodecScanFields || (n > 0 && !fields)) return false;
    for (int i = 0; i < n; ++i) {
        uint64_t worst = 0;
        if (!field_worst(fields[i], headerless, &worst)) return false;
        if (!field_emitted(fields[i])) continue;
        *total += worst;
        if (!headerless) *total += varint_len((uint64_t)fields[i].number << 3) + varint_len(worst);
    }
    return true;
}

bool job_ok(const DeviceMessageJob& j, bool headerless) {
    uint64_t total = 0;
    if (!j.dst || !message_worst(j.fields, j.nfields, headerless, &total)) return false;
    for (int i = 0; i < j.nfields; ++i) {
        const DeviceMessageField& f = j.fields[i];
        if (f.count > 0 && (!f.src || ((uintptr_t)f.src & (elem_bytes(f.kind) - 1)))) return false;
    }
    return true;
}

// Every job that passes the host checks becomes one message of one codec
// request; a job without an emitted field is an empty message and needs no
// device work.
int build_messages(DeviceMessageJob* jobs, int n, bool headerless, int device) {
    if (n <= 0) return 0;
    PooledRequest pooled;
    CodecRequest& req = *pooled.r;
    std::vector<int> row(n, -1);  // job -> its message in the request
    for (int k = 0; k < n; ++k) {
        DeviceMessageJob& j = jobs[k];
        j.len = 0;
        j.err = 0;
        if (!job_ok(j, headerless)) {
            j.err = 2;
            const int nf = j.fields ? std::min(j.nfields, (int)kCodecScanFields) : 0;
            for (int i = 0; i < nf; ++i) j.fields[i].off = j.fields[i].len = 0;
            g_build_err.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        PbMsgJob m;
        m.dst = static_cast<uint8_t*>(j.dst);
        m.cap = j.cap;
        m.first_field = (uint32_t)req.msg_fields.size();
        m.nfields = 0;
        for (int i = 0; i < j.nfields; ++i) {
            DeviceMessageField& f = j.fields[i];
            f.off = f.len = 0;
            if (!field_emitted(f)) continue;
            PbMsgField mf;
            mf.msg = (uint32_t)req.msgs.size();
            mf.tag = (f.number << 3) | 2;
            mf.first_chunk = (uint32_t)req.msg_chunks.size();
            mf.headerless = headerless ? 1 : 0;
            mf.pad = 0;
            const uint32_t eb = elem_bytes(f.kind);
            const uint64_t per = f.kind == kDeviceFieldBytes ? kPbMsgBytesChunk : kPbRunChunkElems;
            for (uint64_t o = 0; o < f.count; o += per) {
                PbMsgChunk c;
                c.src = static_cast<const uint8_t*>(f.src) + o * eb;
                c.count = (uint32_t)std::min<uint64_t>(per, f.count - o);
                c.kind = f.kind;
                c.field = (uint32_t)req.msg_fields.size();
                c.first = mf.first_chunk;
                req.msg_chunks.push_back(c);
            }
            mf.nchunks = (uint32_t)req.msg_chunks.size() - mf.first_chunk;
            req.msg_fields.push_back(mf);
            ++m.nfields;
        }
        if (m.nfields == 0) continue;
        row[k] = (int)req.msgs.size();
        req.msgs.push_back(m);
    }
    if (!req.msgs.empty() && RunCodecRequest(&req, device) != 0) return -1;
    for (int k = 0; k < n; ++k) {
        DeviceMessageJob& j = jobs[k];
        if (j.err) continue;
        int64_t nf = 0;
        if (row[k] >= 0) {
            const PbMsgResult& r = req.msg_res[row[k]];
            j.len = r.len;
            j.err = r.err;
            if (j.err) {
                g_build_err.fetch_add(1, std::memory_order_relaxed);
                continue;
            }
            size_t at = req.msgs[row[k]].first_field;
            for (int i = 0; i < j.nfields; ++i) {
                DeviceMessageField& f = j.fields[i];
                if (!field_emitted(f)) continue;
                f.off = req.msg_field_res[at].off;
                f.len = req.msg_field_res[at].len;
                ++at;
                ++nf;
            }
        }
        g_built.fetch_add(1, std::memory_order_relaxed);
        g_built_fields.fetch_add(nf, std::memory_order_relaxed);
        g_built_bytes.fetch_add((int64_t)j.len, std::memory_order_relaxed);
    }
    return 0;
}

struct ArenaBlock {
    size_t n;
    int device;
};
void free_arena_block(void* p, void* arg) {
    ArenaBlock* a = static_cast<ArenaBlock*>(arg);
    HbmFree(p, a->n, a->device);
    delete a;
}

}  // namespace

uint64_t DeviceMessageWorstCaseBytes(const DeviceMessageField* fields, int n) {
    uint64_t total = 0;
    return message_worst(fields, n, false, &total) ? total : 0;
}

int DeviceBuildMessages(DeviceMessageJob* jobs, int n, int device) { return build_messages(jobs, n, false, device); }

int BuildDeviceMessage(DeviceMessageField* fields, int n, Buf* out, int device) {
    uint64_t worst = 0;
    if (!out || !message_worst(fields, n, false, &worst)) {
        g_build_err.fetch_add(1, std::memory_order_relaxed);
        return 2;
    }
    // an arena block even for an empty message: the job needs a destination
    const size_t cap = (size_t)std::max<uint64_t>(worst, 16);
    HbmBlock dst(cap, device);
    if (!dst) return -1;
    DeviceMessageJob job;
    job.fields = fields;
    job.nfields = n;
    job.dst = dst.p;
    job.cap = cap;
    const int rc = DeviceBuildMessages(&job, 1, device);
    if (rc != 0 || job.err != 0 || job.len == 0) return rc != 0 ? -1 : job.err;
    ArenaBlock* a = new ArenaBlock{cap, device};
    if (AppendDevice(out, dst.p, (size_t)job.len, device, free_arena_block, a) != 0) {
        delete a;
        return -1;
    }
    dst.release();  // the Buf block owns it now
    return 0;
}

int DeviceEncodePackedRuns(DevicePackedEncodeRun* runs, int n, int device) {
    if (n <= 0) return 0;
    std::vector<DeviceMessageField> fields(n);
    std::vector<DeviceMessageJob> jobs(n);
    for (int i = 0; i < n; ++i) {
        fields[i].kind = runs[i].kind;
        fields[i].src = runs[i].src;
        fields[i].count = runs[i].count;
        jobs[i].fields = &fields[i];
        // a bare run has no bytes kind: refused through the field count
        jobs[i].nfields = runs[i].kind <= PB_RUN_BOOL ? 1 : -1;
        jobs[i].dst = runs[i].dst;
        jobs[i].cap = runs[i].cap;
    }
    const int rc = build_messages(jobs.data(), n, true, device);
    for (int i = 0; i < n; ++i) {
        runs[i].bytes = rc == 0 && jobs[i].err == 0 ? jobs[i].len : 0;
        runs[i].err = rc == 0 ? jobs[i].err : 0;
    }
    return rc;
}

namespace {

// What the host can check of a rows job without reading device memory.
bool rows_job_ok(const DeviceRowsJob& j) {
    if (pb_rows::WorstCaseBytes(j.number, j.inner, j.kind, j.count, j.rows) == 0) return false;
    if (!j.row_ends || ((uintptr_t)j.row_ends & 3) != 0 || !j.dst) return false;
    return j.count == 0 || (j.src && ((uintptr_t)j.src & (pb_rows::SourceBytes(j.kind) - 1)) == 0);
}

static_assert(kDeviceRecordMaxColumns == pb_records::kRecordMaxColumns, "one column limit");

// The job as the rules see it; false when it has no column table to look at.
bool records_view(const DeviceRecordsJob& j, pb_records::Column* cols, pb_records::Job* out) {
    if (!j.columns || j.ncols < 1 || j.ncols > kDeviceRecordMaxColumns) return false;
    for (uint32_t c = 0; c < j.ncols; ++c) {
        const DeviceRecordColumn& in = j.columns[c];
        cols[c].inner = in.inner;
        cols[c].kind = in.kind;
        cols[c].src = in.src;
        cols[c].count = in.count;
        cols[c].row_ends = in.row_ends;
    }
    out->number = j.number;
    out->columns = cols;
    out->ncols = j.ncols;
    out->rows = j.rows;
    return true;
}

// What the host can check of a records job without reading device memory.
bool records_job_ok(const DeviceRecordsJob& j) {
    pb_records::Column cols[pb_records::kRecordMaxColumns];
    pb_records::Job view;
    if (!records_view(j, cols, &view) || pb_records::WorstCaseBytes(view) == 0 || !j.dst) return false;
    for (uint32_t c = 0; c < j.ncols; ++c) {
        const DeviceRecordColumn& col = j.columns[c];
        if (((uintptr_t)col.row_ends & 3) != 0) return false;
        if (col.count > 0 && (!col.src || ((uintptr_t)col.src & (pb_rows::SourceBytes(col.kind) - 1)) != 0)) return false;
    }
    return true;
}

// What the two fronts of the builder say about their job type: the host's
// gate, the columns, where the offender goes and which counters a built job
// moves. A rows job is one column, headerless (base/pb_records.h) when its
// inner is 0.
bool build_job_ok(const DeviceRowsJob& j) { return rows_job_ok(j); }
bool build_job_ok(const DeviceRecordsJob& j) { return records_job_ok(j); }
uint32_t build_ncols(const DeviceRowsJob&) { return 1; }
uint32_t build_ncols(const DeviceRecordsJob& j) { return j.ncols; }
DeviceRecordColumn build_column(const DeviceRowsJob& j, uint32_t) {
    return DeviceRecordColumn{j.inner, j.kind, j.src, j.count, j.row_ends};
}
const DeviceRecordColumn& build_column(const DeviceRecordsJob& j, uint32_t c) { return j.columns[c]; }
// the row part of the row << 4 | column key: a rows job has one column
void build_offender(DeviceRowsJob& j, uint32_t row, uint32_t) { j.first_bad = row; }
void build_offender(DeviceRecordsJob& j, uint32_t row, uint32_t column) {
    j.first_bad = row;
    j.bad_column = column;
}
void build_count(const DeviceRowsJob& j) {
    g_built_row_jobs.fetch_add(1, std::memory_order_relaxed);
    g_built_rows.fetch_add((int64_t)j.rows, std::memory_order_relaxed);
    g_built_row_bytes.fetch_add((int64_t)j.len, std::memory_order_relaxed);
}
void build_count(const DeviceRecordsJob& j) {
    g_built_record_jobs.fetch_add(1, std::memory_order_relaxed);
    g_built_records.fetch_add((int64_t)j.rows, std::memory_order_relaxed);
    g_built_record_bytes.fetch_add((int64_t)j.len, std::memory_order_relaxed);
}

// The builder behind DeviceBuildRows and DeviceBuildRecords. The jobs go to a
// pool stream of their own rather than into the cross-RPC codec batch: a job
// brings scratch sized by its rows and groups (a word per row and two per row
// and column), which the batch's recycled tables do not hold, and its seven
// launches share nothing with the small codec jobs of other RPCs.
template <typename Job>
int build_records(Job* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    std::vector<int> live;  // the jobs that go to the device, in order
    uint64_t nchunks = 0, nrblocks = 0, ngroups = 0, nrows = 0, ncolrows = 0, ncols = 0;
    for (int i = 0; i < n; ++i) {
        Job& j = jobs[i];
        j.len = 0;
        build_offender(j, 0xFFFFFFFFu, 0xFFFFFFFFu);
        j.err = 0;
        if (!build_job_ok(j)) {
            j.err = 2;
            g_build_err.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        const uint32_t jcols = build_ncols(j);
        for (uint32_t c = 0; c < jcols; ++c) {
            const DeviceRecordColumn& col = build_column(j, c);
            nchunks += (col.count + kPbRowsChunkElems - 1) / kPbRowsChunkElems;
            if (pb_rows::IsVarintKind(col.kind)) ngroups += col.count / kPbRowsGroupElems + 2;
        }
        nrblocks += (j.rows + kPbRowsBlockRows - 1) / kPbRowsBlockRows;
        nrows += j.rows;
        ncolrows += j.rows * jcols;
        ncols += jcols;
        live.push_back(i);
    }
    if (live.empty()) return 0;
    // one grid per pass, 32-bit table indices
    if (nchunks > 0x7FFFFFFFull || nrblocks > 0x7FFFFFFFull || ngroups > 0x7FFFFFFFull || ncolrows > 0x7FFFFFFFull) {
        return -1;
    }
    const size_t nlive = live.size();
    // the most aligned first: jobs, columns and offender words are all 8-byte
    const size_t jobs_bytes = nlive * sizeof(PbRecordsJob), cols_bytes = (size_t)ncols * sizeof(PbRowsJob);
    PinnedBlock tables(jobs_bytes + cols_bytes + nlive * sizeof(PbRecordsResult));
    const size_t words = (size_t)ngroups + (size_t)nrows + 2 * (size_t)ncolrows + (size_t)nrblocks + nlive;
    HbmBlock scratch(jobs_bytes + cols_bytes + nlive * sizeof(uint64_t) + words * sizeof(uint32_t), device);
    if (!tables || !scratch) return -1;
    PbRecordsJob* tj = tables.as<PbRecordsJob>();
    PbRowsJob* tc = reinterpret_cast<PbRowsJob*>(tj + nlive);
    PbRecordsResult* tr = reinterpret_cast<PbRecordsResult*>(tc + ncols);
    PbRecordsTables t;
    for (size_t k = 0; k < nlive; ++k) {
        const Job& j = jobs[live[k]];
        PbRecordsJob& o = tj[k];
        o.dst = static_cast<uint8_t*>(j.dst);
        o.cap = j.cap;
        o.rows = (uint32_t)j.rows;
        o.number = j.number;
        o.ncols = build_ncols(j);
        o.first_col = (uint32_t)t.ncols;
        o.first_rblock = t.nrblocks;
        o.first_row = t.nrows;
        for (uint32_t c = 0; c < o.ncols; ++c) {
            const DeviceRecordColumn& in = build_column(j, c);
            PbRowsJob& col = tc[t.ncols++];
            col.src = in.src;
            col.row_ends = in.row_ends;
            col.dst = o.dst;
            col.cap = o.cap;
            col.count = (uint32_t)in.count;
            col.rows = o.rows;
            col.number = j.number;
            col.inner = in.inner;
            col.kind = in.kind;
            col.first_chunk = t.nchunks;
            col.nchunks = (uint32_t)((in.count + kPbRowsChunkElems - 1) / kPbRowsChunkElems);
            col.first_rblock = (uint32_t)k;  // a column's: its record job
            col.first_row = t.ncolrows;
            col.first_group = t.ngroups;
            t.nchunks += col.nchunks;
            t.ncolrows += o.rows;
            if (pb_rows::IsVarintKind(in.kind)) t.ngroups += col.count / kPbRowsGroupElems + 2;
        }
        t.nrblocks += (uint32_t)((j.rows + kPbRowsBlockRows - 1) / kPbRowsBlockRows);
        t.nrows += o.rows;
        tr[k] = PbRecordsResult{0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0};
    }
    t.jobs = tj;
    t.njobs = (int)nlive;
    t.cols = tc;
    t.jobs_dev = scratch.as<PbRecordsJob>();
    t.cols_dev = reinterpret_cast<PbRowsJob*>(t.jobs_dev + nlive);
    t.bad = reinterpret_cast<unsigned long long*>(t.cols_dev + t.ncols);
    t.groups = reinterpret_cast<uint32_t*>(t.bad + nlive);
    t.row_size = t.groups + t.ngroups;
    t.col_pay = t.row_size + t.nrows;
    t.col_delta = t.col_pay + t.ncolrows;
    t.block_off = t.col_delta + t.ncolrows;
    t.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchPbRecordsBuild(t, s); }) != 0) return -1;
    for (size_t k = 0; k < nlive; ++k) {
        Job& j = jobs[live[k]];
        j.len = tr[k].len;
        j.err = tr[k].err;
        if (j.err == 1) build_offender(j, tr[k].first_bad, tr[k].bad_column);
        if (j.err) {
            g_build_err.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        build_count(j);
    }
    return 0;
}

// The job's records (or rows) into a fresh arena block of the worst-case
// size, appended to *out as one DEVICE block.
template <typename Job>
int build_into_buf(const Job& job, uint64_t worst, Buf* out, int device) {
    if (!out || worst == 0) {
        g_build_err.fetch_add(1, std::memory_order_relaxed);
        return 2;
    }
    const size_t cap = (size_t)std::max<uint64_t>(worst, 16);
    HbmBlock dst(cap, device);
    if (!dst) return -1;
    Job j = job;
    j.dst = dst.p;
    j.cap = cap;
    const int rc = build_records(&j, 1, device);
    if (rc != 0 || j.err != 0) return rc != 0 ? -1 : j.err;
    ArenaBlock* a = new ArenaBlock{cap, device};
    if (AppendDevice(out, dst.p, (size_t)j.len, device, free_arena_block, a) != 0) {
        delete a;
        return -1;
    }
    dst.release();  // the Buf block owns it now
    return 0;
}

}  // namespace

uint64_t DeviceRowsWorstCaseBytes(const DeviceRowsJob& job) {
    return pb_rows::WorstCaseBytes(job.number, job.inner, job.kind, job.count, job.rows);
}

int DeviceBuildRows(DeviceRowsJob* jobs, int n, int device) { return build_records(jobs, n, device); }

int BuildDeviceRows(const DeviceRowsJob& job, Buf* out, int device) {
    return build_into_buf(job, DeviceRowsWorstCaseBytes(job), out, device);
}

uint64_t DeviceRecordsWorstCaseBytes(const DeviceRecordsJob& job) {
    pb_records::Column cols[pb_records::kRecordMaxColumns];
    pb_records::Job view;
    return records_view(job, cols, &view) ? pb_records::WorstCaseBytes(view) : 0;
}

int DeviceBuildRecords(DeviceRecordsJob* jobs, int n, int device) { return build_records(jobs, n, device); }

int BuildDeviceRecords(const DeviceRecordsJob& job, Buf* out, int device) {
    return build_into_buf(job, DeviceRecordsWorstCaseBytes(job), out, device);
}

namespace {

static_assert(kDeviceSplitMaxBytes < (1ull << 28), "the splitter's offender word and row table hold 28-bit offsets");

bool split_job_ok(const DeviceRowsSplitJob& j) {
    if (!pb_rows::FieldsOk(j.number, j.inner, j.kind) || j.n > kDeviceSplitMaxBytes) return false;
    if ((j.n > 0 && !j.msg) || (j.cap > 0 && !j.values) || (j.row_cap > 0 && !j.row_ends)) return false;
    return ((uintptr_t)j.values & (pb_rows::SourceBytes(j.kind) - 1)) == 0 && ((uintptr_t)j.row_ends & 3) == 0;
}

}  // namespace

// On a pool stream of its own, as DeviceBuildRows and for its reason: the
// scratch is sized by the message.
int DeviceSplitRows(DeviceRowsSplitJob* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    std::vector<int> live;
    uint64_t nchunks = 0, nrblocks = 0, nochunks = 0, nrows = 0;
    for (int i = 0; i < n; ++i) {
        DeviceRowsSplitJob& j = jobs[i];
        j.count = j.rows = j.others = 0;
        j.first_bad = ~0ull;
        j.err = 0;
        if (!split_job_ok(j)) {
            j.err = pb_rows::kSplitRefused;
            continue;
        }
        if (j.n == 0) {  // no field: no row, nothing to launch
            g_split_row_jobs.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        live.push_back(i);
    }
    if (live.empty()) return 0;
    const size_t nlive = live.size();
    PinnedBlock tables(nlive * (sizeof(PbSplitJob) + sizeof(PbSplitResult)));
    if (!tables) return -1;
    PbSplitJob* tj = tables.as<PbSplitJob>();
    PbSplitResult* tr = reinterpret_cast<PbSplitResult*>(tj + nlive);
    PbSplitTables t;
    for (size_t k = 0; k < nlive; ++k) {
        const DeviceRowsSplitJob& j = jobs[live[k]];
        PbSplitJob& o = tj[k];
        o.msg = static_cast<const uint8_t*>(j.msg);
        o.values = j.values;
        o.row_ends = j.row_ends;
        o.cap = j.cap;
        o.row_cap = j.row_cap;
        o.n = (uint32_t)j.n;
        o.number = j.number;
        o.inner = j.inner;
        o.kind = j.kind;
        const bool varints = pb_rows::WireIsVarint(j.kind);
        const uint64_t most_rows = j.n / 2;  // a row has a tag and a length
        o.first_chunk = (uint32_t)nchunks;
        o.nchunks = (uint32_t)((j.n + kPbSplitChunk - 1) / kPbSplitChunk);
        o.first_rblock = (uint32_t)nrblocks;
        o.nrblocks = (uint32_t)std::max<uint64_t>(1, (most_rows + kPbSplitBlockRows - 1) / kPbSplitBlockRows);
        o.first_ochunk = (uint32_t)nochunks;
        o.nochunks = varints ? 0
                             : (uint32_t)((std::min(j.cap, j.n / pb_rows::SourceBytes(j.kind)) + kPbSplitOutChunk - 1) /
                                          kPbSplitOutChunk);
        o.first_row = (uint32_t)nrows;
        nchunks += o.nchunks;
        nrblocks += o.nrblocks;
        nochunks += o.nochunks;
        if (varints) {
            nrows += std::min(j.row_cap, most_rows);
            t.any_varint = true;
        }
        tr[k] = PbSplitResult{0, 0, 0, kPbSplitNone, 0};
    }
    // exit[] (later the row table) by itself; then the 8-byte tables, then the words
    const size_t exit_bytes = (size_t)nchunks * kPbSplitChunk * sizeof(uint32_t);
    const size_t jobs_bytes = (nlive * sizeof(PbSplitJob) + 7) & ~(size_t)7;
    const size_t masks = 2 * (size_t)nchunks * 64;
    const size_t words = (size_t)nchunks * 64 + 3 * ((size_t)nchunks + 1) + (size_t)nrblocks + 1 + (size_t)nrows +
                         3 * nlive;
    t.skip_hops = (uint32_t)std::max(1, std::min(64, FLAGS_device_split_skip));
    const bool skips = t.skip_hops > 1 && nchunks > t.skip_hops;  // a short message is chased directly
    if (!skips) t.skip_hops = 1;
    HbmBlock exit_block(exit_bytes, device), skip_block(skips ? exit_bytes : 0, device);
    HbmBlock scratch(jobs_bytes + masks * sizeof(uint64_t) + (words + (skips ? nchunks : 0)) * sizeof(uint32_t), device);
    if (!exit_block || !scratch || (skips && !skip_block)) return -1;
    t.skip = skip_block.as<uint32_t>();
    t.jobs = tj;
    t.njobs = (int)nlive;
    t.nchunks = (uint32_t)nchunks;
    t.nrblocks = (uint32_t)nrblocks;
    t.nochunks = (uint32_t)nochunks;
    t.nrows = (uint32_t)nrows;
    t.exit = exit_block.as<uint32_t>();
    t.jobs_dev = scratch.as<PbSplitJob>();
    t.term_mask = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch.p) + jobs_bytes);
    t.row_mask = t.term_mask + nchunks * 64;
    t.term_group = reinterpret_cast<uint32_t*>(t.row_mask + nchunks * 64);
    t.term_chunk = t.term_group + nchunks * 64;
    t.row_chunk = t.term_chunk + nchunks + 1;
    t.entry = t.row_chunk + nchunks + 1;
    t.block_sum = t.entry + nchunks + 1;
    t.row_bias = t.block_sum + nrblocks + 1;
    t.bad = t.row_bias + nrows;
    t.others = t.bad + nlive;
    t.ok = reinterpret_cast<int32_t*>(t.others + nlive);
    t.land = skips ? reinterpret_cast<uint32_t*>(t.ok + nlive) : nullptr;
    t.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchPbRowsSplit(t, s); }) != 0) return -1;
    for (size_t k = 0; k < nlive; ++k) {
        DeviceRowsSplitJob& j = jobs[live[k]];
        j.err = tr[k].err;
        j.count = tr[k].count;
        j.rows = tr[k].rows;
        j.others = tr[k].others;
        if (j.err == pb_rows::kSplitMalformed || j.err == pb_rows::kSplitUnsupported) j.first_bad = tr[k].first_bad;
        if (j.err) continue;
        g_split_row_jobs.fetch_add(1, std::memory_order_relaxed);
        g_split_rows.fetch_add((int64_t)j.rows, std::memory_order_relaxed);
    }
    return 0;
}

namespace {

constexpr uint64_t kArenaLargestBlock = 256ull << 20;  // gpu/hbm_pool.cc: class 28

// What the host can check of a record split job without reading device memory.
bool record_split_job_ok(const DeviceRecordsSplitJob& j) {
    if (!j.columns || j.ncols < 1 || j.ncols > kDeviceRecordMaxColumns) return false;
    pb_records::SplitColumn cols[pb_records::kRecordMaxColumns];
    for (uint32_t c = 0; c < j.ncols; ++c) {
        cols[c].inner = j.columns[c].inner;
        cols[c].kind = j.columns[c].kind;
        cols[c].scalar = j.columns[c].scalar;
    }
    if (!pb_records::SplitColumnsOk(j.number, cols, j.ncols) || j.n > kDeviceSplitMaxBytes || (j.n > 0 && !j.msg)) {
        return false;
    }
    for (uint32_t c = 0; c < j.ncols; ++c) {
        const DeviceRecordSplitColumn& col = j.columns[c];
        if ((col.cap > 0 && !col.values) || ((uintptr_t)col.values & (pb_rows::SourceBytes(col.kind) - 1)) != 0) return false;
        if (!col.scalar && ((j.row_cap > 0 && !col.row_ends) || ((uintptr_t)col.row_ends & 3) != 0)) return false;
    }
    // the record table is one arena block
    return std::min(j.row_cap, j.n / 2) * j.ncols * sizeof(uint64_t) <= kArenaLargestBlock;
}

}  // namespace

// On a pool stream of its own, as DeviceSplitRows and for its reason.
int DeviceSplitRecords(DeviceRecordsSplitJob* jobs, int n, int device) {
    if (n <= 0) return 0;
    if (!jobs || device < 0) return -1;
    std::vector<int> live;
    size_t ncols = 0;
    for (int i = 0; i < n; ++i) {
        DeviceRecordsSplitJob& j = jobs[i];
        j.rows = j.others = 0;
        j.first_bad = ~0ull;
        j.err = 0;
        for (uint32_t c = 0; j.columns && c < j.ncols && c < kDeviceRecordMaxColumns; ++c) {
            j.columns[c].count = j.columns[c].absent = 0;
        }
        if (!record_split_job_ok(j)) {
            j.err = pb_rows::kSplitRefused;
            continue;
        }
        if (j.n == 0) {  // no field: no record, nothing to launch
            g_split_record_jobs.fetch_add(1, std::memory_order_relaxed);
            continue;
        }
        ncols += j.ncols;
        live.push_back(i);
    }
    if (live.empty()) return 0;
    const size_t nlive = live.size();
    // the most aligned first: every struct here is 8-byte aligned
    PinnedBlock tables(nlive * (sizeof(PbSplitJob) + sizeof(PbRecSplitJob) + sizeof(PbRecSplitResult)) +
                       ncols * sizeof(PbRecSplitCol));
    if (!tables) return -1;
    PbSplitJob* tj = tables.as<PbSplitJob>();
    PbRecSplitJob* rj = reinterpret_cast<PbRecSplitJob*>(tj + nlive);
    PbRecSplitResult* tr = reinterpret_cast<PbRecSplitResult*>(rj + nlive);
    PbRecSplitCol* tc = reinterpret_cast<PbRecSplitCol*>(tr + nlive);
    PbRecSplitTables r;
    PbSplitTables& t = r.front;
    uint64_t nchunks = 0, nrblocks = 0, nbsums = 0, nochunks = 0, nentries = 0, ntags = 0;
    for (size_t k = 0; k < nlive; ++k) {
        const DeviceRecordsSplitJob& j = jobs[live[k]];
        // the row splitter's passes see an occurrence of `number`, whatever it holds
        PbSplitJob& o = tj[k];
        o = PbSplitJob{};
        o.msg = static_cast<const uint8_t*>(j.msg);
        o.n = (uint32_t)j.n;
        o.number = j.number;
        o.kind = pb_rows::kKindBytes;
        o.first_chunk = (uint32_t)nchunks;
        o.nchunks = (uint32_t)((j.n + kPbSplitChunk - 1) / kPbSplitChunk);
        o.nrblocks = 1;
        nchunks += o.nchunks;
        PbRecSplitJob& q = rj[k];
        q = PbRecSplitJob{};
        q.row_cap = j.row_cap;
        q.rec_cap = (uint32_t)std::min(j.row_cap, j.n / 2);  // a record has a tag and a length
        q.first_entry = nentries;
        q.first_tag = (uint32_t)ntags;
        q.first_col = (uint32_t)r.ncols;
        q.ncols = j.ncols;
        q.first_rblock = (uint32_t)nrblocks;
        q.nrblocks = (uint32_t)std::max<uint64_t>(1, ((uint64_t)q.rec_cap + kPbSplitBlockRows - 1) / kPbSplitBlockRows);
        for (uint32_t c = 0; c < j.ncols; ++c) {
            const DeviceRecordSplitColumn& in = j.columns[c];
            PbRecSplitCol& col = tc[r.ncols++];
            col = PbRecSplitCol{};
            col.values = in.values;
            col.row_ends = in.row_ends;
            col.cap = in.cap;
            col.inner = in.inner;
            col.kind = in.kind;
            col.scalar = in.scalar;
            col.job = (uint32_t)k;
            col.index = c;
            col.first_ochunk = (uint32_t)nochunks;
            if (!in.scalar && !pb_rows::WireIsVarint(in.kind)) {
                col.nochunks = (uint32_t)((std::min(in.cap, j.n / pb_rows::SourceBytes(in.kind)) + kPbSplitOutChunk - 1) /
                                          kPbSplitOutChunk);
            } else if (!in.scalar) {
                q.any_varint = 1;
                r.any_varint = true;
            }
            nochunks += col.nochunks;
            col.first_bsum = (uint32_t)nbsums;
            nbsums += q.nrblocks;
        }
        nrblocks += q.nrblocks;
        nentries += (uint64_t)q.rec_cap * q.ncols;
        ntags += q.rec_cap;
        tr[k] = PbRecSplitResult{};
        tr[k].first_bad = kPbSplitNone;
    }
    if (nbsums > 0x7FFFFFFEull || nochunks > 0x7FFFFFFEull || ntags > 0xFFFFFFFFull) return -1;
    const size_t exit_bytes = (size_t)nchunks * kPbSplitChunk * sizeof(uint32_t);
    const size_t masks = 2 * (size_t)nchunks * 64;
    t.skip_hops = (uint32_t)std::max(1, std::min(64, FLAGS_device_split_skip));
    const bool skips = t.skip_hops > 1 && nchunks > t.skip_hops;  // a short message is chased directly
    if (!skips) t.skip_hops = 1;
    // 8-byte tables, then the words
    const size_t eights = masks * sizeof(uint64_t) + nlive * (sizeof(PbSplitJob) + sizeof(PbRecSplitJob)) +
                          r.ncols * sizeof(PbRecSplitCol);
    const size_t words = (size_t)nchunks * 64 + 3 * ((size_t)nchunks + 1) + 2 + (size_t)nbsums + 1 + 3 * nlive +
                         (skips ? (size_t)nchunks : 0) + (size_t)r.ncols * (1 + sizeof(pb_records::SplitColumn) / 4);
    HbmBlock exit_block(exit_bytes, device), skip_block(skips ? exit_bytes : 0, device);
    HbmBlock entry_block(std::max<size_t>(nentries * sizeof(uint64_t), 16), device);
    HbmBlock bias_block(std::max<size_t>((nentries + ntags) * sizeof(uint32_t), 16), device);
    HbmBlock scratch(eights + words * sizeof(uint32_t), device);
    if (!exit_block || !scratch || !entry_block || !bias_block || (skips && !skip_block)) return -1;
    t.any_varint = r.any_varint;
    t.skip = skip_block.as<uint32_t>();
    t.jobs = tj;
    t.njobs = (int)nlive;
    t.nchunks = (uint32_t)nchunks;
    t.nrblocks = 1;
    t.exit = exit_block.as<uint32_t>();
    t.term_mask = scratch.as<uint64_t>();
    t.row_mask = t.term_mask + nchunks * 64;
    t.jobs_dev = reinterpret_cast<PbSplitJob*>(t.row_mask + nchunks * 64);
    r.jobs_dev = reinterpret_cast<PbRecSplitJob*>(t.jobs_dev + nlive);
    r.cols_dev = reinterpret_cast<PbRecSplitCol*>(r.jobs_dev + nlive);
    t.term_group = reinterpret_cast<uint32_t*>(r.cols_dev + r.ncols);
    t.term_chunk = t.term_group + nchunks * 64;
    t.row_chunk = t.term_chunk + nchunks + 1;
    t.entry = t.row_chunk + nchunks + 1;
    t.block_sum = t.entry + nchunks + 1;  // the row splitter's: one block, unused here
    r.block_sum = t.block_sum + 2;
    t.bad = r.block_sum + nbsums + 1;
    t.others = t.bad + nlive;
    t.ok = reinterpret_cast<int32_t*>(t.others + nlive);
    r.absent = reinterpret_cast<uint32_t*>(t.ok + nlive);
    r.specs = reinterpret_cast<pb_records::SplitColumn*>(r.absent + r.ncols);
    t.land = skips ? reinterpret_cast<uint32_t*>(r.specs + r.ncols) : nullptr;
    r.jobs = rj;
    r.cols = tc;
    r.nrblocks = (uint32_t)nrblocks;
    r.nbsums = (uint32_t)nbsums;
    r.nochunks = (uint32_t)nochunks;
    r.entry = entry_block.as<uint64_t>();
    r.bias = bias_block.as<uint32_t>();
    r.rec_tag = r.bias + nentries;
    r.res = tr;
    if (RunOnPoolStream(device, [&](hipStream_t s) { return LaunchPbRecordsSplit(r, s); }) != 0) return -1;
    for (size_t k = 0; k < nlive; ++k) {
        DeviceRecordsSplitJob& j = jobs[live[k]];
        j.err = tr[k].err;
        j.rows = tr[k].rows;
        j.others = tr[k].others;
        for (uint32_t c = 0; c < j.ncols; ++c) {
            j.columns[c].count = tr[k].count[c];
            j.columns[c].absent = tr[k].absent[c];
        }
        if (j.err == pb_rows::kSplitMalformed || j.err == pb_rows::kSplitUnsupported) j.first_bad = tr[k].first_bad;
        if (j.err) continue;
        g_split_record_jobs.fetch_add(1, std::memory_order_relaxed);
        g_split_records.fetch_add((int64_t)j.rows, std::memory_order_relaxed);
    }
    return 0;
}

DeviceCodecStats GetDeviceCodecStats() {
    DeviceCodecStats s;
    s.split_row_jobs = g_split_row_jobs.load();
    s.split_rows = g_split_rows.load();
    s.split_record_jobs = g_split_record_jobs.load();
    s.split_records = g_split_records.load();
    s.built_row_jobs = g_built_row_jobs.load();
    s.built_rows = g_built_rows.load();
    s.built_row_bytes = g_built_row_bytes.load();
    s.built_record_jobs = g_built_record_jobs.load();
    s.built_records = g_built_records.load();
    s.built_record_bytes = g_built_record_bytes.load();
    s.built_messages = g_built.load();
    s.built_fields = g_built_fields.load();
    s.built_bytes = g_built_bytes.load();
    s.build_errors = g_build_err.load();
    s.encodes = g_encodes.load();
    s.encoded_bytes = g_enc_bytes.load();
    s.encoded_out_bytes = g_enc_out.load();
    s.decodes = g_decodes.load();
    s.decoded_bytes = g_dec_bytes.load();
    s.bad_tables = g_bad_tables.load();
    s.decode_errors = g_dec_err.load();
    s.scans = g_scans.load();
    s.packed_runs = g_runs.load();
    s.packed_bytes = g_run_bytes.load();
    s.packed_elems = g_run_elems.load();
    s.packed_errors = g_run_err.load();
    return s;
}

}  // namespace gpu
}  // namespace mrpc
