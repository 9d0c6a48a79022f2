// Bindings of the device kernels for torch tensors. Python passes raw
// device pointers (tensor.data_ptr()) and the HIP stream handle
// (torch.cuda.current_stream().cuda_stream) so the native module never
// links libtorch; the ops run stream-ordered with torch's own work.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "base/time.h"
#include "fiber/fiber.h"
#include "gpu/base64_offload.h"
#include "gpu/copy_engine.h"
#include "gpu/device_codec.h"
#include "policy/device_payload.h"
#include "gpu/gpu.h"
#include "gpu/json_offload.h"
#include "gpu/json_string_offload.h"
#include "gpu/kernels.h"
#include "json/json.h"

namespace py = pybind11;
using namespace mrpc;

static hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

static void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + " failed: " + hipGetErrorString(hipGetLastError()));
}

namespace {
struct ParkedWaiters {
    std::vector<fiber::fiber_t> tids;
    std::vector<int64_t> waited_us;
    std::vector<int> rcs;
    int device = 0;
    uint64_t us = 0;
};
struct ParkArg {
    ParkedWaiters* p;
    size_t i;
};
void* park_on_kernel(void* arg) {
    ParkArg* a = static_cast<ParkArg*>(arg);
    ParkedWaiters* p = a->p;
    const size_t i = a->i;
    delete a;
    hipSetDevice(p->device);
    hipStream_t s = gpu::PoolStream(p->device);
    hipEvent_t ev = gpu::AcquireEvent();
    const int64_t t0 = monotonic_us();
    int rc = -1;
    if (s && ev && gpu::LaunchSleepKernel(p->us, s) == 0 && hipEventRecord(ev, s) == hipSuccess) {
        rc = gpu::WaitEvent(ev);  // parks this fiber, never the worker
    }
    p->waited_us[i] = monotonic_us() - t0;
    p->rcs[i] = rc;
    if (ev) gpu::ReleaseEvent(ev);
    return nullptr;
}
}  // namespace

namespace {
// Device buffer owned for the duration of one benchmark call.
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t n) {
        if (hipMalloc(&p, n ? n : 1) != hipSuccess) p = nullptr;
    }
    ~DevBuf() {
        if (p) hipFree(p);
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p); }
};

// (number, kind, device pointer, count) rows of device_build_message
typedef std::tuple<uint32_t, uint32_t, uintptr_t, uint64_t> MessageFieldRow;
// (number, inner, kind, src, count, row_ends, rows, dst, cap) rows of device_build_rows
typedef std::tuple<uint32_t, uint32_t, uint32_t, uintptr_t, uint64_t, uintptr_t, uint64_t, uintptr_t, uint64_t> RowsJobRow;
// (inner, kind, src, count, row_ends) columns of device_build_records; row_ends 0: a scalar column
typedef std::tuple<uint32_t, uint32_t, uintptr_t, uint64_t, uintptr_t> RecordColumnRow;
// (number, columns, rows, dst, cap) rows of device_build_records
typedef std::tuple<uint32_t, std::vector<RecordColumnRow>, uint64_t, uintptr_t, uint64_t> RecordsJobRow;
// (inner, kind, scalar, values, cap, row_ends) columns and (number, columns,
// msg, n, row_cap) rows of device_split_records
typedef std::tuple<uint32_t, uint32_t, bool, uintptr_t, uint64_t, uintptr_t> RecordSplitColumnRow;
typedef std::tuple<uint32_t, std::vector<RecordSplitColumnRow>, uintptr_t, uint64_t, uint64_t> RecordsSplitJobRow;
// (key, kind, text form, src, count, row_ends) columns and (columns, rows,
// brackets, dst, cap) rows of device_json_print_records
typedef std::tuple<py::bytes, uint32_t, uint32_t, uintptr_t, uint64_t, uintptr_t> RecordPrintColumnRow;
typedef std::tuple<std::vector<RecordPrintColumnRow>, uint64_t, bool, uintptr_t, uint64_t> RecordPrintJobRow;
// the keys are copied to *keys, which must outlive the columns
std::vector<gpu::DeviceRecordPrintColumn> record_print_columns(const std::vector<RecordPrintColumnRow>& rows,
                                                               std::vector<std::string>* keys) {
    std::vector<gpu::DeviceRecordPrintColumn> cs(rows.size());
    keys->resize(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        (*keys)[i] = std::get<0>(rows[i]);
        cs[i].key = (*keys)[i].data();
        cs[i].key_len = (uint32_t)(*keys)[i].size();
        cs[i].kind = std::get<1>(rows[i]);
        cs[i].text = std::get<2>(rows[i]);
        cs[i].src = (const void*)std::get<3>(rows[i]);
        cs[i].count = std::get<4>(rows[i]);
        cs[i].row_ends = (const uint32_t*)std::get<5>(rows[i]);
    }
    return cs;
}
std::vector<gpu::DeviceMessageField> message_fields(const std::vector<MessageFieldRow>& rows) {
    std::vector<gpu::DeviceMessageField> fs(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        fs[i].number = std::get<0>(rows[i]);
        fs[i].kind = std::get<1>(rows[i]);
        fs[i].src = (const void*)std::get<2>(rows[i]);
        fs[i].count = std::get<3>(rows[i]);
    }
    return fs;
}
std::vector<gpu::DeviceRecordColumn> record_columns(const std::vector<RecordColumnRow>& rows) {
    std::vector<gpu::DeviceRecordColumn> cs(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        cs[i].inner = std::get<0>(rows[i]);
        cs[i].kind = std::get<1>(rows[i]);
        cs[i].src = (const void*)std::get<2>(rows[i]);
        cs[i].count = std::get<3>(rows[i]);
        cs[i].row_ends = (const uint32_t*)std::get<4>(rows[i]);
    }
    return cs;
}

}  // namespace

void bind_gpu_ops(py::module_& g) {
    // n fibers each launch a kernel that runs `us` microseconds and wait for
    // its event; returns a handle for park_join (tests of the fiber-aware
    // GPU wait: RPCs must keep flowing on the same workers meanwhile)
    g.def("park_start", [](int n, uint64_t us, int device) {
        ParkedWaiters* p = new ParkedWaiters;
        p->device = device;
        p->us = us;
        p->tids.resize(n);
        p->waited_us.assign(n, 0);
        p->rcs.assign(n, -1);
        for (int i = 0; i < n; ++i) {
            if (fiber::start_background(&p->tids[i], &fiber::ATTR_NORMAL, park_on_kernel, new ParkArg{p, (size_t)i}) != 0) {
                throw std::runtime_error("fiber start failed");
            }
        }
        return reinterpret_cast<uintptr_t>(p);
    }, py::arg("n"), py::arg("us"), py::arg("device") = 0);
    g.def("park_join", [](uintptr_t h) {
        ParkedWaiters* p = reinterpret_cast<ParkedWaiters*>(h);
        {
            py::gil_scoped_release nogil;
            for (fiber::fiber_t t : p->tids) fiber::join(t, nullptr);
        }
        py::list waited, rcs;
        for (int64_t w : p->waited_us) waited.append(w);
        for (int r : p->rcs) rcs.append(r);
        delete p;
        return py::make_tuple(waited, rcs);
    });
    g.def("crc32c_lds_launch", [](const std::vector<uintptr_t>& ptrs, const std::vector<uint64_t>& lens, uintptr_t out,
                              uintptr_t stream) {
        if (ptrs.size() != lens.size()) throw std::invalid_argument("ptrs/lens size mismatch");
        std::vector<gpu::Segment> segs(ptrs.size());
        for (size_t i = 0; i < ptrs.size(); ++i) segs[i] = gpu::Segment{(const void*)ptrs[i], nullptr, lens[i]};
        check(gpu::LaunchCrc32c(segs.data(), (int)segs.size(), (uint32_t*)out, as_stream(stream)), "crc32c");
    }, py::arg("ptrs"), py::arg("lens"), py::arg("out"), py::arg("stream") = 0);
    g.def("crc32c_scratch_bytes", &gpu::Crc32cScratchBytes);
    g.def("crc32c_segments_launch", [](uintptr_t starts, uintptr_t lens, int64_t nseg, uint64_t total_bytes,
                                       uint64_t max_seg_len, uintptr_t out, uintptr_t scratch, uintptr_t stream) {
        check(gpu::LaunchCrc32cSegments((const uint64_t*)starts, (const uint64_t*)lens, nseg, total_bytes, max_seg_len,
                                        (uint32_t*)out, (void*)scratch, as_stream(stream)),
              "crc32c_segments");
    });
    g.def("crc32c_sync", [](uintptr_t ptr, uint64_t len, int device) {
        uint32_t out = 0;
        const void* p = (const void*)ptr;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::Crc32cDevice(&p, &len, 1, &out, device);
        }
        check(rc, "crc32c_sync");
        return out;
    }, py::arg("ptr"), py::arg("len"), py::arg("device") = -1);
    g.def("batched_copy_launch", [](const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
                                    const std::vector<uint64_t>& lens, uintptr_t stream) {
        if (srcs.size() != lens.size() || dsts.size() != lens.size()) throw std::invalid_argument("size mismatch");
        std::vector<gpu::Segment> segs(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) segs[i] = gpu::Segment{(const void*)srcs[i], (void*)dsts[i], lens[i]};
        check(gpu::LaunchBatchedCopy(segs.data(), (int)segs.size(), as_stream(stream)), "batched_copy");
    }, py::arg("srcs"), py::arg("dsts"), py::arg("lens"), py::arg("stream") = 0);
    // The copy engine itself (gpu/copy_engine.h): blocks until the batch it
    // joined completed; with_crc returns one CRC32C per segment (or, with
    // fold, one for the concatenation). A 0 dst only checksums.
    g.def("engine_copy", [](const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
                            const std::vector<uint64_t>& lens, int device, bool with_crc, bool fold) {
        if (srcs.size() != lens.size() || dsts.size() != lens.size()) throw std::invalid_argument("size mismatch");
        std::vector<gpu::Segment> segs(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) segs[i] = gpu::Segment{(const void*)srcs[i], (void*)dsts[i], lens[i]};
        std::vector<uint32_t> crcs(with_crc ? segs.size() : 0);
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::BatchedCopy(segs.data(), (int)segs.size(), device, with_crc ? crcs.data() : nullptr, fold);
        }
        check(rc, "engine_copy");
        if (fold && !crcs.empty()) crcs.resize(1);
        return crcs;
    }, py::arg("srcs"), py::arg("dsts"), py::arg("lens"), py::arg("device") = 0, py::arg("with_crc") = false,
       py::arg("fold") = false);
    // Device-payload codec (gpu/device_codec.h), for numerics tests: encode
    // `len` bytes at src into blocks at dst (layout of -device_payload_block_kb)
    // -> (block_ulen, stride, [clen...]); decode such a table back -> per-job
    // code (0 ok, 1 bad table, 2 malformed block) and the field table when scanned.
    g.def("device_snappy_layout", [](uint64_t len) {
        const gpu::DeviceSnappyLayout l = gpu::DeviceSnappyLayoutFor(len);
        return py::make_tuple(l.block_ulen, l.stride, l.nblocks);
    });
    g.def("device_snappy_encode", [](uintptr_t src, uint64_t len, uintptr_t dst, int device) {
        const gpu::DeviceSnappyLayout l = gpu::DeviceSnappyLayoutFor(len);
        std::vector<uint32_t> clen(l.nblocks);
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceSnappyEncode((const void*)src, len, (void*)dst, l, clen.data(), device);
        }
        check(rc, "device_snappy_encode");
        return clen;
    });
    g.def("device_snappy_decode", [](uintptr_t region, uint64_t region_len, uint32_t block_ulen, uint32_t stride,
                                     const std::vector<uint32_t>& clen, uintptr_t dst, uint64_t len, bool scan,
                                     int device) {
        gpu::DeviceSnappyBlocks j;
        j.region = (const char*)region;
        j.region_len = region_len;
        j.lay.block_ulen = block_ulen;
        j.lay.stride = stride;
        j.lay.nblocks = (uint32_t)clen.size();
        j.clen = clen.data();
        j.dst = (void*)dst;
        j.len = len;
        j.scan = scan;
        int err = 0, rc;
        DevicePayloadIndex idx;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceSnappyDecode(&j, 1, &err, &idx, device);
        }
        check(rc, "device_snappy_decode");
        return py::make_tuple(err, idx.nfields, idx.fields);
    });
    // Packed numeric fields already in HBM -> device arrays (one codec
    // request for all runs): [(count, code)] per run, code 0 ok, 1 malformed
    // or truncated, 2 refused.
    g.def("device_decode_packed", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& lens,
                                     const std::vector<uint32_t>& kinds, const std::vector<uintptr_t>& dsts,
                                     int device) {
        if (srcs.size() != lens.size() || kinds.size() != lens.size() || dsts.size() != lens.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DevicePackedRun> runs(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) {
            runs[i].src = (const void*)srcs[i];
            runs[i].len = lens[i];
            runs[i].kind = kinds[i];
            runs[i].dst = (void*)dsts[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceDecodePackedRuns(runs.data(), (int)runs.size(), device);
        }
        check(rc, "device_decode_packed");
        py::list out;
        for (const gpu::DevicePackedRun& r : runs) out.append(py::make_tuple(r.count, r.err));
        return out;
    }, py::arg("srcs"), py::arg("lens"), py::arg("kinds"), py::arg("dsts"), py::arg("device") = 0);
    // The encode side: device arrays -> one serialized message at dst (cap
    // bytes of device memory). fields = [(number, kind, ptr, count)], kind a
    // PbRunKind or 7 (raw bytes). -> (len, err, [(off, len) per field]); err 0
    // built, 2 refused before any launch, 3 longer than cap (dst untouched).
    g.def("device_build_message", [](const std::vector<MessageFieldRow>& fields, uintptr_t dst, uint64_t cap,
                                     int device) {
        std::vector<gpu::DeviceMessageField> fs = message_fields(fields);
        gpu::DeviceMessageJob job;
        job.fields = fs.data();
        job.nfields = (int)fs.size();
        job.dst = (void*)dst;
        job.cap = cap;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBuildMessages(&job, 1, device);
        }
        check(rc, "device_build_message");
        py::list pos;
        for (const gpu::DeviceMessageField& f : fs) pos.append(py::make_tuple(f.off, f.len));
        return py::make_tuple(job.len, job.err, pos);
    }, py::arg("fields"), py::arg("dst"), py::arg("cap"), py::arg("device") = 0);
    g.def("device_message_worst_case", [](const std::vector<MessageFieldRow>& fields) {
        std::vector<gpu::DeviceMessageField> fs = message_fields(fields);
        return gpu::DeviceMessageWorstCaseBytes(fs.data(), (int)fs.size());
    });
    // Ragged batches: jobs = [(number, inner, kind, src, count, row_ends,
    // rows, dst, cap)], src / row_ends / dst device pointers -> [(len, err,
    // first_bad)] (gpu::DeviceBuildRows; all jobs share one launch sequence).
    g.def("device_build_rows", [](const std::vector<RowsJobRow>& jobs, int device) {
        std::vector<gpu::DeviceRowsJob> js(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) {
            js[i].number = std::get<0>(jobs[i]);
            js[i].inner = std::get<1>(jobs[i]);
            js[i].kind = std::get<2>(jobs[i]);
            js[i].src = (const void*)std::get<3>(jobs[i]);
            js[i].count = std::get<4>(jobs[i]);
            js[i].row_ends = (const uint32_t*)std::get<5>(jobs[i]);
            js[i].rows = std::get<6>(jobs[i]);
            js[i].dst = (void*)std::get<7>(jobs[i]);
            js[i].cap = std::get<8>(jobs[i]);
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBuildRows(js.data(), (int)js.size(), device);
        }
        check(rc, "device_build_rows");
        py::list out;
        for (const gpu::DeviceRowsJob& j : js) out.append(py::make_tuple(j.len, j.err, j.first_bad));
        return out;
    }, py::arg("jobs"), py::arg("device") = 0);
    // The way back: jobs = [(number, inner, kind, msg, n, values, cap,
    // row_ends, row_cap)], msg / values / row_ends device pointers ->
    // [(count, rows, others, err, first_bad)] (gpu::DeviceSplitRows; all jobs
    // share one launch sequence).
    g.def("device_split_rows", [](const std::vector<RowsJobRow>& jobs, int device) {
        std::vector<gpu::DeviceRowsSplitJob> js(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) {
            js[i].number = std::get<0>(jobs[i]);
            js[i].inner = std::get<1>(jobs[i]);
            js[i].kind = std::get<2>(jobs[i]);
            js[i].msg = (const void*)std::get<3>(jobs[i]);
            js[i].n = std::get<4>(jobs[i]);
            js[i].values = (void*)std::get<5>(jobs[i]);
            js[i].cap = std::get<6>(jobs[i]);
            js[i].row_ends = (uint32_t*)std::get<7>(jobs[i]);
            js[i].row_cap = std::get<8>(jobs[i]);
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceSplitRows(js.data(), (int)js.size(), device);
        }
        check(rc, "device_split_rows");
        py::list out;
        for (const gpu::DeviceRowsSplitJob& j : js) {
            out.append(py::make_tuple(j.count, j.rows, j.others, j.err, j.first_bad));
        }
        return out;
    }, py::arg("jobs"), py::arg("device") = 0);
    // Records back into columns: table = [(number, [(inner, kind, scalar,
    // values, cap, row_ends)], msg, n, row_cap)], msg / values / row_ends
    // device pointers (row_ends 0 for a scalar column) -> [(rows, others, err,
    // first_bad, [(count, absent)])] (gpu::DeviceSplitRecords; all jobs share
    // one launch sequence).
    g.def("device_split_records", [](const std::vector<RecordsSplitJobRow>& table, int device) {
        std::vector<gpu::DeviceRecordsSplitJob> js(table.size());
        std::vector<std::vector<gpu::DeviceRecordSplitColumn>> cols(table.size());
        for (size_t i = 0; i < table.size(); ++i) {
            const std::vector<RecordSplitColumnRow>& rows = std::get<1>(table[i]);
            cols[i].resize(rows.size());
            for (size_t c = 0; c < rows.size(); ++c) {
                cols[i][c].inner = std::get<0>(rows[c]);
                cols[i][c].kind = std::get<1>(rows[c]);
                cols[i][c].scalar = std::get<2>(rows[c]);
                cols[i][c].values = (void*)std::get<3>(rows[c]);
                cols[i][c].cap = std::get<4>(rows[c]);
                cols[i][c].row_ends = (uint32_t*)std::get<5>(rows[c]);
            }
            js[i].number = std::get<0>(table[i]);
            js[i].columns = cols[i].data();
            js[i].ncols = (uint32_t)cols[i].size();
            js[i].msg = (const void*)std::get<2>(table[i]);
            js[i].n = std::get<3>(table[i]);
            js[i].row_cap = std::get<4>(table[i]);
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceSplitRecords(js.data(), (int)js.size(), device);
        }
        check(rc, "device_split_records");
        py::list out;
        for (size_t i = 0; i < js.size(); ++i) {
            py::list per;
            // a job refused for its column count reports no column
            for (size_t c = 0; c < cols[i].size(); ++c) per.append(py::make_tuple(cols[i][c].count, cols[i][c].absent));
            out.append(py::make_tuple(js[i].rows, js[i].others, js[i].err, js[i].first_bad, per));
        }
        return out;
    }, py::arg("table"), py::arg("device") = 0);
    g.def("device_split_max_bytes", []() { return gpu::kDeviceSplitMaxBytes; });
    // Records: jobs = [(number, [(inner, kind, src, count, row_ends)], rows,
    // dst, cap)], src / row_ends / dst device pointers, row_ends 0 for a
    // scalar column -> [(len, err, first_bad, bad_column)]
    // (gpu::DeviceBuildRecords; all jobs share one launch sequence).
    g.def("device_build_records", [](const std::vector<RecordsJobRow>& jobs, int device) {
        std::vector<gpu::DeviceRecordsJob> js(jobs.size());
        std::vector<std::vector<gpu::DeviceRecordColumn>> cols(jobs.size());
        for (size_t i = 0; i < jobs.size(); ++i) {
            cols[i] = record_columns(std::get<1>(jobs[i]));
            js[i].number = std::get<0>(jobs[i]);
            js[i].columns = cols[i].data();
            js[i].ncols = (uint32_t)cols[i].size();
            js[i].rows = std::get<2>(jobs[i]);
            js[i].dst = (void*)std::get<3>(jobs[i]);
            js[i].cap = std::get<4>(jobs[i]);
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBuildRecords(js.data(), (int)js.size(), device);
        }
        check(rc, "device_build_records");
        py::list out;
        for (const gpu::DeviceRecordsJob& j : js) out.append(py::make_tuple(j.len, j.err, j.first_bad, j.bad_column));
        return out;
    }, py::arg("jobs"), py::arg("device") = 0);
    g.def("device_records_worst_case", [](uint32_t number, const std::vector<RecordColumnRow>& columns, uint64_t rows) {
        const std::vector<gpu::DeviceRecordColumn> cols = record_columns(columns);
        gpu::DeviceRecordsJob j;
        j.number = number;
        j.columns = cols.data();
        j.ncols = (uint32_t)cols.size();
        j.rows = rows;
        return gpu::DeviceRecordsWorstCaseBytes(j);
    }, py::arg("number"), py::arg("columns"), py::arg("rows"));
    g.def("device_rows_worst_case", [](uint32_t number, uint32_t inner, uint32_t kind, uint64_t count, uint64_t rows) {
        gpu::DeviceRowsJob j;
        j.number = number;
        j.inner = inner;
        j.kind = kind;
        j.count = count;
        j.rows = rows;
        return gpu::DeviceRowsWorstCaseBytes(j);
    }, py::arg("number"), py::arg("inner"), py::arg("kind"), py::arg("count"), py::arg("rows"));
    // Bare packed runs (no tag, no length), the mirror of device_decode_packed:
    // [(bytes, err)] per array.
    g.def("device_encode_packed", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& counts,
                                     const std::vector<uint32_t>& kinds, const std::vector<uintptr_t>& dsts,
                                     const std::vector<uint64_t>& caps, int device) {
        if (srcs.size() != counts.size() || kinds.size() != counts.size() || dsts.size() != counts.size() ||
            caps.size() != counts.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DevicePackedEncodeRun> runs(counts.size());
        for (size_t i = 0; i < counts.size(); ++i) {
            runs[i].src = (const void*)srcs[i];
            runs[i].count = counts[i];
            runs[i].kind = kinds[i];
            runs[i].dst = (void*)dsts[i];
            runs[i].cap = caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceEncodePackedRuns(runs.data(), (int)runs.size(), device);
        }
        check(rc, "device_encode_packed");
        py::list out;
        for (const gpu::DevicePackedEncodeRun& r : runs) out.append(py::make_tuple(r.bytes, r.err));
        return out;
    }, py::arg("srcs"), py::arg("counts"), py::arg("kinds"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    // Float (kind 8) / double (kind 9) arrays in device memory -> JSON text
    // "v,v,...,v" at dst (cap bytes of device memory), all arrays in one
    // launch sequence: [(len, err)] per array; err 0 printed, 2 refused before
    // any launch, 3 longer than cap (dst untouched, len = the size needed).
    g.def("device_json_print_floats", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& counts,
                                         const std::vector<uint32_t>& kinds, const std::vector<uintptr_t>& dsts,
                                         const std::vector<uint64_t>& caps, int device) {
        if (srcs.size() != counts.size() || kinds.size() != counts.size() || dsts.size() != counts.size() ||
            caps.size() != counts.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceFloatPrintJob> jobs(counts.size());
        for (size_t i = 0; i < counts.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].count = counts[i];
            jobs[i].kind = kinds[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DevicePrintFloatArrays(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_print_floats");
        py::list out;
        for (const gpu::DeviceFloatPrintJob& j : jobs) out.append(py::make_tuple(j.len, j.err));
        return out;
    }, py::arg("srcs"), py::arg("counts"), py::arg("kinds"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    g.def("json_float_worst_case", &gpu::FloatPrintWorstCaseBytes);
    // Number arrays (kinds 0..6, 8, 9) in device memory -> JSON text at dst
    // (cap bytes of device memory): "v,..,v", "[v,..,v]" (brackets) or, with
    // a table of row ends in device memory (row_ends != 0, rows entries),
    // "[[v,..],[v,..],..]"; all jobs in one launch sequence
    // (gpu::DevicePrintNumbers): [(len, first_bad, err)] per job; err 0
    // printed, 1 bad row ends (first_bad the lowest bad row), 2 refused before
    // any launch, 3 longer than cap (len = the size needed), 4 the source
    // changed between the passes.
    g.def("device_json_print_numbers", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& counts,
                                          const std::vector<uint32_t>& kinds, const std::vector<uintptr_t>& row_ends,
                                          const std::vector<uint64_t>& rows, const std::vector<bool>& brackets,
                                          const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                          int device) {
        const size_t n = counts.size();
        if (srcs.size() != n || kinds.size() != n || row_ends.size() != n || rows.size() != n ||
            brackets.size() != n || dsts.size() != n || caps.size() != n)
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceNumberPrintJob> jobs(n);
        for (size_t i = 0; i < n; ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].count = counts[i];
            jobs[i].kind = kinds[i];
            jobs[i].row_ends = (const uint32_t*)row_ends[i];
            jobs[i].rows = rows[i];
            jobs[i].brackets = brackets[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DevicePrintNumbers(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_print_numbers");
        py::list out;
        for (const gpu::DeviceNumberPrintJob& j : jobs) out.append(py::make_tuple(j.len, j.first_bad, j.err));
        return out;
    }, py::arg("srcs"), py::arg("counts"), py::arg("kinds"), py::arg("row_ends"), py::arg("rows"),
       py::arg("brackets"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    g.def("json_number_print_worst_case", &gpu::NumberPrintWorstCaseBytes, py::arg("kind"), py::arg("count"),
          py::arg("rows") = 0);
    g.def("json_number_print_chunk_elems", &gpu::JsonNumberPrintChunkElems);
    // Records as JSON objects: table = [([(key, kind, text_form, src, count,
    // row_ends)], rows, brackets, dst, cap)], key raw bytes, text_form 0 (a
    // number kind), 1 (string) or 2 (base64), src / row_ends / dst device
    // pointers, row_ends 0 for a scalar column -> [(len, err, first_bad,
    // bad_column)] (gpu::DevicePrintRecordObjects; all jobs share one launch
    // sequence).
    g.def("device_json_print_records", [](const std::vector<RecordPrintJobRow>& table, int device) {
        std::vector<gpu::DeviceRecordPrintJob> js(table.size());
        std::vector<std::vector<std::string>> keys(table.size());
        std::vector<std::vector<gpu::DeviceRecordPrintColumn>> cols(table.size());
        for (size_t i = 0; i < table.size(); ++i) {
            cols[i] = record_print_columns(std::get<0>(table[i]), &keys[i]);
            js[i].columns = cols[i].data();
            js[i].ncols = (uint32_t)cols[i].size();
            js[i].rows = std::get<1>(table[i]);
            js[i].brackets = std::get<2>(table[i]);
            js[i].dst = (void*)std::get<3>(table[i]);
            js[i].cap = std::get<4>(table[i]);
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DevicePrintRecordObjects(js.data(), (int)js.size(), device);
        }
        check(rc, "device_json_print_records");
        py::list out;
        for (const gpu::DeviceRecordPrintJob& j : js) out.append(py::make_tuple(j.len, j.err, j.first_bad, j.bad_column));
        return out;
    }, py::arg("table"), py::arg("device") = 0);
    g.def("json_records_worst_case", [](const std::vector<RecordPrintColumnRow>& columns, uint64_t rows, bool brackets) {
        std::vector<std::string> keys;
        const std::vector<gpu::DeviceRecordPrintColumn> cols = record_print_columns(columns, &keys);
        gpu::DeviceRecordPrintJob j;
        j.columns = cols.data();
        j.ncols = (uint32_t)cols.size();
        j.rows = rows;
        j.brackets = brackets;
        return gpu::RecordObjectsWorstCaseBytes(j);
    }, py::arg("columns"), py::arg("rows"), py::arg("brackets") = true);
    g.def("json_records_chunk_elems", &gpu::JsonRecordsChunkElems);
    g.def("json_records_block_rows", &gpu::JsonRecordsBlockRows);
    // Host floats / doubles (their memory image) -> the same text through the
    // device (gpu::PrintFloatsOnDevice: pinned stage, one wait).
    g.def("json_print_floats", [](py::bytes values, uint64_t n, uint32_t kind, int device) {
        const std::string data = values;
        const size_t eb = kind == gpu::kJsonFloat32 ? 4 : 8;
        if (kind != gpu::kJsonFloat32 && kind != gpu::kJsonFloat64) throw std::invalid_argument("kind must be 8 or 9");
        if (data.size() != n * eb) throw std::invalid_argument("values must hold n elements");
        // a std::string's buffer need not be aligned for doubles
        std::vector<uint64_t> aligned((data.size() + 7) / 8);
        memcpy(aligned.data(), data.data(), data.size());
        std::string text;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::PrintFloatsOnDevice(aligned.data(), (size_t)n, kind, &text, device);
        }
        check(rc, "json_print_floats");
        return py::bytes(text);
    }, py::arg("values"), py::arg("n"), py::arg("kind"), py::arg("device") = 0);
    // Number arrays as text in device (or pinned) memory -> values, all jobs
    // in one launch (gpu::DeviceParseNumberArrays). Per job: text, seps
    // (count + 1 uint32 offsets), count, mode (0 numbers: 8-byte payload at
    // out and a class byte at classes; 1 float64; 2 float32), out, classes,
    // redo (redo_cap uint32 slots). Returns [(err, first_bad, n_redo)].
    g.def("device_json_parse_numbers", [](const std::vector<uintptr_t>& texts, const std::vector<uintptr_t>& seps,
                                          const std::vector<uint64_t>& counts, const std::vector<uint32_t>& modes,
                                          const std::vector<uintptr_t>& outs, const std::vector<uintptr_t>& classes,
                                          const std::vector<uintptr_t>& redos, const std::vector<uint32_t>& redo_caps,
                                          int device) {
        const size_t n = counts.size();
        if (texts.size() != n || seps.size() != n || modes.size() != n || outs.size() != n || classes.size() != n ||
            redos.size() != n || redo_caps.size() != n)
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceNumberParseJob> jobs(n);
        for (size_t i = 0; i < n; ++i) {
            jobs[i].text = (const char*)texts[i];
            jobs[i].seps = (const uint32_t*)seps[i];
            jobs[i].count = counts[i];
            jobs[i].mode = modes[i];
            jobs[i].out = (void*)outs[i];
            jobs[i].classes = (uint8_t*)classes[i];
            jobs[i].redo = (uint32_t*)redos[i];
            jobs[i].redo_cap = redo_caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceParseNumberArrays(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_parse_numbers");
        py::list out;
        for (const gpu::DeviceNumberParseJob& j : jobs) out.append(py::make_tuple(j.err, j.first_bad, j.n_redo));
        return out;
    }, py::arg("texts"), py::arg("seps"), py::arg("counts"), py::arg("modes"), py::arg("outs"), py::arg("classes"),
       py::arg("redos"), py::arg("redo_caps"), py::arg("device") = 0);
    // Number text in device (or pinned) memory with no separator table ->
    // values, all jobs in one launch sequence (gpu::DeviceParseNumberText).
    // Per job: text, n bytes, mode, out, classes, cap (elements), row_ends,
    // row_cap, redo (2 * redo_cap uint32: {index, offset} pairs), redo_cap.
    // Returns [(err, depth, count, rows, n_redo, first_bad)].
    g.def("device_json_parse_text", [](const std::vector<uintptr_t>& texts, const std::vector<uint64_t>& ns,
                                       const std::vector<uint32_t>& modes, const std::vector<uintptr_t>& outs,
                                       const std::vector<uintptr_t>& classes, const std::vector<uint64_t>& caps,
                                       const std::vector<uintptr_t>& row_ends, const std::vector<uint64_t>& row_caps,
                                       const std::vector<uintptr_t>& redos, const std::vector<uint32_t>& redo_caps,
                                       int device) {
        const size_t n = ns.size();
        if (texts.size() != n || modes.size() != n || outs.size() != n || classes.size() != n || caps.size() != n ||
            row_ends.size() != n || row_caps.size() != n || redos.size() != n || redo_caps.size() != n)
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceNumberTextJob> jobs(n);
        for (size_t i = 0; i < n; ++i) {
            jobs[i].text = (const char*)texts[i];
            jobs[i].n = ns[i];
            jobs[i].mode = modes[i];
            jobs[i].out = (void*)outs[i];
            jobs[i].classes = (uint8_t*)classes[i];
            jobs[i].cap = caps[i];
            jobs[i].row_ends = (uint32_t*)row_ends[i];
            jobs[i].row_cap = row_caps[i];
            jobs[i].redo = (uint32_t*)redos[i];
            jobs[i].redo_cap = redo_caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceParseNumberText(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_parse_text");
        py::list out;
        for (const gpu::DeviceNumberTextJob& j : jobs)
            out.append(py::make_tuple(j.err, j.depth, j.count, j.rows, j.n_redo, j.first_bad));
        return out;
    }, py::arg("texts"), py::arg("ns"), py::arg("modes"), py::arg("outs"), py::arg("classes"), py::arg("caps"),
       py::arg("row_ends"), py::arg("row_caps"), py::arg("redos"), py::arg("redo_caps"), py::arg("device") = 0);
    g.def("json_text_chunk_bytes", &gpu::JsonTextChunkBytes);
    // Host text "[v,v,...]" or "v,v,...,v" -> (payload, classes, n_redo)
    // through the device (gpu::ParseNumbersOnDevice: pinned stage, one wait,
    // redo elements repaired on the host); ValueError when the device
    // declines (a malformed element or too many redo elements).
    g.def("json_parse_numbers", [](py::bytes text, int device) {
        const std::string t = text;
        if (t.size() >= 0xFFFFFFFFull) throw std::invalid_argument("text must be below 4 GiB");
        std::vector<uint32_t> seps;
        json::NumberArraySeparators(t.data(), t.size(), &seps);
        const size_t n = seps.size() - 1;
        std::vector<uint64_t> payload(n);
        std::string classes(n, '\0');
        uint32_t n_redo = 0;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = gpu::ParseNumbersOnDevice(t.data(), seps.data(), seps.size(), payload.data(),
                                           reinterpret_cast<uint8_t*>(&classes[0]), device, &n_redo);
        }
        if (!ok) throw py::value_error("the device declined the array (malformed element or redo overflow)");
        return py::make_tuple(py::bytes(reinterpret_cast<const char*>(payload.data()), n * 8), py::bytes(classes),
                              n_redo);
    }, py::arg("text"), py::arg("device") = 0);
    // Base64 of bytes in device memory, all jobs in one launch
    // (gpu::DeviceBase64Encode / DeviceBase64Decode): n bytes at src -> dst
    // (cap bytes), any alignment. Encode returns [(len, err)], decode
    // [(len, err, first_odd)]; err 0 done, 1 (decode) not canonical text, 2
    // refused before any launch, 3 cap too small (len = the size needed).
    auto base64_jobs = [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                          const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceBase64Job> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
        }
        return jobs;
    };
    g.def("device_base64_encode", [base64_jobs](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                                const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                                int device) {
        std::vector<gpu::DeviceBase64Job> jobs = base64_jobs(srcs, ns, dsts, caps);
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBase64Encode(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_base64_encode");
        py::list out;
        for (const gpu::DeviceBase64Job& j : jobs) out.append(py::make_tuple(j.len, j.err));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    g.def("device_base64_decode", [base64_jobs](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                                const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                                int device) {
        std::vector<gpu::DeviceBase64Job> jobs = base64_jobs(srcs, ns, dsts, caps);
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBase64Decode(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_base64_decode");
        py::list out;
        for (const gpu::DeviceBase64Job& j : jobs) out.append(py::make_tuple(j.len, j.err, j.first_odd));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    g.def("base64_chunk_bytes", [] { return gpu::kBase64ChunkBytes; });
    // Base64 rows in device memory (gpu::DeviceBase64EncodeRows /
    // DeviceBase64DecodeRows): (bytes, uint32 row ends) <-> the text of a JSON
    // array of base64 strings. Encode returns [(len, err, first_bad)], decode
    // [(len, rows, depth, err, first_bad)]; err 3: len and rows say what is
    // needed.
    g.def("device_base64_encode_rows", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                          const std::vector<uintptr_t>& row_ends, const std::vector<uint64_t>& rows,
                                          bool brackets, const std::vector<uintptr_t>& dsts,
                                          const std::vector<uint64_t>& caps, int device) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size() ||
            row_ends.size() != ns.size() || rows.size() != ns.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceBase64RowsEncodeJob> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].row_ends = (const void*)row_ends[i];
            jobs[i].rows = rows[i];
            jobs[i].brackets = brackets;
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBase64EncodeRows(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_base64_encode_rows");
        py::list out;
        for (const gpu::DeviceBase64RowsEncodeJob& j : jobs) out.append(py::make_tuple(j.len, j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("row_ends"), py::arg("rows"), py::arg("brackets"), py::arg("dsts"),
       py::arg("caps"), py::arg("device") = 0);
    g.def("device_base64_decode_rows", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                          const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                          const std::vector<uintptr_t>& ends, const std::vector<uint64_t>& row_caps,
                                          int device) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size() || ends.size() != ns.size() ||
            row_caps.size() != ns.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceBase64RowsDecodeJob> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
            jobs[i].row_ends = (void*)ends[i];
            jobs[i].row_cap = row_caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceBase64DecodeRows(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_base64_decode_rows");
        py::list out;
        for (const gpu::DeviceBase64RowsDecodeJob& j : jobs)
            out.append(py::make_tuple(j.len, j.rows, j.depth, j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"), py::arg("ends"), py::arg("row_caps"),
       py::arg("device") = 0);
    g.def("base64_rows_worst_case", [](uint64_t n, uint64_t rows, bool brackets) {
        return gpu::Base64RowsWorstCaseBytes(n, rows, brackets);
    }, py::arg("n"), py::arg("rows"), py::arg("brackets") = true);
    g.def("base64_rows_max_bytes", [](uint64_t n) { return gpu::Base64RowsMaxBytes(n); });
    g.def("base64_rows_max_rows", [](uint64_t n) { return gpu::Base64RowsMaxRows(n); });
    g.def("base64_rows_encode_chunk_bytes", [] { return gpu::kBase64RowsEncodeChunkBytes; });
    g.def("base64_rows_decode_chunk_bytes", [] { return gpu::kBase64RowsDecodeChunkBytes; });
    g.def("base64_rows_segment_rows", [] { return gpu::kBase64RowsSegmentRows; });
    // JSON string bodies in device memory, all jobs sharing the launches
    // (gpu/json_string_offload.h): escape returns [(len, err, first_bad)]
    // (row_ends[i] 0: one string, else `rows[i]` uint32 in device memory),
    // unescape [(len, err, first_bad)], validate [(err, first_bad)]. err 0
    // done, 1 first_bad is set, 2 refused before any launch, 3 cap too small
    // (len = the size needed).
    g.def("device_json_escape", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                   const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                   const std::vector<uintptr_t>& row_ends, const std::vector<uint64_t>& rows,
                                   bool quote, int device) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size() ||
            (!row_ends.empty() && row_ends.size() != ns.size()) || rows.size() != row_ends.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceJsonEscapeJob> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
            jobs[i].quote = quote;
            if (!row_ends.empty()) {
                jobs[i].row_ends = (const void*)row_ends[i];
                jobs[i].rows = rows[i];
            }
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceEscapeJsonStrings(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_escape");
        py::list out;
        for (const gpu::DeviceJsonEscapeJob& j : jobs) out.append(py::make_tuple(j.len, j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"),
       py::arg("row_ends") = std::vector<uintptr_t>(), py::arg("rows") = std::vector<uint64_t>(),
       py::arg("quote") = true, py::arg("device") = 0);
    g.def("device_json_unescape", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                     const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps, int device) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceJsonUnescapeJob> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceUnescapeJsonStrings(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_unescape");
        py::list out;
        for (const gpu::DeviceJsonUnescapeJob& j : jobs) out.append(py::make_tuple(j.len, j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"), py::arg("device") = 0);
    // The text of an array of strings -> decoded bytes at dsts[i] and uint32 row
    // ends at ends[i]: [(len, rows, depth, err, first_bad)]. err 3: len and rows
    // say what the text holds.
    g.def("device_json_unescape_rows", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns,
                                          const std::vector<uintptr_t>& dsts, const std::vector<uint64_t>& caps,
                                          const std::vector<uintptr_t>& ends, const std::vector<uint64_t>& row_caps,
                                          int device) {
        if (srcs.size() != ns.size() || dsts.size() != ns.size() || caps.size() != ns.size() || ends.size() != ns.size() ||
            row_caps.size() != ns.size())
            throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceJsonStringRowsJob> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
            jobs[i].dst = (void*)dsts[i];
            jobs[i].cap = caps[i];
            jobs[i].row_ends = (void*)ends[i];
            jobs[i].row_cap = row_caps[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceUnescapeJsonStringRows(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_json_unescape_rows");
        py::list out;
        for (const gpu::DeviceJsonStringRowsJob& j : jobs)
            out.append(py::make_tuple(j.len, j.rows, j.depth, j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("dsts"), py::arg("caps"), py::arg("ends"), py::arg("row_caps"),
       py::arg("device") = 0);
    g.def("json_string_rows_max_bytes", [](uint64_t n) { return gpu::JsonStringRowsMaxBytes(n); });
    g.def("json_string_rows_max_rows", [](uint64_t n) { return gpu::JsonStringRowsMaxRows(n); });
    g.def("device_utf8_validate", [](const std::vector<uintptr_t>& srcs, const std::vector<uint64_t>& ns, int device) {
        if (srcs.size() != ns.size()) throw std::invalid_argument("size mismatch");
        std::vector<gpu::DeviceUtf8Job> jobs(ns.size());
        for (size_t i = 0; i < ns.size(); ++i) {
            jobs[i].src = (const void*)srcs[i];
            jobs[i].n = ns[i];
        }
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DeviceValidateUtf8(jobs.data(), (int)jobs.size(), device);
        }
        check(rc, "device_utf8_validate");
        py::list out;
        for (const gpu::DeviceUtf8Job& j : jobs) out.append(py::make_tuple(j.err, j.first_bad));
        return out;
    }, py::arg("srcs"), py::arg("ns"), py::arg("device") = 0);
    g.def("json_escape_worst_case", [](uint64_t n, uint64_t rows) { return gpu::JsonEscapeWorstCaseBytes(n, rows); },
          py::arg("n"), py::arg("rows") = 0);
    g.def("json_string_chunk_bytes", [] { return gpu::kJsonStringChunkBytes; });
    // Field table of a message already in device memory -> (nfields, fields)
    g.def("device_pb_scan", [](uintptr_t buf, uint64_t len, int device) {
        const void* p = (const void*)buf;
        DevicePayloadIndex idx;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DevicePbScan(&p, &len, 1, &idx, device);
        }
        check(rc, "device_pb_scan");
        return py::make_tuple(idx.nfields, idx.fields);
    }, py::arg("buf"), py::arg("len"), py::arg("device") = 0);
    g.def("device_payload_field", [](int nfields, const std::vector<uint64_t>& fields, uint32_t number) -> py::object {
        DevicePayloadIndex idx;
        idx.nfields = nfields;
        idx.fields = fields;
        uint64_t off = 0, len = 0;
        if (!gpu::DevicePayloadField(idx, number, &off, &len)) return py::none();
        return py::make_tuple(off, len);
    });
    g.def("resident_stats", [] {
        const gpu::ResidentStats s = gpu::GetResidentStats();
        py::dict d;
        d["launches"] = s.launches;
        d["batches"] = s.batches;
        d["ring_full_waits"] = s.ring_full_waits;
        return d;
    });
    g.def("batched_copy_crc32c_launch", [](const std::vector<uintptr_t>& srcs, const std::vector<uintptr_t>& dsts,
                                           const std::vector<uint64_t>& lens, uintptr_t out, uintptr_t stream,
                                           bool mfma) {
        if (srcs.size() != lens.size() || dsts.size() != lens.size()) throw std::invalid_argument("size mismatch");
        std::vector<gpu::Segment> segs(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) segs[i] = gpu::Segment{(const void*)srcs[i], (void*)dsts[i], lens[i]};
        check(gpu::LaunchBatchedCopyCrc32c(segs.data(), (int)segs.size(), (uint32_t*)out, as_stream(stream), mfma),
              "batched_copy_crc32c");
    }, py::arg("srcs"), py::arg("dsts"), py::arg("lens"), py::arg("out"), py::arg("stream") = 0,
       py::arg("mfma") = true);
    // The copy engine's launch for -copy_engine_resident=false: out[msg_of[i]]
    // receives the CRC32C of the message segment i belongs to. msg_of is
    // non-decreasing in steps of 0 or 1 (consecutive message numbers, as
    // BatchedCopy builds them); a message of more than 32 segments is refused.
    g.def("batched_copy_crc32c_messages_launch", [](const std::vector<uintptr_t>& srcs,
                                                    const std::vector<uintptr_t>& dsts,
                                                    const std::vector<uint64_t>& lens, const std::vector<int>& msg_of,
                                                    uintptr_t out, uintptr_t stream, bool mfma) {
        if (srcs.size() != lens.size() || dsts.size() != lens.size() || msg_of.size() != lens.size())
            throw std::invalid_argument("size mismatch");
        for (size_t i = 0; i < msg_of.size(); ++i) {
            if (msg_of[i] < 0 || (i > 0 && (msg_of[i] < msg_of[i - 1] || msg_of[i] > msg_of[i - 1] + 1)))
                throw std::invalid_argument("msg_of must be non-negative and rise in steps of 0 or 1");
        }
        std::vector<gpu::Segment> segs(lens.size());
        for (size_t i = 0; i < lens.size(); ++i) segs[i] = gpu::Segment{(const void*)srcs[i], (void*)dsts[i], lens[i]};
        const int rc = gpu::LaunchBatchedCopyCrc32cMessages(segs.data(), msg_of.data(), (int)segs.size(),
                                                            (uint32_t*)out, as_stream(stream), nullptr, mfma);
        if (rc == -2) throw py::value_error("a message has more segments than one launch group holds");
        check(rc, "batched_copy_crc32c_messages");
    }, py::arg("srcs"), py::arg("dsts"), py::arg("lens"), py::arg("msg_of"), py::arg("out"), py::arg("stream") = 0,
       py::arg("mfma") = true);
    g.def("pb_scan_launch", [](uintptr_t buf, uint64_t buf_len, uintptr_t offsets, int64_t n, uint32_t max_fields,
                               uintptr_t fields, uintptr_t nfields, uintptr_t stream) {
        check(gpu::LaunchPbScan((const uint8_t*)buf, buf_len, (const int64_t*)offsets, n, max_fields,
                                (uint64_t*)fields, (int32_t*)nfields, as_stream(stream)),
              "pb_scan");
    });
    g.def("snappy_max_block", [] { return gpu::kSnappyMaxBlock; });
    // jobs: device array of {src, dst, src_len, dst_cap} (4 x u64 per job)
    g.def("snappy_decompress_launch", [](uintptr_t jobs, int n, uint32_t max_ulen, uintptr_t out_len, uintptr_t err,
                                         uintptr_t stream) {
        check(gpu::LaunchSnappyDecompress((const gpu::SnappyJob*)jobs, n, max_ulen, (uint32_t*)out_len, (int*)err,
                                          as_stream(stream)),
              "snappy_decompress");
    });
    // streams: {src, dst, src_len|dst_cap<<32, first|max_pieces<<32}; pieces: 24 B each (device)
    g.def("snappy_max_pieces", [](uint64_t ulen, uint32_t limit) { return gpu::SnappyMaxPieces(ulen, limit); });
    g.def("snappy_piece_bytes", [] { return sizeof(gpu::SnappyPiece); });
    g.def("snappy_split_launch", [](uintptr_t streams, int n, uint32_t limit, uintptr_t pieces, uintptr_t err,
                                    uintptr_t stream) {
        check(gpu::LaunchSnappySplit((const gpu::SnappyStream*)streams, n, limit, (gpu::SnappyPiece*)pieces, (int*)err,
                                     as_stream(stream)),
              "snappy_split");
    });
    g.def("snappy_decompress_pieces_launch", [](uintptr_t pieces, int n, uint32_t lo, uint32_t hi, uintptr_t err,
                                                uintptr_t stream) {
        check(gpu::LaunchSnappyDecompressPieces((const gpu::SnappyPiece*)pieces, n, lo, hi, (int*)err,
                                                as_stream(stream)),
              "snappy_decompress_pieces");
    });
    g.def("snappy_decompress_pieces_serial_launch", [](uintptr_t pieces, int n, uint32_t lo, uint32_t hi,
                                                       uintptr_t err, uintptr_t stream) {
        check(gpu::LaunchSnappyDecompressPiecesSerial((const gpu::SnappyPiece*)pieces, n, lo, hi, (int*)err,
                                                      as_stream(stream)),
              "snappy_decompress_pieces_serial");
    });
    g.def("snappy_compress_stamped_launch", [](uintptr_t jobs, int n, uint32_t max_ulen, uintptr_t scratch,
                                                  uintptr_t out_len, uintptr_t err, uintptr_t stamps, uintptr_t stream) {
        check(gpu::LaunchSnappyCompressStamped((const gpu::SnappyJob*)jobs, n, max_ulen, (void*)scratch,
                                               (uint32_t*)out_len, (int*)err, (uint64_t*)stamps, as_stream(stream)),
              "snappy_compress_stamped");
    });
    g.def("snappy_decompress_pieces_stamped_launch", [](uintptr_t pieces, int n, uint32_t lo, uint32_t hi,
                                                        uintptr_t err, uintptr_t stamps, uintptr_t stream) {
        check(gpu::LaunchSnappyDecompressPiecesStamped((const gpu::SnappyPiece*)pieces, n, lo, hi, (int*)err,
                                                       (uint64_t*)stamps, as_stream(stream)),
              "snappy_decompress_pieces_stamped");
    });
    g.def("snappy_compress_scratch_per_block", [] { return gpu::SnappyCompressScratchPerBlock(); });
    g.def("snappy_max_compressed_length", [](uint64_t n) { return gpu::SnappyMaxCompressedLength(n); });
    g.def("snappy_compress_launch", [](uintptr_t jobs, int n, uint32_t max_ulen, uintptr_t scratch, uintptr_t out_len,
                                       uintptr_t err, uintptr_t stream) {
        check(gpu::LaunchSnappyCompress((const gpu::SnappyJob*)jobs, n, max_ulen, (void*)scratch, (uint32_t*)out_len,
                                        (int*)err, as_stream(stream)),
              "snappy_compress");
    });
    g.def("varint_scratch_bytes", &gpu::VarintScratchBytes);
    g.def("varint_decode_launch", [](uintptr_t in, uint64_t n, uintptr_t out, uint64_t max_out, bool zigzag,
                                     uintptr_t count, uintptr_t err, uintptr_t scratch, uintptr_t stream) {
        check(gpu::LaunchVarintDecode((const uint8_t*)in, n, (uint64_t*)out, max_out, zigzag, (uint64_t*)count,
                                      (int*)err, (void*)scratch, as_stream(stream)),
              "varint_decode");
    });
    g.def("varint_encode_launch", [](uintptr_t in, uint64_t n, bool zigzag, uintptr_t out, uintptr_t nbytes,
                                     uintptr_t scratch, uintptr_t stream) {
        check(gpu::LaunchVarintEncode((const uint64_t*)in, n, zigzag, (uint8_t*)out, (uint64_t*)nbytes,
                                      (void*)scratch, as_stream(stream)),
              "varint_encode");
    });
    g.def("json_index_scratch_bytes", &gpu::JsonIndexScratchBytes);
    g.def("json_index_launch", [](uintptr_t in, uint64_t n, uintptr_t out, uint64_t max_out, uintptr_t count,
                                  uintptr_t err, uintptr_t scratch, uintptr_t stream) {
        check(gpu::LaunchJsonIndex((const uint8_t*)in, n, (uint32_t*)out, max_out, (uint64_t*)count, (int*)err,
                                   (void*)scratch, as_stream(stream)),
              "json_index");
    });
}
