// pybind11 bindings: the Python face of the native runtime (bench.py,
// tests, and torch-side GPU ops). Every call that can block drops the GIL.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sstream>
#include <unistd.h>

#include "base/base64.h"
#include "base/crc32c.h"
#include "base/decimal_to_double.h"
#include "base/json_records.h"
#include "base/number_print.h"
#include "base/util.h"
#include "builtin/cpu_profiler.h"
#include "base/snappy.h"
#include "base/flags.h"
#include "base/logging.h"
#include "fiber/fiber.h"
#include "gpu/gpu.h"
#include "gpu/copy_engine.h"
#include "rpc/compress.h"
#include "gpu/hbm_pool.h"
#include "gpu/scoped.h"
#include "gpu/snappy_offload.h"
#include "gpu/json_offload.h"
#include "gpu/codec_batch.h"
#include "gpu/device_codec.h"
#include "json/json.h"
#include "json/json2pb.h"
#include "pb/descriptor.h"
#include "pb/parser.h"
#include "pb/records.h"
#include "pb/rows.h"
#include "gpu/xgmi.h"
#include "policy/device_payload.h"
#include "gpu/rccl_plane.h"
#include "rdma/rdma.h"
#include "mrpc/proto/echo.pb.h"
#include "base/time.h"
#include "press/press.h"
#include "press/stream_press.h"
#include "rpc/channel.h"
#include "rpc/controller.h"
#include "rpc/protocol.h"
#include "rpc/server.h"
#include "rpc/span.h"
#include "rpc/span_db.h"
#include "services/echo_service.h"
#include "var/variable.h"

namespace py = pybind11;

DECLARE_string(rdma_verbs_library);
using namespace mrpc;

void bind_gpu_ops(py::module_& m);  // gpu_ops.cc

namespace {

class PyServer {
public:
    PyServer() { GlobalInitializeOrDie(); }
    ~PyServer() { stop(); }
    void add_echo_service() {
        if (!_echo) {
            _echo.reset(new EchoServiceImpl);
            if (_server.AddService(_echo.get(), SERVER_DOESNT_OWN_SERVICE) != 0) throw std::runtime_error("AddService failed");
        }
    }
    int start(const std::string& addr, int num_threads, int gpu_device, int idle_timeout_s, bool use_rdma,
              int max_concurrency) {
        ServerOptions opt;
        opt.num_threads = num_threads;
        if (max_concurrency > 0) opt.max_concurrency = max_concurrency;
        if (_echo) _echo->set_gpu_device(gpu_device);
        opt.gpu_device = gpu_device;
        opt.idle_timeout_sec = idle_timeout_s;
        opt.use_rdma = use_rdma;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = addr.find(':') == std::string::npos ? _server.Start(std::stoi(addr), &opt)
                                                     : _server.Start(addr.c_str(), &opt);
        }
        if (rc != 0) throw std::runtime_error("fail to start server on " + addr);
        _running = true;
        return _server.listen_address().port;
    }
    void stop() {
        if (!_running) return;
        py::gil_scoped_release nogil;
        _server.Stop(0);
        _server.Join();
        _running = false;
    }
    int port() const { return _server.listen_address().port; }
    std::string address() const { return _server.listen_address().to_string(); }
    int64_t echo_calls() const { return _echo ? _echo->ncalls() : 0; }
    int64_t gpu_calls() const { return _echo ? _echo->gpu_calls() : 0; }

private:
    Server _server;
    std::unique_ptr<EchoServiceImpl> _echo;
    bool _running = false;
};

class PyChannel {
public:
    typedef std::vector<std::tuple<uint32_t, uint32_t, uintptr_t, uint64_t>> MessageFields;
    typedef std::tuple<uint32_t, uint32_t, uint32_t, uintptr_t, uint64_t, uintptr_t, uint64_t> RowsSource;
    typedef std::vector<std::tuple<uint32_t, uint32_t, uintptr_t, uint64_t, uintptr_t>> RecordColumns;
    PyChannel(const std::string& server, const std::string& lb, const std::string& protocol,
              const std::string& connection_type, int timeout_ms, int max_retry) {
        GlobalInitializeOrDie();
        ChannelOptions o;
        o.protocol = protocol;
        o.connection_type = connection_type;
        o.timeout_ms = timeout_ms;
        o.max_retry = max_retry;
        const int rc = lb.empty() ? _ch.Init(server.c_str(), &o) : _ch.Init(server.c_str(), lb.c_str(), &o);
        if (rc != 0) throw std::runtime_error("fail to init channel to " + server);
    }
    // Returns (message, attachment, latency_us); raises on RPC failure.
    py::tuple echo(const std::string& message, py::bytes attachment, int64_t sleep_us) {
        example::EchoRequest req;
        example::EchoResponse res;
        Controller cntl;
        req.set_message(message);
        if (sleep_us > 0) req.set_sleep_us(sleep_us);
        std::string att = attachment;
        cntl.request_attachment().append(att);
        {
            py::gil_scoped_release nogil;
            example::EchoService_Stub stub(&_ch);
            stub.Echo(&cntl, &req, &res, nullptr);
        }
        if (cntl.Failed()) {
            throw std::runtime_error("[E" + std::to_string(cntl.ErrorCode()) + "] " + cntl.ErrorText());
        }
        return py::make_tuple(res.message(), py::bytes(cntl.response_attachment().to_string()), cntl.latency_us());
    }
    // A Batch composed on the device and sent as a device attachment: the
    // block gpu::BuildDeviceMessage makes of `fields` [(number, kind, ptr,
    // count)], then the block gpu::BuildDeviceRows makes of `rows` (number,
    // inner, kind, src, count, row_ends, nrows), appended to one Buf (protobuf
    // concatenation is merge). Returns the echoed attachment's bytes.
    py::bytes echo_device_rows(const MessageFields& fields, const RowsSource& rows, int device) {
        Controller cntl;
        std::string got;
        int copy_rc = 0;
        echo_rows(fields, rows, device, &cntl, [&]() { copy_rc = gpu::CopyBufToHost(cntl.response_attachment(), &got); });
        if (copy_rc != 0) throw std::runtime_error("copying the echoed attachment to the host failed");
        return py::bytes(got);
    }
    // The same round trip, then the echoed attachment is split where it
    // arrived (gpu::DeviceSplitRows on its device block; blocks that arrived
    // apart are gathered into one in HBM first): only the split's outputs come
    // to the host. Returns (values bytes, row_ends list, others).
    py::tuple echo_device_rows_split(const MessageFields& fields, const RowsSource& rows, int device) {
        Controller cntl;
        gpu::DeviceRowsSplitJob job;
        job.number = std::get<0>(rows);
        job.inner = std::get<1>(rows);
        job.kind = std::get<2>(rows);
        if (!pb_rows::FieldsOk(job.number, job.inner, job.kind)) throw std::invalid_argument("rows job refused");
        std::string values;
        std::vector<uint32_t> row_ends;
        int rc = 0;
        echo_rows(fields, rows, device, &cntl, [&]() {
            const Buf& got = cntl.response_attachment();
            Buf gathered;
            const Buf* one = &got;
            if (got.backing_block_num() != 1 || got.ref_at(0).block->kind != MemKind::DEVICE ||
                got.ref_at(0).block->device != device) {
                if (gpu::GatherToDevice(got, &gathered, device) != 0 || gathered.backing_block_num() != 1) {
                    rc = -1;
                    return;
                }
                one = &gathered;
            }
            job.msg = one->block_data(0);
            job.n = one->block_len(0);
            const size_t eb = pb_rows::SourceBytes(job.kind);
            job.cap = job.n / (pb_rows::WireIsVarint(job.kind) ? 1 : eb);
            job.row_cap = job.n / 2;
            gpu::HbmBlock vals(std::max<size_t>(job.cap * eb, 16), device), ends(std::max<size_t>(job.row_cap * 4, 16), device);
            if (!vals || !ends) {
                rc = -1;
                return;
            }
            job.values = vals.p;
            job.row_ends = ends.as<uint32_t>();
            rc = gpu::DeviceSplitRows(&job, 1, device);
            if (rc != 0 || job.err != 0) return;
            values.resize((size_t)job.count * eb);
            row_ends.resize((size_t)job.rows);
            if (!values.empty()) rc = gpu::CopyDeviceToHost(&values[0], vals.p, values.size(), device);
            if (rc == 0 && !row_ends.empty()) rc = gpu::CopyDeviceToHost(row_ends.data(), ends.p, row_ends.size() * 4, device);
        });
        if (rc != 0) throw std::runtime_error("splitting the echoed attachment on the device failed");
        if (job.err != 0) {
            throw std::runtime_error("the echoed attachment does not split (code " + std::to_string(job.err) + ", offset " +
                                     std::to_string(job.first_bad) + ")");
        }
        return py::make_tuple(py::bytes(values), row_ends, job.others);
    }
    // A Batch whose repeated element has several fields: the block
    // gpu::BuildDeviceMessage makes of `fields`, then the block
    // gpu::BuildDeviceRecords makes of `columns` [(inner, kind, src, count,
    // row_ends)] (row_ends 0: a scalar column) over `rows` records of field
    // `number`, appended to one Buf. Returns the echoed attachment's bytes.
    py::bytes echo_device_records(const MessageFields& fields, uint32_t number, const RecordColumns& columns,
                                  uint64_t rows, int device) {
        Controller cntl;
        std::string got;
        int copy_rc = 0;
        echo_records(fields, number, columns, rows, device, &cntl,
                     [&]() { copy_rc = gpu::CopyBufToHost(cntl.response_attachment(), &got); });
        if (copy_rc != 0) throw std::runtime_error("copying the echoed attachment to the host failed");
        return py::bytes(got);
    }
    // The same round trip, then the echoed attachment is split where it
    // arrived (gpu::DeviceSplitRecords on its device block; blocks that
    // arrived apart are gathered into one in HBM first), with no host copy of
    // it: only the split's outputs come to the host. `split` is [(inner,
    // kind, scalar)], the columns to take. Returns ([(values bytes, row_ends
    // list or None, absent)] per split column, others).
    py::tuple echo_device_records_split(const MessageFields& fields, uint32_t number, const RecordColumns& columns,
                                        uint64_t rows, const std::vector<std::tuple<uint32_t, uint32_t, bool>>& split,
                                        int device) {
        Controller cntl;
        std::vector<gpu::DeviceRecordSplitColumn> cols(split.size());
        for (size_t c = 0; c < split.size(); ++c) {
            cols[c].inner = std::get<0>(split[c]);
            cols[c].kind = std::get<1>(split[c]);
            cols[c].scalar = std::get<2>(split[c]);
            if (!pb_records::ColumnOk(cols[c].inner, cols[c].kind, cols[c].scalar)) {
                throw std::invalid_argument("split column refused");
            }
        }
        if (cols.empty() || cols.size() > gpu::kDeviceRecordMaxColumns) throw std::invalid_argument("1 to 8 split columns");
        gpu::DeviceRecordsSplitJob job;
        job.number = number;
        job.columns = cols.data();
        job.ncols = (uint32_t)cols.size();
        std::vector<std::string> values(cols.size());
        std::vector<std::vector<uint32_t>> row_ends(cols.size());
        int rc = 0;
        echo_records(fields, number, columns, rows, device, &cntl, [&]() {
            const Buf& got = cntl.response_attachment();
            Buf gathered;
            const Buf* one = &got;
            if (got.backing_block_num() != 1 || got.ref_at(0).block->kind != MemKind::DEVICE ||
                got.ref_at(0).block->device != device) {
                if (gpu::GatherToDevice(got, &gathered, device) != 0 || gathered.backing_block_num() != 1) {
                    rc = -1;
                    return;
                }
                one = &gathered;
            }
            job.msg = one->block_data(0);
            job.n = one->block_len(0);
            job.row_cap = job.n / 2;
            std::vector<gpu::HbmBlock> vals, ends;
            for (gpu::DeviceRecordSplitColumn& col : cols) {
                const size_t eb = pb_rows::SourceBytes(col.kind);
                col.cap = col.scalar ? job.row_cap : job.n / (pb_rows::WireIsVarint(col.kind) ? 1 : eb);
                vals.emplace_back(std::max<size_t>(col.cap * eb, 16), device);
                ends.emplace_back(col.scalar ? 0 : std::max<size_t>(job.row_cap * 4, 16), device);
                if (!vals.back() || (!col.scalar && !ends.back())) {
                    rc = -1;
                    return;
                }
                col.values = vals.back().p;
                col.row_ends = ends.back().as<uint32_t>();
            }
            rc = gpu::DeviceSplitRecords(&job, 1, device);
            if (rc != 0 || job.err != 0) return;
            for (size_t c = 0; c < cols.size() && rc == 0; ++c) {
                values[c].resize((size_t)cols[c].count * pb_rows::SourceBytes(cols[c].kind));
                if (!values[c].empty()) rc = gpu::CopyDeviceToHost(&values[c][0], vals[c].p, values[c].size(), device);
                if (cols[c].scalar) continue;
                row_ends[c].resize((size_t)job.rows);
                if (rc == 0 && job.rows > 0) rc = gpu::CopyDeviceToHost(row_ends[c].data(), ends[c].p, job.rows * 4, device);
            }
        });
        if (rc != 0) throw std::runtime_error("splitting the echoed attachment on the device failed");
        if (job.err != 0) {
            throw std::runtime_error("the echoed attachment does not split (code " + std::to_string(job.err) + ", offset " +
                                     std::to_string(job.first_bad) + ")");
        }
        py::list out;
        for (size_t c = 0; c < cols.size(); ++c) {
            out.append(py::make_tuple(py::bytes(values[c]), cols[c].scalar ? py::object(py::none()) : py::cast(row_ends[c]),
                                      cols[c].absent));
        }
        return py::make_tuple(out, job.others);
    }

private:
    // Builds the message block and the records block, echoes them and runs
    // `then` on the response (without the GIL); throws what the build or the
    // RPC reports.
    template <typename F>
    void echo_records(const MessageFields& fields, uint32_t number, const RecordColumns& columns, uint64_t rows,
                      int device, Controller* cntl, F&& then) {
        example::EchoRequest req;
        example::EchoResponse res;
        req.set_message("records");
        std::vector<gpu::DeviceMessageField> fs(fields.size());
        for (size_t i = 0; i < fields.size(); ++i) {
            fs[i].number = std::get<0>(fields[i]);
            fs[i].kind = std::get<1>(fields[i]);
            fs[i].src = (const void*)std::get<2>(fields[i]);
            fs[i].count = std::get<3>(fields[i]);
        }
        std::vector<gpu::DeviceRecordColumn> cols(columns.size());
        for (size_t i = 0; i < columns.size(); ++i) {
            cols[i].inner = std::get<0>(columns[i]);
            cols[i].kind = std::get<1>(columns[i]);
            cols[i].src = (const void*)std::get<2>(columns[i]);
            cols[i].count = std::get<3>(columns[i]);
            cols[i].row_ends = (const uint32_t*)std::get<4>(columns[i]);
        }
        gpu::DeviceRecordsJob job;
        job.number = number;
        job.columns = cols.data();
        job.ncols = (uint32_t)cols.size();
        job.rows = rows;
        int rc = 0;
        {
            py::gil_scoped_release nogil;
            if (!fs.empty()) rc = gpu::BuildDeviceMessage(fs.data(), (int)fs.size(), &cntl->request_attachment(), device);
            if (rc == 0) rc = gpu::BuildDeviceRecords(job, &cntl->request_attachment(), device);
            if (rc == 0) {
                example::EchoService_Stub stub(&_ch);
                stub.Echo(cntl, &req, &res, nullptr);
                if (!cntl->Failed()) then();
            }
        }
        if (rc != 0) throw std::runtime_error("building the attachment on the device failed (code " + std::to_string(rc) + ")");
        if (cntl->Failed()) {
            throw std::runtime_error("[E" + std::to_string(cntl->ErrorCode()) + "] " + cntl->ErrorText());
        }
    }
    // Builds the two blocks, echoes them and runs `then` on the response
    // (without the GIL); throws what the build or the RPC reports.
    template <typename F>
    void echo_rows(const MessageFields& fields, const RowsSource& rows, int device, Controller* cntl, F&& then) {
        example::EchoRequest req;
        example::EchoResponse res;
        req.set_message("rows");
        std::vector<gpu::DeviceMessageField> fs(fields.size());
        for (size_t i = 0; i < fields.size(); ++i) {
            fs[i].number = std::get<0>(fields[i]);
            fs[i].kind = std::get<1>(fields[i]);
            fs[i].src = (const void*)std::get<2>(fields[i]);
            fs[i].count = std::get<3>(fields[i]);
        }
        gpu::DeviceRowsJob job;
        job.number = std::get<0>(rows);
        job.inner = std::get<1>(rows);
        job.kind = std::get<2>(rows);
        job.src = (const void*)std::get<3>(rows);
        job.count = std::get<4>(rows);
        job.row_ends = (const uint32_t*)std::get<5>(rows);
        job.rows = std::get<6>(rows);
        int rc = 0;
        {
            py::gil_scoped_release nogil;
            if (!fs.empty()) rc = gpu::BuildDeviceMessage(fs.data(), (int)fs.size(), &cntl->request_attachment(), device);
            if (rc == 0) rc = gpu::BuildDeviceRows(job, &cntl->request_attachment(), device);
            if (rc == 0) {
                example::EchoService_Stub stub(&_ch);
                stub.Echo(cntl, &req, &res, nullptr);
                if (!cntl->Failed()) then();
            }
        }
        if (rc != 0) throw std::runtime_error("building the attachment on the device failed (code " + std::to_string(rc) + ")");
        if (cntl->Failed()) {
            throw std::runtime_error("[E" + std::to_string(cntl->ErrorCode()) + "] " + cntl->ErrorText());
        }
    }

    Channel _ch;
};

press::PressOptions press_options(const py::dict& d) {
    press::PressOptions o;
    for (auto item : d) {
        const std::string k = py::str(item.first);
        py::handle v = item.second;
        if (k == "server") o.server = v.cast<std::string>();
        else if (k == "lb_policy") o.lb_policy = v.cast<std::string>();
        else if (k == "protocol") o.protocol = v.cast<std::string>();
        else if (k == "connection_type") o.connection_type = v.cast<std::string>();
        else if (k == "timeout_ms") o.timeout_ms = v.cast<int>();
        else if (k == "connect_timeout_ms") o.connect_timeout_ms = v.cast<int>();
        else if (k == "max_retry") o.max_retry = v.cast<int>();
        else if (k == "request_compress_type") o.request_compress_type = v.cast<int>();
        else if (k == "response_compress_type") o.response_compress_type = v.cast<int>();
        else if (k == "concurrency") o.concurrency = v.cast<int>();
        else if (k == "qps") o.qps = v.cast<double>();
        else if (k == "num_channels") o.num_channels = v.cast<int>();
        else if (k == "request_size") o.request_size = v.cast<int>();
        else if (k == "body") o.body = v.cast<std::string>();
        else if (k == "attachment_size") o.attachment_size = v.cast<int>();
        else if (k == "packed_ids") o.packed_ids = v.cast<int>();
        else if (k == "device_attachment") o.device_attachment = v.cast<bool>();
        else if (k == "attachment_body") o.attachment_body = v.cast<std::string>();
        else if (k == "attachment_pb") o.attachment_pb = v.cast<bool>();
        else if (k == "device_compress") o.device_compress = v.cast<int>();
        else if (k == "device_scan") o.device_scan = v.cast<bool>();
        else if (k == "device_build_ids") o.device_build_ids = v.cast<int>();
        else if (k == "verify_device_payload") o.verify_device_payload = v.cast<bool>();
        else if (k == "gpu_device") o.gpu_device = v.cast<int>();
        else if (k == "check_echo") o.check_echo = v.cast<bool>();
        else if (k == "fanout_servers") o.fanout_servers = v.cast<std::string>();
        else if (k == "scatter") o.scatter = v.cast<bool>();
        else if (k == "gpu_process") o.gpu_process = v.cast<bool>();
        else if (k == "cpu_process") o.cpu_process = v.cast<bool>();
        else if (k == "check_every") o.check_every = v.cast<int>();
        else if (k == "use_rdma") o.use_rdma = v.cast<bool>();
        else if (k == "proto_file") o.proto_file = v.cast<std::string>();
        else if (k == "include_paths") o.include_paths = v.cast<std::string>();
        else if (k == "method") o.method = v.cast<std::string>();
        else if (k == "input") o.input = v.cast<std::string>();
        else throw std::invalid_argument("unknown press option: " + k);
    }
    return o;
}

py::dict snapshot_dict(const press::Snapshot& s) {
    py::dict d;
    d["sent"] = s.sent;
    d["success"] = s.success;
    d["error"] = s.error;
    d["elapsed_s"] = s.elapsed_s;
    d["qps"] = s.qps;
    d["avg_us"] = s.avg_us;
    d["min_us"] = s.min_us;
    d["p50_us"] = s.p50_us;
    d["p70_us"] = s.p70_us;
    d["p90_us"] = s.p90_us;
    d["p95_us"] = s.p95_us;
    d["p97_us"] = s.p97_us;
    d["p99_us"] = s.p99_us;
    d["p999_us"] = s.p999_us;
    d["p9999_us"] = s.p9999_us;
    d["max_us"] = s.max_us;
    d["bytes"] = s.bytes;
    d["last_error_code"] = s.last_error_code;
    d["last_error"] = s.last_error;
    py::dict codes;
    for (const auto& kv : s.error_codes) codes[py::str(std::to_string(kv.first))] = py::make_tuple(kv.second.first, kv.second.second);
    d["error_codes"] = codes;
    return d;
}

class PyPress {
public:
    explicit PyPress(const py::dict& d) {
        GlobalInitializeOrDie();
        press::PressOptions o = press_options(d);
        std::string err;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = _s.Init(o, &err);
        }
        if (rc != 0) throw std::runtime_error("press init failed: " + err);
    }
    // Returns the calls never issued because max_seconds (>0) ran out
    // (0: all n ran).
    int64_t run_requests(int64_t n, double max_seconds) {
        py::gil_scoped_release nogil;
        const int64_t deadline = max_seconds > 0 ? monotonic_us() + (int64_t)(max_seconds * 1e6) : 0;
        return _s.RunRequests(n, deadline);
    }
    void run_for(double seconds) {
        py::gil_scoped_release nogil;
        _s.RunFor(seconds, nullptr);
    }
    py::dict stats() const { return snapshot_dict(_s.Stats()); }
    void reset_stats() { _s.ResetStats(); }

private:
    press::PressSession _s;
};

// Streaming-RPC throughput driver (press/stream_press.h).
class PyStreamPress {
public:
    explicit PyStreamPress(const py::dict& d) {
        GlobalInitializeOrDie();
        press::StreamPressOptions o;
        for (auto item : d) {
            const std::string k = py::str(item.first);
            py::handle v = item.second;
            if (k == "server") o.server = v.cast<std::string>();
            else if (k == "chunk_size") o.chunk_size = v.cast<int>();
            else if (k == "chunks_per_step") o.chunks_per_step = v.cast<int>();
            else if (k == "timeout_ms") o.timeout_ms = v.cast<int>();
            else if (k == "max_buf_size") o.max_buf_size = v.cast<int64_t>();
            else if (k == "pipeline_rounds") o.pipeline_rounds = v.cast<int>();
            else if (k == "device_chunks") o.device_chunks = v.cast<bool>();
            else if (k == "gpu_device") o.gpu_device = v.cast<int>();
            else if (k == "relay_chain") o.relay_chain = v.cast<std::string>();
            else throw std::invalid_argument("unknown stream press option: " + k);
        }
        _s.reset(new press::StreamPress);
        std::string err;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = _s->Init(o, &err);
        }
        if (rc != 0) throw std::runtime_error("stream press init failed: " + err);
    }
    // Steps completed; fewer than `steps` when max_seconds (>0) ran out
    // before the rest started.
    int run_steps(int steps, double max_seconds) {
        std::string err;
        int rc, done = 0;
        {
            py::gil_scoped_release nogil;
            const int64_t deadline = max_seconds > 0 ? monotonic_us() + (int64_t)(max_seconds * 1e6) : 0;
            rc = _s->RunSteps(steps, &err, deadline, &done);
        }
        if (rc != 0) throw std::runtime_error(err);
        return done;
    }
    py::dict stats() {
        py::dict d;
        d["bytes_sent"] = _s->bytes_sent();
        d["bytes_acked"] = _s->bytes_acked();
        d["steps"] = _s->steps_done();
        d["streams"] = _s->num_streams();
        return d;
    }
    void close() {
        py::gil_scoped_release nogil;
        _s.reset();
    }

private:
    std::unique_ptr<press::StreamPress> _s;
};

}  // namespace

PYBIND11_MODULE(_native, m) {
    m.doc() = "brpc_amd native runtime (fibers, RPC, press, MI355X device ops)";
    m.def("global_init", [] { GlobalInitializeOrDie(); });
    m.def("set_concurrency", [](int n) { return fiber::set_concurrency(n); });
    m.def("get_concurrency", [] { return fiber::get_concurrency(); });
    m.def("set_flag", [](const std::string& name, const std::string& value) {
        std::string err;
        if (!SetFlag(name, value, false, &err)) throw std::invalid_argument("set_flag " + name + ": " + err);
    });
    // placement on shared hosts: wake-up lateness per CPU, re-confinement
    m.def("probe_cpu_wake", [](const std::vector<int>& cpus, int duration_ms, int period_us, int threshold_us) {
        std::vector<fiber::CpuWakeProbe> r;
        {
            py::gil_scoped_release nogil;
            r = fiber::ProbeCpuWake(cpus, duration_ms, period_us, threshold_us);
        }
        py::list out;
        for (const auto& p : r) {
            py::dict d;
            d["cpu"] = p.cpu;
            d["wakes"] = p.wakes;
            d["late_p50_us"] = p.late_p50_us;
            d["late_p99_us"] = p.late_p99_us;
            d["late_max_us"] = p.late_max_us;
            d["late_over"] = p.late_over;
            d["run_delay_us"] = p.run_delay_us;
            d["nivcsw"] = p.nivcsw;
            out.append(d);
        }
        return out;
    }, py::arg("cpus"), py::arg("duration_ms") = 500, py::arg("period_us") = 1000, py::arg("threshold_us") = 150);
    m.def("rebind_l3_domain", [](int k) { return fiber::RebindL3Domain(k); });
    m.def("get_flag", [](const std::string& name) {
        std::string v;
        if (!GetFlag(name, &v)) throw std::invalid_argument("no flag " + name);
        return v;
    });
    // rpcz: recent spans (memory), spans by trace id / end time (disk store)
    m.def("press_slow_calls", [] { return press::TakeSlowCalls(); });
    // sampling CPU profile of the whole process (folded stacks), e.g. while a
    // press runs in another Python thread
    m.def("profile_cpu", [](double seconds, int hz) {
        std::string folded;
        int64_t n = 0;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = profiler::ProfileCpu(seconds, hz, &folded, nullptr, &n);
        }
        if (!ok) throw std::runtime_error("another CPU profile is running");
        return py::make_tuple(folded, n);
    }, py::arg("seconds"), py::arg("hz") = 999);
    m.def("monotonic_us", [] { return monotonic_us(); });
    m.def("rpcz_recent", [](size_t max) { return ListRecentSpans(max, 0); }, py::arg("max") = 100);
    m.def("rpcz_trace", [](uint64_t trace, size_t max) { return span_db::FindTrace(trace, max); },
          py::arg("trace_id"), py::arg("max") = 100, py::call_guard<py::gil_scoped_release>());
    m.def("rpcz_before", [](int64_t before_us, size_t max) { return span_db::ListBefore(before_us, max); },
          py::arg("before_us") = 0, py::arg("max") = 100, py::call_guard<py::gil_scoped_release>());
    m.def("rpcz_flush", [] { span_db::Flush(); }, py::call_guard<py::gil_scoped_release>());
    m.def("rpcz_stats", [] {
        const span_db::Stats st = span_db::GetStats();
        py::dict d;
        d["written"] = st.written;
        d["dropped"] = st.dropped;
        d["indexed"] = st.indexed;
        d["files"] = st.files;
        d["bytes"] = st.bytes;
        d["reloaded"] = st.reloaded;
        d["dir"] = st.dir;
        return d;
    });
    m.def("list_flags", [] {
        py::dict d;
        for (auto& f : ListFlags()) d[py::str(f.name)] = f.current_value;
        return d;
    });
    m.def("dump_vars", [](const std::string& filter) {
        std::vector<std::pair<std::string, std::string>> out;
        var::Variable::dump_exposed(&out, filter);
        py::dict d;
        for (auto& kv : out) d[py::str(kv.first)] = kv.second;
        return d;
    }, py::arg("filter") = "");
    m.def("dump_prometheus", [] { return var::Variable::dump_prometheus(); });
    m.def("crc32c", [](py::bytes b) {
        std::string s = b;
        return crc32c::Value(s.data(), s.size());
    });
    // Host snappy codec (the CPU half; the GPU decompressor is gpu.snappy_*).
    m.def("echo_body", [](const std::string& kind, size_t size) { return py::bytes(press::EchoBody(kind, size)); });
    m.def("snappy_compress", [](py::bytes b) {
        std::string s = b, out;
        snappy::Compress(s.data(), s.size(), &out);
        return py::bytes(out);
    });
    m.def("snappy_uncompress", [](py::bytes b) {
        std::string s = b, out;
        if (!snappy::Uncompress(s.data(), s.size(), &out)) throw std::invalid_argument("malformed snappy stream");
        return py::bytes(out);
    });
    // The body codec registry (rpc/compress.h) exactly as protocols call it:
    // a registered offload (GPU snappy) applies here too.
    // JSON -> message (type from a .proto loaded at run time) -> JSON, plus
    // the message's wire bytes and the JSON of those bytes parsed back —
    // parity checks against the reference's own JSON fixtures
    m.def("json_proto_roundtrip", [](const std::string& proto_dir, const std::string& proto_file,
                                     const std::string& type_name, py::bytes text, bool base64_to_bytes) {
        pb::Importer imp({proto_dir});
        std::string err;
        if (!imp.Import(proto_file, &err)) throw std::runtime_error("import " + proto_file + ": " + err);
        const pb::Descriptor* d = imp.FindMessageTypeByName(type_name);
        if (!d || !d->prototype) throw std::invalid_argument("unknown message type " + type_name);
        std::unique_ptr<pb::Message> msg(d->prototype->New());
        std::unique_ptr<pb::Message> back(d->prototype->New());
        std::string in = text, out, wire, out2;
        json2pb::Json2PbOptions jo;
        jo.base64_to_bytes = base64_to_bytes;
        json2pb::Pb2JsonOptions po;
        po.bytes_to_base64 = base64_to_bytes;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = json2pb::JsonToProtoMessage(in, msg.get(), jo, &err) &&
                 json2pb::ProtoMessageToJson(*msg, &out, po, &err) && msg->SerializeToString(&wire) &&
                 back->ParseFromString(wire) && json2pb::ProtoMessageToJson(*back, &out2, po, &err);
        }
        if (!ok) throw std::runtime_error(err);
        return py::make_tuple(out, py::bytes(wire), out2);
    }, py::arg("proto_dir"), py::arg("proto_file"), py::arg("type_name"), py::arg("json"),
       py::arg("base64_to_bytes") = false);
    // JsonToProtoMessage's verdict and error text (soft errors of optional
    // fields come back with ok=True), plus the message as JSON
    m.def("json_proto_parse", [](const std::string& proto_dir, const std::string& proto_file,
                                 const std::string& type_name, py::bytes text, bool base64_to_bytes) {
        pb::Importer imp({proto_dir});
        std::string err;
        if (!imp.Import(proto_file, &err)) throw std::runtime_error("import " + proto_file + ": " + err);
        const pb::Descriptor* d = imp.FindMessageTypeByName(type_name);
        if (!d || !d->prototype) throw std::invalid_argument("unknown message type " + type_name);
        std::unique_ptr<pb::Message> msg(d->prototype->New());
        std::string in = text, out, err2;
        json2pb::Json2PbOptions jo;
        jo.base64_to_bytes = base64_to_bytes;
        const bool ok = json2pb::JsonToProtoMessage(in, msg.get(), jo, &err);
        json2pb::Pb2JsonOptions po;
        po.bytes_to_base64 = base64_to_bytes;
        if (ok) json2pb::ProtoMessageToJson(*msg, &out, po, &err2);
        return py::make_tuple(ok, err, out);
    }, py::arg("proto_dir"), py::arg("proto_file"), py::arg("type_name"), py::arg("json"),
       py::arg("base64_to_bytes") = true);
    // wire bytes -> message -> JSON: ProtoMessageToJson's verdict and error
    // (a missing required field is one) plus the JSON
    m.def("json_proto_from_wire", [](const std::string& proto_dir, const std::string& proto_file,
                                     const std::string& type_name, py::bytes wire, bool bytes_to_base64,
                                     bool pretty) {
        pb::Importer imp({proto_dir});
        std::string err;
        if (!imp.Import(proto_file, &err)) throw std::runtime_error("import " + proto_file + ": " + err);
        const pb::Descriptor* d = imp.FindMessageTypeByName(type_name);
        if (!d || !d->prototype) throw std::invalid_argument("unknown message type " + type_name);
        std::unique_ptr<pb::Message> msg(d->prototype->New());
        const std::string in = wire;
        if (!msg->ParsePartialFromArray(in.data(), in.size())) throw std::runtime_error("bad wire bytes for " + type_name);
        std::string out;
        json2pb::Pb2JsonOptions po;
        po.bytes_to_base64 = bytes_to_base64;
        po.pretty_json = pretty;
        const bool ok = json2pb::ProtoMessageToJson(*msg, &out, po, &err);
        return py::make_tuple(ok, err, out);
    }, py::arg("proto_dir"), py::arg("proto_file"), py::arg("type_name"), py::arg("wire"),
       py::arg("bytes_to_base64") = false, py::arg("pretty") = false);
    // wire bytes -> message, nothing else: whether the dynamic host parser
    // (the type imported from a .proto at run time) takes them. The host
    // baseline of benchmarks/device_rows_split_bw.py.
    m.def("pb_dynamic_parse", [](const std::string& proto_dir, const std::string& proto_file,
                                 const std::string& type_name, py::bytes wire) {
        pb::Importer imp({proto_dir});
        std::string err;
        if (!imp.Import(proto_file, &err)) throw std::runtime_error("import " + proto_file + ": " + err);
        const pb::Descriptor* d = imp.FindMessageTypeByName(type_name);
        if (!d || !d->prototype) throw std::invalid_argument("unknown message type " + type_name);
        std::unique_ptr<pb::Message> msg(d->prototype->New());
        char* data = nullptr;
        Py_ssize_t size = 0;
        if (PyBytes_AsStringAndSize(wire.ptr(), &data, &size) != 0) throw py::error_already_set();
        py::gil_scoped_release nogil;
        return msg->ParsePartialFromArray(data, (size_t)size);
    }, py::arg("proto_dir"), py::arg("proto_file"), py::arg("type_name"), py::arg("wire"));
    // the text json::Value prints for a double (json::AppendShortestDouble;
    // non-finite values as quoted strings): the oracle of the array printers
    m.def("json_shortest_double", [](double x) { return py::bytes(json::Value(x).ToString()); });
    // pb2json's host printer of float (kind 8) / double (kind 9) arrays over
    // their memory image: b"v,v,...,v" (json2pb::FormatFloatArray)
    m.def("json_format_floats", [](py::bytes values, uint32_t kind) {
        const std::string data = values;
        if (kind != json2pb::kArrayKindFloat && kind != json2pb::kArrayKindDouble)
            throw std::invalid_argument("kind must be 8 (float) or 9 (double)");
        const size_t eb = kind == json2pb::kArrayKindFloat ? 4 : 8;
        if (data.size() % eb) throw std::invalid_argument("values must hold whole elements");
        std::vector<uint64_t> aligned((data.size() + 7) / 8);
        memcpy(aligned.data(), data.data(), data.size());
        std::string text;
        json2pb::FormatFloatArray(aligned.data(), data.size() / eb, kind, &text);
        return py::bytes(text);
    }, py::arg("values"), py::arg("kind"));
    // One JSON number (RFC 8259 grammar) to the double json::Reader makes of
    // it, an integer literal converted as Value::as_double() does
    // (base/decimal_to_double.h; the exact route where that does not decide)
    m.def("json_parse_double", [](py::bytes text) {
        const std::string t = text;
        decimal_to_double::NumberResult r;
        decimal_to_double::ParseJsonNumber(t.data(), t.data() + t.size(), &r);
        if (r.cls == decimal_to_double::kNeedsExact &&
            !json::ParseNumberExact(t.data(), t.data() + t.size(), &r.bits, &r.cls))
            r.cls = decimal_to_double::kMalformed;
        if (r.cls == decimal_to_double::kMalformed) throw std::invalid_argument("not a JSON number: " + t);
        const uint64_t bits = decimal_to_double::NumberToDoubleBits(r);
        double d;
        memcpy(&d, &bits, sizeof(d));
        return d;
    });
    // The host twin of the device number parser over a whole "[v,v,...]" or
    // bare "v,v,...,v" text (json::ParseNumberArray): (payload, classes), 8
    // bytes and a class byte per element (0 int64, 1 uint64, 2 double bits).
    // exact=False leaves the elements a device lane would hand back as class
    // 3 with payload 0. Raises ValueError naming the first malformed element.
    m.def("json_parse_numbers", [](py::bytes text, bool exact) {
        const std::string t = text;
        if (t.size() >= 0xFFFFFFFFull) throw std::invalid_argument("text must be below 4 GiB");
        std::vector<uint32_t> seps;
        json::NumberArraySeparators(t.data(), t.size(), &seps);
        const size_t n = seps.size() - 1;
        std::vector<uint64_t> payload(n);
        std::string classes(n, '\0');
        size_t bad = 0;
        if (!json::ParseNumberArray(t.data(), seps.data(), seps.size(), payload.data(),
                                    reinterpret_cast<uint8_t*>(&classes[0]), exact, &bad))
            throw py::value_error("element " + std::to_string(bad) + " is not a JSON number");
        return py::make_tuple(py::bytes(reinterpret_cast<const char*>(payload.data()), n * 8), py::bytes(classes));
    }, py::arg("text"), py::arg("exact") = true);
    // The host twin of gpu::DeviceParseNumberText (json::ParseNumberText):
    // bare, "[...]" or "[[...],[...]]" number text with no separator table ->
    // (err, depth, count, rows, first_bad, out, classes, row_ends). mode 0:
    // out holds 8 bytes of payload per element and classes a byte each; 1:
    // doubles; 2: floats. exact=False leaves the elements a device lane would
    // hand back as class 3 / zeros. nested=False refuses depth 2, as the
    // device does without a row_ends buffer.
    m.def("json_parse_number_text", [](py::bytes text, uint32_t mode, bool exact, bool nested) {
        char* p = nullptr;  // read in place
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &p, &n) != 0) throw py::error_already_set();
        json::NumberText r;
        json::ParseNumberText(p, (size_t)n, mode, &r, exact, nested);
        return py::make_tuple(r.err, r.depth, r.count, r.rows, r.first_bad, py::bytes(r.out), py::bytes(r.classes),
                              r.row_ends);
    }, py::arg("text"), py::arg("mode"), py::arg("exact") = true, py::arg("nested") = true);
    // The host twin of gpu::DevicePrintNumbers (json::FormatNumberRows):
    // `values` is the memory image of `count` elements of `kind` (0..6, 8, 9),
    // row_ends None (a flat form, bracketed or bare), a list, or the memory
    // image of a uint32 array as bytes (an empty one: row ends without rows)
    // -> (err, first_bad, text); the text is empty on a code other than 0.
    m.def("json_format_number_rows", [](py::bytes values, uint64_t count, uint32_t kind, py::object row_ends_obj,
                                        bool brackets) {
        std::vector<uint32_t> row_ends;
        const bool nested = !row_ends_obj.is_none();
        if (nested && py::isinstance<py::bytes>(row_ends_obj)) {
            const std::string image = row_ends_obj.cast<std::string>();
            if (image.size() % 4) throw std::invalid_argument("row_ends must hold whole uint32 entries");
            row_ends.resize(image.size() / 4);
            if (!image.empty()) memcpy(row_ends.data(), image.data(), image.size());
        } else if (nested) {
            row_ends = row_ends_obj.cast<std::vector<uint32_t>>();
        }
        const std::string data = values;
        // a kind there is not is the twin's to refuse
        if (number_print::KindValid(kind) && data.size() / number_print::ElemBytes(kind) < count)
            throw std::invalid_argument("values must hold count elements");
        // a std::string's buffer need not be aligned for 8-byte elements
        std::vector<uint64_t> aligned(data.size() / 8 + 1);
        memcpy(aligned.data(), data.data(), data.size());
        const size_t rows = row_ends.size();
        row_ends.push_back(0);  // data() of an empty table is still a table
        std::string text;
        uint32_t first_bad = 0;
        const int err = json::FormatNumberRows(aligned.data(), count, kind, nested ? row_ends.data() : nullptr, rows,
                                               brackets, &text, &first_bad);
        return py::make_tuple(err, first_bad, py::bytes(text));
    }, py::arg("values"), py::arg("count"), py::arg("kind"), py::arg("row_ends") = py::none(),
       py::arg("brackets") = true);
    // The host twin of gpu::DeviceBuildRows (pb::SerializeRows): `values`
    // holds the elements of all rows in the kind's vector layout, row_ends[r]
    // the elements in rows 0..r (a list, or the memory image of a uint32
    // array as bytes) -> (err, first_bad, wire bytes).
    m.def("pb_serialize_rows", [](uint32_t number, uint32_t inner, uint32_t kind, py::bytes values,
                                  py::object row_ends_obj) {
        std::vector<uint32_t> row_ends;
        if (py::isinstance<py::bytes>(row_ends_obj)) {
            const std::string image = row_ends_obj.cast<std::string>();
            if (image.size() % 4) throw std::invalid_argument("row_ends must hold whole uint32 entries");
            row_ends.resize(image.size() / 4);
            if (!image.empty()) memcpy(row_ends.data(), image.data(), image.size());
        } else {
            row_ends = row_ends_obj.cast<std::vector<uint32_t>>();
        }
        const std::string data = values;
        if (kind > pb_rows::kKindFixed64) throw std::invalid_argument("kind must be 0..9");
        const size_t eb = pb_rows::SourceBytes(kind);
        if (data.size() % eb) throw std::invalid_argument("values must hold whole elements");
        std::vector<uint64_t> aligned((data.size() + 7) / 8);
        if (!data.empty()) memcpy(aligned.data(), data.data(), data.size());
        std::string out;
        uint32_t first_bad = 0xFFFFFFFFu;
        static const uint32_t kNoRows = 0;
        const int err = pb::SerializeRows(number, inner, kind, data.empty() ? nullptr : aligned.data(),
                                          data.size() / eb, row_ends.empty() ? &kNoRows : row_ends.data(),
                                          row_ends.size(), &out, &first_bad);
        return py::make_tuple(err, first_bad, py::bytes(out));
    }, py::arg("number"), py::arg("inner"), py::arg("kind"), py::arg("values"), py::arg("row_ends"));
    // The host twin of gpu::DeviceBuildRecords (pb::SerializeRecords):
    // columns = [(inner, kind, values, row_ends)], values the memory image of
    // the column's elements in the kind's vector layout, row_ends a list or
    // the image of a uint32 array with `rows` entries, or None for a scalar
    // column -> (err, first_bad, bad_column, wire bytes).
    m.def("pb_serialize_records", [](uint32_t number, const std::vector<std::tuple<uint32_t, uint32_t, py::bytes, py::object>>& columns,
                                     uint64_t rows) {
        const size_t n = columns.size();
        std::vector<std::vector<uint64_t>> values(n);
        std::vector<std::vector<uint32_t>> ends(n);
        std::vector<pb_records::Column> cols(n);
        for (size_t c = 0; c < n; ++c) {
            cols[c].inner = std::get<0>(columns[c]);
            cols[c].kind = std::get<1>(columns[c]);
            const std::string data = std::get<2>(columns[c]);
            const size_t eb = cols[c].kind <= pb_rows::kKindFixed64 ? pb_rows::SourceBytes(cols[c].kind) : 1;
            if (data.size() % eb) throw std::invalid_argument("values must hold whole elements");
            values[c].resize(data.size() / 8 + 1);  // aligned for 8-byte elements, never null
            if (!data.empty()) memcpy(values[c].data(), data.data(), data.size());
            cols[c].src = values[c].data();
            cols[c].count = data.size() / eb;
            const py::object& re = std::get<3>(columns[c]);
            if (re.is_none()) continue;
            if (py::isinstance<py::bytes>(re)) {
                const std::string image = re.cast<std::string>();
                if (image.size() % 4) throw std::invalid_argument("row_ends must hold whole uint32 entries");
                ends[c].resize(image.size() / 4);
                if (!image.empty()) memcpy(ends[c].data(), image.data(), image.size());
            } else {
                ends[c] = re.cast<std::vector<uint32_t>>();
            }
            if (ends[c].size() != rows) throw std::invalid_argument("every row_ends must hold `rows` entries");
            ends[c].push_back(0);  // data() of an empty table is still a table
            cols[c].row_ends = ends[c].data();
        }
        pb_records::Job job;
        job.number = number;
        job.columns = cols.data();
        job.ncols = (uint32_t)n;
        job.rows = rows;
        std::string out;
        uint32_t first_bad = 0xFFFFFFFFu, bad_column = 0xFFFFFFFFu;
        const int err = pb::SerializeRecords(job, &out, &first_bad, &bad_column);
        return py::make_tuple(err, first_bad, bad_column, py::bytes(out));
    }, py::arg("number"), py::arg("columns"), py::arg("rows"));
    // The host twin of gpu::DevicePrintRecordObjects
    // (json::FormatRecordObjects): columns = [(key, kind, text_form, values,
    // row_ends)], key raw bytes, text_form 0 (a number kind), 1 (string) or 2
    // (base64), values and row_ends as in pb_serialize_records ->
    // (err, first_bad, bad_column, text); the text is empty on a code other
    // than 0.
    m.def("json_format_record_objects", [](const std::vector<std::tuple<py::bytes, uint32_t, uint32_t, py::bytes, py::object>>& columns,
                                           uint64_t rows, bool brackets) {
        const size_t n = columns.size();
        std::vector<std::string> keys(n);
        std::vector<std::vector<uint64_t>> values(n);
        std::vector<std::vector<uint32_t>> ends(n);
        std::vector<json_records::Column> cols(n);
        for (size_t c = 0; c < n; ++c) {
            keys[c] = std::get<0>(columns[c]);
            cols[c].key = keys[c].data();
            cols[c].key_len = (uint32_t)keys[c].size();
            cols[c].kind = std::get<1>(columns[c]);
            cols[c].text = std::get<2>(columns[c]);
            const std::string data = std::get<3>(columns[c]);
            // a kind there is not is the twin's to refuse
            const size_t eb = cols[c].kind == json_records::kKindBytes || !number_print::KindValid(cols[c].kind)
                                  ? 1
                                  : number_print::ElemBytes(cols[c].kind);
            if (data.size() % eb) throw std::invalid_argument("values must hold whole elements");
            values[c].resize(data.size() / 8 + 1);  // aligned for 8-byte elements, never null
            if (!data.empty()) memcpy(values[c].data(), data.data(), data.size());
            cols[c].src = values[c].data();
            cols[c].count = data.size() / eb;
            const py::object& re = std::get<4>(columns[c]);
            if (re.is_none()) continue;
            if (py::isinstance<py::bytes>(re)) {
                const std::string image = re.cast<std::string>();
                if (image.size() % 4) throw std::invalid_argument("row_ends must hold whole uint32 entries");
                ends[c].resize(image.size() / 4);
                if (!image.empty()) memcpy(ends[c].data(), image.data(), image.size());
            } else {
                ends[c] = re.cast<std::vector<uint32_t>>();
            }
            if (ends[c].size() != rows) throw std::invalid_argument("every row_ends must hold `rows` entries");
            ends[c].push_back(0);  // data() of an empty table is still a table
            cols[c].row_ends = ends[c].data();
        }
        json_records::Job job;
        job.columns = cols.data();
        job.ncols = (uint32_t)n;
        job.rows = rows;
        job.brackets = brackets;
        std::string out;
        uint32_t first_bad = 0xFFFFFFFFu, bad_column = 0xFFFFFFFFu;
        const int err = json::FormatRecordObjects(job, &out, &first_bad, &bad_column);
        return py::make_tuple(err, first_bad, bad_column, py::bytes(out));
    }, py::arg("columns"), py::arg("rows"), py::arg("brackets") = true);
    // The host twin of gpu::DeviceSplitRows (pb::SplitRows): the message's
    // rows of field `number` -> (err, count, rows, others, first_bad, values
    // bytes, row_ends list). max_elems / max_rows are the outputs' capacities
    // (default: what any message of this size can hold); values and row_ends
    // are empty unless err is 0.
    m.def("pb_split_rows", [](uint32_t number, uint32_t inner, uint32_t kind, py::bytes message, py::object max_elems,
                              py::object max_rows) {
        if (kind > pb_rows::kKindFixed64) throw std::invalid_argument("kind must be 0..9");
        const std::string msg = message;
        const size_t eb = pb_rows::SourceBytes(kind);
        const uint64_t cap = max_elems.is_none() ? msg.size() / (pb_rows::WireIsVarint(kind) ? 1 : eb)
                                                 : max_elems.cast<uint64_t>();
        const uint64_t row_cap = max_rows.is_none() ? msg.size() / 2 : max_rows.cast<uint64_t>();
        std::vector<uint64_t> values((size_t)(cap * eb + 7) / 8 + 1);
        std::vector<uint32_t> row_ends((size_t)row_cap + 1);
        uint64_t count = 0, rows = 0, others = 0, first_bad = 0;
        const int err = pb::SplitRows(number, inner, kind, msg.data(), msg.size(), values.data(), cap, row_ends.data(),
                                      row_cap, &count, &rows, &others, &first_bad);
        row_ends.resize(err == 0 ? (size_t)rows : 0);
        return py::make_tuple(err, count, rows, others, first_bad,
                              py::bytes(reinterpret_cast<const char*>(values.data()), err == 0 ? (size_t)count * eb : 0),
                              row_ends);
    }, py::arg("number"), py::arg("inner"), py::arg("kind"), py::arg("message"), py::arg("max_elems") = py::none(),
       py::arg("max_rows") = py::none());
    // The host twin of gpu::DeviceSplitRecords (pb::SplitRecords): the
    // message's records of field `number`, columns = [(inner, kind, scalar)]
    // -> (err, rows, others, first_bad, [(count, absent, values bytes,
    // row_ends list or None)]). max_rows is the capacity of every row_ends
    // and max_elems a list of the columns' capacities (default: what any
    // message of this size can hold); values and row_ends are empty unless
    // err is 0. With ends_as_bytes the row ends come as the memory image of a
    // uint32 array, not as a list.
    m.def("pb_split_records", [](uint32_t number, const std::vector<std::tuple<uint32_t, uint32_t, bool>>& columns,
                                 py::bytes message, py::object max_rows, py::object max_elems, bool ends_as_bytes) {
        const std::string msg = message;
        const size_t nc = columns.size();
        std::vector<uint64_t> caps;
        if (!max_elems.is_none()) {
            caps = max_elems.cast<std::vector<uint64_t>>();
            if (caps.size() != nc) throw std::invalid_argument("max_elems must hold one capacity per column");
        }
        pb::SplitRecordsJob job;
        job.number = number;
        job.msg = msg.data();
        job.n = msg.size();
        job.row_cap = max_rows.is_none() ? msg.size() / 2 : max_rows.cast<uint64_t>();
        std::vector<pb::SplitRecordsColumn> cols(nc);
        std::vector<std::vector<uint64_t>> values(nc);
        std::vector<std::vector<uint32_t>> ends(nc);
        for (size_t c = 0; c < nc; ++c) {
            cols[c].inner = std::get<0>(columns[c]);
            cols[c].kind = std::get<1>(columns[c]);
            cols[c].scalar = std::get<2>(columns[c]);
            const size_t eb = cols[c].kind <= pb_rows::kKindFixed64 ? pb_rows::SourceBytes(cols[c].kind) : 1;
            cols[c].cap = !caps.empty() ? caps[c]
                          : cols[c].scalar ? job.row_cap
                                           : msg.size() / (cols[c].kind >= pb_rows::kKindFixed32 ? eb : 1);
            values[c].resize((size_t)(cols[c].cap * eb + 7) / 8 + 1);
            ends[c].resize((size_t)job.row_cap + 1);
            cols[c].values = values[c].data();
            cols[c].row_ends = cols[c].scalar ? nullptr : ends[c].data();
        }
        job.columns = cols.data();
        job.ncols = (uint32_t)nc;
        const int err = pb::SplitRecords(&job);
        py::list out;
        for (size_t c = 0; c < nc; ++c) {
            const size_t eb = cols[c].kind <= pb_rows::kKindFixed64 ? pb_rows::SourceBytes(cols[c].kind) : 1;
            ends[c].resize(err == 0 ? (size_t)job.rows : 0);
            out.append(py::make_tuple(cols[c].count, cols[c].absent,
                                      py::bytes(reinterpret_cast<const char*>(values[c].data()),
                                                err == 0 ? (size_t)cols[c].count * eb : 0),
                                      cols[c].scalar  ? py::object(py::none())
                                      : ends_as_bytes ? py::object(py::bytes(reinterpret_cast<const char*>(ends[c].data()),
                                                                             ends[c].size() * sizeof(uint32_t)))
                                                      : py::cast(ends[c])));
        }
        return py::make_tuple(err, job.rows, job.others, job.first_bad, out);
    }, py::arg("number"), py::arg("columns"), py::arg("message"), py::arg("max_rows") = py::none(),
       py::arg("max_elems") = py::none(), py::arg("ends_as_bytes") = false);
    // The host base64 coder (base/util.h over base/base64.h), reading the
    // bytes object in place: the text pb2json gives a bytes field, and what
    // json2pb makes of one (None where base64_decode refuses the text).
    m.def("base64_encode", [](py::bytes data) {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(data.ptr(), &p, &n) != 0) throw py::error_already_set();
        const size_t len = (size_t)base64::Base64EncodedBytes((uint64_t)n);
        PyObject* out = PyBytes_FromStringAndSize(nullptr, (Py_ssize_t)len);
        if (!out) throw py::error_already_set();
        base64_encode_to(p, (size_t)n, PyBytes_AS_STRING(out));
        return py::reinterpret_steal<py::bytes>(out);
    });
    m.def("base64_decode", [](py::bytes text) -> py::object {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &p, &n) != 0) throw py::error_already_set();
        std::string out;
        if (!base64_decode(p, (size_t)n, &out)) return py::none();
        return py::bytes(out);
    });
    // The host twins of the device string entries (json/json.h over
    // base/json_string.h), reading the bytes objects in place. json_escape:
    // the quoted (quote=True) or bare escaped body, or with row_ends (uint32
    // little-endian bytes, ascending to len(data)) "r0","r1",... .
    // json_unescape: (bytes, 0), or (None, first_bad) where the twin leaves
    // the body to json::Reader. utf8_first_bad: the offset, or len(data).
    m.def("json_escape", [](py::bytes data, py::object row_ends, bool quote) {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(data.ptr(), &p, &n) != 0) throw py::error_already_set();
        std::string out;
        if (row_ends.is_none()) {
            if (quote) out.push_back('"');
            json::EscapeStringBody(p, (size_t)n, &out);
            if (quote) out.push_back('"');
            return py::bytes(out);
        }
        const std::string ends = py::cast<py::bytes>(row_ends);
        if (ends.size() % 4 != 0) throw py::value_error("row_ends: a multiple of 4 bytes");
        std::vector<uint32_t> e(ends.size() / 4);
        if (!e.empty()) memcpy(e.data(), ends.data(), ends.size());
        if ((e.empty() ? 0u : e.back()) != (uint64_t)n) throw py::value_error("row_ends does not end at len(data)");
        if (!json::EscapeStringRows(p, e.data(), e.size(), &out)) throw py::value_error("row_ends decreases");
        return py::bytes(out);
    }, py::arg("data"), py::arg("row_ends") = py::none(), py::arg("quote") = true);
    m.def("json_unescape", [](py::bytes body) -> py::tuple {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(body.ptr(), &p, &n) != 0) throw py::error_already_set();
        std::string out;
        uint64_t first_bad = 0;
        if (json::UnescapeStringBody(p, (size_t)n, &out, &first_bad) != 0)
            return py::make_tuple(py::none(), first_bad);
        return py::make_tuple(py::bytes(out), 0);
    });
    m.def("utf8_first_bad", [](py::bytes data) {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(data.ptr(), &p, &n) != 0) throw py::error_already_set();
        return json::Utf8FirstBad(p, (size_t)n);
    });
    // json_unescape_rows: the twin of the device's rows unescaper over the text
    // of an array of strings, (bytes, row_ends list, depth), or (None,
    // first_bad) where it leaves the text to json::Reader.
    m.def("json_unescape_rows", [](py::bytes text) -> py::tuple {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &p, &n) != 0) throw py::error_already_set();
        json::StringRows rows;
        if (json::UnescapeStringRows(p, (size_t)n, &rows) != 0) return py::make_tuple(py::none(), rows.first_bad);
        py::list ends;
        for (uint32_t e : rows.row_ends) ends.append(e);
        return py::make_tuple(py::bytes(rows.bytes), ends, rows.depth);
    });
    // The host twins of the device's base64 rows entries (json/json.h over
    // base/base64_rows.h). base64_encode_rows: row_ends as uint32 little-endian
    // bytes ascending to len(data) -> "b0","b1",..., in '[' ']' with brackets.
    // base64_decode_rows: (bytes, row_ends list, depth), or (None, first_bad)
    // where the twin leaves the text to json::Reader and base64_decode.
    m.def("base64_encode_rows", [](py::bytes data, py::bytes row_ends, bool brackets) {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(data.ptr(), &p, &n) != 0) throw py::error_already_set();
        const std::string ends = row_ends;
        if (ends.size() % 4 != 0) throw py::value_error("row_ends: a multiple of 4 bytes");
        std::vector<uint32_t> e(ends.size() / 4);
        if (!e.empty()) memcpy(e.data(), ends.data(), ends.size());
        if ((e.empty() ? 0u : e.back()) != (uint64_t)n) throw py::value_error("row_ends does not end at len(data)");
        std::string out;
        if (!json::EncodeBase64Rows(p, e.data(), e.size(), brackets, &out)) throw py::value_error("row_ends decreases");
        return py::bytes(out);
    }, py::arg("data"), py::arg("row_ends"), py::arg("brackets") = true);
    m.def("base64_decode_rows", [](py::bytes text) -> py::tuple {
        char* p = nullptr;
        Py_ssize_t n = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &p, &n) != 0) throw py::error_already_set();
        json::StringRows rows;
        if (json::DecodeBase64Rows(p, (size_t)n, &rows) != 0) return py::make_tuple(py::none(), rows.first_bad);
        py::list ends;
        for (uint32_t e : rows.row_ends) ends.append(e);
        return py::make_tuple(py::bytes(rows.bytes), ends, rows.depth);
    });
    // What json::Reader makes of the text of an array of strings (a text whose
    // first byte that is no whitespace is not '[' is bracketed first): the list
    // of bytes, or None when it refuses or an element is no string.
    m.def("json_reader_string_array", [](py::bytes text) -> py::object {
        std::string t = (std::string)text;
        const size_t first = t.find_first_not_of(" \t\n\r");
        if (first == std::string::npos || t[first] != '[') t = "[" + t + "]";
        json::Value v;
        if (!json::Parse(t, &v) || !v.is_array()) return py::none();
        py::list out;
        for (const json::Value& e : v.array()) {
            if (!e.is_string()) return py::none();
            out.append(py::bytes(e.as_string()));
        }
        return out;
    });
    // The twins between raw buffers (pinned host memory of a benchmark), the
    // GIL released: op 0 escape (quoted; with row_ends the rows form), 1
    // unescape, 2 validate, 3 unescape rows (row_ends receives up to `rows`
    // uint32), 4 the same through json::Reader and a concatenation, what a
    // handler had before the twin. Returns the bytes written at dst (validate:
    // the first bad offset), -1 when the twin refuses or dst is too small.
    m.def("json_string_twin", [](int op, uintptr_t src, size_t n, uintptr_t dst, size_t cap, uintptr_t row_ends,
                                 size_t rows) -> int64_t {
        py::gil_scoped_release nogil;
        const char* s = reinterpret_cast<const char*>(src);
        if (op == 2) return (int64_t)json::Utf8FirstBad(s, n);
        if (op == 3 || op == 4) {
            json::StringRows got;
            if (op == 3) {
                if (json::UnescapeStringRows(s, n, &got) != 0) return -1;
            } else {
                json::Value v;
                if (!json::Parse(s, n, &v) || !v.is_array()) return -1;
                for (const json::Value& e : v.array()) {
                    if (!e.is_string()) return -1;
                    got.bytes += e.as_string();
                    got.row_ends.push_back((uint32_t)got.bytes.size());
                }
            }
            if (got.bytes.size() > cap || got.row_ends.size() > rows) return -1;
            memcpy(reinterpret_cast<char*>(dst), got.bytes.data(), got.bytes.size());
            memcpy(reinterpret_cast<char*>(row_ends), got.row_ends.data(), got.row_ends.size() * 4);
            return (int64_t)got.bytes.size();
        }
        std::string out;
        if (op == 0 && row_ends) {
            if (!json::EscapeStringRows(s, reinterpret_cast<const uint32_t*>(row_ends), rows, &out)) return -1;
        } else if (op == 0) {
            out.reserve(n + 2);
            out.push_back('"');
            json::EscapeStringBody(s, n, &out);
            out.push_back('"');
        } else if (json::UnescapeStringBody(s, n, &out) != 0) {
            return -1;
        }
        if (out.size() > cap) return -1;
        memcpy(reinterpret_cast<char*>(dst), out.data(), out.size());
        return (int64_t)out.size();
    }, py::arg("op"), py::arg("src"), py::arg("n"), py::arg("dst"), py::arg("cap"), py::arg("row_ends") = 0,
       py::arg("rows") = 0);
    // The base64 rows twins between raw buffers (pinned host memory of a
    // benchmark), the GIL released: op 0 encode (row_ends: `rows` uint32, text
    // at dst), op 1 decode (bytes at dst, row_ends receives up to `rows`
    // uint32). Returns (bytes written at dst, rows), (-1, 0) when the twin
    // refuses or an output is too small.
    m.def("base64_rows_twin", [](int op, uintptr_t src, size_t n, uintptr_t dst, size_t cap, uintptr_t row_ends,
                                 size_t rows, bool brackets) -> std::pair<int64_t, uint64_t> {
        py::gil_scoped_release nogil;
        const char* s = reinterpret_cast<const char*>(src);
        if (op == 0) {
            std::string out;
            if (!json::EncodeBase64Rows(s, reinterpret_cast<const uint32_t*>(row_ends), rows, brackets, &out) ||
                out.size() > cap)
                return {-1, 0};
            memcpy(reinterpret_cast<char*>(dst), out.data(), out.size());
            return {(int64_t)out.size(), rows};
        }
        json::StringRows got;
        if (json::DecodeBase64Rows(s, n, &got) != 0 || got.bytes.size() > cap || got.row_ends.size() > rows) return {-1, 0};
        memcpy(reinterpret_cast<char*>(dst), got.bytes.data(), got.bytes.size());
        memcpy(reinterpret_cast<char*>(row_ends), got.row_ends.data(), got.row_ends.size() * 4);
        return {(int64_t)got.bytes.size(), got.row_ends.size()};
    }, py::arg("op"), py::arg("src"), py::arg("n"), py::arg("dst"), py::arg("cap"), py::arg("row_ends"), py::arg("rows"),
       py::arg("brackets") = true);
    // What json::Reader makes of '"' + body + '"': the bytes, or None where it refuses.
    m.def("json_reader_string", [](py::bytes body) -> py::object {
        std::string text = "\"";
        text += (std::string)body;
        text += '"';
        json::Value v;
        if (!json::Parse(text, &v) || !v.is_string()) return py::none();
        return py::bytes(v.as_string());
    });
    m.def("narrow_double_bits",[](uint64_t bits) { return decimal_to_double::NarrowDoubleBits(bits); });
    m.def("json_max_device_number_chars", [] { return decimal_to_double::kMaxDeviceNumberChars; });
    // json::Parse alone (the DOM is dropped): (ok, error). packed=False parses
    // number arrays element by element, as before packed numbers.
    m.def("json_parse_check", [](py::bytes text, bool packed) {
        char* t = nullptr;  // read in place
        Py_ssize_t tn = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &t, &tn) != 0) throw py::error_already_set();
        std::string err;
        bool ok;
        {
            py::gil_scoped_release nogil;
            json::Value v;
            json::SetPackedNumberArrays(packed);
            ok = json::Parse(t, (size_t)tn, &v, &err);
            json::SetPackedNumberArrays(true);
        }
        return py::make_tuple(ok, err);
    }, py::arg("text"), py::arg("packed") = true);
    m.def("json_to_pb_to_json", [](const std::string& type_name, py::bytes text) {
        const pb::Descriptor* d = pb::DescriptorPool::generated_pool()->FindMessageTypeByName(type_name);
        if (!d || !d->prototype) throw std::invalid_argument("unknown message type " + type_name);
        std::unique_ptr<pb::Message> msg(d->prototype->New());
        std::string in = text, err, out;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = json2pb::JsonToProtoMessage(in, msg.get(), json2pb::Json2PbOptions(), &err) &&
                 json2pb::ProtoMessageToJson(*msg, &out, json2pb::Pb2JsonOptions(), &err);
        }
        if (!ok) throw std::runtime_error(err);
        return out;
    });
    m.def("compress", [](int type, py::bytes b) {
        std::string s = b;
        Buf in(s), out;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = CompressBuf((CompressType)type, in, &out);
        }
        if (!ok) throw std::invalid_argument("compression failed");
        return py::bytes(out.to_string());
    });
    m.def("decompress", [](int type, py::bytes b) {
        std::string s = b;
        Buf in(s), out;
        bool ok;
        {
            py::gil_scoped_release nogil;
            ok = DecompressBuf((CompressType)type, in, &out);
        }
        if (!ok) throw std::invalid_argument("decompression failed");
        return py::bytes(out.to_string());
    });
    m.def("fiber_stats", [] {
        py::dict d;
        d["fibers"] = fiber::fiber_count();
        d["switches"] = fiber::switch_count();
        d["steals"] = fiber::steal_count();
        d["workers"] = fiber::get_concurrency();
        return d;
    });

    py::class_<PyServer>(m, "Server")
        .def(py::init<>())
        .def("add_echo_service", &PyServer::add_echo_service)
        .def("start", &PyServer::start, py::arg("addr"), py::arg("num_threads") = -1, py::arg("gpu_device") = -1,
             py::arg("idle_timeout_s") = -1, py::arg("use_rdma") = false, py::arg("max_concurrency") = 0)
        .def("stop", &PyServer::stop)
        .def_property_readonly("port", &PyServer::port)
        .def_property_readonly("address", &PyServer::address)
        .def_property_readonly("echo_calls", &PyServer::echo_calls)
        .def_property_readonly("gpu_calls", &PyServer::gpu_calls);

    py::class_<PyChannel>(m, "Channel")
        .def(py::init<const std::string&, const std::string&, const std::string&, const std::string&, int, int>(),
             py::arg("server"), py::arg("lb") = "", py::arg("protocol") = "baidu_std",
             py::arg("connection_type") = "", py::arg("timeout_ms") = 1000, py::arg("max_retry") = 3)
        .def("echo", &PyChannel::echo, py::arg("message"), py::arg("attachment") = py::bytes(),
             py::arg("sleep_us") = 0)
        .def("echo_device_rows", &PyChannel::echo_device_rows, py::arg("fields"), py::arg("rows"),
             py::arg("device") = 0)
        .def("echo_device_records", &PyChannel::echo_device_records, py::arg("fields"), py::arg("number"),
             py::arg("columns"), py::arg("rows"), py::arg("device") = 0)
        .def("echo_device_rows_split", &PyChannel::echo_device_rows_split, py::arg("fields"), py::arg("rows"),
             py::arg("device") = 0)
        .def("echo_device_records_split", &PyChannel::echo_device_records_split, py::arg("fields"), py::arg("number"),
             py::arg("columns"), py::arg("rows"), py::arg("split"), py::arg("device") = 0);

    py::class_<PyStreamPress>(m, "StreamPress")
        .def(py::init<const py::dict&>())
        .def("run_steps", &PyStreamPress::run_steps, py::arg("steps"), py::arg("max_seconds") = 0.0)
        .def("stats", &PyStreamPress::stats)
        .def("close", &PyStreamPress::close);

    py::class_<PyPress>(m, "Press")
        .def(py::init<const py::dict&>())
        .def("run_requests", &PyPress::run_requests, py::arg("n"), py::arg("max_seconds") = 0.0)
        .def("run_for", &PyPress::run_for)
        .def("stats", &PyPress::stats)
        .def("reset_stats", &PyPress::reset_stats);

    py::module_ g = m.def_submodule("gpu", "MI355X device runtime");
    g.def("device_count", [] { return gpu::DeviceCount(); });
    g.def("available", [] { return gpu::Available(); });
    g.def("init", [](int dev) {
        std::string err;
        if (gpu::Init(dev, &err) != 0) throw std::runtime_error(err);
    }, py::arg("device") = -1);
    g.def("device_arch", [](int dev) { return gpu::DeviceArch(dev); }, py::arg("device") = 0);
    g.def("device_name", [](int dev) { return gpu::DeviceName(dev); }, py::arg("device") = 0);
    g.def("pci_bus_id", [](int dev) { return gpu::PciBusId(dev); }, py::arg("device") = 0);
    g.def("polled_events", [] { return gpu::PolledEvents(); });
    g.def("enable_xgmi", [](int dev) {
        std::string err;
        if (gpu::EnableXgmiTransport(dev, &err) != 0) throw std::runtime_error(err);
    }, py::arg("device") = 0);
    g.def("xgmi_stats", [] {
        const gpu::XgmiStats s = gpu::GetXgmiStats();
        py::dict d;
        d["sent_bytes"] = s.sent_bytes;
        d["recv_bytes"] = s.recv_bytes;
        d["sent_payloads"] = s.sent_payloads;
        d["recv_payloads"] = s.recv_payloads;
        d["ring_full_fallbacks"] = s.ring_full_fallbacks;
        d["crc_failures"] = s.crc_failures;
        d["lent_outstanding"] = s.lent_outstanding;
        d["copied_into_arena"] = s.copied_into_arena;
        d["released_unconsumed"] = s.released_unconsumed;
        d["cross_device_payloads"] = s.cross_device_payloads;
        d["cross_device_bytes"] = s.cross_device_bytes;
        d["cross_device_pull_failures"] = s.cross_device_pull_failures;
        d["peer_access_enabled"] = s.peer_access_enabled;
        d["attach_failures"] = s.attach_failures;
        d["peer_maps"] = s.peer_maps;
        d["compressed_sent"] = s.compressed_sent;
        d["compressed_recv"] = s.compressed_recv;
        d["compress_skipped_raw"] = s.compress_skipped_raw;
        d["compress_failures"] = s.compress_failures;
        d["compress_skipped_adaptive"] = s.compress_skipped_adaptive;
        int64_t staged = 0, staged_bytes = 0;
        GetStagedStats(&staged, &staged_bytes);
        d["staged_payloads"] = staged;
        d["staged_bytes"] = staged_bytes;
        const gpu::CopyEngineStats c = gpu::GetCopyEngineStats();
        d["copy_submits"] = c.submits;
        d["copy_launches"] = c.launches;
        d["copy_segments"] = c.segments;
        d["copy_bytes"] = c.bytes;
        d["copy_queue_us"] = c.queue_us;
        d["copy_api_us"] = c.api_us;
        d["copy_gpu_us"] = c.gpu_us;
        d["copy_wake_us"] = c.wake_us;
        d["copy_kernel_ticks"] = c.kernel_ticks;
        d["copy_kernel_timed"] = c.kernel_timed;
        d["copy_start_delay_us"] = c.start_delay_us;
        d["copy_notice_us"] = c.notice_us;
        return d;
    });
    g.def("reap_lent", [] { gpu::ReapLentBlocks(); });
    // RCCL data plane (gpu/rccl_plane.h): collective init from every rank
    g.def("rccl_unique_id", [] {
        std::string err;
        std::string id = gpu::rccl::UniqueId(&err);
        if (id.empty()) throw std::runtime_error(err);
        return py::bytes(id);
    });
    g.def("rccl_init", [](int rank, int world, py::bytes uid, int dev) {
        std::string err, id = uid;
        int rc;
        {
            py::gil_scoped_release nogil;  // blocks until every rank joined
            rc = gpu::rccl::Init(rank, world, id, dev, &err);
        }
        if (rc != 0) throw std::runtime_error(err);
    }, py::arg("rank"), py::arg("world"), py::arg("unique_id"), py::arg("device"));
    // GPUDirect RDMA registration of REAL HBM (arena memory) through the HIP
    // dmabuf export (hipMemGetHandleForAddressRange) and the ibverbs
    // provider loaded from `verbs_library` (the stub on hosts without an HCA)
    g.def("dmabuf_register_probe", [](const std::string& verbs_library, size_t nbytes, int dev) {
        py::dict d;
        std::string err;
        if (gpu::Init(dev, &err) != 0 || gpu::InitHbmPool(dev, &err) != 0) throw std::runtime_error(err);
        Buf hold;
        void* p = gpu::AppendNewDeviceBlock(&hold, nbytes, dev);
        if (!p) throw std::runtime_error("no HBM");
        d["arena_offset"] = gpu::ArenaOffset(p, dev);
        // the export itself: a dmabuf fd naming the HBM range
        int fd = -1;
        uint64_t off = 0;
        rdma::DmabufExportFn ex = rdma::GetDmabufExportHook();
        d["export_rc"] = ex ? ex(p, nbytes, dev, &fd, &off) : -100;
        d["export_offset"] = off;
        std::string kind;
        if (fd >= 0) {
            char link[256] = {0};
            const std::string path = "/proc/self/fd/" + std::to_string(fd);
            const ssize_t n = readlink(path.c_str(), link, sizeof(link) - 1);
            if (n > 0) kind.assign(link, (size_t)n);
            close(fd);
        }
        d["fd_target"] = kind;
        // registration through the provider (ibv_reg_dmabuf_mr)
        FLAGS_rdma_verbs_library = verbs_library;
        std::string why;
        std::unique_ptr<rdma::Provider> pr = rdma::CreateIbverbsProvider(&why);
        d["provider"] = pr ? std::string(pr->name()) : "none: " + why;
        if (pr) {
            uint32_t lkey = 0;
            d["register_rc"] = pr->RegisterMemory(p, nbytes, true, dev, &lkey);
            d["lkey"] = lkey;
            pr->DeregisterMemory(p);
        }
        return d;
    }, py::arg("verbs_library"), py::arg("nbytes") = 1 << 20, py::arg("device") = 0);
    g.def("rccl_active", [] { return gpu::rccl::Active(); });
    g.def("rccl_abort_for_test", [](const std::string& why) { gpu::rccl::AbortForTest(why); });
    g.def("rccl_shutdown", [] {
        py::gil_scoped_release nogil;
        gpu::rccl::Shutdown();
    });
    g.def("rccl_stats", [] {
        const gpu::rccl::Stats s = gpu::rccl::GetStats();
        py::dict d;
        d["sent_payloads"] = s.sent_payloads;
        d["sent_bytes"] = s.sent_bytes;
        d["recv_payloads"] = s.recv_payloads;
        d["recv_bytes"] = s.recv_bytes;
        d["discarded"] = s.discarded;
        d["rounds"] = s.rounds;
        d["payload_rounds"] = s.payload_rounds;
        d["pair_rounds"] = s.pair_rounds;
        d["withdrawals"] = s.withdrawals;
        d["group_us"] = s.group_us;
        d["aborts"] = s.aborts;
        d["credit_stalls"] = s.credit_stalls;
        d["stash_expired"] = s.stash_expired;
        d["recv_timeouts"] = s.recv_timeouts;
        d["doorbells"] = s.doorbells;
        d["withdrawn"] = s.withdrawn;
        d["stash_payloads"] = s.stash_payloads;
        d["stash_bytes"] = s.stash_bytes;
        d["world"] = s.world;
        d["host_memory"] = s.host_memory;
        return d;
    });
    // packed_only (-gpu_snappy_packed_only): the device codec takes only
    // messages with large packed numeric fields; False forces every snappy
    // body of at least min_bytes onto the device (the A/B and the tests)
    g.def("enable_snappy", [](int dev, size_t min_bytes, bool packed_only) {
        std::string err;
        SetFlag("gpu_snappy_packed_only", packed_only ? "true" : "false");
        if (gpu::EnableGpuSnappy(dev, min_bytes, &err) != 0) throw std::runtime_error(err);
    }, py::arg("device") = 0, py::arg("min_bytes") = 32768, py::arg("packed_only") = true);
    g.def("disable_snappy", [] { gpu::DisableGpuSnappy(); });
    g.def("snappy_stats", [] {
        const gpu::GpuSnappyStats s = gpu::GetGpuSnappyStats();
        py::dict d;
        d["compress_calls"] = s.compress_calls;
        d["decompress_calls"] = s.decompress_calls;
        d["fallbacks"] = s.fallbacks;
        d["indexed_parses"] = s.indexed_parses;
        d["plain_routed"] = s.plain_routed;
        d["index_fallbacks"] = s.index_fallbacks;
        d["packs"] = s.packs;
        d["pack_runs"] = s.pack_runs;
        d["pack_run_chunks"] = s.pack_run_chunks;
        d["unpack_runs"] = s.unpack_runs;
        d["unpack_fallbacks"] = s.unpack_fallbacks;
        return d;
    });
    g.def("device_codec_stats", [] {
        const gpu::DeviceCodecStats s = gpu::GetDeviceCodecStats();
        py::dict d;
        d["encodes"] = s.encodes;
        d["encoded_bytes"] = s.encoded_bytes;
        d["encoded_out_bytes"] = s.encoded_out_bytes;
        d["decodes"] = s.decodes;
        d["decoded_bytes"] = s.decoded_bytes;
        d["bad_tables"] = s.bad_tables;
        d["decode_errors"] = s.decode_errors;
        d["scans"] = s.scans;
        d["packed_runs"] = s.packed_runs;
        d["packed_bytes"] = s.packed_bytes;
        d["packed_elems"] = s.packed_elems;
        d["packed_errors"] = s.packed_errors;
        d["built_messages"] = s.built_messages;
        d["built_row_jobs"] = s.built_row_jobs;
        d["built_rows"] = s.built_rows;
        d["built_row_bytes"] = s.built_row_bytes;
        d["split_row_jobs"] = s.split_row_jobs;
        d["split_rows"] = s.split_rows;
        d["split_record_jobs"] = s.split_record_jobs;
        d["split_records"] = s.split_records;
        d["built_record_jobs"] = s.built_record_jobs;
        d["built_records"] = s.built_records;
        d["built_record_bytes"] = s.built_record_bytes;
        d["built_fields"] = s.built_fields;
        d["built_bytes"] = s.built_bytes;
        d["build_errors"] = s.build_errors;
        return d;
    });
    g.def("codec_batch_stats", [] {
        const gpu::CodecBatchStats s = gpu::GetCodecBatchStats();
        py::dict d;
        d["requests"] = s.requests;
        d["launches"] = s.launches;
        d["run_chunks"] = s.run_chunks;
        d["decode_chunks"] = s.decode_chunks;
        d["fused_launches"] = s.fused_launches;
        d["msg_chunks"] = s.msg_chunks;
        d["timed"] = s.timed;
        d["queue_us"] = s.queue_us;
        d["api_us"] = s.api_us;
        d["gpu_us"] = s.gpu_us;
        d["wake_us"] = s.wake_us;
        return d;
    });
    // numeric run (vector layout bytes) -> varints / JSON numbers on the device (tests)
    g.def("pb_run_encode", [](py::bytes values, size_t n, uint32_t kind, uint32_t format, int dev) {
        std::string v = values;
        std::string out;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::EncodeRunOnDevice(v.data(), n, kind, format, &out, dev);
        }
        if (rc != 0) throw std::runtime_error("pb_run_encode failed");
        return py::bytes(out);
    }, py::arg("values"), py::arg("n"), py::arg("kind"), py::arg("format") = 0, py::arg("device") = 0);
    g.def("pb_run_decode", [](py::bytes payload, uint32_t kind, int dev) {
        std::string v = payload;
        std::string out;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::DecodeRunOnDevice(v.data(), v.size(), kind, &out, dev);
        }
        if (rc != 0) throw std::runtime_error("pb_run_decode failed (malformed run or device error)");
        return py::bytes(out);
    }, py::arg("payload"), py::arg("kind"), py::arg("device") = 0);
    g.def("enable_json_index", [](int dev, size_t min_bytes) {
        std::string err;
        if (gpu::EnableGpuJsonIndex(dev, min_bytes, &err) != 0) throw std::runtime_error(err);
    }, py::arg("device") = 0, py::arg("min_bytes") = 65536);
    g.def("disable_json_index", [] { gpu::DisableGpuJsonIndex(); });
    g.def("json_stats", [] {
        const gpu::GpuJsonStats s = gpu::GetGpuJsonStats();
        py::dict d;
        d["indexed_bodies"] = s.indexed_bodies;
        d["indexed_bytes"] = s.indexed_bytes;
        d["failures"] = s.failures;
        d["pb2json_arrays"] = s.pb2json_arrays;
        d["pb2json_elems"] = s.pb2json_elems;
        d["pb2json_failures"] = s.pb2json_failures;
        d["pb2json_float_arrays"] = s.pb2json_float_arrays;
        d["record_print_jobs"] = s.record_print_jobs;
        d["record_print_rows"] = s.record_print_rows;
        d["pb2json_float_elems"] = s.pb2json_float_elems;
        d["int_arrays"] = s.int_arrays;
        d["int_array_fallbacks"] = s.int_array_fallbacks;
        d["sparse_skips"] = s.sparse_skips;
        d["number_arrays"] = s.number_arrays;
        d["number_elems"] = s.number_elems;
        d["number_array_fallbacks"] = s.number_array_fallbacks;
        d["number_redo_elems"] = s.number_redo_elems;
        return d;
    });
    // json::ParseWithIndex over a structural index (the uint32 positions of
    // json_index_bytes as bytes) with whatever array offloads are installed;
    // the DOM is dropped: (ok, error)
    g.def("json_parse_with_index", [](py::bytes text, py::bytes index_u32) {
        // read in place: a copy of a 20 MB body would show in what this is used to time
        char *t = nullptr, *raw = nullptr;
        Py_ssize_t tn = 0, rawn = 0;
        if (PyBytes_AsStringAndSize(text.ptr(), &t, &tn) != 0 || PyBytes_AsStringAndSize(index_u32.ptr(), &raw, &rawn) != 0)
            throw py::error_already_set();
        if (((uintptr_t)raw & 3) != 0) throw std::invalid_argument("index must be 4-byte aligned");
        std::string err;
        bool ok;
        {
            py::gil_scoped_release nogil;
            json::Value v;
            ok = json::ParseWithIndex(t, (size_t)tn, reinterpret_cast<const uint32_t*>(raw), (size_t)rawn / 4, &v, &err);
        }
        return py::make_tuple(ok, err);
    });
    // host bytes -> structural positions through the device (tests)
    g.def("json_index_bytes", [](py::bytes b, int dev) {
        std::string data = b;
        std::vector<uint32_t> pos;
        int rc;
        {
            py::gil_scoped_release nogil;
            rc = gpu::JsonIndex(data.data(), data.size(), &pos, dev);
        }
        if (rc != 0) throw std::runtime_error("json index failed (device error or unterminated string)");
        return pos;
    }, py::arg("data"), py::arg("device") = 0);
    g.def("hbm_pool_stats", [](int dev) {
        const gpu::HbmPoolStats s = gpu::GetHbmPoolStats(dev);
        py::dict d;
        d["arena_bytes"] = s.arena_bytes;
        d["carved_bytes"] = s.carved_bytes;
        d["live_blocks"] = s.live_blocks;
        d["live_bytes"] = s.live_bytes;
        d["fallback_allocs"] = s.fallback_allocs;
        d["splits"] = s.splits;
        d["pinned_bytes"] = gpu::PinnedBytes();
        d["pinned_blocks_in_use"] = gpu::PinnedBlocksInUse();
        return d;
    }, py::arg("device") = 0);
    bind_gpu_ops(g);
}
