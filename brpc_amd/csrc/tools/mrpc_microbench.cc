// Runtime microbenchmarks against the reference's published primitive
// costs: fiber creation (<200 ns, docs/cn/memory_management.md:32),
// create -> run scheduling delay (median ~3 us, p90 <10 us, p99.99 <30 us,
// docs/cn/bthread_or_not.md:55), metric counter updates (~20 ns flat from 1
// to 24 threads, docs/cn/bvar.md:9), the IOBuf cut -> copy -> merge -> write
// pipeline (240 / 790 / 1520 MB/s for 12+16 / 12+128 / 12+1024 B,
// docs/en/iobuf.md:101-103) and a contended atomic fetch_add (~700 ns,
// docs/en/atomic_instructions.md:23). One JSON line per measurement.
//
//   build/bin/mrpc_microbench [--seconds S] [--threads 1,2,4,8,16] [--only pb]
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdarg>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "base/buf.h"
#include "base/flags.h"
#include "base/time.h"
#include "fiber/fiber.h"
#include "fiber/sync.h"
#include "mrpc/proto/echo.pb.h"
#include "mrpc/proto/rpc_meta.pb.h"
#include "var/reducer.h"

using namespace mrpc;

namespace {

double g_seconds = 1.0;
std::vector<int> g_threads = {1, 2, 4, 8, 16};

void emit(const std::string& json) {
    printf("%s\n", json.c_str());
    fflush(stdout);
}

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// ---------------------------------------------------------------- fibers
void* noop(void*) { return nullptr; }

// start + join of short fibers from a fiber (the runtime's common case: a
// handler spawning work), amortised over a batch started before joining
void bench_fiber_create() {
    struct Arg {
        double ns_start = 0, ns_total = 0;
        int64_t n = 0;
    } arg;
    fiber::CountdownEvent done(1);
    fiber::start([&] {
        const int kBatch = 256;
        std::vector<fiber::fiber_t> tids(kBatch);
        const int64_t end = monotonic_us() + (int64_t)(g_seconds * 1e6);
        int64_t start_ns = 0, total_ns = 0, n = 0;
        while (monotonic_us() < end) {
            const int64_t t0 = monotonic_ns();
            for (int i = 0; i < kBatch; ++i) fiber::start_background(&tids[i], nullptr, noop, nullptr);
            const int64_t t1 = monotonic_ns();
            for (int i = 0; i < kBatch; ++i) fiber::join(tids[i]);
            const int64_t t2 = monotonic_ns();
            start_ns += t1 - t0;
            total_ns += t2 - t0;
            n += kBatch;
        }
        arg.ns_start = (double)start_ns / n;
        arg.ns_total = (double)total_ns / n;
        arg.n = n;
        done.signal();
    });
    done.wait();
    emit(fmt("{\"bench\": \"fiber_create\", \"ns_per_start\": %.1f, \"ns_per_start_run_join\": %.1f, \"fibers\": %lld, "
             "\"reference\": \"bthread creation < 200 ns average\"}",
             arg.ns_start, arg.ns_total, (long long)arg.n));
}

// the same batch started with ATTR_NOSIGNAL and one flush(): creation
// without waking an idle worker per fiber
void bench_fiber_create_nosignal() {
    double ns_start = 0, ns_total = 0;
    int64_t total_n = 0;
    fiber::CountdownEvent done(1);
    fiber::start([&] {
        const int kBatch = 256;
        std::vector<fiber::fiber_t> tids(kBatch);
        fiber::Attr attr = fiber::ATTR_NORMAL;
        attr.flags |= fiber::ATTR_NOSIGNAL;
        const int64_t end = monotonic_us() + (int64_t)(g_seconds * 1e6);
        int64_t start_ns = 0, all_ns = 0, n = 0;
        while (monotonic_us() < end) {
            const int64_t t0 = monotonic_ns();
            for (int i = 0; i < kBatch; ++i) fiber::start_background(&tids[i], &attr, noop, nullptr);
            const int64_t t1 = monotonic_ns();
            fiber::flush();
            for (int i = 0; i < kBatch; ++i) fiber::join(tids[i]);
            const int64_t t2 = monotonic_ns();
            start_ns += t1 - t0;
            all_ns += t2 - t0;
            n += kBatch;
        }
        ns_start = (double)start_ns / n;
        ns_total = (double)all_ns / n;
        total_n = n;
        done.signal();
    });
    done.wait();
    emit(fmt("{\"bench\": \"fiber_create_nosignal\", \"ns_per_start\": %.1f, \"ns_per_start_run_join\": %.1f, "
             "\"fibers\": %lld}",
             ns_start, ns_total, (long long)total_n));
}

// create -> first instruction of the new fiber, measured by the fiber
struct DelayArg {
    int64_t created_ns;
    int64_t* out;
};
void* record_delay(void* p) {
    DelayArg* a = static_cast<DelayArg*>(p);
    *a->out = monotonic_ns() - a->created_ns;
    return nullptr;
}

void bench_sched_delay() {
    const int kN = 20000;
    std::vector<int64_t> delays(kN);
    std::vector<DelayArg> args(kN);
    fiber::CountdownEvent done(1);
    fiber::start([&] {
        for (int i = 0; i < kN; ++i) {
            args[i].out = &delays[i];
            args[i].created_ns = monotonic_ns();
            fiber::fiber_t t;
            fiber::start_background(&t, nullptr, record_delay, &args[i]);
            fiber::join(t);  // one at a time: a non-busy runtime, as the reference's figure
        }
        done.signal();
    });
    done.wait();
    std::sort(delays.begin(), delays.end());
    auto q = [&](double p) { return delays[std::min<size_t>(kN - 1, (size_t)(p * kN))] / 1000.0; };
    emit(fmt("{\"bench\": \"fiber_sched_delay\", \"median_us\": %.2f, \"p90_us\": %.2f, \"p99_us\": %.2f, "
             "\"p9999_us\": %.2f, \"samples\": %d, "
             "\"reference\": \"median ~3 us, p90 < 10 us, p99.99 < 30 us (non-busy machine)\"}",
             q(0.5), q(0.9), q(0.99), q(0.9999), kN));
}

// ---------------------------------------------------------------- metrics
void bench_adder() {
    for (int nt : g_threads) {
        var::Adder<int64_t> adder;
        std::atomic<bool> go{false}, stop{false};
        std::vector<int64_t> ops(nt, 0);
        std::vector<std::thread> ts;
        for (int t = 0; t < nt; ++t) {
            ts.emplace_back([&, t] {
                while (!go.load(std::memory_order_acquire)) {
                }
                int64_t n = 0;
                while (!stop.load(std::memory_order_relaxed)) {
                    for (int i = 0; i < 1000; ++i) adder << 1;
                    n += 1000;
                }
                ops[t] = n;
            });
        }
        const int64_t t0 = monotonic_ns();
        go.store(true, std::memory_order_release);
        usleep((useconds_t)(g_seconds * 1e6 / 2));
        stop.store(true);
        for (auto& t : ts) t.join();
        const int64_t dt = monotonic_ns() - t0;
        int64_t total = 0;
        for (int64_t o : ops) total += o;
        const bool ok = adder.get_value() == total;
        // per-thread cost: each thread ran for dt
        emit(fmt("{\"bench\": \"var_adder\", \"threads\": %d, \"ns_per_update_per_thread\": %.2f, \"consistent\": %s, "
                 "\"reference\": \"bvar counter ~20 ns, flat from 1 to 24 threads\"}",
                 nt, (double)dt * nt / (double)total, ok ? "true" : "false"));
    }
}

void bench_contended_atomic() {
    for (int nt : g_threads) {
        if (nt < 2) continue;
        std::atomic<int64_t> counter{0};
        std::atomic<bool> go{false}, stop{false};
        std::vector<int64_t> ops(nt, 0);
        std::vector<std::thread> ts;
        for (int t = 0; t < nt; ++t) {
            ts.emplace_back([&, t] {
                while (!go.load(std::memory_order_acquire)) {
                }
                int64_t n = 0;
                while (!stop.load(std::memory_order_relaxed)) {
                    counter.fetch_add(1, std::memory_order_relaxed);
                    ++n;
                }
                ops[t] = n;
            });
        }
        const int64_t t0 = monotonic_ns();
        go.store(true, std::memory_order_release);
        usleep((useconds_t)(g_seconds * 1e6 / 4));
        stop.store(true);
        for (auto& t : ts) t.join();
        const int64_t dt = monotonic_ns() - t0;
        int64_t total = 0;
        for (int64_t o : ops) total += o;
        emit(fmt("{\"bench\": \"contended_fetch_add\", \"threads\": %d, \"ns_per_op_per_thread\": %.1f, "
                 "\"reference\": \"~700 ns on E5-2620\"}",
                 nt, (double)dt * nt / (double)total));
    }
}

// ---------------------------------------------------------------- Buf
// The reference's pipeline (docs/en/iobuf.md:101-103): a 12-byte header
// plus a body are cut from a source buffer, copied into a new buffer,
// merged into an output buffer, and the output is written to a pipe (read
// back by a drain thread).
void bench_buf_pipeline() {
    for (size_t body : {16u, 128u, 1024u}) {
        const size_t msg = 12 + body;
        int fds[2];
        if (pipe(fds) != 0) return;
        fcntl(fds[1], F_SETPIPE_SZ, 1 << 20);
        std::atomic<bool> stop{false};
        std::thread drain([&] {
            std::vector<char> b(1 << 20);
            while (!stop.load(std::memory_order_relaxed)) {
                if (read(fds[0], b.data(), b.size()) <= 0) break;
            }
        });
        std::string payload(msg * 1024, 'x');
        Buf src;
        int64_t ops = 0, bytes = 0;
        const int64_t t0 = monotonic_ns(), end = t0 + (int64_t)(g_seconds * 1e9);
        while (monotonic_ns() < end) {
            if (src.size() < msg) src.append(payload);
            Buf out;
            for (int i = 0; i < 64 && src.size() >= msg; ++i) {
                Buf head, piece;
                src.cutn(&head, 12);
                src.cutn(&piece, body);
                Buf copy(piece);
                head.append(std::move(copy));
                out.append(std::move(head));
                ++ops;
                bytes += (int64_t)msg;
            }
            while (!out.empty()) {
                if (out.cut_into_fd(fds[1]) < 0) break;
            }
        }
        const double dt = (double)(monotonic_ns() - t0) / 1e9;
        stop.store(true);
        close(fds[1]);
        drain.join();
        close(fds[0]);
        emit(fmt("{\"bench\": \"buf_pipeline\", \"message\": \"12+%zu B\", \"MB_per_s\": %.0f, \"Mops_per_s\": %.2f, "
                 "\"reference\": \"%s\"}",
                 body, bytes / dt / 1e6, ops / dt / 1e6,
                 body == 16 ? "240 MB/s (8.59 M ops/s)" : body == 128 ? "790 MB/s (5.64 M ops/s)" : "1520 MB/s (1.47 M ops/s)"));
    }
}

// ---------------------------------------------------------------- timers
std::atomic<int64_t> g_fired{0};
void on_timer(void*) { g_fired.fetch_add(1, std::memory_order_relaxed); }

void bench_timer() {
    // schedule + unschedule of timers far in the future (the RPC timeout
    // pattern: most timers are cancelled before they fire)
    const int kN = 200000;
    std::vector<fiber::TimerId> ids(kN);
    const int64_t t0 = monotonic_ns();
    for (int i = 0; i < kN; ++i) fiber::timer_add_us(&ids[i], 10 * 1000 * 1000, on_timer, nullptr);
    const int64_t t1 = monotonic_ns();
    for (int i = 0; i < kN; ++i) fiber::timer_del(ids[i]);
    const int64_t t2 = monotonic_ns();
    emit(fmt("{\"bench\": \"timer_schedule_cancel\", \"ns_per_add\": %.1f, \"ns_per_del\": %.1f, \"fired\": %lld}",
             (double)(t1 - t0) / kN, (double)(t2 - t1) / kN, (long long)g_fired.load()));
}

// ---------------------------------------------------------------- pb codec
// The four messages every 32 B baidu_std echo encodes and decodes, filled
// as that path fills them, and one wide case (16384 packed ids): ns per
// serialize (IsInitialized + SerializeToBuf), per ParseFromArray, and per
// Clear of a parsed message. `--only pb` runs this section alone.
template <typename F>
double ns_per_op(F&& op) {
    for (int i = 0; i < 200; ++i) op();
    int64_t n = 0;
    const int64_t t0 = monotonic_ns(), end = t0 + (int64_t)(g_seconds * 1e9 / 4);
    int64_t t1 = t0;
    while (t1 < end) {
        for (int i = 0; i < 64; ++i) op();
        n += 64;
        t1 = monotonic_ns();
    }
    return (double)(t1 - t0) / (double)n;
}

void bench_pb_message(const char* name, const pb::Message& filled) {
    const std::string wire = filled.SerializeAsString();
    bool ok = true;
    const double ser = ns_per_op([&] {
        Buf out;
        ok &= filled.IsInitialized() && filled.SerializeToBuf(&out);
    });
    std::unique_ptr<pb::Message> m(filled.New());
    const double parse = ns_per_op([&] { ok &= m->ParseFromArray(wire.data(), wire.size()); });
    // Clear: a batch of parsed messages, only the Clear calls inside the clock
    const int kBatch = wire.size() > 4096 ? 8 : 256;
    std::vector<std::unique_ptr<pb::Message>> batch;
    for (int i = 0; i < kBatch; ++i) batch.emplace_back(filled.New());
    int64_t clear_ns = 0, cleared = 0;
    const int64_t end = monotonic_ns() + (int64_t)(g_seconds * 1e9 / 4);
    while (monotonic_ns() < end) {
        for (auto& b : batch) ok &= b->ParseFromArray(wire.data(), wire.size());
        const int64_t t0 = monotonic_ns();
        for (auto& b : batch) b->Clear();
        clear_ns += monotonic_ns() - t0;
        cleared += kBatch;
    }
    emit(fmt("{\"bench\": \"pb\", \"message\": \"%s\", \"wire_bytes\": %zu, \"serialize_ns\": %.1f, \"parse_ns\": %.1f, "
             "\"clear_ns\": %.1f, \"ok\": %s}",
             name, wire.size(), ser, parse, (double)clear_ns / (double)cleared, ok ? "true" : "false"));
}

void bench_pb() {
    policy::RpcMeta req_meta;
    req_meta.mutable_request()->set_service_name("example.EchoService");
    req_meta.mutable_request()->set_method_name("Echo");
    req_meta.set_compress_type(0);
    req_meta.set_correlation_id(0x100000001ll * 77);
    bench_pb_message("RpcMeta_request", req_meta);
    policy::RpcMeta res_meta;
    res_meta.set_compress_type(0);
    res_meta.set_correlation_id(0x100000001ll * 77);
    bench_pb_message("RpcMeta_response", res_meta);
    example::EchoRequest req;
    req.set_message(std::string(32, 'x'));
    bench_pb_message("EchoRequest_32B", req);
    example::EchoResponse res;
    res.set_message(std::string(32, 'x'));
    bench_pb_message("EchoResponse_32B", res);
    example::EchoRequest wide;
    wide.set_message("ids");
    for (int i = 0; i < 16384; ++i) wide.add_ids((int64_t)i * 2654435761ll >> (i % 40));
    bench_pb_message("EchoRequest_ids16k", wide);
}

}  // namespace

int main(int argc, char** argv) {
    std::string only;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--seconds") && i + 1 < argc) {
            g_seconds = atof(argv[++i]);
        } else if (!strcmp(argv[i], "--threads") && i + 1 < argc) {
            g_threads.clear();
            std::string s = argv[++i];
            size_t b = 0;
            while (b < s.size()) {
                size_t e = s.find(',', b);
                if (e == std::string::npos) e = s.size();
                g_threads.push_back(atoi(s.substr(b, e - b).c_str()));
                b = e + 1;
            }
        } else if (!strcmp(argv[i], "--flag") && i + 1 < argc) {
            const std::string kv = argv[++i];
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !SetFlag(kv.substr(0, eq), kv.substr(eq + 1))) {
                fprintf(stderr, "bad --flag %s\n", kv.c_str());
                return 2;
            }
        } else if (!strcmp(argv[i], "--only") && i + 1 < argc) {
            only = argv[++i];
        } else {
            fprintf(stderr, "usage: %s [--seconds S] [--threads 1,2,4] [--only pb] [--flag name=value]...\n", argv[0]);
            return 2;
        }
    }
    if (only == "pb") {
        bench_pb();
        return 0;
    }
    if (!only.empty()) {
        fprintf(stderr, "unknown section %s\n", only.c_str());
        return 2;
    }
    fiber::init_runtime();
    bench_fiber_create();
    bench_fiber_create_nosignal();
    bench_sched_delay();
    bench_adder();
    bench_contended_atomic();
    bench_buf_pipeline();
    bench_timer();
    bench_pb();
    return 0;
}
