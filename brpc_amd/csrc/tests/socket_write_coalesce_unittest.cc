// The writer's linger (net/socket.cc KeepWriteLoop, -socket_write_linger): a
// KeepWrite fiber that drained the queue yields once before it gives up the
// writer role, so that what the other runnable fibers write goes out in one
// call. Checked here: a lone caller never pays for it, a held writer batches,
// no request is lost in the window between the yield and IsWriteComplete,
// failure and half-close behave as without it. Each case runs with the flag
// at 1 and at 0. All over AF_UNIX socketpairs.
#include <fcntl.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "base/flags.h"
#include "base/time.h"
#include "fiber/butex.h"
#include "fiber/call_id.h"
#include "fiber/fiber.h"
#include "net/socket.h"
#include "rpc/errno.h"
#include "tests/test.h"
#include "var/var.h"

DECLARE_int32(socket_write_linger);

using namespace mrpc;

namespace {

int64_t var_value(const char* name) { return atoll(var::Variable::describe_exposed(name).c_str()); }

struct LingerFlag {
    int32_t saved;
    explicit LingerFlag(int32_t v) : saved(FLAGS_socket_write_linger) { FLAGS_socket_write_linger = v; }
    ~LingerFlag() { FLAGS_socket_write_linger = saved; }
};

// Frames: [0] total length (8..64), [1] writer, [2] 1 = last of its burst,
// [3] 0, [4..8) sequence number, then filler.
const size_t kMaxFrame = 64;

std::string make_frame(size_t len, int writer, bool last, uint32_t seq) {
    std::string f(len, (char)('a' + writer % 26));
    f[0] = (char)len;
    f[1] = (char)writer;
    f[2] = last ? 1 : 0;
    f[3] = 0;
    memcpy(&f[4], &seq, 4);
    return f;
}

uint32_t frame_seq(const uint8_t* f) {
    uint32_t s;
    memcpy(&s, f + 4, 4);
    return s;
}

int write_str(SocketId id, const std::string& s, const WriteOptions* wo = nullptr) {
    SocketUniquePtr p;
    if (Socket::Address(id, &p) != 0) return -1;
    Buf b(s);
    return p->Write(&b, wo);
}

// The `user` of a socket whose input is cut into frames by OnFrames.
struct FrameSink {
    virtual ~FrameSink() {}
    virtual void OnFrame(Socket* s, const uint8_t* f, size_t n) = 0;
    std::atomic<int> bad_frames{0};
};

void OnFrames(Socket* m) {
    FrameSink* sink = static_cast<FrameSink*>(m->user());
    int progress = Socket::PROGRESS_INIT;
    for (;;) {
        const ssize_t nr = m->DoRead(8192);
        if (nr == 0) break;
        if (nr < 0) {
            if (errno == EINTR) continue;
            if (errno != EAGAIN && errno != EWOULDBLOCK) break;
            if (!m->MoreReadEvents(&progress)) break;
            continue;
        }
        for (;;) {
            uint8_t len = 0;
            if (m->_read_buf.copy_to(&len, 1) < 1) break;
            if (len < 8 || len > kMaxFrame) {
                sink->bad_frames.fetch_add(1);
                m->_read_buf.clear();
                break;
            }
            if (m->_read_buf.size() < len) break;
            uint8_t f[kMaxFrame];
            m->_read_buf.cutn(f, len);
            sink->OnFrame(m, f, len);
        }
    }
}

// Two Sockets joined by a socketpair, each feeding a FrameSink.
struct SocketPair {
    SocketId a = INVALID_SOCKET_ID, b = INVALID_SOCKET_ID;
    SocketUniquePtr pa, pb;
    SocketPair(FrameSink* sink_a, FrameSink* sink_b) {
        int fds[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) return;
        SocketOptions o;
        o.on_edge_triggered_events = OnFrames;
        o.fd = fds[0];
        o.user = sink_a;
        Socket::Create(o, &a);
        o.fd = fds[1];
        o.user = sink_b;
        Socket::Create(o, &b);
        Socket::Address(a, &pa);
        Socket::Address(b, &pb);
    }
    // Fails both ends and waits until no event or writer fiber holds them, so
    // that the sinks may go away.
    ~SocketPair() {
        Socket::SetFailed(a);
        Socket::SetFailed(b);
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
        while (monotonic_us() < deadline && ((pa && pa->nref() > 1) || (pb && pb->nref() > 1))) usleep(1000);
    }
};

// One Socket whose far end is a plain fd that the test reads itself.
struct HalfPair {
    int peer = -1;
    SocketId id = INVALID_SOCKET_ID;
    SocketUniquePtr ptr;
    explicit HalfPair(int sndbuf = 0) {
        int fds[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) return;
        if (sndbuf > 0) setsockopt(fds[0], SOL_SOCKET, SO_SNDBUF, &sndbuf, sizeof(sndbuf));
        peer = fds[1];
        SocketOptions o;
        o.fd = fds[0];
        Socket::Create(o, &id);
        Socket::Address(id, &ptr);
    }
    // Fails the socket and waits until its writer fiber has let go of it (the
    // fiber reads the flag that the test restores next).
    ~HalfPair() {
        Socket::SetFailed(id);
        if (peer >= 0) close(peer);
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
        while (monotonic_us() < deadline && ptr && ptr->nref() > 1) usleep(1000);
    }
    // Reads n bytes (fewer on EOF or after timeout_ms).
    std::string read_n(size_t n, int timeout_ms = 5000 * mtest::kSlowdown) {
        std::string out(n, '\0');
        size_t got = 0;
        const int64_t deadline = monotonic_us() + (int64_t)timeout_ms * 1000;
        while (got < n && monotonic_us() < deadline) {
            pollfd p{peer, POLLIN, 0};
            if (poll(&p, 1, 50) <= 0) continue;
            const ssize_t r = read(peer, &out[got], n - got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        out.resize(got);
        return out;
    }
};

bool wait_until(const std::function<bool()>& cond, int64_t timeout_ms = 5000) {
    const int64_t deadline = monotonic_us() + timeout_ms * 1000 * mtest::kSlowdown;
    while (!cond()) {
        if (monotonic_us() > deadline) return false;
        usleep(500);
    }
    return true;
}

std::string pattern(size_t n, int seed) {
    std::string s(n, '\0');
    for (size_t i = 0; i < n; ++i) s[i] = (char)((i * 131 + seed * 7 + (i >> 10)) & 0xff);
    return s;
}

// ---------------------------------------------------------------- ping-pong

struct EchoSink : FrameSink {
    void OnFrame(Socket* s, const uint8_t* f, size_t n) override {
        Buf b;
        b.append(f, n);
        s->Write(&b);
    }
};

struct CountSink : FrameSink {
    std::atomic<int>* echoes = fiber::butex_create();
    CountSink() { echoes->store(0); }
    ~CountSink() override { fiber::butex_destroy(echoes); }
    void OnFrame(Socket*, const uint8_t*, size_t) override {
        echoes->fetch_add(1, std::memory_order_release);
        fiber::butex_wake_all(echoes);
    }
};

void ping_pong_never_lingers(int linger) {
    LingerFlag flag(linger);
    const int kRounds = 1000;
    CountSink client;
    EchoSink server;
    SocketPair p(&client, &server);
    ASSERT_TRUE(p.pa && p.pb);
    const int64_t calls0 = p.pa->write_calls.load(), lingers0 = var_value("socket_write_lingers");
    struct Arg {
        SocketId id;
        CountSink* sink;
        int sent = 0;
    } arg{p.a, &client};
    fiber::fiber_t th;
    ASSERT_EQ(fiber::start_background(&th, nullptr,
                                      [](void* x) -> void* {
                                          Arg* a = static_cast<Arg*>(x);
                                          const int64_t deadline = monotonic_us() + 10000000LL * mtest::kSlowdown;
                                          for (int i = 0; i < kRounds; ++i) {
                                              if (write_str(a->id, make_frame(32, 0, true, (uint32_t)i)) != 0) break;
                                              ++a->sent;
                                              int seen;
                                              while ((seen = a->sink->echoes->load(std::memory_order_acquire)) <= i) {
                                                  if (monotonic_us() > deadline) return nullptr;
                                                  timespec ts = realtime_after_us(100000);
                                                  fiber::butex_wait(a->sink->echoes, seen, &ts);
                                              }
                                          }
                                          return nullptr;
                                      },
                                      &arg),
              0);
    fiber::join(th, nullptr);
    EXPECT_EQ(arg.sent, kRounds);
    EXPECT_EQ(client.echoes->load(), kRounds);
    // one call per message on either side, and no writer fiber to linger
    EXPECT_EQ(p.pa->write_calls.load() - calls0, (int64_t)kRounds);
    EXPECT_EQ(p.pb->write_calls.load(), (int64_t)kRounds);
    EXPECT_EQ(var_value("socket_write_lingers") - lingers0, 0);
    EXPECT_EQ(client.bad_frames.load() + server.bad_frames.load(), 0);
}

// ---------------------------------------------------------------- held writer

// Per-writer order of the frames in `bytes`; the number of frames, -1 on a
// frame out of order or malformed.
int check_frames(const std::string& bytes, int nwriters) {
    std::vector<uint32_t> next(nwriters, 0);
    size_t off = 0;
    int n = 0;
    while (off < bytes.size()) {
        const uint8_t* f = (const uint8_t*)bytes.data() + off;
        if (f[0] < 8 || f[0] > kMaxFrame || off + f[0] > bytes.size() || f[1] >= nwriters) return -1;
        if (frame_seq(f) != next[f[1]]++) return -1;
        if (f[f[0] - 1] != (uint8_t)('a' + f[1] % 26)) return -1;
        off += f[0];
        ++n;
    }
    return n;
}

void held_writer_batches(int linger) {
    LingerFlag flag(linger);
    // SO_SNDBUF 4096 becomes 8192 in the kernel, and an AF_UNIX stream socket
    // then takes a write in pieces of 8192/2 - 64 = 4032 bytes until 8192 are
    // unread: every call that is not refused moves at least 4032 bytes, so
    // the 32 KiB write takes at most 9 calls that make progress. That leaves
    // room under both bounds below at any scheduling.
    HalfPair p(4096);
    ASSERT_TRUE((bool)p.ptr);
    const int kWriters = 8, kEach = 8;  // 64 small writes
    const std::string big = pattern(32768, 5);
    ASSERT_EQ(write_str(p.id, big), 0);
    // the KeepWrite fiber is parked on EPOLLOUT once a write was refused
    ASSERT_TRUE(wait_until([&] { return p.ptr->write_eagains.load() >= 1; }));
    const int64_t calls0 = p.ptr->write_calls.load();
    struct Arg {
        SocketId id;
        int idx;
    };
    std::vector<Arg> args(kWriters);
    std::vector<fiber::fiber_t> ts(kWriters);
    size_t small_bytes = 0;
    for (int i = 0; i < kWriters; ++i) {
        for (int m = 0; m < kEach; ++m) small_bytes += 24 + (size_t)((i * kEach + m) % 41);
        args[i] = Arg{p.id, i};
        ASSERT_EQ(fiber::start_background(&ts[i], nullptr,
                                          [](void* x) -> void* {
                                              Arg* a = static_cast<Arg*>(x);
                                              for (int m = 0; m < kEach; ++m) {
                                                  const size_t len = 24 + (size_t)((a->idx * kEach + m) % 41);
                                                  write_str(a->id, make_frame(len, a->idx, false, (uint32_t)m));
                                              }
                                              return nullptr;
                                          },
                                          &args[i]),
                  0);
    }
    for (auto t : ts) fiber::join(t, nullptr);
    EXPECT_EQ(p.ptr->out_messages.load(), (int64_t)(1 + kWriters * kEach));
    // now the peer drains
    const std::string got = p.read_n(big.size() + small_bytes);
    ASSERT_EQ(got.size(), big.size() + small_bytes);
    EXPECT_TRUE(got.compare(0, big.size(), big) == 0);
    EXPECT_EQ(check_frames(got.substr(big.size()), kWriters), kWriters * kEach);
    EXPECT_TRUE(wait_until([&] { return p.ptr->unwritten_bytes() == 0; }));
    const int64_t calls = p.ptr->write_calls.load(), eagains = p.ptr->write_eagains.load();
    fprintf(stderr, "  held writer, linger=%d: %ld calls (%ld refused) for %ld messages, %ld calls after the small writes\n",
            linger, (long)calls, (long)eagains, (long)p.ptr->out_messages.load(), (long)(calls - calls0));
    EXPECT_LT(calls - calls0, (int64_t)(kWriters * kEach));
    EXPECT_LE(calls, p.ptr->out_messages.load() + eagains);
}

// ---------------------------------------------------------------- hand-over

const int kHandoverWriters = 16;

// Server end: checks the per-writer order and acknowledges each burst.
struct BurstServerSink : FrameSink {
    uint32_t next[kHandoverWriters] = {0};  // one reader fiber at a time
    std::atomic<int64_t> received{0}, out_of_order{0};
    void OnFrame(Socket* s, const uint8_t* f, size_t n) override {
        const int w = f[1];
        if (w >= kHandoverWriters || frame_seq(f) != next[w] || f[n - 1] != (uint8_t)('a' + w % 26)) {
            out_of_order.fetch_add(1);
            return;
        }
        ++next[w];
        received.fetch_add(1, std::memory_order_relaxed);
        if (f[2]) {
            Buf b;
            b.append(make_frame(8, w, true, frame_seq(f)));
            s->Write(&b);
        }
    }
};

// Client end: an acknowledgement carries the sequence number of the burst's
// last frame; publish "next sequence number" to the writer.
struct AckSink : FrameSink {
    std::atomic<int>* acked[kHandoverWriters];
    AckSink() {
        for (auto& b : acked) {
            b = fiber::butex_create();
            b->store(0);
        }
    }
    ~AckSink() override {
        for (auto& b : acked) fiber::butex_destroy(b);
    }
    void OnFrame(Socket*, const uint8_t* f, size_t) override {
        const int w = f[1];
        if (w >= kHandoverWriters) {
            bad_frames.fetch_add(1);
            return;
        }
        acked[w]->store((int)frame_seq(f) + 1, std::memory_order_release);
        fiber::butex_wake_all(acked[w]);
    }
};

void no_lost_handover(int linger) {
    LingerFlag flag(linger);
    const int kRounds = 2000;
    AckSink client;
    BurstServerSink server;
    SocketPair p(&client, &server);
    ASSERT_TRUE(p.pa && p.pb);
    const int64_t lingers0 = var_value("socket_write_lingers"), hits0 = var_value("socket_write_linger_hits");
    const int64_t t0 = monotonic_us();
    struct Arg {
        SocketId id;
        AckSink* sink;
        int idx;
        int64_t deadline;
        int64_t sent = 0;
        int rounds = 0;
    };
    std::vector<Arg> args(kHandoverWriters);
    std::vector<fiber::fiber_t> ts(kHandoverWriters);
    for (int i = 0; i < kHandoverWriters; ++i) {
        args[i].id = p.a;
        args[i].sink = &client;
        args[i].idx = i;
        args[i].deadline = t0 + 10000000LL * mtest::kSlowdown;
        ASSERT_EQ(fiber::start_background(&ts[i], nullptr,
                                          [](void* x) -> void* {
                                              Arg* a = static_cast<Arg*>(x);
                                              uint32_t rnd = 12345u + 977u * (uint32_t)a->idx, seq = 0;
                                              for (int r = 0; r < kRounds; ++r) {
                                                  rnd = rnd * 1664525u + 1013904223u;
                                                  const int burst = 1 + (int)((rnd >> 16) % 3);
                                                  for (int k = 0; k < burst; ++k) {
                                                      rnd = rnd * 1664525u + 1013904223u;
                                                      const size_t len = 24 + (rnd >> 16) % 41;
                                                      if (write_str(a->id, make_frame(len, a->idx, k + 1 == burst, seq)) != 0) {
                                                          return nullptr;
                                                      }
                                                      ++seq;
                                                      ++a->sent;
                                                  }
                                                  std::atomic<int>* b = a->sink->acked[a->idx];
                                                  int seen;
                                                  while ((seen = b->load(std::memory_order_acquire)) != (int)seq) {
                                                      if (monotonic_us() > a->deadline) return nullptr;
                                                      timespec ts = realtime_after_us(100000);
                                                      fiber::butex_wait(b, seen, &ts);
                                                  }
                                                  ++a->rounds;
                                              }
                                              return nullptr;
                                          },
                                          &args[i]),
                  0);
    }
    for (auto t : ts) fiber::join(t, nullptr);
    const int64_t took_us = monotonic_us() - t0;
    int64_t sent = 0;
    for (auto& a : args) {
        EXPECT_EQ(a.rounds, kRounds);
        sent += a.sent;
    }
    EXPECT_LT(took_us, 10000000LL * mtest::kSlowdown);
    EXPECT_EQ(server.received.load(), sent);  // with the order check: each exactly once
    EXPECT_EQ(server.out_of_order.load(), 0);
    EXPECT_EQ(client.bad_frames.load() + server.bad_frames.load(), 0);
    const int64_t lingers = var_value("socket_write_lingers") - lingers0;
    fprintf(stderr, "  hand-over, linger=%d: %ld frames in %ld ms, %ld+%ld write calls, %ld lingers, %ld hits\n", linger,
            (long)sent, (long)(took_us / 1000), (long)p.pa->write_calls.load(), (long)p.pb->write_calls.load(),
            (long)lingers, (long)(var_value("socket_write_linger_hits") - hits0));
    if (linger > 0) {
        EXPECT_GT(lingers, 0);
    } else {
        EXPECT_EQ(lingers, 0);
    }
}

// ---------------------------------------------------------------- failure

struct IdOutcome {
    std::atomic<int> errors{0};
};

int on_id_error(fiber::CallId id, void* data, int, const std::string&) {
    static_cast<IdOutcome*>(data)->errors.fetch_add(1);
    return fiber::call_id_unlock_and_destroy(id);
}

void failure_while_lingering(int linger) {
    LingerFlag flag(linger);
    const int kWriters = 32, kWindow = 4;
    const int64_t nsocket0 = Socket::nsocket();
    IdOutcome outcome;
    std::atomic<int> written{0}, succeeded{0}, created{0};
    std::atomic<bool> stop_reading{false};
    struct Arg {
        Socket* s;  // the test's own reference outlives the writers: Write() itself must refuse
        int idx;
        IdOutcome* outcome;
        std::atomic<int>*written, *succeeded, *created;
        int64_t deadline;
        bool refused = false;             // ended by a write that the failed socket refused
        std::vector<fiber::CallId> open;  // ids not yet completed by this writer
    };
    std::vector<Arg> args(kWriters);
    std::vector<fiber::fiber_t> ts(kWriters);
    SocketId sid;
    {
        HalfPair p;
        ASSERT_TRUE((bool)p.ptr);
        sid = p.id;
        std::thread reader([&] {
            char buf[65536];
            while (!stop_reading.load()) {
                pollfd pf{p.peer, POLLIN, 0};
                if (poll(&pf, 1, 20) <= 0) continue;
                if (read(p.peer, buf, sizeof(buf)) <= 0) break;
            }
        });
        for (int i = 0; i < kWriters; ++i) {
            args[i] = Arg{p.ptr.get(), i, &outcome, &written, &succeeded, &created, monotonic_us() + 10000000LL * mtest::kSlowdown,
                          false, {}};
            fiber::start_background(&ts[i], nullptr,
                                    [](void* x) -> void* {
                                        Arg* a = static_cast<Arg*>(x);
                                        // until the socket fails under us
                                        for (int m = 0; monotonic_us() < a->deadline; ++m) {
                                            fiber::CallId cid;
                                            if (fiber::call_id_create(&cid, a->outcome, on_id_error) != 0) break;
                                            a->created->fetch_add(1);
                                            a->open.push_back(cid);
                                            WriteOptions wo;
                                            wo.id_wait = cid;
                                            Buf b(make_frame(40, a->idx, false, (uint32_t)m));
                                            if (a->s->Write(&b, &wo) != 0) {
                                                a->refused = true;
                                                break;
                                            }
                                            a->written->fetch_add(1);
                                            // the "response" to an earlier write arrives: complete its id,
                                            // unless an error has done so
                                            if (a->open.size() > (size_t)kWindow) {
                                                const fiber::CallId old = a->open.front();
                                                a->open.erase(a->open.begin());
                                                if (fiber::call_id_lock(old, nullptr) == 0) {
                                                    fiber::call_id_unlock_and_destroy(old);
                                                    a->succeeded->fetch_add(1);
                                                }
                                            }
                                            if (m % 8 == 7) fiber::yield();
                                        }
                                        return nullptr;
                                    },
                                    &args[i]);
        }
        // part-way through: the writers are mid-stream, some KeepWrite fiber may be lingering
        EXPECT_TRUE(wait_until([&] { return written.load() >= 4000; }));
        p.ptr->SetFailed(ECLOSE, "failed by test");
        for (auto t : ts) fiber::join(t, nullptr);
        for (auto& a : args) EXPECT_TRUE(a.refused);  // the failure landed while each was writing
        // every id still open is completed by the error, none is left
        for (auto& a : args) {
            for (fiber::CallId cid : a.open) {
                EXPECT_TRUE(wait_until([&] { return !fiber::call_id_exists(cid); }));
            }
        }
        EXPECT_EQ(succeeded.load() + outcome.errors.load(), created.load());
        EXPECT_TRUE(wait_until([&] { return p.ptr->unwritten_bytes() == 0; }));
        EXPECT_EQ(p.ptr->unwritten_bytes(), 0);
        stop_reading.store(true);
        reader.join();
    }
    // all references dropped: the id is dead and the slot recycled
    SocketUniquePtr again;
    EXPECT_NE(Socket::Address(sid, &again), 0);
    EXPECT_TRUE(wait_until([&] { return Socket::nsocket() == nsocket0; }));
    fprintf(stderr, "  failure, linger=%d: %d ids, %d completed by the writer, %d by an error\n", linger, created.load(),
            succeeded.load(), outcome.errors.load());
}

// ---------------------------------------------------------------- half-close

void shutdown_write_after_is_not_delayed(int linger) {
    LingerFlag flag(linger);
    HalfPair p(4096);
    ASSERT_TRUE((bool)p.ptr);
    const std::string big = pattern(32768, 11);
    ASSERT_EQ(write_str(p.id, big), 0);
    ASSERT_TRUE(wait_until([&] { return p.ptr->write_eagains.load() >= 1; }));
    // queued behind the parked KeepWrite fiber: it is that fiber which writes
    // the last request and half-closes
    const int64_t lingers0 = var_value("socket_write_lingers");
    WriteOptions wo;
    wo.shutdown_write_after = true;
    ASSERT_EQ(write_str(p.id, "bye", &wo), 0);
    const std::string got = p.read_n(big.size() + 3);
    ASSERT_EQ(got.size(), big.size() + 3);
    EXPECT_TRUE(got.compare(0, big.size(), big) == 0);
    EXPECT_EQ(got.substr(big.size()), "bye");
    char c;
    pollfd pf{p.peer, POLLIN, 0};
    ASSERT_GT(poll(&pf, 1, 2000 * mtest::kSlowdown), 0);
    EXPECT_EQ(read(p.peer, &c, 1), 0);  // EOF
    EXPECT_EQ(var_value("socket_write_lingers") - lingers0, 0);
}

}  // namespace

TEST(SocketWriteCoalesce, counters_are_exposed) {
    HalfPair p;
    ASSERT_TRUE((bool)p.ptr);
    const int64_t w0 = var_value("socket_write_calls"), m0 = var_value("socket_out_messages");
    ASSERT_EQ(write_str(p.id, "abc"), 0);
    EXPECT_EQ(p.read_n(3), "abc");
    EXPECT_EQ(p.ptr->write_calls.load(), 1);
    EXPECT_EQ(p.ptr->out_messages.load(), 1);
    EXPECT_EQ(var_value("socket_write_calls") - w0, 1);
    EXPECT_EQ(var_value("socket_out_messages") - m0, 1);
    for (const char* name : {"socket_read_calls", "socket_in_messages", "socket_write_lingers", "socket_write_linger_hits"}) {
        EXPECT_FALSE_M(var::Variable::describe_exposed(name).empty(), name);
    }
    // reloadable, and negative values are refused
    EXPECT_TRUE(SetFlag("socket_write_linger", "2", true));
    EXPECT_EQ(FLAGS_socket_write_linger, 2);
    EXPECT_FALSE(SetFlag("socket_write_linger", "-1", true));
    EXPECT_TRUE(SetFlag("socket_write_linger", "1", true));
}

TEST(SocketWriteCoalesce, read_calls_and_in_messages_count) {
    CountSink client;
    EchoSink server;
    SocketPair p(&client, &server);
    ASSERT_TRUE(p.pa && p.pb);
    const int64_t r0 = var_value("socket_read_calls");
    ASSERT_EQ(write_str(p.a, make_frame(32, 0, true, 0)), 0);
    ASSERT_TRUE(wait_until([&] { return client.echoes->load() == 1; }));
    // each side read the frame and then ran into EAGAIN at least once
    EXPECT_GE(p.pa->read_calls.load(), 1);
    EXPECT_GE(p.pb->read_calls.load(), 1);
    EXPECT_GE(var_value("socket_read_calls") - r0, p.pa->read_calls.load() + p.pb->read_calls.load());
}

TEST(SocketWriteCoalesce, ping_pong_never_lingers_linger1) { ping_pong_never_lingers(1); }
TEST(SocketWriteCoalesce, ping_pong_never_lingers_linger0) { ping_pong_never_lingers(0); }
TEST(SocketWriteCoalesce, held_writer_batches_linger1) { held_writer_batches(1); }
TEST(SocketWriteCoalesce, held_writer_batches_linger0) { held_writer_batches(0); }
TEST(SocketWriteCoalesce, no_lost_handover_linger1) { no_lost_handover(1); }
TEST(SocketWriteCoalesce, no_lost_handover_linger0) { no_lost_handover(0); }
TEST(SocketWriteCoalesce, failure_while_lingering_linger1) { failure_while_lingering(1); }
TEST(SocketWriteCoalesce, failure_while_lingering_linger0) { failure_while_lingering(0); }
TEST(SocketWriteCoalesce, shutdown_write_after_is_not_delayed_linger1) { shutdown_write_after_is_not_delayed(1); }
TEST(SocketWriteCoalesce, shutdown_write_after_is_not_delayed_linger0) { shutdown_write_after_is_not_delayed(0); }
