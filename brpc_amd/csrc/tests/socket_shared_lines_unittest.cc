// What many workers share on one connection (net/socket.h, the groups of
// fields laid out by writer): the reader's prepaid socket references balance
// at every way out of InputMessenger::OnNewMessages, the single-writer
// counters are exact once the socket is quiet, a response that comes after
// its connection failed is dropped and lets the socket go, and the sharded
// wait list of call ids ends every call once, loses none to a concurrent
// SetFailed and stays bounded. The layout itself is checked at compile time
// (Socket::CheckLayout).
#include <arpa/inet.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "base/flags.h"
#include "base/time.h"
#include "fiber/call_id.h"
#include "fiber/fiber.h"
#include "mrpc/proto/echo.pb.h"
#include "net/input_messenger.h"
#include "net/socket.h"
#include "rpc/controller.h"
#include "rpc/errno.h"
#include "rpc/server.h"
#include "tests/baidu_std_frame_util.h"
#include "tests/test.h"

DECLARE_int32(socket_write_linger);

using namespace mrpc;

namespace {

bool wait_until(const std::function<bool()>& cond, int64_t timeout_ms = 5000) {
    const int64_t deadline = monotonic_us() + timeout_ms * 1000 * mtest::kSlowdown;
    while (!cond()) {
        if (monotonic_us() > deadline) return false;
        usleep(200);
    }
    return true;
}

// With a pointer of its own: a reference taken by an earlier try must not linger.
bool address_fails(SocketId id) {
    SocketUniquePtr p;
    return Socket::Address(id, &p) != 0;
}

bool write_all(int fd, const std::string& s) {
    size_t off = 0;
    while (off < s.size()) {
        const ssize_t n = write(fd, s.data() + off, s.size() - off);
        if (n < 0 && (errno == EINTR || errno == EAGAIN)) {
            pollfd p{fd, POLLOUT, 0};
            poll(&p, 1, 100);
            continue;
        }
        if (n <= 0) return false;
        off += (size_t)n;
    }
    return true;
}

// ------------------------------------------------------ a counting protocol
// Frames: the first byte is the frame's whole length L, 1..200. 0 and 0xFF
// are parse errors.

struct Counted {
    std::atomic<int64_t> messages{0}, bytes{0};
};

ParseResult ParseCounted(Buf* source, Socket*, bool, const void*) {
    uint8_t len = 0;
    if (source->copy_to(&len, 1) < 1) return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    if (len == 0 || len == 0xFF) return MakeParseError(PARSE_ERROR_ABSOLUTELY_WRONG);
    if (source->size() < len) return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    MostCommonMessage* msg = MostCommonMessage::Get();
    source->cutn(&msg->payload, len);
    return MakeMessage(msg);
}

void ProcessCounted(InputMessageBase* base) {
    MostCommonMessage* msg = static_cast<MostCommonMessage*>(base);
    Counted* c = const_cast<Counted*>(static_cast<const Counted*>(msg->arg()));
    const int64_t n = (int64_t)msg->payload.size();
    msg->Destroy();  // gives the message's socket reference back
    c->bytes.fetch_add(n);
    c->messages.fetch_add(1, std::memory_order_release);
}

struct CountingMessenger {
    Counted counted;
    InputMessenger messenger;
    CountingMessenger() {
        InputMessageHandler h;
        h.parse = ParseCounted;
        h.process = ProcessCounted;
        h.arg = &counted;
        h.name = "counted";
        messenger.AddHandler(h);
    }
};

// One messenger for the whole run, never destroyed (as the client side's
// messenger is): a reader fiber may still be leaving OnNewMessages when a
// test is over. Each test starts it from zero, with no socket of its own left.
CountingMessenger& counting_messenger() {
    static CountingMessenger* cm = new CountingMessenger;
    cm->counted.messages.store(0);
    cm->counted.bytes.store(0);
    return *cm;
}

std::string counted_frame(size_t len, char fill) {
    std::string f(len, fill);
    f[0] = (char)(uint8_t)len;
    return f;
}

// ---------------------------------------------------------------- references

enum Ending { PLAIN, PARTIAL_FRAME, END_OF_FILE, PARSE_ERROR };

void references_balance(size_t nframes, Ending ending) {
    const int64_t nsocket0 = Socket::nsocket();
    CountingMessenger& cm = counting_messenger();
    int fds[2];
    ASSERT_EQ(socketpair(AF_UNIX, SOCK_STREAM, 0, fds), 0);
    SocketOptions o;
    o.fd = fds[0];
    SocketId id = INVALID_SOCKET_ID;
    ASSERT_EQ(cm.messenger.Create(o, &id), 0);
    std::string bytes;
    for (size_t i = 0; i < nframes; ++i) bytes += counted_frame(8, (char)('a' + i % 26));
    if (ending == PARTIAL_FRAME) bytes += counted_frame(8, 'p').substr(0, 3);
    if (ending == PARSE_ERROR) bytes += std::string(1, (char)0xFF);
    // one write: the reader cuts the whole batch from one read
    ASSERT_EQ(write(fds[1], bytes.data(), bytes.size()), (ssize_t)bytes.size());
    if (ending == END_OF_FILE) {
        close(fds[1]);
        fds[1] = -1;
    }
    EXPECT_TRUE(wait_until([&] { return cm.counted.messages.load(std::memory_order_acquire) == (int64_t)nframes; }));
    if (ending == END_OF_FILE || ending == PARSE_ERROR) {
        // the reader fails the socket itself
        EXPECT_TRUE(wait_until([&] { return address_fails(id); }));
    }
    Socket::SetFailed(id);
    EXPECT_TRUE(address_fails(id));
    // a reference that leaked keeps the socket; one released twice is fatal in Dereference
    EXPECT_TRUE(wait_until([&] { return Socket::nsocket() == nsocket0; }));
    EXPECT_EQ(cm.counted.messages.load(), (int64_t)nframes);
    if (fds[1] >= 0) close(fds[1]);
}

void references_balance_all(Ending ending) {
    const size_t chunk = InputMessenger::kPrepaidRefs;
    for (size_t n : {(size_t)1, (size_t)2, chunk - 1, chunk, chunk + 1, 3 * chunk + 1}) references_balance(n, ending);
}

// ---------------------------------------------------------------- counters

struct LingerFlag {
    int32_t saved;
    explicit LingerFlag(int32_t v) : saved(FLAGS_socket_write_linger) { FLAGS_socket_write_linger = v; }
    ~LingerFlag() { FLAGS_socket_write_linger = saved; }
};

void counters_exact(int linger) {
    LingerFlag flag(linger);
    const int64_t nsocket0 = Socket::nsocket();
    const int kWriters = 16, kEach = 2000;
    CountingMessenger& cm = counting_messenger();
    int fds[2];
    ASSERT_EQ(socketpair(AF_UNIX, SOCK_STREAM, 0, fds), 0);
    SocketOptions o;
    o.fd = fds[0];
    SocketId a = INVALID_SOCKET_ID, b = INVALID_SOCKET_ID;
    ASSERT_EQ(Socket::Create(o, &a), 0);  // the writers' end reads nothing
    o.fd = fds[1];
    ASSERT_EQ(cm.messenger.Create(o, &b), 0);
    {
        SocketUniquePtr pa, pb;
        ASSERT_EQ(Socket::Address(a, &pa), 0);
        ASSERT_EQ(Socket::Address(b, &pb), 0);
        std::atomic<int64_t> total_bytes{0};
        std::atomic<int> write_failures{0};
        std::vector<std::thread> writers;
        for (int t = 0; t < kWriters; ++t) {
            writers.emplace_back([&, t] {
                int64_t sum = 0;
                for (int m = 0; m < kEach; ++m) {
                    const size_t len = 1 + (size_t)((t * kEach + m) * 7 % 200);  // 1..200
                    Buf buf(counted_frame(len, (char)('a' + t)));
                    if (pa->Write(&buf) != 0) write_failures.fetch_add(1);
                    sum += (int64_t)len;
                }
                total_bytes.fetch_add(sum);
            });
        }
        for (auto& w : writers) w.join();
        EXPECT_EQ(write_failures.load(), 0);
        const int64_t n = (int64_t)kWriters * kEach;
        EXPECT_TRUE(wait_until([&] { return cm.counted.messages.load(std::memory_order_acquire) == n; }, 20000));
        // quiet: the writer fiber and the reader fiber gave their references
        // back (the creator's and this test's are left)
        EXPECT_TRUE(wait_until([&] { return pa->nref() <= 2 && pb->nref() <= 2 && pa->unwritten_bytes() == 0; }));
        EXPECT_EQ(pa->out_messages.load(), n);
        EXPECT_EQ(pa->out_bytes.load(), total_bytes.load());
        EXPECT_EQ(pb->in_messages.load(), n);
        EXPECT_EQ(pb->in_bytes.load(), total_bytes.load());
        EXPECT_EQ(cm.counted.bytes.load(), total_bytes.load());
        EXPECT_GE(pa->write_calls.load(), 1);
        EXPECT_GE(pb->read_calls.load(), 1);
        EXPECT_EQ(pa->in_messages.load(), 0);
        EXPECT_EQ(pb->out_messages.load(), 0);
        fprintf(stderr, "  linger=%d: %ld messages, %ld bytes in %ld write calls and %ld read calls\n", linger, (long)n,
                (long)total_bytes.load(), (long)pa->write_calls.load(), (long)pb->read_calls.load());
    }
    Socket::SetFailed(a);
    Socket::SetFailed(b);
    EXPECT_TRUE(wait_until([&] { return Socket::nsocket() == nsocket0; }));
}

// ---------------------------------------------------------------- late response

// Holds the call until the test lets it go.
class HoldingEcho : public example::EchoService {
public:
    void Echo(RpcController* cntl_base, const example::EchoRequest* request, example::EchoResponse* response,
              Closure* done) override {
        response->set_message(request->message());
        socket_id = static_cast<Controller*>(cntl_base)->_server_socket_id;
        held_done = done;
        held.store(true, std::memory_order_release);
    }
    std::atomic<bool> held{false};
    Closure* held_done = nullptr;
    SocketId socket_id = INVALID_SOCKET_ID;
};

int connect_loopback(int port) {
    const int fd = socket(AF_INET, SOCK_STREAM, 0);
    if (fd < 0) return -1;
    sockaddr_in sa;
    memset(&sa, 0, sizeof(sa));
    sa.sin_family = AF_INET;
    sa.sin_port = htons((uint16_t)port);
    sa.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    if (connect(fd, (sockaddr*)&sa, sizeof(sa)) != 0) {
        close(fd);
        return -1;
    }
    return fd;
}

void late_response(bool fail_by_hand) {
    const int64_t nsocket0 = Socket::nsocket();
    {
        Server server;
        HoldingEcho svc;
        ASSERT_EQ(server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE), 0);
        ServerOptions so;
        so.has_builtin_services = false;
        ASSERT_EQ(server.Start("127.0.0.1:0", &so), 0);
        const int64_t nsocket_listening = Socket::nsocket();
        const int fd = connect_loopback(server.listen_port());
        ASSERT_GE(fd, 0);
        example::EchoRequest req;
        req.set_message("late");
        ASSERT_TRUE(write_all(fd, frame_util::MakeRequestFrame("example.EchoService", "Echo", 7, req.SerializeAsString(), "")));
        ASSERT_TRUE(wait_until([&] { return svc.held.load(std::memory_order_acquire); }));
        const SocketId sid = svc.socket_id;
        if (fail_by_hand) {
            ASSERT_EQ(Socket::SetFailed(sid), 0);
        } else {
            close(fd);  // the client goes away: the server reads EOF and fails the socket
        }
        EXPECT_TRUE(wait_until([&] { return address_fails(sid); }));
        svc.held_done->Run();  // the response of a call whose connection is gone
        // The call's controller owns the last reference of the connection:
        // the socket goes back to the pool only if the controller was
        // destroyed, and nothing was written on the way.
        EXPECT_TRUE(wait_until([&] { return Socket::nsocket() == nsocket_listening; }));
        if (fail_by_hand) {
            // our end is still open: it sees the end of the stream and not one byte before it
            char c;
            pollfd pf{fd, POLLIN, 0};
            ASSERT_GT(poll(&pf, 1, 2000 * mtest::kSlowdown), 0);
            EXPECT_LE(read(fd, &c, 1), 0);
            close(fd);
        }
        server.Stop(0);
        server.Join();
    }
    EXPECT_TRUE(wait_until([&] { return Socket::nsocket() == nsocket0; }));
}

// ---------------------------------------------------------------- wait list

struct IdOutcome {
    std::mutex mu;
    std::vector<std::pair<uint64_t, int>> errors;  // (id, error code), one entry per on_error call
};

int on_id_error(fiber::CallId id, void* data, int error_code, const std::string&) {
    IdOutcome* o = static_cast<IdOutcome*>(data);
    {
        std::lock_guard<std::mutex> g(o->mu);
        o->errors.emplace_back(id.value, error_code);
    }
    return fiber::call_id_unlock_and_destroy(id);
}

// A socket whose peer is a plain fd; `drain` reads the peer in a thread.
struct OneEnd {
    int peer = -1;
    SocketId id = INVALID_SOCKET_ID;
    SocketUniquePtr ptr;
    std::thread reader;
    std::atomic<bool> stop{false};
    explicit OneEnd(bool drain) {
        int fds[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) return;
        peer = fds[1];
        SocketOptions o;
        o.fd = fds[0];
        Socket::Create(o, &id);
        Socket::Address(id, &ptr);
        if (drain) {
            reader = std::thread([this] {
                char buf[65536];
                while (!stop.load()) {
                    pollfd pf{peer, POLLIN, 0};
                    if (poll(&pf, 1, 10) <= 0) continue;
                    if (read(peer, buf, sizeof(buf)) <= 0) break;
                }
            });
        }
    }
    ~OneEnd() {
        Socket::SetFailed(id);
        stop.store(true);
        if (reader.joinable()) reader.join();
        if (peer >= 0) close(peer);
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
        while (monotonic_us() < deadline && ptr && ptr->nref() > 1) usleep(500);
    }
};

}  // namespace

TEST(SocketSharedLines, references_balance_single_write) { references_balance_all(PLAIN); }
TEST(SocketSharedLines, references_balance_trailing_partial_frame) { references_balance_all(PARTIAL_FRAME); }
TEST(SocketSharedLines, references_balance_eof) { references_balance_all(END_OF_FILE); }
TEST(SocketSharedLines, references_balance_parse_error) { references_balance_all(PARSE_ERROR); }

TEST(SocketSharedLines, counters_exact_linger1) { counters_exact(1); }
TEST(SocketSharedLines, counters_exact_linger0) { counters_exact(0); }

TEST(SocketSharedLines, late_response_after_client_closed) { late_response(false); }
TEST(SocketSharedLines, late_response_after_set_failed) { late_response(true); }

// 8 threads hold 50 outstanding calls between them on one connection:
// SetFailed ends each exactly once, with the socket's error.
TEST(SocketSharedLines, wait_list_fails_every_call_once) {
    const int kThreads = 8, kCalls = 50;
    IdOutcome outcome;
    std::vector<fiber::CallId> ids;
    std::mutex ids_mu;
    {
        OneEnd e(true);
        ASSERT_TRUE((bool)e.ptr);
        std::atomic<int> failures{0};
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t) {
            const int mine = kCalls / kThreads + (t < kCalls % kThreads ? 1 : 0);
            ts.emplace_back([&, mine] {
                for (int i = 0; i < mine; ++i) {
                    fiber::CallId cid;
                    if (fiber::call_id_create(&cid, &outcome, on_id_error) != 0) {
                        failures.fetch_add(1);
                        return;
                    }
                    {
                        std::lock_guard<std::mutex> g(ids_mu);
                        ids.push_back(cid);
                    }
                    WriteOptions wo;
                    wo.id_wait = cid;
                    Buf b("request");
                    if (e.ptr->Write(&b, &wo) != 0) failures.fetch_add(1);
                }
            });
        }
        for (auto& t : ts) t.join();
        ASSERT_EQ(failures.load(), 0);
        ASSERT_EQ((int)ids.size(), kCalls);
        EXPECT_EQ(e.ptr->id_wait_count(), (size_t)kCalls);
        ASSERT_EQ(e.ptr->SetFailed(ECLOSE, "failed by test"), 0);
        for (fiber::CallId cid : ids) EXPECT_TRUE(wait_until([&] { return !fiber::call_id_exists(cid); }));
        EXPECT_EQ(e.ptr->id_wait_count(), (size_t)0);
    }
    std::lock_guard<std::mutex> g(outcome.mu);
    ASSERT_EQ((int)outcome.errors.size(), kCalls);
    std::vector<uint64_t> seen;
    for (auto& er : outcome.errors) {
        EXPECT_EQ(er.second, (int)ECLOSE);
        seen.push_back(er.first);
    }
    std::sort(seen.begin(), seen.end());
    EXPECT_TRUE(std::adjacent_find(seen.begin(), seen.end()) == seen.end());
}

// A call that registers while SetFailed runs must not be left to its
// timeout. The ids here have no timeout at all: one that SetFailed missed
// and Write did not end would stay for ever, so ending within a second is
// the stricter form of "a 10 s timeout, ended within 1 s".
TEST(SocketSharedLines, wait_list_call_concurrent_with_set_failed_ends_at_once) {
    const int kRounds = 200;
    for (int r = 0; r < kRounds; ++r) {
        IdOutcome outcome;
        OneEnd e(false);
        ASSERT_TRUE((bool)e.ptr);
        fiber::CallId cid;
        ASSERT_EQ(fiber::call_id_create(&cid, &outcome, on_id_error), 0);
        std::atomic<int> go{0};
        std::thread failer([&] {
            go.fetch_add(1);
            while (go.load() < 2) {
            }
            for (int spin = 0; spin < (r % 16) * 40; ++spin) __asm__ volatile("pause");
            e.ptr->SetFailed(ECLOSE, "failed by test");
        });
        go.fetch_add(1);
        while (go.load() < 2) {
        }
        const int64_t t0 = monotonic_us();
        WriteOptions wo;
        wo.id_wait = cid;
        Buf b("request");
        e.ptr->Write(&b, &wo);  // accepted or refused, either is right
        failer.join();
        ASSERT_TRUE(wait_until([&] { return !fiber::call_id_exists(cid); }, 1000));
        EXPECT_LT(monotonic_us() - t0, 1000000LL * mtest::kSlowdown);
        std::lock_guard<std::mutex> g(outcome.mu);
        EXPECT_GE((int)outcome.errors.size(), 1);
    }
}

// Completed calls do not pile up: each shard compacts itself as before.
TEST(SocketSharedLines, wait_list_stays_bounded) {
    const int kThreads = 8, kEach = 12500, kWindow = 6;  // 100 000 calls, at most 48 live
    IdOutcome outcome;
    OneEnd e(true);
    ASSERT_TRUE((bool)e.ptr);
    const size_t bound = (size_t)Socket::kIdWaitShards * std::max<size_t>(256, 2 * (size_t)kThreads * kWindow);
    std::atomic<int> failures{0};
    std::atomic<size_t> max_seen{0};
    std::vector<std::thread> ts;
    for (int t = 0; t < kThreads; ++t) {
        ts.emplace_back([&] {
            std::vector<fiber::CallId> open;
            for (int i = 0; i < kEach; ++i) {
                fiber::CallId cid;
                if (fiber::call_id_create(&cid, &outcome, on_id_error) != 0) {
                    failures.fetch_add(1);
                    break;
                }
                open.push_back(cid);
                WriteOptions wo;
                wo.id_wait = cid;
                Buf b("r");
                if (e.ptr->Write(&b, &wo) != 0) failures.fetch_add(1);
                if (open.size() >= (size_t)kWindow) {  // the oldest call completes
                    if (fiber::call_id_lock(open.front(), nullptr) == 0) fiber::call_id_unlock_and_destroy(open.front());
                    open.erase(open.begin());
                }
                if (i % 1000 == 999) {
                    const size_t n = e.ptr->id_wait_count();
                    size_t m = max_seen.load();
                    while (n > m && !max_seen.compare_exchange_weak(m, n)) {
                    }
                }
            }
            for (fiber::CallId cid : open) {
                if (fiber::call_id_lock(cid, nullptr) == 0) fiber::call_id_unlock_and_destroy(cid);
            }
        });
    }
    for (auto& t : ts) t.join();
    EXPECT_EQ(failures.load(), 0);
    EXPECT_LE(max_seen.load(), bound);
    EXPECT_LE(e.ptr->id_wait_count(), bound);
    fprintf(stderr, "  %d calls: at most %zu ids stored, %zu at the end (bound %zu)\n", kThreads * kEach, max_seen.load(),
            e.ptr->id_wait_count(), bound);
    std::lock_guard<std::mutex> g(outcome.mu);
    EXPECT_EQ((int)outcome.errors.size(), 0);
}
