// baidu_std frames through the parser and both processing functions
// (policy/baidu_std.cc), however the bytes arrive: split in two reads at
// every offset, and placed in the read blocks so that the frame, or its meta
// alone, lies across one and two block boundaries. What the server's service
// and the client's call get out of a frame must be what is recorded in
// tests/golden/baidu_std_frame/outcomes.txt. That file was recorded by this
// same test (MRPC_BAIDU_STD_FRAME_RECORD=<path> records instead of
// comparing) when the parser still cut meta and payload into two Bufs.
//
// The bytes go through a BufPortal that reads them from a socketpair, as a
// Socket's read buffer does. Requests are handed to process_request with a
// socket whose peer the test reads the response from. Responses complete
// calls that a Channel sent to a listener which never answers: the test
// takes the correlation id from the request it reads there.
#include <arpa/inet.h>
#include <netinet/in.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "base/flags.h"
#include "base/time.h"
#include "fiber/sync.h"
#include "mrpc/proto/echo.pb.h"
#include "net/socket.h"
#include "rpc/channel.h"
#include "rpc/controller.h"
#include "rpc/errno.h"
#include "rpc/protocol.h"
#include "rpc/server.h"
#include "tests/baidu_std_frame_util.h"
#include "tests/test.h"

DECLARE_uint64(max_body_size);

using namespace mrpc;

namespace {

std::string hex(const std::string& s) {
    static const char* d = "0123456789abcdef";
    if (s.empty()) return "-";
    std::string o;
    for (unsigned char c : s) {
        o += d[c >> 4];
        o += d[c & 15];
    }
    return o;
}

// Long fields are recorded as length and FNV-1a hash.
std::string brief(const std::string& s) {
    if (s.size() <= 48) return hex(s);
    uint64_t h = 1469598103934665603ULL;
    for (unsigned char c : s) h = (h ^ c) * 1099511628211ULL;
    char buf[64];
    snprintf(buf, sizeof(buf), "%zu:%016llx", s.size(), (unsigned long long)h);
    return buf;
}

std::string pattern(size_t n, int seed) {
    std::string s(n, '\0');
    for (size_t i = 0; i < n; ++i) s[i] = (char)('A' + (i * 7 + seed + (i >> 8)) % 26);
    return s;
}

std::string GoldenPath() {
    char buf[4096];
    const ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    if (n <= 0) return "tests/golden/baidu_std_frame/outcomes.txt";
    std::string p(buf, (size_t)n);
    for (int up = 0; up < 3; ++up) {  // build/bin/<program>
        const size_t slash = p.rfind('/');
        if (slash == std::string::npos) break;
        p.resize(slash);
    }
    return p + "/tests/golden/baidu_std_frame/outcomes.txt";
}

// name -> outcome. In recording mode the outcomes are collected and written.
struct Golden {
    std::map<std::string, std::string> expected, recorded;
    const char* record_path = getenv("MRPC_BAIDU_STD_FRAME_RECORD");
    bool loaded = false;
    bool Load() {
        if (record_path || loaded) return true;
        std::ifstream in(GoldenPath());
        if (!in) return false;
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            const size_t tab = line.find('\t');
            if (tab == std::string::npos) return false;
            expected[line.substr(0, tab)] = line.substr(tab + 1);
        }
        loaded = true;
        return true;
    }
    // True if `outcome` is what the golden file holds for `name`.
    bool Check(const std::string& name, const std::string& outcome) {
        if (record_path) {
            auto it = recorded.find(name);
            if (it != recorded.end()) return it->second == outcome;  // every delivery of a case agrees
            recorded[name] = outcome;
            return true;
        }
        auto it = expected.find(name);
        return it != expected.end() && it->second == outcome;
    }
    void Save() {
        if (!record_path) return;
        // the cases of one run are added to what earlier suites of the run wrote
        std::map<std::string, std::string> all;
        {
            std::ifstream in(record_path);
            std::string line;
            while (std::getline(in, line)) {
                const size_t tab = line.find('\t');
                if (line.empty() || line[0] == '#' || tab == std::string::npos) continue;
                all[line.substr(0, tab)] = line.substr(tab + 1);
            }
        }
        for (auto& kv : recorded) all[kv.first] = kv.second;
        std::ofstream out(record_path);
        out << "# recorded by baidu_std_frame_unittest.cc (MRPC_BAIDU_STD_FRAME_RECORD): what the service, the\n"
               "# response on the wire and the client's call hold after one baidu_std frame, one case per line\n";
        for (auto& kv : all) out << kv.first << "\t" << kv.second << "\n";
    }
};

// ------------------------------------------------------------ byte delivery

// A read buffer fed through a socketpair, as Socket::_read_buf is.
struct Feed {
    int fds[2] = {-1, -1};
    BufPortal portal;
    Feed() {
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) fds[0] = fds[1] = -1;
    }
    ~Feed() {
        if (fds[0] >= 0) close(fds[0]);
        if (fds[1] >= 0) close(fds[1]);
    }
    bool Read(const std::string& bytes) {
        if (bytes.empty()) return true;
        if (write(fds[1], bytes.data(), bytes.size()) != (ssize_t)bytes.size()) return false;
        size_t got = 0;
        while (got < bytes.size()) {
            const ssize_t n = portal.append_from_fd(fds[0], bytes.size() - got);
            if (n <= 0) return false;
            got += (size_t)n;
        }
        return true;
    }
};

// Bytes that one read block holds.
size_t BlockCapacity() {
    static size_t cap = [] {
        Feed f;
        f.Read(std::string(3 * Buf::DEFAULT_BLOCK_SIZE, 'x'));
        return f.portal.backing_block_num() >= 2 ? f.portal.block_len(0) : (size_t)0;
    }();
    return cap;
}

const Protocol* BaiduStd() { return FindProtocol(PROTOCOL_BAIDU_STD); }

// One way of delivering a frame: `split` bytes in a first read (the parser
// must ask for more), the rest in a second; `lead` bytes of an earlier,
// consumed message in front, which place the frame in the blocks.
struct Delivery {
    size_t lead = 0;
    size_t split = (size_t)-1;  // (size_t)-1: one read
    std::string text() const { return "lead=" + std::to_string(lead) + " split=" + std::to_string((long)split); }
};

// Feeds `frame` as `d` says and cuts the message. Null, with *why set, if the parser did anything else.
MostCommonMessage* CutFrame(Feed* feed, const std::string& frame, const Delivery& d, Socket* sock, std::string* why) {
    const Protocol* p = BaiduStd();
    if (d.lead) {
        if (!feed->Read(std::string(d.lead, '.'))) return *why = "feeding the lead failed", nullptr;
        feed->portal.pop_front(d.lead);
    }
    if (d.split != (size_t)-1 && d.split < frame.size()) {
        if (!feed->Read(frame.substr(0, d.split))) return *why = "feeding the first part failed", nullptr;
        ParseResult r = p->parse(&feed->portal, sock, false, nullptr);
        if (r.is_ok() || r.error() != PARSE_ERROR_NOT_ENOUGH_DATA) {
            return *why = "a partial frame did not ask for more data", nullptr;
        }
        if (!feed->Read(frame.substr(d.split))) return *why = "feeding the second part failed", nullptr;
    } else if (!feed->Read(frame)) {
        return *why = "feeding the frame failed", nullptr;
    }
    ParseResult r = p->parse(&feed->portal, sock, false, nullptr);
    if (!r.is_ok()) return *why = std::string("parse error ") + ParseErrorToString(r.error()), nullptr;
    if (!feed->portal.empty()) return *why = "bytes left behind the frame", nullptr;
    return static_cast<MostCommonMessage*>(r.message());
}

// Every split of a frame, and the placements that put `span` bytes from
// `span_offset` of the frame (the whole frame, or its meta) across one and
// across two block boundaries, where they are long enough for two.
std::vector<Delivery> SplitsOf(const std::string& frame) {
    std::vector<Delivery> out;
    for (size_t k = 0; k <= frame.size(); ++k) {
        Delivery d;
        d.split = k;
        out.push_back(d);
    }
    return out;
}

std::vector<Delivery> PlacementsOf(size_t span_offset, size_t span) {
    const size_t cap = BlockCapacity();
    std::vector<Delivery> out;
    // the boundary falls 1 byte, half way and span-1 bytes into the span
    for (size_t into : {(size_t)1, span / 2, span - 1}) {
        if (into == 0 || into >= span || cap < span_offset + into) continue;
        Delivery d;
        d.lead = cap - span_offset - into;
        out.push_back(d);
        d.split = span_offset + into;  // and the second read starts at the boundary
        out.push_back(d);
    }
    if (span > cap + 1) {
        // two boundaries inside the span: it starts 1 byte and (span-cap-1) bytes before the first
        for (size_t into : {(size_t)1, span - cap - 1}) {
            if (into == 0 || cap < span_offset + into) continue;
            Delivery d;
            d.lead = cap - span_offset - into;
            out.push_back(d);
        }
    }
    return out;
}

// ------------------------------------------------------------ request side

class RecordingEcho : public example::EchoService {
public:
    void Echo(RpcController* cntl_base, const example::EchoRequest* request, example::EchoResponse* response,
              Closure* done) override {
        Controller* cntl = static_cast<Controller*>(cntl_base);
        seen = "msg=" + brief(request->message()) + " att=" + brief(cntl->request_attachment().to_string()) +
               " log_id=" + std::to_string(cntl->log_id()) + " request_id=" + brief(cntl->request_id());
        response->set_message("re:" + request->message());
        if (!cntl->request_attachment().empty()) cntl->response_attachment().append(cntl->request_attachment());
        done->Run();
    }
    std::string seen;
};

// A running server, and a connection of it whose far end the test reads.
struct RequestBench {
    Server server;
    RecordingEcho svc;
    int peer = -1;
    SocketId sid = INVALID_SOCKET_ID;
    SocketUniquePtr sock;
    bool ok = false;
    RequestBench() {
        ServerOptions so;
        so.has_builtin_services = false;
        if (server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE) != 0 || server.Start("127.0.0.1:0", &so) != 0) return;
        int fds[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) return;
        peer = fds[1];
        SocketOptions o;
        o.fd = fds[0];
        ok = Socket::Create(o, &sid) == 0 && Socket::Address(sid, &sock) == 0;
    }
    ~RequestBench() {
        sock.reset();
        Socket::SetFailed(sid);
        if (peer >= 0) close(peer);
        server.Stop(0);
        server.Join();
    }
    // The next response frame on the wire, as "meta=.. body=.. att=..".
    std::string ReadResponse() {
        std::string head = ReadN(12);
        if (head.size() != 12 || head.compare(0, 4, "PRPC") != 0) return "no response frame";
        const uint32_t body_size = frame_util::ReadBe32(head.data() + 4), meta_size = frame_util::ReadBe32(head.data() + 8);
        const std::string body = ReadN(body_size);
        policy::RpcMeta meta;
        if (body.size() != body_size || meta_size > body_size || !meta.ParseFromString(body.substr(0, meta_size))) {
            return "bad response frame";
        }
        const size_t att = (size_t)meta.attachment_size();
        if (att > body_size - meta_size) return "bad attachment size";
        return "meta=" + hex(body.substr(0, meta_size)) + " body=" + brief(body.substr(meta_size, body_size - meta_size - att)) +
               " att=" + brief(body.substr(body_size - att));
    }
    std::string ReadN(size_t n) {
        std::string out(n, '\0');
        size_t got = 0;
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
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
    // Delivers one request frame and returns what the service saw and what went back.
    std::string Run(const std::string& frame, const Delivery& d) {
        Feed feed;
        std::string why;
        MostCommonMessage* msg = CutFrame(&feed, frame, d, sock.get(), &why);
        if (!msg) return why;
        svc.seen = "not called";
        sock->AddRef();
        msg->_socket.reset(sock.get());
        msg->_arg = &server;
        msg->_received_us = monotonic_us();
        BaiduStd()->process_request(msg);
        const std::string response = ReadResponse();
        return "service{" + svc.seen + "} response{" + response + "}";
    }
};

struct RequestCase {
    std::string name, frame;
    size_t meta_size;
};

std::vector<RequestCase> RequestCases() {
    example::EchoRequest req;
    req.set_message("frame-golden-request");
    const std::string body = req.SerializeAsString();
    std::vector<RequestCase> out;
    auto add = [&](const std::string& name, const std::string& frame) {
        out.push_back(RequestCase{name, frame, frame_util::ReadBe32(frame.data() + 8)});
    };
    add("request", frame_util::MakeRequestFrame("example.EchoService", "Echo", 77, body, "", 42, "rid-1"));
    add("request_attachment",
        frame_util::MakeRequestFrame("example.EchoService", "Echo", 78, body, "ATTACHMENT-0123456789", 43, "rid-2"));
    // no meta at all: the server answers that the request meta is missing
    add("request_meta0", frame_util::MakeFrame("", body, ""));
    add("request_meta0_attachment", frame_util::MakeFrame("", body, "ATTACHMENT-0123456789"));
    return out;
}

// Long enough for two block boundaries inside the meta, and inside the rest of the frame.
std::vector<RequestCase> LongRequestCases() {
    example::EchoRequest req;
    req.set_message("frame-golden-long");
    const std::string body = req.SerializeAsString();
    const size_t cap = BlockCapacity();
    std::vector<RequestCase> out;
    auto add = [&](const std::string& name, const std::string& frame) {
        out.push_back(RequestCase{name, frame, frame_util::ReadBe32(frame.data() + 8)});
    };
    add("request_long_meta", frame_util::MakeRequestFrame("example.EchoService", "Echo", 79, body, "", 44, pattern(cap + 300, 3)));
    add("request_long_attachment",
        frame_util::MakeRequestFrame("example.EchoService", "Echo", 80, body, pattern(cap + 300, 5), 45, "rid-4"));
    return out;
}

void CheckRequests(const std::vector<RequestCase>& cases, bool every_split) {
    Golden golden;
    ASSERT_TRUE_M(golden.Load(), GoldenPath());
    ASSERT_GT(BlockCapacity(), (size_t)0);
    RequestBench bench;
    ASSERT_TRUE(bench.ok);
    size_t runs = 0;
    for (const RequestCase& c : cases) {
        std::vector<Delivery> ds;
        if (every_split) ds = SplitsOf(c.frame);
        for (const Delivery& d : PlacementsOf(0, c.frame.size())) ds.push_back(d);
        if (c.meta_size > 1) {
            for (const Delivery& d : PlacementsOf(12, c.meta_size)) ds.push_back(d);
        }
        for (const Delivery& d : ds) {
            const std::string outcome = bench.Run(c.frame, d);
            ++runs;
            if (!golden.Check(c.name, outcome)) {
                EXPECT_TRUE_M(false, c.name + " " + d.text() + ": " + outcome);
                break;  // one report per case
            }
        }
    }
    fprintf(stderr, "  %zu request frames delivered\n", runs);
    golden.Save();
}

// ------------------------------------------------------------ response side

// A listener that reads the requests of one connection and never answers.
struct SilentListener {
    int lfd = -1, cfd = -1, port = 0;
    SilentListener() {
        lfd = socket(AF_INET, SOCK_STREAM, 0);
        sockaddr_in sa;
        memset(&sa, 0, sizeof(sa));
        sa.sin_family = AF_INET;
        sa.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
        socklen_t len = sizeof(sa);
        if (lfd < 0 || bind(lfd, (sockaddr*)&sa, sizeof(sa)) != 0 || listen(lfd, 8) != 0 ||
            getsockname(lfd, (sockaddr*)&sa, &len) != 0) {
            return;
        }
        port = ntohs(sa.sin_port);
    }
    ~SilentListener() {
        if (cfd >= 0) close(cfd);
        if (lfd >= 0) close(lfd);
    }
    bool ReadN(char* out, size_t n) {
        size_t got = 0;
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
        while (got < n && monotonic_us() < deadline) {
            pollfd p{cfd >= 0 ? cfd : lfd, POLLIN, 0};
            if (poll(&p, 1, 50) <= 0) continue;
            if (cfd < 0) {
                cfd = accept(lfd, nullptr, nullptr);
                continue;
            }
            const ssize_t r = read(cfd, out + got, n - got);
            if (r <= 0) return false;
            got += (size_t)r;
        }
        return got == n;
    }
    // The correlation id of the next request on the connection; -1 if none comes.
    int64_t NextCorrelationId() {
        char head[12];
        if (!ReadN(head, 12) || memcmp(head, "PRPC", 4) != 0) return -1;
        const uint32_t body_size = frame_util::ReadBe32(head + 4), meta_size = frame_util::ReadBe32(head + 8);
        std::string body(body_size, '\0');
        policy::RpcMeta meta;
        if (!ReadN(&body[0], body_size) || meta_size > body_size || !meta.ParseFromString(body.substr(0, meta_size))) return -1;
        return meta.correlation_id();
    }
};

struct ResponseCase {
    std::string name;
    std::function<std::string(int64_t)> frame;  // for a correlation id
    // false: the frame names no call, so it is dropped and the test cancels the call afterwards
    bool completes = true;
};

std::vector<ResponseCase> ResponseCases(bool with_long) {
    example::EchoResponse res;
    res.set_message("frame-golden-response");
    const std::string body = res.SerializeAsString();
    const size_t cap = BlockCapacity();
    std::vector<ResponseCase> out;
    if (!with_long) {
        out.push_back({"response", [=](int64_t cid) { return frame_util::MakeResponseFrame(cid, body, ""); }});
        out.push_back({"response_attachment",
                       [=](int64_t cid) { return frame_util::MakeResponseFrame(cid, body, "ATTACHMENT-9876543210"); }});
        out.push_back({"response_error", [=](int64_t cid) { return frame_util::MakeResponseFrame(cid, "", "", 2004, "no such thing"); }});
        // no meta at all: no correlation id, nothing to complete
        out.push_back({"response_meta0", [=](int64_t) { return frame_util::MakeFrame("", body, ""); }, false});
        out.push_back({"response_meta0_attachment",
                       [=](int64_t) { return frame_util::MakeFrame("", body, "ATTACHMENT-9876543210"); }, false});
    } else {
        out.push_back({"response_long_meta", [=](int64_t cid) {
                           return frame_util::MakeResponseFrame(cid, "", "", 2004, pattern(cap + 300, 9));
                       }});
        out.push_back({"response_long_attachment",
                       [=](int64_t cid) { return frame_util::MakeResponseFrame(cid, body, pattern(cap + 300, 11)); }});
    }
    return out;
}

void CheckResponses(bool with_long) {
    Golden golden;
    ASSERT_TRUE_M(golden.Load(), GoldenPath());
    ASSERT_GT(BlockCapacity(), (size_t)0);
    SilentListener listener;
    ASSERT_GT(listener.port, 0);
    Channel ch;
    ChannelOptions opt;
    opt.timeout_ms = 10000 * mtest::kSlowdown;
    opt.max_retry = 0;
    ASSERT_EQ(ch.Init(("127.0.0.1:" + std::to_string(listener.port)).c_str(), &opt), 0);
    example::EchoService_Stub stub(&ch);
    // the socket that the response messages name as theirs
    int fds[2];
    ASSERT_EQ(socketpair(AF_UNIX, SOCK_STREAM, 0, fds), 0);
    SocketOptions o;
    o.fd = fds[0];
    SocketId sid;
    ASSERT_EQ(Socket::Create(o, &sid), 0);
    SocketUniquePtr sock;
    ASSERT_EQ(Socket::Address(sid, &sock), 0);
    size_t runs = 0;
    for (const ResponseCase& c : ResponseCases(with_long)) {
        // the frame's length depends on the correlation id: take the deliveries from a first frame
        const std::string sample = c.frame(1);
        const size_t sample_meta = frame_util::ReadBe32(sample.data() + 8);
        std::vector<Delivery> ds;
        if (!with_long) ds = SplitsOf(sample);
        for (const Delivery& d : PlacementsOf(0, sample.size())) ds.push_back(d);
        if (sample_meta > 1) {
            for (const Delivery& d : PlacementsOf(12, sample_meta)) ds.push_back(d);
        }
        bool reported = false;
        for (size_t i = 0; i < ds.size() && !reported; ++i) {
            Controller cntl;
            example::EchoRequest req;
            example::EchoResponse res;
            req.set_message("ask");
            fiber::CountdownEvent finished(1);
            stub.Echo(&cntl, &req, &res, NewCallback([&finished] { finished.signal(); }));
            const int64_t cid = listener.NextCorrelationId();
            std::string outcome;
            Feed feed;
            MostCommonMessage* msg = nullptr;
            if (cid < 0) {
                outcome = "the request did not reach the listener";
            } else {
                const std::string frame = c.frame(cid);
                Delivery d = ds[i];
                if (d.split != (size_t)-1 && d.split > frame.size()) d.split = frame.size();
                msg = CutFrame(&feed, frame, d, sock.get(), &outcome);
            }
            if (msg) {
                sock->AddRef();
                msg->_socket.reset(sock.get());
                msg->_received_us = monotonic_us();
                BaiduStd()->process_response(msg);
                if (!c.completes) cntl.StartCancel();
            } else {
                cntl.StartCancel();
            }
            finished.wait();
            ++runs;
            if (msg) {
                outcome = "code=" + std::to_string(cntl.ErrorCode()) + " text=" + brief(cntl.ErrorText()) +
                          " msg=" + brief(res.message()) + " att=" + brief(cntl.response_attachment().to_string());
            }
            if (!golden.Check(c.name, outcome)) {
                EXPECT_TRUE_M(false, c.name + " " + ds[i].text() + ": " + outcome);
                reported = true;
            }
        }
    }
    fprintf(stderr, "  %zu response frames delivered\n", runs);
    sock.reset();
    Socket::SetFailed(sid);
    close(fds[1]);
    golden.Save();
}

}  // namespace

TEST(BaiduStdFrame, requests_split_at_every_offset_and_across_blocks) { CheckRequests(RequestCases(), true); }
TEST(BaiduStdFrame, long_requests_across_two_block_boundaries) { CheckRequests(LongRequestCases(), false); }
TEST(BaiduStdFrame, responses_split_at_every_offset_and_across_blocks) { CheckResponses(false); }
TEST(BaiduStdFrame, long_responses_across_two_block_boundaries) { CheckResponses(true); }

// The placements do what their names say: the blocks under the frame are as many as intended.
TEST(BaiduStdFrame, placements_cross_block_boundaries) {
    const size_t cap = BlockCapacity();
    ASSERT_GT(cap, (size_t)0);
    const std::string frame = LongRequestCases()[0].frame;
    const size_t meta_size = frame_util::ReadBe32(frame.data() + 8);
    ASSERT_GT(meta_size, cap + 1);
    int two_boundaries = 0;
    for (const Delivery& d : PlacementsOf(12, meta_size)) {
        if (d.split != (size_t)-1) continue;
        Feed feed;
        ASSERT_TRUE(feed.Read(std::string(d.lead, '.')));
        feed.portal.pop_front(d.lead);
        ASSERT_TRUE(feed.Read(frame));
        // bytes of the frame in the first block, then whole blocks
        const size_t first = feed.portal.block_len(0);
        EXPECT_EQ(first, cap - d.lead);
        EXPECT_GT(first, (size_t)12);               // the meta starts in the first block
        EXPECT_LT(first, 12 + meta_size);           // and does not end there
        if (first + cap < 12 + meta_size) ++two_boundaries;
    }
    EXPECT_GE(two_boundaries, 2);
}

// Frames that the parser refuses are refused as before.
TEST(BaiduStdFrame, bad_sizes_yield_the_same_errors) {
    Golden golden;
    ASSERT_TRUE_M(golden.Load(), GoldenPath());
    int fds[2];
    ASSERT_EQ(socketpair(AF_UNIX, SOCK_STREAM, 0, fds), 0);
    SocketOptions o;
    o.fd = fds[0];
    SocketId sid;
    ASSERT_EQ(Socket::Create(o, &sid), 0);
    SocketUniquePtr sock;
    ASSERT_EQ(Socket::Address(sid, &sock), 0);
    {
        // meta_size > body_size: an error once the whole body is there, and the frame is dropped
        std::string f("PRPC");
        frame_util::AppendBe32(&f, 10);
        frame_util::AppendBe32(&f, 11);
        f += "0123456789";
        Feed feed;
        ASSERT_TRUE(feed.Read(f.substr(0, 15)));
        ParseResult r1 = BaiduStd()->parse(&feed.portal, sock.get(), false, nullptr);
        ASSERT_TRUE(feed.Read(f.substr(15) + "next"));
        ParseResult r2 = BaiduStd()->parse(&feed.portal, sock.get(), false, nullptr);
        const std::string outcome = std::string("partial=") + ParseErrorToString(r1.error()) + " whole=" +
                                    ParseErrorToString(r2.error()) + " left=" + hex(feed.portal.to_string());
        EXPECT_TRUE_M(golden.Check("meta_size_above_body_size", outcome), outcome);
        EXPECT_EQ((int)r2.error(), (int)PARSE_ERROR_ABSOLUTELY_WRONG);
    }
    {
        // a body above -max_body_size: refused from the header alone
        std::string f("PRPC");
        frame_util::AppendBe32(&f, (uint32_t)std::min<uint64_t>(FLAGS_max_body_size + 1, 0xFFFFFFFFu));
        frame_util::AppendBe32(&f, 4);
        Feed feed;
        ASSERT_TRUE(feed.Read(f));
        ParseResult r = BaiduStd()->parse(&feed.portal, sock.get(), false, nullptr);
        const std::string outcome = std::string("header=") + ParseErrorToString(r.error()) + " left=" + std::to_string(feed.portal.size());
        EXPECT_TRUE_M(golden.Check("oversize_body", outcome), outcome);
        EXPECT_EQ((int)r.error(), (int)PARSE_ERROR_TOO_BIG_DATA);
    }
    sock.reset();
    Socket::SetFailed(sid);
    close(fds[1]);
    golden.Save();
}
