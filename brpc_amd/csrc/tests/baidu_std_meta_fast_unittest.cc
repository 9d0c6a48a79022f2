// The RpcMeta of plain baidu_std calls packed and scanned without a message
// object (policy/baidu_std_meta.h): the packers write the generic
// serializer's bytes, the scanners yield the generic parser's values or
// decline, a declined meta ends as it does with -baidu_std_meta_fast_path
// off, the counters say which way each call went, Server's lookup by two
// string views agrees with the one by strings, and the messages cut from one
// read carry one receive stamp.
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "base/flags.h"
#include "base/time.h"
#include "fiber/fiber.h"
#include "mrpc/proto/echo.pb.h"
#include "net/input_messenger.h"
#include "net/socket.h"
#include "pb/descriptor.h"
#include "policy/baidu_std_meta.h"
#include "rpc/authenticator.h"
#include "rpc/channel.h"
#include "rpc/controller.h"
#include "rpc/errno.h"
#include "rpc/protocol.h"
#include "rpc/server.h"
#include "tests/baidu_std_frame_util.h"
#include "tests/test.h"

DECLARE_bool(baidu_std_meta_fast_path);
DECLARE_bool(baidu_protocol_use_fullname);

using namespace mrpc;
using policy::RpcMeta;

namespace {

struct BoolFlag {
    bool* flag;
    bool saved;
    BoolFlag(bool* f, bool v) : flag(f), saved(*f) { *f = v; }
    ~BoolFlag() { *flag = saved; }
};

const int64_t kInt64Max = 0x7fffffffffffffffLL;
const int32_t kInt32Max = 0x7fffffff;

// ---------------------------------------------------------------- the values

struct RequestValues {
    std::string service, method;
    int64_t cid = 0;
    int32_t compress_type = 0;
    int32_t attachment_size = 0;  // 0: absent
    bool has_log_id = false;
    int64_t log_id = 0;
    int32_t timeout_ms = 0;  // 0: absent
};

std::string GenericRequestMeta(const RequestValues& v) {
    RpcMeta meta;
    meta.mutable_request()->set_service_name(v.service);
    meta.mutable_request()->set_method_name(v.method);
    if (v.has_log_id) meta.mutable_request()->set_log_id(v.log_id);
    if (v.timeout_ms) meta.mutable_request()->set_timeout_ms(v.timeout_ms);
    meta.set_compress_type(v.compress_type);
    meta.set_correlation_id(v.cid);
    if (v.attachment_size) meta.set_attachment_size(v.attachment_size);
    return meta.SerializeAsString();
}

// Header and meta as the fast packer writes them, for `payload` bytes behind.
std::string FastRequestFrameHead(const RequestValues& v, const std::string& name_fields, size_t payload) {
    policy::PlainRequestMeta m;
    m.name_fields = name_fields;
    m.has_log_id = v.has_log_id;
    m.log_id = v.log_id;
    m.timeout_ms = v.timeout_ms;
    m.compress_type = v.compress_type;
    m.correlation_id = v.cid;
    m.attachment_size = v.attachment_size;
    Buf out;
    policy::PackPlainRequestMeta(&out, m, payload);
    return out.to_string();
}

// A method whose service has the given full and short names.
struct NamedMethod {
    pb::ServiceDescriptor sd;
    NamedMethod(const std::string& full, const std::string& brief, const std::string& method) {
        sd.full_name = full;
        sd.name = brief;
        sd.methods.resize(1);
        sd.methods[0].name = method;
        sd.methods[0].service = &sd;
    }
    const pb::MethodDescriptor* md() const { return &sd.methods[0]; }
};

// True if the generic parser reads `bytes` as exactly the values of `s` and nothing else.
bool GenericAgrees(const std::string& bytes, const policy::ScannedRequestMeta& s, std::string* why) {
    RpcMeta m;
    if (!m.ParseFromArray(bytes.data(), bytes.size())) return *why = "the generic parser refuses it", false;
    const policy::RpcRequestMeta& r = m.request();
    if (!m.has_request() || m.has_response() || m.has_chunk_info() || m.has_authentication_data() ||
        m.has_stream_settings() || m.device_payload_size() || m.has_xgmi_hello() || m.has_plane_hello() ||
        r.has_trace_id() || r.has_span_id() || r.has_parent_span_id() || r.has_request_id()) {
        return *why = "the generic parser finds more fields", false;
    }
    if (r.service_name() != s.service_name || r.method_name() != s.method_name) return *why = "names differ", false;
    if (r.has_log_id() != s.has_log_id || r.log_id() != s.log_id) return *why = "log_id differs", false;
    if (r.has_timeout_ms() != s.has_timeout_ms || r.timeout_ms() != s.timeout_ms) return *why = "timeout_ms differs", false;
    if (m.compress_type() != s.compress_type) return *why = "compress_type differs", false;
    if (m.correlation_id() != s.correlation_id) return *why = "correlation_id differs", false;
    if (m.attachment_size() != s.attachment_size) return *why = "attachment_size differs", false;
    return true;
}

std::string Describe(const RequestValues& v) {
    return "service=" + std::to_string(v.service.size()) + " method=" + std::to_string(v.method.size()) +
           " cid=" + std::to_string(v.cid) + " ct=" + std::to_string(v.compress_type) + " att=" +
           std::to_string(v.attachment_size) + " log_id=" + (v.has_log_id ? std::to_string(v.log_id) : "-") +
           " timeout=" + std::to_string(v.timeout_ms);
}

// Every combination of the scalar values, for one pair of names.
void ForEachScalarCombination(RequestValues v, const std::function<void(const RequestValues&)>& fn) {
    struct LogId {
        bool has;
        int64_t v;
    };
    for (int64_t cid : {(int64_t)1, (int64_t)127, (int64_t)128, (int64_t)1 << 32, ((int64_t)1 << 32) + 1, kInt64Max}) {
        for (int32_t ct : {0, 1, 2}) {
            for (int32_t att : {0, 1, 127, 128, kInt32Max}) {
                for (LogId log : {LogId{false, 0}, LogId{true, 1}, LogId{true, kInt64Max}, LogId{true, -1}}) {
                    for (int32_t timeout : {0, 1, kInt32Max}) {
                        v.cid = cid;
                        v.compress_type = ct;
                        v.attachment_size = att;
                        v.has_log_id = log.has;
                        v.log_id = log.v;
                        v.timeout_ms = timeout;
                        fn(v);
                    }
                }
            }
        }
    }
}

// The name pairs: every length of the table for service and method, and two
// pairs that put the request submessage at 127 and at 128 bytes when it
// holds nothing but the names (2 + 100 + 2 + 23, and one more).
std::vector<std::pair<size_t, size_t>> NameLengths() {
    std::vector<std::pair<size_t, size_t>> out;
    for (size_t s : {1, 15, 16, 127, 128, 300}) {
        for (size_t m : {1, 15, 16, 127, 128, 300}) out.emplace_back(s, m);
    }
    out.emplace_back(100, 23);
    out.emplace_back(100, 24);
    return out;
}

// One pass over every request meta of the table: `fn` gets the values, the
// generic bytes, and the method whose cached names the fast packer uses
// (`brief`: the short service name is the one on the wire).
void ForEachRequestMeta(const std::function<void(const RequestValues&, const std::string& generic,
                                                 const NamedMethod&, bool brief)>& fn) {
    for (auto& len : NameLengths()) {
        for (bool brief : {false, true}) {
            // the name that is not on the wire has another length
            const std::string wire_service(len.first, 's');
            const std::string other_service(len.first + 3, 'o');
            NamedMethod nm(brief ? other_service : wire_service, brief ? wire_service : other_service,
                           std::string(len.second, 'm'));
            RequestValues v;
            v.service = wire_service;
            v.method = nm.md()->name;
            ForEachScalarCombination(v, [&](const RequestValues& x) { fn(x, GenericRequestMeta(x), nm, brief); });
        }
    }
}

}  // namespace

// ------------------------------------------------------------ pack identity

TEST(BaiduStdMetaFast, request_pack_is_the_generic_serializers_bytes) {
    size_t n = 0, sub127 = 0, sub128 = 0;
    bool reported = false;
    ForEachRequestMeta([&](const RequestValues& v, const std::string& generic, const NamedMethod& nm, bool brief) {
        if (reported) return;
        const pb::MethodWireNames* names = nm.md()->wire_names();
        const std::string& fields = brief ? names->brief : names->full;
        // a body behind the meta, and the attachment's bytes where they can be had
        const std::string body = "BODY";
        const std::string attachment(v.attachment_size <= 128 ? (size_t)v.attachment_size : 0, 'A');
        const std::string expect = frame_util::MakeFrame(generic, body, attachment).substr(0, 12 + generic.size());
        const std::string got = FastRequestFrameHead(v, fields, body.size() + attachment.size());
        if (got != expect) {
            EXPECT_TRUE_M(false, Describe(v) + (brief ? " short name" : " full name"));
            reported = true;
        }
        // the submessage's length: the byte after the first tag when it is one byte
        if ((uint8_t)generic[1] == 127) ++sub127;
        if ((uint8_t)generic[1] == 0x80 && (uint8_t)generic[2] == 1) ++sub128;
        ++n;
    });
    EXPECT_EQ(n, (size_t)(38 * 2 * 6 * 3 * 5 * 4 * 3));
    EXPECT_GT(sub127, (size_t)0);
    EXPECT_GT(sub128, (size_t)0);
}

TEST(BaiduStdMetaFast, cached_names_are_built_once_and_copies_start_without) {
    NamedMethod nm("pkg.Service", "Service", "Method");
    const pb::MethodWireNames* a = nm.md()->wire_names();
    EXPECT_TRUE(a == nm.md()->wire_names());
    EXPECT_EQ(a->full, std::string("\x0a\x0bpkg.Service\x12\x06Method"));
    EXPECT_EQ(a->brief, std::string("\x0a\x07Service\x12\x06Method"));
    pb::MethodDescriptor copy = *nm.md();
    EXPECT_TRUE(copy.wire_names_cache.get() == nullptr);
    copy.name = "Other";
    EXPECT_EQ(copy.wire_names()->brief, std::string("\x0a\x07Service\x12\x05Other"));
    copy = *nm.md();  // assigned over: the names of the old content go
    EXPECT_TRUE(copy.wire_names_cache.get() == nullptr);
    EXPECT_EQ(copy.wire_names()->full, a->full);
}

TEST(BaiduStdMetaFast, response_pack_is_the_generic_serializers_bytes) {
    size_t n = 0;
    for (int64_t cid : {(int64_t)1, (int64_t)127, (int64_t)128, (int64_t)1 << 32, ((int64_t)1 << 32) + 1, kInt64Max}) {
        for (int32_t ct : {0, 1, 2}) {
            for (int32_t att : {0, 1, 127, 128, kInt32Max}) {
                RpcMeta meta;
                meta.set_compress_type(ct);
                meta.set_correlation_id(cid);
                if (att) meta.set_attachment_size(att);
                const std::string generic = meta.SerializeAsString();
                const std::string body = "BODY";
                const std::string attachment(att <= 128 ? (size_t)att : 0, 'A');
                policy::PlainResponseMeta m;
                m.compress_type = ct;
                m.correlation_id = cid;
                m.attachment_size = att;
                Buf out;
                policy::PackPlainResponseMeta(&out, m, body.size() + attachment.size());
                EXPECT_EQ(out.to_string(), frame_util::MakeFrame(generic, body, attachment).substr(0, 12 + generic.size()));
                // and back
                policy::ScannedResponseMeta s;
                ASSERT_TRUE(policy::ScanPlainResponseMeta(generic.data(), generic.size(), &s));
                EXPECT_EQ(s.compress_type, ct);
                EXPECT_EQ(s.correlation_id, cid);
                EXPECT_EQ(s.attachment_size, att);
                ++n;
            }
        }
    }
    EXPECT_EQ(n, (size_t)90);
    // the plain reply of the golden file
    policy::PlainResponseMeta m;
    m.correlation_id = 77;
    Buf out;
    policy::PackPlainResponseMeta(&out, m, 0);
    EXPECT_EQ(out.to_string().substr(12), std::string("\x18\x00\x20\x4d", 4));
}

// ---------------------------------------------------------- scan equivalence

// A proper prefix of a packed meta is declined, except where it ends
// between two fields behind the request submessage: such a prefix is a
// whole meta itself, with the later fields absent (it is one of the table's
// own strings when only attachment_size is cut off), so there the scanner
// must agree with the generic parser instead.
TEST(BaiduStdMetaFast, scan_yields_the_generic_parsers_values_and_declines_prefixes) {
    size_t prefixes = 0, whole_prefixes = 0;
    bool reported = false;
    ForEachRequestMeta([&](const RequestValues& v, const std::string& bytes, const NamedMethod&, bool) {
        if (reported) return;
        policy::ScannedRequestMeta s;
        std::string why;
        if (!policy::ScanPlainRequestMeta(bytes.data(), bytes.size(), &s)) {
            EXPECT_TRUE_M(false, "declined: " + Describe(v));
            reported = true;
            return;
        }
        if (!GenericAgrees(bytes, s, &why) || s.service_name != v.service || s.method_name != v.method ||
            s.correlation_id != v.cid || s.log_id != v.log_id || s.timeout_ms != v.timeout_ms ||
            s.attachment_size != v.attachment_size || s.compress_type != v.compress_type) {
            EXPECT_TRUE_M(false, why + ": " + Describe(v));
            reported = true;
            return;
        }
        for (size_t k = 0; k < bytes.size() && !reported; ++k) {
            ++prefixes;
            policy::ScannedRequestMeta p;
            // a copy of its own, so that a read past the prefix is a read past an allocation
            const std::string prefix = bytes.substr(0, k);
            if (!policy::ScanPlainRequestMeta(prefix.data(), prefix.size(), &p)) continue;
            ++whole_prefixes;
            if (!GenericAgrees(prefix, p, &why)) {
                EXPECT_TRUE_M(false, "prefix " + std::to_string(k) + " " + why + ": " + Describe(v));
                reported = true;
            }
        }
    });
    fprintf(stderr, "  %zu prefixes, %zu of them whole metas\n", prefixes, whole_prefixes);
    EXPECT_GT(prefixes, whole_prefixes * 10);
}

namespace {

void PutVarint(std::string* out, uint64_t v) {
    while (v >= 0x80) {
        out->push_back((char)(v | 0x80));
        v >>= 7;
    }
    out->push_back((char)v);
}
std::string VarintField(int number, uint64_t v) {
    std::string s;
    PutVarint(&s, (uint64_t)number << 3);
    PutVarint(&s, v);
    return s;
}
std::string BytesField(int number, const std::string& v) {
    std::string s;
    PutVarint(&s, ((uint64_t)number << 3) | 2);
    PutVarint(&s, v.size());
    return s + v;
}
std::string Fixed32Field(int number) {
    std::string s;
    PutVarint(&s, ((uint64_t)number << 3) | 5);
    return s + std::string("\1\0\0\0", 4);
}
std::string Fixed64Field(int number) {
    std::string s;
    PutVarint(&s, ((uint64_t)number << 3) | 1);
    return s + std::string("\1\0\0\0\0\0\0\0", 8);
}

const std::string kNames = BytesField(1, "example.EchoService") + BytesField(2, "Echo");

struct MetaCase {
    std::string name, meta;
    bool may_accept = false;  // the permutations: accepted with equal values, or declined
};

std::vector<MetaCase> DeclinedMetas() {
    const std::string request = BytesField(1, kNames + VarintField(3, 42));
    const std::string tail = VarintField(3, 0) + VarintField(4, 77);
    std::vector<MetaCase> out;
    auto add = [&](const std::string& name, const std::string& meta) { out.push_back(MetaCase{name, meta, false}); };
    out.push_back({"permuted_top_level", VarintField(4, 77) + VarintField(5, 0) + request + VarintField(3, 0), true});
    out.push_back({"permuted_names", BytesField(1, VarintField(3, 42) + BytesField(2, "Echo") + BytesField(1, "example.EchoService")) + tail, true});
    add("duplicate_correlation_id", request + tail + VarintField(4, 78));
    add("duplicate_compress_type", request + VarintField(3, 0) + tail);
    add("duplicate_attachment_size", request + tail + VarintField(5, 0) + VarintField(5, 0));
    add("duplicate_log_id", BytesField(1, kNames + VarintField(3, 42) + VarintField(3, 43)) + tail);
    add("duplicate_service_name", BytesField(1, kNames + BytesField(1, "example.EchoService")) + tail);
    add("duplicate_request", request + request + tail);
    add("unknown_field_9", request + tail + VarintField(9, 1));
    add("unknown_field_2000", request + tail + VarintField(2000, 1));
    add("response_field_2", request + tail + BytesField(2, ""));
    add("field_6_chunk_info", request + tail + BytesField(6, ""));
    add("field_7_authentication_data", request + tail + BytesField(7, "who"));
    add("field_8_stream_settings", request + tail + BytesField(8, ""));
    add("field_100_device_payload", request + tail + BytesField(100, ""));
    add("field_101_xgmi_hello", request + tail + BytesField(101, ""));
    add("field_102_plane_hello", request + tail + BytesField(102, ""));
    add("request_field_4_trace_id", BytesField(1, kNames + VarintField(4, 5)) + tail);
    add("request_field_5_span_id", BytesField(1, kNames + VarintField(5, 5)) + tail);
    add("request_field_6_parent_span_id", BytesField(1, kNames + VarintField(6, 5)) + tail);
    add("request_field_7_request_id", BytesField(1, kNames + BytesField(7, "rid")) + tail);
    add("request_unknown_field_9", BytesField(1, kNames + VarintField(9, 5)) + tail);
    add("wire_type_request_varint", VarintField(1, 5) + tail);
    add("wire_type_compress_type_bytes", request + BytesField(3, "") + VarintField(4, 77));
    add("wire_type_correlation_id_fixed64", request + VarintField(3, 0) + Fixed64Field(4));
    add("wire_type_attachment_size_fixed32", request + tail + Fixed32Field(5));
    add("wire_type_service_name_varint", BytesField(1, VarintField(1, 5) + BytesField(2, "Echo")) + tail);
    add("wire_type_method_name_varint", BytesField(1, BytesField(1, "example.EchoService") + VarintField(2, 5)) + tail);
    add("wire_type_log_id_bytes", BytesField(1, kNames + BytesField(3, "x")) + tail);
    add("wire_type_timeout_ms_fixed32", BytesField(1, kNames + Fixed32Field(8)) + tail);
    add("varint_of_11_bytes", request + VarintField(3, 0) + std::string("\x20") + std::string(10, (char)0x80) + std::string("\0", 1));
    {
        // the method name says one byte more than the submessage holds
        std::string sub = BytesField(1, "example.EchoService") + std::string("\x12\x05") + "Echo";
        add("name_length_one_past_the_submessage", BytesField(1, sub) + tail);
        // the submessage says one byte more than the meta holds
        std::string m = std::string("\x0a");
        PutVarint(&m, kNames.size() + 1);
        add("request_length_one_past_the_meta", m + kNames);
    }
    add("missing_service_name", BytesField(1, BytesField(2, "Echo")) + tail);
    add("missing_method_name", BytesField(1, BytesField(1, "example.EchoService")) + tail);
    add("missing_request", tail);
    add("empty_meta", "");
    return out;
}

// ---- one frame through process_request, as the frame suite delivers it

class SeenEcho : public example::EchoService {
public:
    void Echo(RpcController* cntl_base, const example::EchoRequest* request, example::EchoResponse* response,
              Closure* done) override {
        Controller* cntl = static_cast<Controller*>(cntl_base);
        {
            std::lock_guard<std::mutex> g(mu);
            seen = "msg=" + request->message() + " att=" + cntl->request_attachment().to_string() +
                   " log_id=" + std::to_string(cntl->log_id()) + " request_id=" + cntl->request_id();
        }
        response->set_message(request->message());
        cntl->response_attachment().append(cntl->request_attachment());
        done->Run();
    }
    std::mutex mu;
    std::string seen;
};

std::string Hex(const std::string& s) {
    static const char* d = "0123456789abcdef";
    std::string o;
    for (unsigned char c : s) {
        o += d[c >> 4];
        o += d[c & 15];
    }
    return o;
}

struct FrameBench {
    Server server;
    SeenEcho svc;
    bool ok = false;
    FrameBench() {
        ServerOptions so;
        so.has_builtin_services = false;
        ok = server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE) == 0 && server.Start("127.0.0.1:0", &so) == 0;
    }
    ~FrameBench() {
        server.Stop(0);
        server.Join();
    }
    static std::string ReadN(int fd, size_t n) {
        std::string out(n, '\0');
        size_t got = 0;
        const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
        while (got < n && monotonic_us() < deadline) {
            pollfd p{fd, POLLIN, 0};
            if (poll(&p, 1, 50) <= 0) continue;
            const ssize_t r = read(fd, &out[got], n - got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        out.resize(got);
        return out;
    }
    // What the service saw and what went back for one request frame, on a connection of its own.
    std::string Run(const std::string& frame) {
        int fds[2], feed[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0 || socketpair(AF_UNIX, SOCK_STREAM, 0, feed) != 0) return "no socketpair";
        SocketOptions o;
        o.fd = fds[0];
        SocketId sid = INVALID_SOCKET_ID;
        SocketUniquePtr sock;
        std::string outcome;
        if (Socket::Create(o, &sid) != 0 || Socket::Address(sid, &sock) != 0) {
            outcome = "no socket";
        } else {
            BufPortal portal;
            size_t got = 0;
            if (write(feed[1], frame.data(), frame.size()) != (ssize_t)frame.size()) outcome = "feeding failed";
            while (outcome.empty() && got < frame.size()) {
                const ssize_t n = portal.append_from_fd(feed[0], frame.size() - got);
                if (n <= 0) outcome = "feeding failed";
                else got += (size_t)n;
            }
            const Protocol* p = FindProtocol(PROTOCOL_BAIDU_STD);
            if (outcome.empty()) {
                ParseResult r = p->parse(&portal, sock.get(), false, nullptr);
                if (!r.is_ok()) {
                    outcome = std::string("parse error ") + ParseErrorToString(r.error());
                } else {
                    MostCommonMessage* msg = static_cast<MostCommonMessage*>(r.message());
                    {
                        std::lock_guard<std::mutex> g(svc.mu);
                        svc.seen = "not called";
                    }
                    sock->AddRef();
                    msg->_socket.reset(sock.get());
                    msg->_arg = &server;
                    msg->_received_us = monotonic_us();
                    p->process_request(msg);
                    if (sock->Failed()) {
                        outcome = "connection failed";
                    } else {
                        const std::string head = ReadN(fds[1], 12);
                        if (head.size() != 12) {
                            outcome = "no response";
                        } else {
                            const std::string rest = ReadN(fds[1], frame_util::ReadBe32(head.data() + 4));
                            outcome = "response=" + Hex(head + rest);
                        }
                    }
                    std::lock_guard<std::mutex> g(svc.mu);
                    outcome = "service{" + svc.seen + "} " + outcome;
                }
            }
        }
        sock.reset();
        if (sid != INVALID_SOCKET_ID) Socket::SetFailed(sid);
        close(fds[1]);
        close(feed[0]);
        close(feed[1]);
        return outcome;
    }
};

std::string EchoBody(const std::string& text) {
    example::EchoRequest req;
    req.set_message(text);
    return req.SerializeAsString();
}

}  // namespace

TEST(BaiduStdMetaFast, declined_metas_end_as_with_the_flag_off) {
    FrameBench bench;
    ASSERT_TRUE(bench.ok);
    const std::string body = EchoBody("declined");
    size_t accepted = 0;
    for (const MetaCase& c : DeclinedMetas()) {
        policy::ScannedRequestMeta s;
        const std::string copy(c.meta);  // an allocation of exactly its size
        const bool took = policy::ScanPlainRequestMeta(copy.data(), copy.size(), &s);
        if (c.may_accept) {
            if (took) {
                std::string why;
                EXPECT_TRUE_M(GenericAgrees(copy, s, &why), c.name + ": " + why);
                ++accepted;
            }
        } else {
            EXPECT_FALSE_M(took, c.name);
        }
        const std::string frame = frame_util::MakeFrame(c.meta, body, "");
        std::string on, off;
        {
            BoolFlag f(&FLAGS_baidu_std_meta_fast_path, true);
            on = bench.Run(frame);
        }
        {
            BoolFlag f(&FLAGS_baidu_std_meta_fast_path, false);
            off = bench.Run(frame);
        }
        EXPECT_TRUE_M(on == off, c.name + ": on{" + on + "} off{" + off + "}");
        EXPECT_TRUE_M(on.find("service{") == 0, c.name + ": " + on);
    }
    // the response scanner: anything but fields 3, 4 and 5, once each
    const std::string plain = VarintField(3, 1) + VarintField(4, 77) + VarintField(5, 9);
    policy::ScannedResponseMeta r;
    EXPECT_TRUE(policy::ScanPlainResponseMeta(plain.data(), plain.size(), &r));
    const std::string permuted = VarintField(5, 9) + VarintField(4, 77) + VarintField(3, 1);
    EXPECT_TRUE(policy::ScanPlainResponseMeta(permuted.data(), permuted.size(), &r));
    EXPECT_EQ(r.correlation_id, (int64_t)77);
    EXPECT_EQ(r.attachment_size, 9);
    EXPECT_EQ(r.compress_type, 1);
    // behind a whole plain meta: other fields (the error of a failed call
    // among them), duplicates, and a field cut short
    for (const std::string& more :
         {BytesField(1, kNames), BytesField(2, ""), BytesField(2, VarintField(1, 2004)), BytesField(6, ""), BytesField(7, "x"),
          BytesField(8, ""), BytesField(100, ""), BytesField(101, ""), BytesField(102, ""), VarintField(9, 1),
          VarintField(3, 1), VarintField(4, 1), VarintField(5, 1), std::string("\x0a\x05")}) {
        const std::string meta = plain + more;
        EXPECT_FALSE_M(policy::ScanPlainResponseMeta(meta.data(), meta.size(), &r), Hex(meta));
    }
    // in the place of a field of their number: other wire types, a varint of 11 bytes, a tag alone
    for (const std::string& bad :
         {VarintField(4, 77) + BytesField(3, ""), VarintField(3, 1) + Fixed64Field(4), VarintField(4, 77) + Fixed32Field(5),
          VarintField(3, 1) + std::string("\x20") + std::string(10, (char)0x80) + std::string("\0", 1),
          VarintField(4, 77) + std::string("\x18")}) {
        EXPECT_FALSE_M(policy::ScanPlainResponseMeta(bad.data(), bad.size(), &r), Hex(bad));
    }
    EXPECT_FALSE(policy::ScanPlainResponseMeta("", 0, &r));
    for (size_t k = 1; k < plain.size(); ++k) {
        const std::string prefix = plain.substr(0, k);
        // whole fields in front are a whole meta
        const bool whole = k == 2 || k == 4;
        EXPECT_EQ(policy::ScanPlainResponseMeta(prefix.data(), prefix.size(), &r), whole);
    }
}

// -------------------------------------------------------------- which path ran

namespace {

struct Counts {
    int64_t v[policy::META_PATH_COUNTERS];
    static Counts Now() {
        Counts c;
        for (int i = 0; i < policy::META_PATH_COUNTERS; ++i) c.v[i] = policy::MetaPathCount((policy::MetaPathCounter)i);
        return c;
    }
    // "pack request, parse request, pack response, parse response", each F (fast), G (generic), or a count pair
    std::string Since(const Counts& before) const {
        std::string out;
        for (int i = 0; i < policy::META_PATH_COUNTERS; i += 2) {
            const int64_t fast = v[i] - before.v[i], generic = v[i + 1] - before.v[i + 1];
            if (fast == 1 && generic == 0) out += 'F';
            else if (fast == 0 && generic == 1) out += 'G';
            else out += "(" + std::to_string(fast) + "," + std::to_string(generic) + ")";
        }
        return out;
    }
};

class FixedAuth : public Authenticator {
public:
    int GenerateCredential(std::string* auth_str) const override {
        *auth_str = "let-me-in";
        return 0;
    }
    int VerifyCredential(const std::string& auth_str, const EndPoint&, AuthContext*) const override {
        return auth_str == "let-me-in" ? 0 : -1;
    }
};

struct CallSpec {
    std::string message = std::string(32, 'x');
    std::string attachment;
    uint64_t log_id = 0;
    std::string request_id;
    const pb::MethodDescriptor* method = nullptr;  // null: EchoService.Echo
};

struct CallResult {
    int code = 0;
    std::string text, message, attachment;
};

CallResult Call(Channel* ch, const CallSpec& spec) {
    Controller cntl;
    example::EchoRequest req;
    example::EchoResponse res;
    req.set_message(spec.message);
    if (!spec.attachment.empty()) cntl.request_attachment().append(spec.attachment);
    if (spec.log_id) cntl.set_log_id(spec.log_id);
    if (!spec.request_id.empty()) cntl.set_request_id(spec.request_id);
    const pb::MethodDescriptor* md = spec.method ? spec.method : example::EchoService::descriptor()->method(0);
    ch->CallMethod(md, &cntl, &req, &res, nullptr);
    CallResult r;
    r.code = cntl.ErrorCode();
    r.text = cntl.ErrorText();
    r.message = res.message();
    r.attachment = cntl.response_attachment().to_string();
    return r;
}

int InitChannel(Channel* ch, const Server& server, const Authenticator* auth = nullptr, bool device = false) {
    ChannelOptions opt;
    opt.timeout_ms = 10000 * mtest::kSlowdown;
    opt.max_retry = 0;
    opt.auth = auth;
    opt.use_device_transport = device;
    return ch->Init(("127.0.0.1:" + std::to_string(server.listen_port())).c_str(), &opt);
}

// A method of the echo service's shape under other names.
struct OtherMethod {
    pb::ServiceDescriptor sd;
    OtherMethod(const std::string& service_full, const std::string& service_brief, const std::string& method) {
        const pb::MethodDescriptor* echo = example::EchoService::descriptor()->method(0);
        sd.full_name = service_full;
        sd.name = service_brief;
        sd.methods.push_back(*echo);
        sd.methods[0].name = method;
        sd.methods[0].full_name = service_full + "." + method;
        sd.methods[0].service = &sd;
    }
    const pb::MethodDescriptor* md() const { return &sd.methods[0]; }
};

}  // namespace

TEST(BaiduStdMetaFast, counters_say_which_path_each_call_took) {
    BoolFlag on(&FLAGS_baidu_std_meta_fast_path, true);
    FrameBench bench;
    ASSERT_TRUE(bench.ok);
    Channel ch;
    ASSERT_EQ(InitChannel(&ch, bench.server), 0);
    // the first call of a connection offers the plane hello: generic all the way
    Counts c0 = Counts::Now();
    CallResult r = Call(&ch, CallSpec());
    ASSERT_EQ(r.code, 0);
    EXPECT_EQ(Counts::Now().Since(c0), std::string("GGGG"));
    // plain from then on
    c0 = Counts::Now();
    r = Call(&ch, CallSpec());
    EXPECT_EQ(r.code, 0);
    EXPECT_EQ(r.message, std::string(32, 'x'));
    EXPECT_EQ(Counts::Now().Since(c0), std::string("FFFF"));
    {
        CallSpec s;
        s.attachment = "host-attachment";
        c0 = Counts::Now();
        r = Call(&ch, s);
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(r.attachment, s.attachment);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("FFFF"));
    }
    {
        CallSpec s;
        s.log_id = 0xFFFFFFFFFFFFFFFFull;  // -1 on the wire: ten bytes
        c0 = Counts::Now();
        r = Call(&ch, s);
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("FFFF"));
        std::lock_guard<std::mutex> g(bench.svc.mu);
        EXPECT_TRUE_M(bench.svc.seen.find("log_id=18446744073709551615 ") != std::string::npos, bench.svc.seen);
    }
    {
        CallSpec s;
        s.request_id = "rid-9";
        c0 = Counts::Now();
        r = Call(&ch, s);
        EXPECT_EQ(r.code, 0);
        // the reply to it is plain again
        EXPECT_EQ(Counts::Now().Since(c0), std::string("GGFF"));
        std::lock_guard<std::mutex> g(bench.svc.mu);
        EXPECT_TRUE_M(bench.svc.seen.find("request_id=rid-9") != std::string::npos, bench.svc.seen);
    }
    {
        // the short service name on the wire
        BoolFlag brief(&FLAGS_baidu_protocol_use_fullname, false);
        c0 = Counts::Now();
        r = Call(&ch, CallSpec());
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(r.message, std::string(32, 'x'));
        EXPECT_EQ(Counts::Now().Since(c0), std::string("FFFF"));
    }
    {
        // a channel that asks for the device transport, which this connection has not got
        Channel dev;
        ASSERT_EQ(InitChannel(&dev, bench.server, nullptr, true), 0);
        c0 = Counts::Now();
        r = Call(&dev, CallSpec());
        EXPECT_EQ(r.code, 0);
        const std::string path = Counts::Now().Since(c0);
        EXPECT_EQ(path[0], 'G');
    }
    // error replies: the request is plain, the reply is not; text and code are those of the flag off
    OtherMethod no_method("example.EchoService", "EchoService", "Nope");
    OtherMethod no_service("example.NoSuchService", "NoSuchService", "Echo");
    for (const OtherMethod* m : {&no_method, &no_service}) {
        CallSpec s;
        s.method = m->md();
        c0 = Counts::Now();
        r = Call(&ch, s);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("FFGG"));
        EXPECT_EQ(r.code, m == &no_method ? ENOMETHOD : ENOSERVICE);
        BoolFlag off(&FLAGS_baidu_std_meta_fast_path, false);
        c0 = Counts::Now();
        const CallResult r_off = Call(&ch, s);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("GGGG"));
        EXPECT_EQ(r.code, r_off.code);
        EXPECT_EQ(r.text, r_off.text);
        EXPECT_FALSE(r.text.empty());
    }
    {
        // flag off: only the generic counters move
        BoolFlag off(&FLAGS_baidu_std_meta_fast_path, false);
        c0 = Counts::Now();
        CallSpec s;
        s.attachment = "host-attachment";
        r = Call(&ch, s);
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(r.attachment, s.attachment);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("GGGG"));
    }
}

TEST(BaiduStdMetaFast, first_call_with_an_authenticator_is_generic) {
    BoolFlag on(&FLAGS_baidu_std_meta_fast_path, true);
    FixedAuth auth;
    Server server;
    SeenEcho svc;
    ServerOptions so;
    so.has_builtin_services = false;
    so.auth = &auth;
    ASSERT_EQ(server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE), 0);
    ASSERT_EQ(server.Start("127.0.0.1:0", &so), 0);
    {
        Channel ch;
        ASSERT_EQ(InitChannel(&ch, server, &auth), 0);
        Counts c0 = Counts::Now();
        CallResult r = Call(&ch, CallSpec());
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(Counts::Now().Since(c0)[0], 'G');
        // later calls of the connection send no credential
        c0 = Counts::Now();
        r = Call(&ch, CallSpec());
        EXPECT_EQ(r.code, 0);
        EXPECT_EQ(Counts::Now().Since(c0), std::string("FFFF"));
    }
    server.Stop(0);
    server.Join();
}

TEST(BaiduStdMetaFast, twelve_fibers_on_one_connection) {
    BoolFlag on(&FLAGS_baidu_std_meta_fast_path, true);
    FrameBench bench;
    ASSERT_TRUE(bench.ok);
    Channel ch;
    ASSERT_EQ(InitChannel(&ch, bench.server), 0);
    const int kFibers = 12, kEach = 2000;
    const Counts c0 = Counts::Now();
    std::atomic<int> mismatches{0}, failures{0};
    std::vector<fiber::fiber_t> ts(kFibers);
    for (int f = 0; f < kFibers; ++f) {
        ASSERT_EQ(fiber::start(
                      [&, f] {
                          for (int i = 0; i < kEach; ++i) {
                              CallSpec s;
                              s.message = "fiber " + std::to_string(f) + " call " + std::to_string(i);
                              if (i % 3 == 0) s.attachment = "att-" + s.message;
                              if (i % 5 == 0) s.log_id = (uint64_t)(f * kEach + i + 1);
                              if (i % 7 == 0) s.request_id = "rid";
                              const CallResult r = Call(&ch, s);
                              if (r.code != 0) failures.fetch_add(1);
                              else if (r.message != s.message || r.attachment != s.attachment) mismatches.fetch_add(1);
                          }
                      },
                      false, nullptr, &ts[f]),
                  0);
    }
    for (fiber::fiber_t t : ts) fiber::join(t, nullptr);
    EXPECT_EQ(failures.load(), 0);
    EXPECT_EQ(mismatches.load(), 0);
    const Counts c1 = Counts::Now();
    const int64_t calls = (int64_t)kFibers * kEach;
    int64_t fast = 0;
    for (int i = 0; i < policy::META_PATH_COUNTERS; i += 2) {
        EXPECT_EQ(c1.v[i] - c0.v[i] + c1.v[i + 1] - c0.v[i + 1], calls);
        fast += c1.v[i] - c0.v[i];
    }
    EXPECT_GT(fast, calls * 3);  // most legs of most calls
}

// ---------------------------------------------------------------------- lookup

TEST(BaiduStdMetaFast, lookup_by_views_agrees_with_lookup_by_strings) {
    Server server;
    SeenEcho svc;
    ASSERT_EQ(server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE), 0);
    struct Pair {
        std::string service, method;
        bool found;
    };
    const std::string long_name(300, 'n');
    for (const Pair& p : {Pair{"example.EchoService", "Echo", true}, Pair{"EchoService", "Echo", true},
                          Pair{"example.NoSuchService", "Echo", false}, Pair{"NoSuchService", "Echo", false},
                          Pair{"example.EchoService", "Nope", false}, Pair{"EchoService", "Nope", false},
                          Pair{"", "", false}, Pair{"example.EchoService", "", false}, Pair{"", "Echo", false},
                          Pair{"example", "EchoService.Echo", true}, Pair{long_name, long_name, false}}) {
        // views of bytes that end where the name ends
        const std::string framed = "<" + p.service + "|" + p.method + ">";
        const std::string_view service(framed.data() + 1, p.service.size());
        const std::string_view method(framed.data() + 2 + p.service.size(), p.method.size());
        const Server::MethodProperty* by_view = server.FindMethodPropertyByFullName(service, method);
        const Server::MethodProperty* by_string = server.FindMethodPropertyByFullName(p.service, p.method);
        EXPECT_TRUE_M(by_view == by_string, p.service + " / " + p.method);
        EXPECT_TRUE_M((by_view != nullptr) == p.found, p.service + " / " + p.method);
        if (by_view) EXPECT_TRUE(by_view->service == &svc);
    }
    EXPECT_TRUE(server.FindMethodPropertyByFullName("example.EchoService.Echo") != nullptr);
    // the index follows the services
    ASSERT_EQ(server.RemoveService(&svc), 0);
    EXPECT_TRUE(server.FindMethodPropertyByFullName(std::string_view("example.EchoService"), std::string_view("Echo")) == nullptr);
    ASSERT_EQ(server.AddService(&svc, SERVER_DOESNT_OWN_SERVICE), 0);
    EXPECT_TRUE(server.FindMethodPropertyByFullName(std::string_view("EchoService"), std::string_view("Echo")) != nullptr);
    server.ClearServices();
    EXPECT_TRUE(server.FindMethodPropertyByFullName(std::string_view("EchoService"), std::string_view("Echo")) == nullptr);
}

// --------------------------------------------------------------- receive stamp

namespace {

struct Stamps {
    std::mutex mu;
    std::vector<int64_t> received_us;
    std::atomic<int> n{0};
};

ParseResult ParseFourBytes(Buf* source, Socket*, bool, const void*) {
    if (source->size() < 4) return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    MostCommonMessage* msg = MostCommonMessage::Get();
    source->cutn(&msg->payload, 4);
    return MakeMessage(msg);
}

void ProcessStamp(InputMessageBase* base) {
    MostCommonMessage* msg = static_cast<MostCommonMessage*>(base);
    Stamps* s = const_cast<Stamps*>(static_cast<const Stamps*>(msg->arg()));
    {
        std::lock_guard<std::mutex> g(s->mu);
        s->received_us.push_back(msg->received_us());
    }
    msg->Destroy();
    s->n.fetch_add(1, std::memory_order_release);
}

}  // namespace

TEST(BaiduStdMetaFast, messages_of_one_read_carry_one_receive_stamp) {
    // never destroyed: a reader fiber may still be leaving OnNewMessages
    static Stamps* stamps = new Stamps;
    static InputMessenger* messenger = [] {
        InputMessenger* m = new InputMessenger;
        InputMessageHandler h;
        h.parse = ParseFourBytes;
        h.process = ProcessStamp;
        h.arg = stamps;
        h.name = "four_bytes";
        m->AddHandler(h);
        return m;
    }();
    int fds[2];
    ASSERT_EQ(socketpair(AF_UNIX, SOCK_STREAM, 0, fds), 0);
    const int64_t before = monotonic_us();
    // both frames are there before the reader exists: its first read takes them together
    ASSERT_EQ(write(fds[1], "aaaabbbb", 8), (ssize_t)8);
    SocketOptions o;
    o.fd = fds[0];
    SocketId id = INVALID_SOCKET_ID;
    ASSERT_EQ(messenger->Create(o, &id), 0);
    const int64_t deadline = monotonic_us() + 5000000LL * mtest::kSlowdown;
    while (stamps->n.load(std::memory_order_acquire) < 2 && monotonic_us() < deadline) usleep(200);
    const int64_t after = monotonic_us();
    ASSERT_EQ(stamps->n.load(), 2);
    {
        std::lock_guard<std::mutex> g(stamps->mu);
        EXPECT_EQ(stamps->received_us[0], stamps->received_us[1]);
        EXPECT_GE(stamps->received_us[0], before);
        EXPECT_LE(stamps->received_us[0], after);
    }
    Socket::SetFailed(id);
    close(fds[1]);
}
