// baidu_std protocol (role of src/brpc/policy/baidu_rpc_protocol.cpp:57-767):
//   "PRPC" | body_size (u32 BE) | meta_size (u32 BE) | RpcMeta | payload | attachment
// MI355X-native: attachment blocks that live in HBM are moved by the
// socket's device transport and described in RpcMeta.device_payload
// (policy/device_payload.h); everything else is byte-identical to baidu_std.
#include <cerrno>
#include <memory>

#include "base/flags.h"
#include "base/logging.h"
#include "base/time.h"
#include "base/util.h"
#include "fiber/call_id.h"
#include "gpu/rccl_plane.h"
#include "gpu/xgmi.h"
#include "mrpc/proto/rpc_meta.pb.h"
#include "policy/baidu_std_meta.h"
#include "policy/device_payload.h"
#include "policy/policies.h"
#include "rpc/controller.h"
#include "rpc/errno.h"
#include "rpc/protocol.h"
#include "rpc/server.h"
#include "rpc/span.h"
#include "rpc/rpc_dump.h"
#include "rpc/stream_internal.h"
#include "rpc/usercode_backup_pool.h"

DECLARE_uint64(max_body_size);
DEFINE_bool(baidu_protocol_use_fullname, true, "put the full service name in requests");
DEFINE_bool(baidu_std_protocol_deliver_timeout_ms, false, "put timeout_ms in request meta");

namespace mrpc {
namespace policy {

static inline void PackRpcHeader(char* h, uint32_t meta_size, uint32_t payload_size) {
    memcpy(h, "PRPC", 4);
    pack_be32(h + 4, meta_size + payload_size);
    pack_be32(h + 8, meta_size);
}

void SerializeRpcHeaderAndMeta(Buf* out, const RpcMeta& meta, size_t payload_size) {
    const uint32_t meta_size = (uint32_t)meta.ByteSizeLong();
    char* p = out->append_contiguous(12 + meta_size);
    PackRpcHeader(p, meta_size, (uint32_t)payload_size);
    meta.SerializeWithCachedSizesToArray((uint8_t*)p + 12);
}

ParseResult ParseRpcMessage(Buf* source, Socket* socket, bool, const void*) {
    char header[12];
    const size_t n = source->copy_to(header, sizeof(header));
    if (n >= 4) {
        if (memcmp(header, "PRPC", 4) != 0) return MakeParseError(PARSE_ERROR_TRY_OTHERS);
    } else {
        if (memcmp(header, "PRPC", n) != 0) return MakeParseError(PARSE_ERROR_TRY_OTHERS);
        return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    }
    if (n < sizeof(header)) return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    const uint32_t body_size = unpack_be32(header + 4);
    const uint32_t meta_size = unpack_be32(header + 8);
    if (body_size > FLAGS_max_body_size) {
        LOG(ERROR) << "body_size=" << body_size << " from " << socket->remote_side() << " is too large";
        return MakeParseError(PARSE_ERROR_TOO_BIG_DATA);
    }
    if (source->size() < sizeof(header) + body_size) return MakeParseError(PARSE_ERROR_NOT_ENOUGH_DATA);
    if (meta_size > body_size) {
        LOG(ERROR) << "meta_size=" << meta_size << " is bigger than body_size=" << body_size;
        source->pop_front(sizeof(header) + body_size);
        return MakeParseError(PARSE_ERROR_ABSOLUTELY_WRONG);
    }
    source->pop_front(sizeof(header));
    // One cut for meta and payload: each Buf cut here takes references of
    // the read blocks that a worker gives back, on lines both of them write.
    MostCommonMessage* msg = MostCommonMessage::Get();
    source->cutn(&msg->payload, body_size);
    msg->meta_size = meta_size;
    return MakeMessage(msg);
}

// Parses the RpcMeta at the front of a frame cut by ParseRpcMessage: in place
// when one block holds it, else through the Buf parser. The frame is left as
// it is; the caller pops meta_size bytes to get at the payload.
static bool ParseFrameMeta(RpcMeta* meta, const MostCommonMessage* msg) {
    const size_t n = msg->meta_size;
    const Buf& frame = msg->payload;
    if (n > FLAGS_max_body_size || n > frame.size()) return false;
    if (n == 0) return meta->ParseFromArray("", 0);
    if (frame.block_len(0) >= n && IsHostAccessible(frame.ref_at(0).block->kind)) {
        return meta->ParseFromArray(frame.block_data(0), n);
    }
    Buf copy(frame), spanning;
    copy.cutn(&spanning, n);
    return ParsePbFromBuf(meta, spanning);
}

void SerializeRpcRequest(Buf* buf, Controller* cntl, const pb::Message* request) {
    if (!request) {
        cntl->SetFailed(EREQUEST, "request is NULL");
        return;
    }
    if (!request->IsInitialized()) {
        cntl->SetFailed(EREQUEST, "Missing required fields in request: %s", request->InitializationErrorString().c_str());
        return;
    }
    if (!SerializeAsCompressedData(*request, buf, cntl->request_compress_type())) {
        cntl->SetFailed(EREQUEST, "Fail to compress request");
    }
}

// A request is plain when its meta holds nothing but the names, log_id,
// timeout_ms, compress type, correlation id and attachment size: no
// credential, stream, trace, request_id, hello or device payload.
static bool IsPlainRequest(const Controller* cntl, const Authenticator* auth) {
    if (auth || cntl->_request_stream || cntl->trace_id() || !cntl->request_id().empty()) return false;
    Socket* const sock = cntl->_pack_socket;
    if (sock) {
        if (sock->plane_rank() == Socket::kPlaneUnknown) return false;         // a plane hello is due
        if (cntl->_use_device_transport && !sock->transport()) return false;  // an xGMI hello is due
    }
    if (cntl->_packed_payloads && cntl->_packed_payloads->descs.size() > 0) return false;
    return AttachmentStaysInline(sock, cntl->request_attachment(), cntl->verify_device_payload());
}

static void PackPlainRpcRequest(Buf* packet, uint64_t correlation_id, const pb::MethodDescriptor* method,
                                const Controller* cntl, const Buf& request_buf) {
    const pb::MethodWireNames* names = method->wire_names();
    const Buf& attachment = cntl->request_attachment();
    PlainRequestMeta m;
    m.name_fields = FLAGS_baidu_protocol_use_fullname ? names->full : names->brief;
    m.has_log_id = cntl->log_id() != 0;
    m.log_id = (int64_t)cntl->log_id();
    if (FLAGS_baidu_std_protocol_deliver_timeout_ms && cntl->timeout_ms() > 0) m.timeout_ms = (int32_t)cntl->timeout_ms();
    m.compress_type = cntl->request_compress_type();
    m.correlation_id = (int64_t)correlation_id;
    m.attachment_size = (int32_t)attachment.size();
    PackPlainRequestMeta(packet, m, request_buf.size() + attachment.size());
    packet->append(request_buf);
    packet->append(attachment);
}

void PackRpcRequest(Buf* packet, uint64_t correlation_id, const pb::MethodDescriptor* method, Controller* cntl,
                    const Buf& request_buf, const Authenticator* auth) {
    if (!method) {
        cntl->SetFailed(EREQUEST, "method is NULL");
        return;
    }
    if (MetaFastPathEnabled() && IsPlainRequest(cntl, auth)) {
        PackPlainRpcRequest(packet, correlation_id, method, cntl, request_buf);
        CountMetaPath(META_REQUEST_PACKED_FAST);
        return;
    }
    CountMetaPath(META_REQUEST_PACKED_GENERIC);
    RpcMeta meta;
    RpcRequestMeta* rm = meta.mutable_request();
    rm->set_service_name(FLAGS_baidu_protocol_use_fullname ? method->service->full_name : method->service->name);
    rm->set_method_name(method->name);
    meta.set_compress_type(cntl->request_compress_type());
    meta.set_correlation_id((int64_t)correlation_id);
    if (cntl->log_id()) rm->set_log_id((int64_t)cntl->log_id());
    if (cntl->trace_id()) {
        rm->set_trace_id((int64_t)cntl->trace_id());
        rm->set_span_id((int64_t)cntl->span_id());
        if (cntl->_parent_span_id) rm->set_parent_span_id((int64_t)cntl->_parent_span_id);
    }
    if (!cntl->request_id().empty()) rm->set_request_id(cntl->request_id());
    if (FLAGS_baidu_std_protocol_deliver_timeout_ms && cntl->timeout_ms() > 0) rm->set_timeout_ms((int32_t)cntl->timeout_ms());
    if (auth) {
        std::string cred;
        if (auth->GenerateCredential(&cred) != 0) {
            cntl->SetFailed(ERPCAUTH, "Fail to generate credential");
            return;
        }
        meta.set_authentication_data(cred);
    }
    StreamId sid = cntl->_request_stream;
    if (sid) FillStreamSettings(sid, meta.mutable_stream_settings());
    // xGMI hello: offered on every request until the connection has a
    // device transport, so each response that could carry device payloads
    // also carries the server's arena description.
    if (cntl->_use_device_transport && cntl->_pack_socket && !cntl->_pack_socket->transport()) {
        gpu::FillXgmiHello(meta.mutable_xgmi_hello());
    }
    // RCCL plane hello: offered until a response told us whether the
    // server is a rank of our plane
    if (cntl->_pack_socket && cntl->_pack_socket->plane_rank() == Socket::kPlaneUnknown) {
        gpu::rccl::FillHello(meta.mutable_plane_hello());
    }
    Buf host_attachment;
    if (!SplitDevicePayload(cntl, /*request=*/true, cntl->request_attachment(), &host_attachment, &meta)) return;
    if (host_attachment.size()) meta.set_attachment_size((int32_t)host_attachment.size());
    SerializeRpcHeaderAndMeta(packet, meta, request_buf.size() + host_attachment.size());
    packet->append(request_buf);
    packet->append(std::move(host_attachment));
}

// Header, meta, body and attachment of a response through an RpcMeta
// message: whatever a plain reply cannot say.
static void PackGenericRpcResponse(Buf* packet, int64_t correlation_id, Controller* cntl, Socket* sock, Buf* res_body_in) {
    Buf& res_body = *res_body_in;
    RpcMeta meta;
    Buf host_attachment;
    if (cntl->Failed()) {
        meta.mutable_response()->set_error_code(cntl->ErrorCode());
        meta.mutable_response()->set_error_text(cntl->ErrorText());
        res_body.clear();
    } else {
        meta.set_compress_type(cntl->response_compress_type());
        if (!SplitDevicePayload(cntl, /*request=*/false, cntl->response_attachment(), &host_attachment, &meta, sock)) {
            res_body.clear();
            meta.Clear();
            meta.mutable_response()->set_error_code(cntl->ErrorCode());
            meta.mutable_response()->set_error_text(cntl->ErrorText());
        } else if (host_attachment.size()) {
            meta.set_attachment_size((int32_t)host_attachment.size());
        }
    }
    meta.set_correlation_id(correlation_id);
    if (cntl->_reply_xgmi_hello) gpu::FillXgmiHello(meta.mutable_xgmi_hello());
    if (cntl->_reply_plane_hello) gpu::rccl::FillHello(meta.mutable_plane_hello());
    if (cntl->_response_stream) FillStreamSettings(cntl->_response_stream, meta.mutable_stream_settings());
    SerializeRpcHeaderAndMeta(packet, meta, res_body.size() + host_attachment.size());
    packet->append(std::move(res_body));
    packet->append(std::move(host_attachment));
}

static void SendRpcResponse(int64_t correlation_id, Controller* cntl, pb::Message* req, pb::Message* res,
                            Server* server, MethodStatus* method_status, int64_t received_us) {
    std::unique_ptr<Controller> cntl_guard(cntl);
    std::unique_ptr<pb::Message> req_guard(req);
    std::unique_ptr<pb::Message> res_guard(res);
    ConcurrencyRemover remover(method_status, cntl, received_us, server);
    SocketUniquePtr addressed;
    Socket* const sock = cntl->ServerSocketForResponse(&addressed);
    if (!sock) return;  // client gone
    if (cntl->IsCloseConnection()) {
        sock->SetFailed(ECLOSE, "close connection by user");
        return;
    }
    Span* span = cntl->_span;
    if (span) span->start_send_real_us = realtime_us();
    Buf res_body;
    if (!cntl->Failed() && res) {
        if (!res->IsInitialized()) {
            cntl->SetFailed(ERESPONSE, "Missing required fields in response: %s", res->InitializationErrorString().c_str());
        } else if (!SerializeAsCompressedData(*res, &res_body, cntl->response_compress_type())) {
            cntl->SetFailed(ERESPONSE, "Fail to serialize response");
        }
    }
    Buf packet;
    // A reply is plain when its meta holds nothing but compress type,
    // correlation id and attachment size: no error, hello, stream or
    // device payload.
    if (MetaFastPathEnabled() && !cntl->Failed() && !cntl->_reply_xgmi_hello && !cntl->_reply_plane_hello &&
        !cntl->_response_stream &&
        AttachmentStaysInline(sock, cntl->response_attachment(), cntl->verify_device_payload())) {
        const Buf& attachment = cntl->response_attachment();
        PlainResponseMeta m;
        m.compress_type = cntl->response_compress_type();
        m.correlation_id = correlation_id;
        m.attachment_size = (int32_t)attachment.size();
        PackPlainResponseMeta(&packet, m, res_body.size() + attachment.size());
        packet.append(std::move(res_body));
        packet.append(attachment);
        CountMetaPath(META_RESPONSE_PACKED_FAST);
    } else {
        CountMetaPath(META_RESPONSE_PACKED_GENERIC);
        PackGenericRpcResponse(&packet, correlation_id, cntl, sock, &res_body);
    }
    if (span) span->response_size = (int64_t)packet.size();
    WriteOptions wopt;
    wopt.ignore_eovercrowded = true;
    if (sock->Write(&packet, &wopt) != 0) {
        LOG_EVERY_SECOND(WARNING) << "Fail to write response into " << sock->description();
    }
    if (cntl->_response_stream) OnServerStreamCreated(cntl->_response_stream, sock->id());
    if (span) {
        span->sent_real_us = realtime_us();
        span->error_code = cntl->ErrorCode();
        Span::Submit(span, monotonic_us());
        cntl->_span = nullptr;
    }
}

// The meta bytes of a frame when its first block holds them all in host
// memory (what the scanners read); null when they span blocks.
static const char* ContiguousFrameMeta(const MostCommonMessage* msg) {
    const size_t n = msg->meta_size;
    const Buf& frame = msg->payload;
    if (n == 0 || n > frame.size() || frame.block_len(0) < n || !IsHostAccessible(frame.ref_at(0).block->kind)) return nullptr;
    return frame.block_data(0);
}

// What a request's meta says, from the scanner or from the parsed message.
// The names are views of the frame (scanned) or of *meta (parsed).
struct RequestHead {
    ScannedRequestMeta s;
    bool has_request = false;
    const RpcMeta* meta = nullptr;  // parsed metas only: whatever a plain one cannot say
};

static void ProcessRpcRequestWithHead(MostCommonMessage* msg, const RequestHead& head, int64_t start_parse_us);

void ProcessRpcRequest(InputMessageBase* msg_base) {
    const int64_t start_parse_us = monotonic_us();
    MostCommonMessage* msg = static_cast<MostCommonMessage*>(msg_base);
    RequestHead head;
    if (MetaFastPathEnabled()) {
        const char* bytes = ContiguousFrameMeta(msg);
        if (bytes && ScanPlainRequestMeta(bytes, msg->meta_size, &head.s)) {
            CountMetaPath(META_REQUEST_PARSED_FAST);
            head.has_request = true;
            ProcessRpcRequestWithHead(msg, head, start_parse_us);
            return;
        }
    }
    CountMetaPath(META_REQUEST_PARSED_GENERIC);
    RpcMeta meta;
    if (!ParseFrameMeta(&meta, msg)) {
        Socket* socket = msg->socket();
        LOG(WARNING) << "Fail to parse RpcMeta from " << socket->remote_side();
        socket->SetFailed(EREQUEST, "fail to parse RpcMeta");
        msg->Destroy();
        return;
    }
    const RpcRequestMeta& rm = meta.request();
    head.s = ScannedRequestMeta();  // a declined scan may have left values behind
    head.s.service_name = rm.service_name();
    head.s.method_name = rm.method_name();
    head.s.has_log_id = rm.has_log_id();
    head.s.log_id = rm.log_id();
    head.s.has_timeout_ms = rm.has_timeout_ms();
    head.s.timeout_ms = rm.timeout_ms();
    head.s.compress_type = meta.compress_type();
    head.s.correlation_id = meta.correlation_id();
    head.s.attachment_size = meta.attachment_size();
    head.has_request = meta.has_request();
    head.meta = &meta;
    ProcessRpcRequestWithHead(msg, head, start_parse_us);
}

// The frame stays whole (meta in front) until the names have been used: a
// scanned head's names are views of the meta bytes.
static void ProcessRpcRequestWithHead(MostCommonMessage* msg, const RequestHead& head, int64_t start_parse_us) {
    struct Destroyer {
        MostCommonMessage* m;
        ~Destroyer() { if (m) m->Destroy(); }
    } destroyer{msg};
    Socket* socket = msg->socket();
    Server* server = const_cast<Server*>(static_cast<const Server*>(msg->arg()));
    const RpcMeta* const gm = head.meta;
    const ScannedRequestMeta& rm = head.s;
    const size_t payload_size = msg->payload.size() - msg->meta_size;  // body and attachment
    Controller* cntl = new Controller;
    cntl->_server = server;
    cntl->_server_socket_id = socket->id();
    cntl->_remote_side = socket->remote_side();
    cntl->_local_side = socket->local_side();
    cntl->_server_correlation_id = rm.correlation_id;
    cntl->_received_us = msg->received_us();
    cntl->_begin_us = msg->received_us();
    if (rm.has_log_id) cntl->set_log_id((uint64_t)rm.log_id);
    cntl->set_request_compress_type((CompressType)rm.compress_type);
    if (gm && gm->request().has_request_id()) cntl->set_request_id(gm->request().request_id());
    if (rm.has_timeout_ms && rm.timeout_ms > 0) cntl->_deadline_us = msg->received_us() + (int64_t)rm.timeout_ms * 1000;
    if (IsRpczEnabled()) {
        // a plain meta has no trace ids: zeros, as absent fields read
        const RpcRequestMeta& ids = gm ? gm->request() : RpcRequestMeta::default_instance();
        cntl->_span = Span::CreateServerSpan((uint64_t)ids.trace_id(), (uint64_t)ids.span_id(), (uint64_t)ids.parent_span_id(),
                                             std::string(rm.service_name) + "." + std::string(rm.method_name),
                                             realtime_us() - (monotonic_us() - msg->received_us()));
        if (cntl->_span) {
            cntl->_span->remote_side = socket->remote_side();
            cntl->_span->start_parse_real_us = realtime_us();
            cntl->_span->request_size = (int64_t)(msg->meta_size + payload_size + 12);
            cntl->_span->log_id = (uint64_t)rm.log_id;
            cntl->_trace_id = cntl->_span->trace_id;
            cntl->_span_id = cntl->_span->span_id;
        }
    }
    if (gm && gm->has_xgmi_hello() && gpu::XgmiEnabled()) {
        std::string err;
        if (gpu::AttachXgmiPeer(socket, gm->xgmi_hello(), &err) == 0) {
            cntl->_reply_xgmi_hello = true;
        } else {
            LOG_EVERY_SECOND(WARNING) << "xGMI peer " << socket->remote_side() << " not attached: " << err;
        }
    }
    if (gm && gm->has_plane_hello()) {
        socket->set_plane_rank(gpu::rccl::PeerRank(gm->plane_hello()));
        cntl->_reply_plane_hello = true;
    }
    if (SampledRequest* sample = AskToBeSampled()) {
        sample->meta.set_service_name(std::string(rm.service_name));
        sample->meta.set_method_name(std::string(rm.method_name));
        sample->meta.set_compress_type((CompressType)rm.compress_type);
        sample->meta.set_protocol_type(PROTOCOL_BAIDU_STD);
        sample->meta.set_attachment_size(rm.attachment_size);
        if (gm && gm->has_authentication_data()) sample->meta.set_authentication_data(gm->authentication_data());
        sample->request = msg->payload;  // shares the blocks
        sample->request.pop_front(msg->meta_size);
        sample->submit();
    }
    const int64_t corr = rm.correlation_id;
    MethodStatus* ms = nullptr;
    pb::Message* req = nullptr;
    pb::Message* res = nullptr;
    bool concurrency_added = false;
    bool device_payload_taken = false;  // pulled, or released by the merge on failure
    const Server::MethodProperty* mp = nullptr;
    do {
        if (!server->IsRunning()) {
            cntl->SetFailed(ELOGOFF, "Server is stopping");
            break;
        }
        if (!server->AddConcurrency(cntl)) {
            cntl->SetFailed(ELIMIT, "Reached server's max_concurrency=%d", server->max_concurrency());
            break;
        }
        concurrency_added = true;
        if (!head.has_request) {
            cntl->SetFailed(EREQUEST, "RpcMeta has no request meta");
            break;
        }
        mp = server->FindMethodPropertyByFullName(rm.service_name, rm.method_name);
        if (!mp) {
            const std::string service(rm.service_name), method(rm.method_name);
            if (!server->FindServiceByFullName(service) && !server->FindServiceByName(service)) {
                cntl->SetFailed(ENOSERVICE, "Fail to find service=%s", service.c_str());
            } else {
                cntl->SetFailed(ENOMETHOD, "Fail to find method=%s of service=%s", method.c_str(), service.c_str());
            }
            break;
        }
        int rejected = 0;
        if (!mp->status->OnRequested(&rejected, cntl)) {
            ms = nullptr;
            mp->status->OnResponded(ELIMIT, 0);
            cntl->SetFailed(ELIMIT, "Reached method's max_concurrency=%d", rejected - 1);
            break;
        }
        ms = mp->status.get();
        msg->payload.pop_front(msg->meta_size);  // the names are not looked at again
        Buf req_buf;
        const int attach_size = rm.attachment_size;
        if (attach_size > 0) {
            if ((size_t)attach_size > msg->payload.size()) {
                cntl->SetFailed(EREQUEST, "attachment_size=%d is larger than payload=%zu", attach_size, msg->payload.size());
                break;
            }
            msg->payload.cutn(&req_buf, msg->payload.size() - attach_size);
            cntl->request_attachment().swap(msg->payload);
        } else {
            req_buf.swap(msg->payload);
        }
        device_payload_taken = true;
        if (gm && gm->device_payload_size() > 0) {
            Span::set_tls_parent(cntl->_span);  // rpcz: annotate the xGMI pull
            if (!MergeDevicePayload(cntl, socket, *gm, /*request=*/true, &cntl->request_attachment())) break;
        }
        if (gm && gm->has_stream_settings()) OnRequestStreamSettings(cntl, socket, gm->stream_settings());
        req = mp->service->GetRequestPrototype(mp->method).New();
        if (!ParseFromCompressedData(req_buf, req, (CompressType)rm.compress_type)) {
            cntl->SetFailed(EREQUEST, "Fail to parse request message, CompressType=%d, size=%zu", rm.compress_type,
                            req_buf.size());
            break;
        }
        res = mp->service->GetResponsePrototype(mp->method).New();
    } while (false);
    // rejected before the attachment was looked at: the sender's lent HBM
    // blocks must still be given back, or they stay pinned on its side
    if (gm && !device_payload_taken) ReleaseDevicePayload(socket, *gm);
    cntl->_server_socket = std::move(msg->socket_ptr());  // the message's reference stays with the call
    msg->Destroy();
    destroyer.m = nullptr;
    if (!concurrency_added) server = nullptr;  // nothing to remove
    if (cntl->Failed()) {
        SendRpcResponse(corr, cntl, req, res, server, ms, start_parse_us);
        return;
    }
    if (cntl->_span) cntl->_span->start_callback_real_us = realtime_us();
    Span::set_tls_parent(cntl->_span);
    Closure* done = NewCallback([corr, cntl, req, res, server, ms, start_parse_us] {
        SendRpcResponse(corr, cntl, req, res, server, ms, start_parse_us);
    });
    CallServiceMethod(mp->service, mp->method, cntl, req, res, done);
}

bool VerifyRpcRequest(const InputMessageBase* msg_base) {
    const MostCommonMessage* msg = static_cast<const MostCommonMessage*>(msg_base);
    const Server* server = static_cast<const Server*>(msg->arg());
    const Authenticator* auth = server->options().auth;
    if (!auth) return true;
    RpcMeta meta;
    if (!ParseFrameMeta(&meta, msg)) return false;
    AuthContext ctx;
    return auth->VerifyCredential(meta.authentication_data(), msg->socket()->remote_side(), &ctx) == 0;
}

// `gm`: the parsed meta, null for a scanned (plain) one, which has nothing
// but the three values of `rm`. The frame's meta bytes are popped already.
static void ProcessRpcResponseWithMeta(MostCommonMessage* msg, const ScannedResponseMeta& rm, const RpcMeta* gm);

void ProcessRpcResponse(InputMessageBase* msg_base) {
    MostCommonMessage* msg = static_cast<MostCommonMessage*>(msg_base);
    ScannedResponseMeta rm;
    if (MetaFastPathEnabled()) {
        const char* bytes = ContiguousFrameMeta(msg);
        if (bytes && ScanPlainResponseMeta(bytes, msg->meta_size, &rm)) {
            CountMetaPath(META_RESPONSE_PARSED_FAST);
            msg->payload.pop_front(msg->meta_size);
            ProcessRpcResponseWithMeta(msg, rm, nullptr);
            return;
        }
    }
    CountMetaPath(META_RESPONSE_PARSED_GENERIC);
    RpcMeta meta;
    if (!ParseFrameMeta(&meta, msg)) {
        LOG(WARNING) << "Fail to parse RpcMeta from " << msg->socket()->remote_side();
        msg->Destroy();
        return;
    }
    msg->payload.pop_front(msg->meta_size);
    if (meta.has_stream_settings() && !meta.has_correlation_id()) {
        ReleaseDevicePayload(msg->socket(), meta);
        msg->Destroy();
        return;
    }
    rm.compress_type = meta.compress_type();
    rm.correlation_id = meta.correlation_id();
    rm.attachment_size = meta.attachment_size();
    ProcessRpcResponseWithMeta(msg, rm, &meta);
}

static void ProcessRpcResponseWithMeta(MostCommonMessage* msg, const ScannedResponseMeta& rm, const RpcMeta* gm) {
    const fiber::CallId cid{(uint64_t)rm.correlation_id};
    Controller* cntl = nullptr;
    if (fiber::call_id_lock(cid, (void**)&cntl) != 0) {
        if (gm) ReleaseDevicePayload(msg->socket(), *gm);
        msg->Destroy();  // timed out / canceled / duplicated response
        return;
    }
    if (cid != cntl->current_id() && cid != cntl->_unfinished_call.id) {
        fiber::call_id_unlock(cid);  // response of an obsolete attempt
        if (gm) ReleaseDevicePayload(msg->socket(), *gm);
        msg->Destroy();
        return;
    }
    if (cntl->_span) {
        const int64_t now = realtime_us();
        cntl->_span->start_parse_real_us = now;
        cntl->_span->cut_real_us = now - (monotonic_us() - msg->received_us());
    }
    if (gm && gm->has_xgmi_hello() && gpu::XgmiEnabled()) {
        std::string err;
        if (gpu::AttachXgmiPeer(msg->socket(), gm->xgmi_hello(), &err) != 0) {
            LOG_EVERY_SECOND(WARNING) << "xGMI peer " << msg->socket()->remote_side() << " not attached: " << err;
        }
    }
    if (msg->socket()->plane_rank() == Socket::kPlaneUnknown) {
        msg->socket()->set_plane_rank(gm && gm->has_plane_hello() ? gpu::rccl::PeerRank(gm->plane_hello()) : -1);
    }
    msg->socket()->DeviceHelloAnswered();  // requests waiting to learn the transports go ahead
    int saved_error = 0;
    bool device_payload_taken = false;
    if (gm && gm->response().error_code() != 0) {
        const RpcResponseMeta& failure = gm->response();
        cntl->_error_code = 0;
        cntl->_error_text.clear();
        cntl->SetFailed(failure.error_code(), "%s", failure.error_text().c_str());
        saved_error = failure.error_code();
    } else {
        Buf res_buf;
        const int attach_size = rm.attachment_size;
        cntl->response_attachment().clear();
        if (attach_size > 0) {
            if ((size_t)attach_size > msg->payload.size()) {
                cntl->SetFailed(ERESPONSE, "attachment_size=%d > payload", attach_size);
                saved_error = ERESPONSE;
            } else {
                msg->payload.cutn(&res_buf, msg->payload.size() - attach_size);
                cntl->response_attachment().swap(msg->payload);
            }
        } else {
            res_buf.swap(msg->payload);
        }
        if (!saved_error && gm && gm->device_payload_size() > 0) {
            device_payload_taken = true;
            Span* const prev_span = Span::tls_parent();
            Span::set_tls_parent(cntl->_span);  // rpcz: annotate the xGMI pull
            if (!MergeDevicePayload(cntl, msg->socket(), *gm, /*request=*/false, &cntl->response_attachment())) {
                saved_error = cntl->ErrorCode();
            }
            Span::set_tls_parent(prev_span);
        }
        if (!saved_error && gm && gm->has_stream_settings()) OnResponseStreamSettings(cntl, msg->socket(), gm->stream_settings());
        if (!saved_error && cntl->_response &&
            !ParseFromCompressedData(res_buf, cntl->_response, (CompressType)rm.compress_type)) {
            cntl->SetFailed(ERESPONSE, "Fail to parse response message, CompressType=%d, size=%zu", rm.compress_type,
                            res_buf.size());
            saved_error = ERESPONSE;
        }
        if (!saved_error) cntl->set_response_compress_type((CompressType)rm.compress_type);
    }
    if (gm && !device_payload_taken) ReleaseDevicePayload(msg->socket(), *gm);
    cntl->_local_side = msg->socket()->local_side();
    msg->Destroy();
    cntl->OnVersionedRPCReturned(cid, saved_error);
}

void RegisterBaiduStdProtocol() {
    Protocol p;
    p.parse = ParseRpcMessage;
    p.serialize_request = SerializeRpcRequest;
    p.pack_request = PackRpcRequest;
    p.process_request = ProcessRpcRequest;
    p.process_response = ProcessRpcResponse;
    p.verify = VerifyRpcRequest;
    p.supported_connection_type = CONNECTION_TYPE_SINGLE | CONNECTION_TYPE_POOLED | CONNECTION_TYPE_SHORT;
    p.name = "baidu_std";
    RegisterProtocol(PROTOCOL_BAIDU_STD, p);
}

}  // namespace policy
}  // namespace mrpc
