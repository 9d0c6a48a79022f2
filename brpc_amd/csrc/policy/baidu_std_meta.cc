#include "policy/baidu_std_meta.h"

#include <cstring>

#include "base/buf.h"
#include "base/flags.h"
#include "base/util.h"
#include "pb/wire.h"
#include "var/var.h"

DEFINE_bool(baidu_std_meta_fast_path, true,
            "pack and scan the RpcMeta of plain baidu_std calls without a message object");
MRPC_VALIDATE_FLAG(baidu_std_meta_fast_path, mrpc::PassValidator);

namespace mrpc {
namespace policy {

bool MetaFastPathEnabled() { return FLAGS_baidu_std_meta_fast_path; }

namespace {

struct MetaPathVars {
    var::Adder<int64_t> v[META_PATH_COUNTERS] = {
        var::Adder<int64_t>("baidu_std_meta_request_packed_fast"),
        var::Adder<int64_t>("baidu_std_meta_request_packed_generic"),
        var::Adder<int64_t>("baidu_std_meta_request_parsed_fast"),
        var::Adder<int64_t>("baidu_std_meta_request_parsed_generic"),
        var::Adder<int64_t>("baidu_std_meta_response_packed_fast"),
        var::Adder<int64_t>("baidu_std_meta_response_packed_generic"),
        var::Adder<int64_t>("baidu_std_meta_response_parsed_fast"),
        var::Adder<int64_t>("baidu_std_meta_response_parsed_generic"),
    };
};

MetaPathVars& meta_path_vars() {
    static MetaPathVars* v = new MetaPathVars;
    return *v;
}

// Tags of the fields a plain meta may hold (all below 128: one byte each).
const uint8_t kTagRequest = 0x0A;         // RpcMeta.request = 1, length-delimited
const uint8_t kTagCompressType = 0x18;    // RpcMeta.compress_type = 3
const uint8_t kTagCorrelationId = 0x20;   // RpcMeta.correlation_id = 4
const uint8_t kTagAttachmentSize = 0x28;  // RpcMeta.attachment_size = 5
const uint8_t kTagServiceName = 0x0A;     // RpcRequestMeta.service_name = 1
const uint8_t kTagMethodName = 0x12;      // RpcRequestMeta.method_name = 2
const uint8_t kTagLogId = 0x18;           // RpcRequestMeta.log_id = 3
const uint8_t kTagTimeoutMs = 0x40;       // RpcRequestMeta.timeout_ms = 8

// An int32 goes on the wire sign-extended to 64 bits.
inline uint64_t wire_of_int32(int32_t v) { return (uint64_t)(int64_t)v; }

inline void pack_header(char* h, uint32_t meta_size, uint32_t payload_size) {
    memcpy(h, "PRPC", 4);
    pack_be32(h + 4, meta_size + payload_size);
    pack_be32(h + 8, meta_size);
}

inline size_t tail_size(int32_t compress_type, int64_t correlation_id, int32_t attachment_size) {
    size_t n = 1 + pb::varint_size(wire_of_int32(compress_type)) + 1 + pb::varint_size((uint64_t)correlation_id);
    if (attachment_size != 0) n += 1 + pb::varint_size(wire_of_int32(attachment_size));
    return n;
}

inline uint8_t* write_tail(uint8_t* p, int32_t compress_type, int64_t correlation_id, int32_t attachment_size) {
    *p++ = kTagCompressType;
    p = pb::write_varint(p, wire_of_int32(compress_type));
    *p++ = kTagCorrelationId;
    p = pb::write_varint(p, (uint64_t)correlation_id);
    if (attachment_size != 0) {
        *p++ = kTagAttachmentSize;
        p = pb::write_varint(p, wire_of_int32(attachment_size));
    }
    return p;
}

// One varint field of a scan: declined when seen before.
template <typename T>
inline bool scan_varint(pb::CodedInput* in, bool* seen, T* out) {
    uint64_t v;
    if (*seen || !in->read_varint(&v)) return false;
    *seen = true;
    *out = (T)v;
    return true;
}

inline bool scan_string(pb::CodedInput* in, bool* seen, std::string_view* out) {
    uint64_t len;
    const uint8_t* d;
    if (*seen || !in->read_varint(&len) || len > in->bytes_left() || !in->read_bytes((size_t)len, &d)) return false;
    *seen = true;
    *out = std::string_view((const char*)d, (size_t)len);
    return true;
}

bool scan_request_submessage(const uint8_t* data, size_t n, ScannedRequestMeta* out) {
    pb::CodedInput in(data, n);
    bool service = false, method = false, log_id = false, timeout = false;
    while (!in.at_limit()) {
        uint64_t tag;
        if (!in.read_varint(&tag)) return false;
        switch (tag) {
        case kTagServiceName:
            if (!scan_string(&in, &service, &out->service_name)) return false;
            break;
        case kTagMethodName:
            if (!scan_string(&in, &method, &out->method_name)) return false;
            break;
        case kTagLogId:
            if (!scan_varint(&in, &log_id, &out->log_id)) return false;
            break;
        case kTagTimeoutMs:
            if (!scan_varint(&in, &timeout, &out->timeout_ms)) return false;
            break;
        default:
            return false;
        }
    }
    out->has_log_id = log_id;
    out->has_timeout_ms = timeout;
    return service && method;
}

}  // namespace

void CountMetaPath(MetaPathCounter c) { meta_path_vars().v[c] << 1; }
int64_t MetaPathCount(MetaPathCounter c) { return meta_path_vars().v[c].get_value(); }

void PackPlainRequestMeta(Buf* out, const PlainRequestMeta& m, size_t payload_size) {
    size_t sub = m.name_fields.size();
    if (m.has_log_id) sub += 1 + pb::varint_size((uint64_t)m.log_id);
    if (m.timeout_ms > 0) sub += 1 + pb::varint_size(wire_of_int32(m.timeout_ms));
    const size_t meta_size =
        1 + pb::varint_size(sub) + sub + tail_size(m.compress_type, m.correlation_id, m.attachment_size);
    char* const h = out->append_contiguous(12 + meta_size);
    pack_header(h, (uint32_t)meta_size, (uint32_t)payload_size);
    uint8_t* p = (uint8_t*)h + 12;
    *p++ = kTagRequest;
    p = pb::write_varint(p, sub);
    memcpy(p, m.name_fields.data(), m.name_fields.size());
    p += m.name_fields.size();
    if (m.has_log_id) {
        *p++ = kTagLogId;
        p = pb::write_varint(p, (uint64_t)m.log_id);
    }
    if (m.timeout_ms > 0) {
        *p++ = kTagTimeoutMs;
        p = pb::write_varint(p, wire_of_int32(m.timeout_ms));
    }
    write_tail(p, m.compress_type, m.correlation_id, m.attachment_size);
}

void PackPlainResponseMeta(Buf* out, const PlainResponseMeta& m, size_t payload_size) {
    const size_t meta_size = tail_size(m.compress_type, m.correlation_id, m.attachment_size);
    char* const h = out->append_contiguous(12 + meta_size);
    pack_header(h, (uint32_t)meta_size, (uint32_t)payload_size);
    write_tail((uint8_t*)h + 12, m.compress_type, m.correlation_id, m.attachment_size);
}

bool ScanPlainRequestMeta(const char* data, size_t n, ScannedRequestMeta* out) {
    pb::CodedInput in(data, n);
    bool request = false, compress = false, cid = false, attachment = false;
    while (!in.at_limit()) {
        uint64_t tag;
        if (!in.read_varint(&tag)) return false;
        switch (tag) {
        case kTagRequest: {
            uint64_t len;
            const uint8_t* d;
            if (request || !in.read_varint(&len) || len > in.bytes_left() || !in.read_bytes((size_t)len, &d)) return false;
            if (!scan_request_submessage(d, (size_t)len, out)) return false;
            request = true;
            break;
        }
        case kTagCompressType:
            if (!scan_varint(&in, &compress, &out->compress_type)) return false;
            break;
        case kTagCorrelationId:
            if (!scan_varint(&in, &cid, &out->correlation_id)) return false;
            break;
        case kTagAttachmentSize:
            if (!scan_varint(&in, &attachment, &out->attachment_size)) return false;
            break;
        default:
            return false;
        }
    }
    return request;
}

bool ScanPlainResponseMeta(const char* data, size_t n, ScannedResponseMeta* out) {
    if (n == 0) return false;
    pb::CodedInput in(data, n);
    bool compress = false, cid = false, attachment = false;
    while (!in.at_limit()) {
        uint64_t tag;
        if (!in.read_varint(&tag)) return false;
        switch (tag) {
        case kTagCompressType:
            if (!scan_varint(&in, &compress, &out->compress_type)) return false;
            break;
        case kTagCorrelationId:
            if (!scan_varint(&in, &cid, &out->correlation_id)) return false;
            break;
        case kTagAttachmentSize:
            if (!scan_varint(&in, &attachment, &out->attachment_size)) return false;
            break;
        default:
            return false;
        }
    }
    return true;
}

}  // namespace policy
}  // namespace mrpc
