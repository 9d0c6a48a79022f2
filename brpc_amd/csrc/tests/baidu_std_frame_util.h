// baidu_std frames put together by hand for tests that feed a connection its
// bytes themselves:
//   "PRPC" | body_size (u32 BE) | meta_size (u32 BE) | RpcMeta | body | attachment
#pragma once

#include <cstdint>
#include <string>

#include "mrpc/proto/rpc_meta.pb.h"

namespace frame_util {

inline void AppendBe32(std::string* out, uint32_t v) {
    const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
    out->append(b, 4);
}

inline uint32_t ReadBe32(const char* p) {
    const unsigned char* u = (const unsigned char*)p;
    return ((uint32_t)u[0] << 24) | ((uint32_t)u[1] << 16) | ((uint32_t)u[2] << 8) | u[3];
}

// `meta_bytes` is a serialized RpcMeta (may be empty); the caller has put
// attachment.size() into its attachment_size.
inline std::string MakeFrame(const std::string& meta_bytes, const std::string& body, const std::string& attachment) {
    std::string f("PRPC");
    AppendBe32(&f, (uint32_t)(meta_bytes.size() + body.size() + attachment.size()));
    AppendBe32(&f, (uint32_t)meta_bytes.size());
    f += meta_bytes;
    f += body;
    f += attachment;
    return f;
}

inline std::string MakeRequestFrame(const std::string& service, const std::string& method, int64_t correlation_id,
                                    const std::string& body, const std::string& attachment, int64_t log_id = 0,
                                    const std::string& request_id = std::string()) {
    mrpc::policy::RpcMeta meta;
    meta.mutable_request()->set_service_name(service);
    meta.mutable_request()->set_method_name(method);
    if (log_id) meta.mutable_request()->set_log_id(log_id);
    if (!request_id.empty()) meta.mutable_request()->set_request_id(request_id);
    meta.set_correlation_id(correlation_id);
    if (!attachment.empty()) meta.set_attachment_size((int32_t)attachment.size());
    return MakeFrame(meta.SerializeAsString(), body, attachment);
}

inline std::string MakeResponseFrame(int64_t correlation_id, const std::string& body, const std::string& attachment,
                                     int error_code = 0, const std::string& error_text = std::string()) {
    mrpc::policy::RpcMeta meta;
    if (error_code) {
        meta.mutable_response()->set_error_code(error_code);
        meta.mutable_response()->set_error_text(error_text);
    }
    meta.set_correlation_id(correlation_id);
    if (!attachment.empty()) meta.set_attachment_size((int32_t)attachment.size());
    return MakeFrame(meta.SerializeAsString(), body, attachment);
}

}  // namespace frame_util
