// baidu_std RpcMeta of a plain call, packed and scanned without a message
// object. A plain request carries the two names, the correlation id, the
// compress type and at most log_id, timeout_ms and attachment_size; a plain
// response carries compress type, correlation id and at most attachment_size.
// The packers write exactly the bytes the generic serializer writes for the
// same values. The scanners either accept a meta, yielding what the generic
// parser would yield, or decline it; a declined meta goes through the generic
// parser, so a scanner never decides an error.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string_view>

namespace mrpc {

class Buf;

namespace policy {

// -baidu_std_meta_fast_path, read per call.
bool MetaFastPathEnabled();

struct PlainRequestMeta {
    std::string_view name_fields;  // pb::MethodWireNames::full or ::brief
    bool has_log_id = false;
    int64_t log_id = 0;
    int32_t timeout_ms = 0;  // on the wire when > 0
    int32_t compress_type = 0;
    int64_t correlation_id = 0;
    int32_t attachment_size = 0;  // on the wire when not 0
};

struct PlainResponseMeta {
    int32_t compress_type = 0;
    int64_t correlation_id = 0;
    int32_t attachment_size = 0;  // on the wire when not 0
};

// Append "PRPC", the two sizes and the meta to *out. payload_size: the bytes
// of body and attachment that the caller appends next.
void PackPlainRequestMeta(Buf* out, const PlainRequestMeta& m, size_t payload_size);
void PackPlainResponseMeta(Buf* out, const PlainResponseMeta& m, size_t payload_size);

struct ScannedRequestMeta {
    std::string_view service_name;  // views of the scanned bytes
    std::string_view method_name;
    bool has_log_id = false;
    int64_t log_id = 0;
    bool has_timeout_ms = false;
    int32_t timeout_ms = 0;
    int32_t compress_type = 0;
    int64_t correlation_id = 0;
    int32_t attachment_size = 0;
};

struct ScannedResponseMeta {
    int32_t compress_type = 0;
    int64_t correlation_id = 0;
    int32_t attachment_size = 0;
};

// True if [data, data + n) is the meta of a plain request: top-level fields
// 1, 3, 4 and 5 only, each at most once, and in field 1 the fields 1, 2, 3
// and 8 only, each at most once, with both names there. Anything else (an
// other field, another wire type, a varint beyond 10 bytes, a length past
// the end, a duplicate, a missing name, no bytes at all) is declined.
bool ScanPlainRequestMeta(const char* data, size_t n, ScannedRequestMeta* out);
// The same for a plain response: top-level fields 3, 4 and 5 only.
bool ScanPlainResponseMeta(const char* data, size_t n, ScannedResponseMeta* out);

// Which way the metas of this process went (/vars baidu_std_meta_*).
enum MetaPathCounter {
    META_REQUEST_PACKED_FAST,
    META_REQUEST_PACKED_GENERIC,
    META_REQUEST_PARSED_FAST,
    META_REQUEST_PARSED_GENERIC,
    META_RESPONSE_PACKED_FAST,
    META_RESPONSE_PACKED_GENERIC,
    META_RESPONSE_PARSED_FAST,
    META_RESPONSE_PARSED_GENERIC,
    META_PATH_COUNTERS
};
void CountMetaPath(MetaPathCounter c);
int64_t MetaPathCount(MetaPathCounter c);

}  // namespace policy
}  // namespace mrpc
