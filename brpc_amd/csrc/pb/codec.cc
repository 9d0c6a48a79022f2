// The hot half of Message: size, serialize, parse, Clear and IsInitialized,
// driven by the type's CodecPlan (pb/plan.h). Each operation asks for the
// descriptor once, then walks 24-byte entries: presence from the has word,
// the pre-encoded tag, one switch on the entry's kind. The FieldDescriptor
// is touched only on rare paths (explicit defaults, oneof siblings, new
// sub-messages). Reflection, MergeFrom and the text format stay in
// message.cc on the descriptor walk.
#include <algorithm>
#include <cstring>

#include "base/logging.h"
#include "pb/message.h"
#include "pb/plan.h"

namespace mrpc {
namespace pb {

namespace {

uint8_t* write_scalar(uint8_t* o, FieldType t, const void* p) {
    switch (t) {
    case FieldType::DOUBLE:
    case FieldType::FIXED64:
    case FieldType::SFIXED64: return write_fixed64(o, *(const uint64_t*)p);
    case FieldType::FLOAT:
    case FieldType::FIXED32:
    case FieldType::SFIXED32: return write_fixed32(o, *(const uint32_t*)p);
    case FieldType::BOOL: *o++ = (*(const uint8_t*)p) ? 1 : 0; return o;
    case FieldType::INT32:
    case FieldType::ENUM: return write_varint(o, (uint64_t)(int64_t)*(const int32_t*)p);
    case FieldType::SINT32: return write_varint(o, zigzag32(*(const int32_t*)p));
    case FieldType::UINT32: return write_varint(o, *(const uint32_t*)p);
    case FieldType::INT64: return write_varint(o, (uint64_t)*(const int64_t*)p);
    case FieldType::SINT64: return write_varint(o, zigzag64(*(const int64_t*)p));
    case FieldType::UINT64: return write_varint(o, *(const uint64_t*)p);
    default: return o;
    }
}

// Payload bytes of elements [0, n) of a repeated scalar field in its vector
// layout: typed, branch-free loops (varint size = (bit width * 9 + 64) / 64)
// instead of a per-element switch and loop; packed runs of 10^4..10^5
// elements are sized twice per serialization.
inline size_t vsize64(uint64_t v) { return (size_t)(((63 - __builtin_clzll(v | 1)) * 9 + 73) >> 6); }
size_t repeated_payload_bytes(FieldType t, const char* data, size_t n) {
    size_t s = 0;
    switch (t) {
    case FieldType::DOUBLE:
    case FieldType::FIXED64:
    case FieldType::SFIXED64: return 8 * n;
    case FieldType::FLOAT:
    case FieldType::FIXED32:
    case FieldType::SFIXED32: return 4 * n;
    case FieldType::BOOL: return n;
    case FieldType::INT32:
    case FieldType::ENUM: {
        const int32_t* v = reinterpret_cast<const int32_t*>(data);
        for (size_t i = 0; i < n; ++i) s += vsize64((uint64_t)(int64_t)v[i]);
        return s;
    }
    case FieldType::SINT32: {
        const int32_t* v = reinterpret_cast<const int32_t*>(data);
        for (size_t i = 0; i < n; ++i) s += vsize64(zigzag32(v[i]));
        return s;
    }
    case FieldType::UINT32: {
        const uint32_t* v = reinterpret_cast<const uint32_t*>(data);
        for (size_t i = 0; i < n; ++i) s += vsize64(v[i]);
        return s;
    }
    case FieldType::INT64:
    case FieldType::UINT64: {
        const uint64_t* v = reinterpret_cast<const uint64_t*>(data);
        for (size_t i = 0; i < n; ++i) s += vsize64(v[i]);
        return s;
    }
    case FieldType::SINT64: {
        const int64_t* v = reinterpret_cast<const int64_t*>(data);
        for (size_t i = 0; i < n; ++i) s += vsize64(zigzag64(v[i]));
        return s;
    }
    default: return 0;
    }
}

// Storage bytes of one element of each kind (0: string, message).
constexpr uint8_t kKindWidth[10] = {4, 4, 4, 8, 8, 1, 4, 8, 0, 0};

// Repeated scalars are std::vector<T>; what the codec does with them
// (size, data, clear, append of raw elements) depends on sizeof(T) alone,
// so it views them as vectors of the unsigned type of that width.
using Vec1 = std::vector<uint8_t>;
using Vec4 = std::vector<uint32_t>;
using Vec8 = std::vector<uint64_t>;

struct RawVec {
    const char* data;
    size_t n;
};
inline RawVec raw_repeated(const char* p, PlanKind k) {
    switch (kKindWidth[k]) {
    case 1: {
        const Vec1& v = *reinterpret_cast<const Vec1*>(p);
        return RawVec{(const char*)v.data(), v.size()};
    }
    case 4: {
        const Vec4& v = *reinterpret_cast<const Vec4*>(p);
        return RawVec{(const char*)v.data(), v.size()};
    }
    default: {
        const Vec8& v = *reinterpret_cast<const Vec8*>(p);
        return RawVec{(const char*)v.data(), v.size()};
    }
    }
}

template <typename T>
inline T load(const char* p) {
    T v;
    memcpy(&v, p, sizeof(T));
    return v;
}

inline bool is_zero(PlanKind k, const char* p) {
    switch (k) {
    case K_BOOL: return load<uint8_t>(p) == 0;
    case K_INT64:
    case K_SINT64:
    case K_FIXED64: return load<uint64_t>(p) == 0;
    case K_STRING: return reinterpret_cast<const std::string*>(p)->empty();
    case K_MESSAGE: return load<const Message*>(p) == nullptr;
    default: return load<uint32_t>(p) == 0;
    }
}

// Presence of a singular field: the pointer for messages, the has-bit where
// there is one, else (proto3 implicit presence) a non-zero value.
inline bool present(const PlanEntry& e, const char* base, const uint32_t* hb) {
    if (e.kind() == K_MESSAGE) return load<const Message*>(base + e.offset) != nullptr;
    if (e.has_bit >= 0) return (hb[e.has_bit >> 5] >> (e.has_bit & 31)) & 1;
    return !is_zero(e.kind(), base + e.offset);
}

inline size_t scalar_size(PlanKind k, const char* p) {
    switch (k) {
    case K_INT32: return int32_size(load<int32_t>(p));
    case K_UINT32: return varint_size(load<uint32_t>(p));
    case K_SINT32: return varint_size(zigzag32(load<int32_t>(p)));
    case K_INT64: return varint_size(load<uint64_t>(p));
    case K_SINT64: return varint_size(zigzag64(load<int64_t>(p)));
    case K_BOOL: return 1;
    case K_FIXED32: return 4;
    case K_FIXED64: return 8;
    default: return 0;
    }
}

inline uint8_t* write_scalar(uint8_t* o, PlanKind k, const char* p) {
    switch (k) {
    case K_INT32: return write_varint(o, (uint64_t)(int64_t)load<int32_t>(p));
    case K_UINT32: return write_varint(o, load<uint32_t>(p));
    case K_SINT32: return write_varint(o, zigzag32(load<int32_t>(p)));
    case K_INT64: return write_varint(o, load<uint64_t>(p));
    case K_SINT64: return write_varint(o, zigzag64(load<int64_t>(p)));
    case K_BOOL: *o++ = load<uint8_t>(p) ? 1 : 0; return o;
    case K_FIXED32: memcpy(o, p, 4); return o + 4;
    case K_FIXED64: memcpy(o, p, 8); return o + 8;
    default: return o;
    }
}

inline uint8_t* put_tag(uint8_t* o, const uint8_t* tag, unsigned len) {
    *o = tag[0];
    for (unsigned i = 1; i < len; ++i) o[i] = tag[i];
    return o + len;
}

inline uint8_t* put_bytes(uint8_t* o, const std::string& s) {
    o = write_varint(o, s.size());
    memcpy(o, s.data(), s.size());
    return o + s.size();
}

inline void set_has(uint32_t* hb, const PlanEntry& e) {
    if (e.has_bit >= 0) hb[e.has_bit >> 5] |= 1u << (e.has_bit & 31);
}

// A set singular scalar or string back to its default.
inline void reset_singular(Message* m, const Descriptor* d, const PlanEntry& e) {
    char* p = reinterpret_cast<char*>(m) + e.offset;
    if (e.flags & PF_NONZERO_DEFAULT) {
        // the value lives in the FieldDescriptor; ClearField's has-bit store is harmless here
        Reflection::ClearField(m, &d->fields[e.field]);
        return;
    }
    switch (kKindWidth[e.kind()]) {
    case 1: *p = 0; break;
    case 4: memset(p, 0, 4); break;
    case 8: memset(p, 0, 8); break;
    default:
        if (e.kind() == K_STRING) reinterpret_cast<std::string*>(p)->clear();
    }
}

inline void clear_repeated(char* p, PlanKind k) {
    switch (k) {
    case K_STRING: reinterpret_cast<std::vector<std::string>*>(p)->clear(); break;
    case K_MESSAGE: reinterpret_cast<RepeatedPtrBase*>(p)->Clear(); break;
    default:
        switch (kKindWidth[k]) {
        case 1: reinterpret_cast<Vec1*>(p)->clear(); break;
        case 4: reinterpret_cast<Vec4*>(p)->clear(); break;
        default: reinterpret_cast<Vec8*>(p)->clear(); break;
        }
    }
}

// A decoded varint/fixed value in the field's storage form, as the low
// kKindWidth bytes of the result.
inline uint64_t to_storage(PlanKind k, uint64_t raw) {
    switch (k) {
    case K_SINT32: return (uint32_t)unzigzag32((uint32_t)raw);
    case K_SINT64: return (uint64_t)unzigzag64(raw);
    case K_BOOL: return raw != 0;
    default: return raw;
    }
}

// Store a decoded number into entry e (singular or repeated).
void store_number(Message* m, const Descriptor* d, uint32_t* hb, const PlanEntry& e, uint64_t raw) {
    char* p = reinterpret_cast<char*>(m) + e.offset;
    const uint64_t v = to_storage(e.kind(), raw);
    const unsigned w = kKindWidth[e.kind()];
    if (e.repeated()) {
        switch (w) {
        case 1: reinterpret_cast<Vec1*>(p)->push_back((uint8_t)v); break;
        case 4: reinterpret_cast<Vec4*>(p)->push_back((uint32_t)v); break;
        default: reinterpret_cast<Vec8*>(p)->push_back(v); break;
        }
        return;
    }
    memcpy(p, &v, w);  // little-endian, as the fixed-width wire helpers assume
    if (e.flags & PF_ONEOF) ClearOneofSiblings(m, &d->fields[e.field]);
    set_has(hb, e);
}

// Packed payload p[0, len) appended to a repeated scalar field in bulk:
// fixed-width types are one memcpy, varints are counted first (one pass
// over the terminator bits, so the vector grows once) and decoded by a
// typed loop instead of a per-element switch. Same results and the same
// failures as the element-wise path.
template <typename T, typename Conv>
bool bulk_varints(char* field, const uint8_t* p, size_t len, Conv conv) {
    size_t n = 0;
    for (size_t i = 0; i < len; ++i) n += (p[i] >> 7) ^ 1;
    auto& vec = *reinterpret_cast<std::vector<T>*>(field);
    const size_t base = vec.size();
    vec.resize(base + n);
    T* out = vec.data() + base;
    CodedInput in(p, len);
    for (size_t k = 0; k < n; ++k) {
        uint64_t v;
        if (!in.read_varint(&v)) {
            vec.resize(base + k);
            return false;
        }
        out[k] = conv(v);
    }
    return in.at_limit();
}

template <typename T>
bool bulk_fixed(char* field, const uint8_t* p, size_t len) {
    if (len % sizeof(T)) return false;
    auto& vec = *reinterpret_cast<std::vector<T>*>(field);
    const size_t base = vec.size();
    vec.resize(base + len / sizeof(T));
    if (len) memcpy(vec.data() + base, p, len);
    return true;
}

bool parse_packed(char* field, PlanKind k, const uint8_t* p, size_t len) {
    switch (k) {
    case K_INT32:
    case K_UINT32: return bulk_varints<uint32_t>(field, p, len, [](uint64_t v) { return (uint32_t)v; });
    case K_SINT32: return bulk_varints<uint32_t>(field, p, len, [](uint64_t v) { return (uint32_t)unzigzag32((uint32_t)v); });
    case K_INT64: return bulk_varints<uint64_t>(field, p, len, [](uint64_t v) { return v; });
    case K_SINT64: return bulk_varints<uint64_t>(field, p, len, [](uint64_t v) { return (uint64_t)unzigzag64(v); });
    case K_BOOL: return bulk_varints<uint8_t>(field, p, len, [](uint64_t v) { return (uint8_t)(v != 0); });
    case K_FIXED32: return bulk_fixed<uint32_t>(field, p, len);
    case K_FIXED64: return bulk_fixed<uint64_t>(field, p, len);
    default: return false;
    }
}

bool parse_entry(Message* m, const Descriptor* d, uint32_t* hb, const PlanEntry& e, uint32_t tag, CodedInput* in) {
    const uint32_t wt = tag & 7;
    const PlanKind k = e.kind();
    char* p = reinterpret_cast<char*>(m) + e.offset;
    if (e.repeated() && k < K_STRING && wt == WIRETYPE_LENGTH_DELIMITED) {
        // packed and unpacked forms are both accepted, whatever the field declares
        uint64_t len;
        const uint8_t* s;
        if (!in->read_varint(&len) || !in->read_bytes((size_t)len, &s)) return false;
        return parse_packed(p, k, s, (size_t)len);
    }
    if (wt != e.wire_type() || (e.flags & PF_GROUP)) {
        // Mismatched wire type, or a group: keep as unknown field (protobuf semantics).
        return in->skip_field(tag, m->mutable_unknown_fields());
    }
    switch (k) {
    case K_STRING: {
        uint64_t len;
        const uint8_t* s;
        if (!in->read_varint(&len) || !in->read_bytes((size_t)len, &s)) return false;
        if (e.repeated()) {
            reinterpret_cast<std::vector<std::string>*>(p)->emplace_back((const char*)s, (size_t)len);
        } else {
            if (e.flags & PF_ONEOF) ClearOneofSiblings(m, &d->fields[e.field]);
            reinterpret_cast<std::string*>(p)->assign((const char*)s, (size_t)len);
            set_has(hb, e);
        }
        return true;
    }
    case K_MESSAGE: {
        uint64_t len;
        const uint8_t* old;
        if (!in->read_varint(&len) || !in->push_limit((size_t)len, &old)) return false;
        Message* sub;
        if (e.repeated()) sub = Reflection::AddMessage(m, &d->fields[e.field]);
        else if (!(sub = load<Message*>(p))) sub = Reflection::MutableMessage(m, &d->fields[e.field]);
        if (!in->inc_depth()) return false;
        if (!sub->MergePartialFromCodedInput(in)) return false;
        in->dec_depth();
        if (!in->at_limit()) return false;
        in->pop_limit(old);
        return true;
    }
    case K_FIXED32: {
        uint32_t v;
        if (!in->read_fixed32(&v)) return false;
        store_number(m, d, hb, e, v);
        return true;
    }
    case K_FIXED64: {
        uint64_t v;
        if (!in->read_fixed64(&v)) return false;
        store_number(m, d, hb, e, v);
        return true;
    }
    default: {
        uint64_t v;
        if (!in->read_varint(&v)) return false;
        store_number(m, d, hb, e, v);
        return true;
    }
    }
}

}  // namespace

// ---------------------------------------------------------------- Clear

void Message::Clear() {
    const Descriptor* d = GetDescriptor();
    const CodecPlan* plan = PlanOf(d);
    char* base = reinterpret_cast<char*>(this);
    // set fields with a has-bit: found from the has words, which are zeroed on the way
    uint32_t* hb = reinterpret_cast<uint32_t*>(base + plan->has_bits_offset);
    for (uint32_t w = 0; w < plan->has_words; ++w) {
        uint32_t word = hb[w];
        if (!word) continue;
        hb[w] = 0;
        do {
            const uint16_t idx = plan->by_has_bit[w * 32 + __builtin_ctz(word)];
            word &= word - 1;
            if (idx != CodecPlan::kNone) reset_singular(this, d, plan->entries[idx]);
        } while (word);
    }
    // the rest: sub-messages, repeated fields, implicit-presence scalars
    for (const uint16_t idx : plan->no_has_bit) {
        const PlanEntry& e = plan->entries[idx];
        char* p = base + e.offset;
        if (e.repeated()) {
            clear_repeated(p, e.kind());
        } else if (e.kind() == K_MESSAGE) {
            if (Message* sub = load<Message*>(p)) {
                delete sub;
                memset(p, 0, sizeof(Message*));
            }
        } else if ((e.flags & PF_NONZERO_DEFAULT) || !is_zero(e.kind(), p)) {
            reset_singular(this, d, e);
        }
    }
    if (!_unknown.empty()) _unknown.clear();
}

// ---------------------------------------------------------------- size

size_t Message::ByteSizeLong() const {
    const CodecPlan* plan = PlanOf(GetDescriptor());
    const char* base = reinterpret_cast<const char*>(this);
    const uint32_t* hb = reinterpret_cast<const uint32_t*>(base + plan->has_bits_offset);
    size_t total = 0;
    for (const PlanEntry& e : plan->entries) {
        const char* p = base + e.offset;
        const PlanKind k = e.kind();
        const size_t tag_size = e.tag_len;
        if (e.repeated()) {
            switch (k) {
            case K_STRING: {
                const auto& v = *reinterpret_cast<const std::vector<std::string>*>(p);
                for (const auto& s : v) total += tag_size + varint_size(s.size()) + s.size();
                break;
            }
            case K_MESSAGE: {
                const auto& v = *reinterpret_cast<const RepeatedPtrBase*>(p);
                for (int i = 0; i < v.size(); ++i) {
                    const size_t s = v.Get(i)->ByteSizeLong();
                    total += tag_size + varint_size(s) + s;
                }
                break;
            }
            default: {
                const RawVec rv = raw_repeated(p, k);
                if (rv.n == 0) break;
                const size_t data = repeated_payload_bytes((FieldType)e.ftype, rv.data, rv.n);
                if (e.cls() == C_REP_PACKED) total += tag_size + varint_size(data) + data;
                else total += tag_size * rv.n + data;
            }
            }
            continue;
        }
        if (!present(e, base, hb)) continue;
        switch (k) {
        case K_STRING: {
            const auto& s = *reinterpret_cast<const std::string*>(p);
            total += tag_size + varint_size(s.size()) + s.size();
            break;
        }
        case K_MESSAGE: {
            const size_t s = load<const Message*>(p)->ByteSizeLong();
            total += tag_size + varint_size(s) + s;
            break;
        }
        default: total += tag_size + scalar_size(k, p);
        }
    }
    total += _unknown.size();
    _cached_size = (int)total;
    return total;
}

// ---------------------------------------------------------------- serialize

static thread_local PackedRunSink* tls_run_sink = nullptr;

PackedRunSink* SetThreadPackedRunSink(PackedRunSink* sink) {
    PackedRunSink* prev = tls_run_sink;
    tls_run_sink = sink;
    return prev;
}

bool IsVarintFieldType(FieldType t) {
    switch (t) {
    case FieldType::INT32:
    case FieldType::ENUM:
    case FieldType::SINT32:
    case FieldType::UINT32:
    case FieldType::INT64:
    case FieldType::SINT64:
    case FieldType::UINT64:
    case FieldType::BOOL: return true;
    default: return false;
    }
}

void EncodePackedRunOnHost(const PackedRun& run) {
    uint8_t* o = run.dst;
    const char* v = static_cast<const char*>(run.values);
    for (size_t i = 0; i < run.n; ++i) o = write_scalar(o, run.type, v + i * run.elem_bytes);
}

uint8_t* Message::SerializeWithCachedSizesToArray(uint8_t* o) const {
    const CodecPlan* plan = PlanOf(GetDescriptor());
    const char* base = reinterpret_cast<const char*>(this);
    const uint32_t* hb = reinterpret_cast<const uint32_t*>(base + plan->has_bits_offset);
    for (const PlanEntry& e : plan->entries) {
        const char* p = base + e.offset;
        const PlanKind k = e.kind();
        if (e.repeated()) {
            switch (k) {
            case K_STRING: {
                for (const auto& s : *reinterpret_cast<const std::vector<std::string>*>(p)) {
                    o = put_bytes(put_tag(o, e.tag, e.tag_len), s);
                }
                break;
            }
            case K_MESSAGE: {
                const auto& v = *reinterpret_cast<const RepeatedPtrBase*>(p);
                for (int i = 0; i < v.size(); ++i) {
                    const Message* sub = v.Get(i);
                    o = put_tag(o, e.tag, e.tag_len);
                    o = write_varint(o, (uint64_t)sub->GetCachedSize());
                    o = sub->SerializeWithCachedSizesToArray(o);
                }
                break;
            }
            default: {
                const RawVec rv = raw_repeated(p, k);
                if (rv.n == 0) break;
                const size_t eb = kKindWidth[k];
                const FieldType type = (FieldType)e.ftype;
                const bool packed = e.cls() == C_REP_PACKED;
                PackedRunSink* sink = tls_run_sink;
                if (packed && sink && rv.n >= sink->min_elems() && IsVarintFieldType(type)) {
                    PackedRun run;
                    run.values = rv.data;
                    run.n = rv.n;
                    run.elem_bytes = eb;
                    run.type = type;
                    run.chunk_bytes.reserve((rv.n + kPackedRunChunkElems - 1) / kPackedRunChunkElems);
                    size_t data = 0;
                    for (size_t c = 0; c < rv.n; c += kPackedRunChunkElems) {
                        const size_t end = std::min(rv.n, c + kPackedRunChunkElems);
                        const size_t cb = repeated_payload_bytes(type, rv.data + c * eb, end - c);
                        run.chunk_bytes.push_back((uint32_t)cb);
                        data += cb;
                    }
                    o = put_tag(o, e.ptag, e.tag_len);
                    o = write_varint(o, data);
                    run.dst = o;
                    run.bytes = data;
                    o += data;
                    sink->Take(std::move(run));
                } else if (packed) {
                    const size_t data = repeated_payload_bytes(type, rv.data, rv.n);
                    o = put_tag(o, e.ptag, e.tag_len);
                    o = write_varint(o, data);
                    for (size_t i = 0; i < rv.n; ++i) o = write_scalar(o, k, rv.data + i * eb);
                } else {
                    for (size_t i = 0; i < rv.n; ++i) {
                        o = put_tag(o, e.tag, e.tag_len);
                        o = write_scalar(o, k, rv.data + i * eb);
                    }
                }
            }
            }
            continue;
        }
        if (!present(e, base, hb)) continue;
        o = put_tag(o, e.tag, e.tag_len);
        switch (k) {
        case K_STRING: o = put_bytes(o, *reinterpret_cast<const std::string*>(p)); break;
        case K_MESSAGE: {
            const Message* sub = load<const Message*>(p);
            o = write_varint(o, (uint64_t)sub->GetCachedSize());
            o = sub->SerializeWithCachedSizesToArray(o);
            break;
        }
        default: o = write_scalar(o, k, p);
        }
    }
    if (!_unknown.empty()) {
        memcpy(o, _unknown.data(), _unknown.size());
        o += _unknown.size();
    }
    return o;
}

// ---------------------------------------------------------------- parse

bool Message::MergePartialFromCodedInput(CodedInput* in) {
    const Descriptor* d = GetDescriptor();
    const CodecPlan* plan = PlanOf(d);
    uint32_t* hb = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(this) + plan->has_bits_offset);
    for (;;) {
        const uint32_t tag = in->read_tag();
        if (tag == 0) return true;
        if (tag == 0xFFFFFFFFu || (tag >> 3) == 0) return false;
        if ((tag & 7) == WIRETYPE_END_GROUP) return false;
        const PlanEntry* e = plan->Find(tag >> 3);
        if (!e) {
            if (!in->skip_field(tag, &_unknown)) return false;
            continue;
        }
        if (!parse_entry(this, d, hb, *e, tag, in)) return false;
    }
}

bool Message::IsInitialized() const {
    const CodecPlan* plan = PlanOf(GetDescriptor());
    if (!plan->needs_init_check) return true;
    const char* base = reinterpret_cast<const char*>(this);
    const uint32_t* hb = reinterpret_cast<const uint32_t*>(base + plan->has_bits_offset);
    for (const uint16_t idx : plan->init_entries) {
        const PlanEntry& e = plan->entries[idx];
        if ((e.flags & PF_REQUIRED) && !present(e, base, hb)) return false;
        if (!(e.flags & PF_SUB_NEEDS_INIT)) continue;
        if (e.repeated()) {
            const auto& v = *reinterpret_cast<const RepeatedPtrBase*>(base + e.offset);
            for (int i = 0; i < v.size(); ++i) {
                if (!v.Get(i)->IsInitialized()) return false;
            }
        } else if (const Message* sub = load<const Message*>(base + e.offset)) {
            if (!sub->IsInitialized()) return false;
        }
    }
    return true;
}

bool Message::MergeFromFieldTable(const uint8_t* data, size_t size, const uint64_t* fields, int nfields,
                                  PackedRunDecoder* decoder) {
    const Descriptor* d = GetDescriptor();
    const CodecPlan* plan = PlanOf(d);
    uint32_t* hb = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(this) + plan->has_bits_offset);
    // large packed varint runs go to the decoder first, all in one call
    std::vector<PackedRunIn> runs;
    std::vector<int> run_of;  // field row -> runs index (or -1)
    if (decoder) {
        const size_t min = std::max<size_t>(1, decoder->min_bytes());
        for (int i = 0; i < nfields; ++i) {
            const uint64_t tag = fields[2 * i], v = fields[2 * i + 1];
            if ((tag & 7) != WIRETYPE_LENGTH_DELIMITED || (v & 0xFFFFFFFFu) < min) continue;
            const PlanEntry* e = tag >> 3 <= 0xFFFFFFFFu ? plan->Find((uint32_t)(tag >> 3)) : nullptr;
            if (!e || !e->repeated() || e->kind() >= K_STRING || !IsVarintFieldType((FieldType)e->ftype)) continue;
            const size_t off = (size_t)(v >> 32), len = (size_t)(v & 0xFFFFFFFFu);
            if (off > size || len > size - off) return false;
            if (run_of.empty()) run_of.assign(nfields, -1);
            run_of[i] = (int)runs.size();
            PackedRunIn r;
            r.p = data + off;
            r.len = len;
            r.type = (FieldType)e->ftype;
            r.elem_bytes = kKindWidth[e->kind()];
            runs.push_back(r);
        }
        if (!runs.empty()) decoder->Decode(&runs);
    }
    for (int i = 0; i < nfields; ++i) {
        const uint64_t tag = fields[2 * i], v = fields[2 * i + 1];
        const uint32_t wt = (uint32_t)(tag & 7);
        const PlanEntry* e = tag >> 3 <= 0xFFFFFFFFu ? plan->Find((uint32_t)(tag >> 3)) : nullptr;
        if (!run_of.empty() && run_of[i] >= 0 && runs[run_of[i]].values) {
            // decoded elements are already in the field's vector layout
            const PackedRunIn& r = runs[run_of[i]];
            char* p = reinterpret_cast<char*>(this) + e->offset;
            switch (kKindWidth[e->kind()]) {
            case 1: {
                const uint8_t* s = static_cast<const uint8_t*>(r.values);
                Vec1& vec = *reinterpret_cast<Vec1*>(p);
                vec.insert(vec.end(), s, s + r.count);
                break;
            }
            case 4: {
                const uint32_t* s = static_cast<const uint32_t*>(r.values);
                Vec4& vec = *reinterpret_cast<Vec4*>(p);
                vec.insert(vec.end(), s, s + r.count);
                break;
            }
            default: {
                const uint64_t* s = static_cast<const uint64_t*>(r.values);
                Vec8& vec = *reinterpret_cast<Vec8*>(p);
                vec.insert(vec.end(), s, s + r.count);
            }
            }
            continue;
        }
        if (!e || (e->flags & PF_GROUP)) return false;
        if (wt != WIRETYPE_LENGTH_DELIMITED) {
            if (wt != e->wire_type()) return false;
            store_number(this, d, hb, *e, v);
            continue;
        }
        const size_t off = (size_t)(v >> 32), len = (size_t)(v & 0xFFFFFFFFu);
        if (off > size || len > size - off) return false;
        const uint8_t* s = data + off;
        char* p = reinterpret_cast<char*>(this) + e->offset;
        if (e->repeated() && e->kind() < K_STRING) {
            if (!parse_packed(p, e->kind(), s, len)) return false;
            continue;
        }
        switch (e->kind()) {
        case K_STRING:
            if (e->repeated()) {
                reinterpret_cast<std::vector<std::string>*>(p)->emplace_back((const char*)s, len);
            } else {
                if (e->flags & PF_ONEOF) ClearOneofSiblings(this, &d->fields[e->field]);
                reinterpret_cast<std::string*>(p)->assign((const char*)s, len);
                set_has(hb, *e);
            }
            break;
        case K_MESSAGE: {
            const FieldDescriptor* f = &d->fields[e->field];
            Message* sub = e->repeated() ? Reflection::AddMessage(this, f) : Reflection::MutableMessage(this, f);
            CodedInput in(s, len);
            if (!sub->MergePartialFromCodedInput(&in) || !in.at_limit()) return false;
            break;
        }
        default:
            return false;  // a scalar field sent length-delimited but not packable
        }
    }
    return true;
}

}  // namespace pb
}  // namespace mrpc
