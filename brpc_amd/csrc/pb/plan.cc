#include "pb/plan.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "pb/wire.h"

namespace mrpc {
namespace pb {

namespace {

PlanKind kind_of(FieldType t) {
    switch (t) {
    case FieldType::INT32:
    case FieldType::ENUM: return K_INT32;
    case FieldType::UINT32: return K_UINT32;
    case FieldType::SINT32: return K_SINT32;
    case FieldType::INT64:
    case FieldType::UINT64: return K_INT64;
    case FieldType::SINT64: return K_SINT64;
    case FieldType::BOOL: return K_BOOL;
    case FieldType::FLOAT:
    case FieldType::FIXED32:
    case FieldType::SFIXED32: return K_FIXED32;
    case FieldType::DOUBLE:
    case FieldType::FIXED64:
    case FieldType::SFIXED64: return K_FIXED64;
    case FieldType::STRING:
    case FieldType::BYTES: return K_STRING;
    case FieldType::GROUP:
    case FieldType::MESSAGE: return K_MESSAGE;
    }
    return K_INT32;
}

WireType natural_wire(PlanKind k) {
    switch (k) {
    case K_FIXED32: return WIRETYPE_FIXED32;
    case K_FIXED64: return WIRETYPE_FIXED64;
    case K_STRING:
    case K_MESSAGE: return WIRETYPE_LENGTH_DELIMITED;
    default: return WIRETYPE_VARINT;
    }
}

// True iff `d` or a type reachable through message fields has a required
// field. The visited set ends the walk on recursive types.
bool reaches_required(const Descriptor* d, std::set<const Descriptor*>* seen) {
    if (!d || !seen->insert(d).second) return false;
    for (const FieldDescriptor& f : d->fields) {
        if (f.is_required()) return true;
    }
    for (const FieldDescriptor& f : d->fields) {
        if (f.cpp_type() == CppType::MESSAGE && reaches_required(f.message_type, seen)) return true;
    }
    return false;
}

bool nonzero_default(const FieldDescriptor& f) {
    switch (f.cpp_type()) {
    case CppType::BOOL: return f.default_int != 0;
    case CppType::INT32:
    case CppType::ENUM: return (int32_t)f.default_int != 0;
    case CppType::UINT32: return (uint32_t)f.default_uint != 0;
    case CppType::INT64: return f.default_int != 0;
    case CppType::UINT64: return f.default_uint != 0;
    case CppType::FLOAT: {
        const float v = (float)f.default_double;
        uint32_t bits;
        memcpy(&bits, &v, 4);
        return bits != 0;
    }
    case CppType::DOUBLE: {
        uint64_t bits;
        memcpy(&bits, &f.default_double, 8);
        return bits != 0;
    }
    case CppType::STRING: return !f.default_string.empty();
    case CppType::MESSAGE: return false;
    }
    return false;
}

}  // namespace

const CodecPlan* CompileCodecPlan(const Descriptor* d) {
    CodecPlan* p = new CodecPlan;
    p->has_bits_offset = d->has_bits_offset;
    p->has_words = (d->num_has_bits + 31) / 32;
    for (uint16_t& x : p->dense) x = CodecPlan::kNone;
    p->by_has_bit.assign(p->has_words * 32, CodecPlan::kNone);
    p->entries.reserve(d->fields.size());
    for (size_t i = 0; i < d->fields.size() && i < CodecPlan::kNone; ++i) {
        const FieldDescriptor& f = d->fields[i];
        PlanEntry e;
        memset(&e, 0, sizeof(e));
        e.offset = f.offset;
        e.has_bit = f.has_bit;
        e.field = (uint16_t)i;
        e.ftype = (uint8_t)f.type;
        const PlanKind k = kind_of(f.type);
        PlanClass c = C_OPT;
        if (f.is_repeated()) c = f.packed && k < K_STRING ? C_REP_PACKED : C_REP;
        else if (k != K_MESSAGE && f.has_bit < 0) c = C_IMPLICIT;
        e.op = PlanOp(c, k);
        if (f.is_required()) e.flags |= PF_REQUIRED;
        if (f.oneof_index >= 0) e.flags |= PF_ONEOF;
        if (f.type == FieldType::GROUP) e.flags |= PF_GROUP;
        if (!f.is_repeated() && nonzero_default(f)) e.flags |= PF_NONZERO_DEFAULT;
        if (k == K_MESSAGE) {
            std::set<const Descriptor*> seen;
            if (reaches_required(f.message_type, &seen)) e.flags |= PF_SUB_NEEDS_INIT;
        }
        e.tag_len = (uint8_t)(write_varint(e.tag, make_tag(f.number, natural_wire(k))) - e.tag);
        write_varint(e.ptag, make_tag(f.number, WIRETYPE_LENGTH_DELIMITED));
        const uint16_t idx = (uint16_t)p->entries.size();
        p->entries.push_back(e);
        // a number listed twice resolves to its last field, as FindFieldByNumber does
        if (f.number > 0 && f.number < CodecPlan::kDense) p->dense[f.number] = idx;
        else if (f.number > 0) p->sparse.emplace_back((uint32_t)f.number, idx);
        if (e.flags & (PF_REQUIRED | PF_SUB_NEEDS_INIT)) p->init_entries.push_back(idx);
        // Clear() finds set scalars and strings from the has words; sub-messages go by their pointer
        if (!f.is_repeated() && k != K_MESSAGE && f.has_bit >= 0 && (size_t)f.has_bit < p->by_has_bit.size()) p->by_has_bit[f.has_bit] = idx;
        else p->no_has_bit.push_back(idx);
    }
    std::stable_sort(p->sparse.begin(), p->sparse.end(),
                     [](const std::pair<uint32_t, uint16_t>& a, const std::pair<uint32_t, uint16_t>& b) {
                         return a.first < b.first;
                     });
    for (size_t i = 0; i + 1 < p->sparse.size();) {
        if (p->sparse[i].first == p->sparse[i + 1].first) p->sparse.erase(p->sparse.begin() + i);
        else ++i;
    }
    p->needs_init_check = !p->init_entries.empty();

    const CodecPlan* expected = nullptr;
    if (d->codec_plan.compare_exchange_strong(expected, p, std::memory_order_acq_rel, std::memory_order_acquire)) return p;
    delete p;
    return expected;
}

void DeleteCodecPlan(const CodecPlan* p) { delete p; }

}  // namespace pb
}  // namespace mrpc
