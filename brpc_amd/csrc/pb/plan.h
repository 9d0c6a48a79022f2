// CodecPlan: what the codec needs of a Descriptor, compiled once into
// contiguous 24-byte entries. Size, serialize, parse, Clear and
// IsInitialized (message.cc) walk these instead of the FieldDescriptors,
// which are several cache lines each and re-derive the storage type, the
// wire type and the tag on every visit. Entries stand in d->fields order, so
// the wire output keeps its field order.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "pb/descriptor.h"

namespace mrpc {
namespace pb {

// Storage x wire encoding of one element. Kinds below K_STRING are packable;
// types that store and decode alike share a kind (int64/uint64, the 4-byte
// and the 8-byte fixed types).
enum PlanKind : uint8_t {
    K_INT32 = 0,  // int32, enum: varint, negatives sign-extended to 10 bytes
    K_UINT32,
    K_SINT32,
    K_INT64,  // int64, uint64
    K_SINT64,
    K_BOOL,
    K_FIXED32,  // fixed32, sfixed32, float
    K_FIXED64,  // fixed64, sfixed64, double
    K_STRING,   // string, bytes
    K_MESSAGE,  // message (and group, which the parser only skips)
};
// Label x presence rule.
enum PlanClass : uint8_t {
    C_OPT = 0,       // singular with a has-bit; messages: present iff non-null
    C_IMPLICIT = 1,  // proto3 singular without has-bit: present iff non-zero
    C_REP = 2,       // repeated, one tag per element
    C_REP_PACKED = 3,
};
constexpr uint8_t PlanOp(PlanClass c, PlanKind k) { return (uint8_t)((c << 4) | k); }
enum : uint8_t {
    OPT_INT32 = PlanOp(C_OPT, K_INT32),
    OPT_STRING = PlanOp(C_OPT, K_STRING),
    OPT_MESSAGE = PlanOp(C_OPT, K_MESSAGE),
    IMPLICIT_INT32 = PlanOp(C_IMPLICIT, K_INT32),
    REP_STRING = PlanOp(C_REP, K_STRING),
    REP_MESSAGE = PlanOp(C_REP, K_MESSAGE),
    REP_PACKED_INT64 = PlanOp(C_REP_PACKED, K_INT64),
};

enum PlanFlag : uint8_t {
    PF_REQUIRED = 1,
    PF_ONEOF = 2,
    PF_NONZERO_DEFAULT = 4,  // Clear() must go to the FieldDescriptor for the value
    PF_GROUP = 8,            // parse: always skipped into the unknown fields
    PF_SUB_NEEDS_INIT = 16,  // message field whose type can reach a required field
};

struct PlanEntry {
    uint32_t offset;
    int32_t has_bit;  // or -1
    uint16_t field;   // index into Descriptor::fields, for the rare paths
    uint8_t op;       // PlanOp(class, kind)
    uint8_t flags;
    uint8_t ftype;  // FieldType, for the packed-run hook and the typed loops
    uint8_t tag_len;
    uint8_t tag[5];   // tag with the natural wire type
    uint8_t ptag[5];  // tag with WIRETYPE_LENGTH_DELIMITED (packed form)

    PlanKind kind() const { return (PlanKind)(op & 15); }
    PlanClass cls() const { return (PlanClass)(op >> 4); }
    bool repeated() const { return (op >> 4) >= C_REP; }
    uint32_t wire_type() const { return tag[0] & 7u; }
};
static_assert(sizeof(PlanEntry) == 24, "PlanEntry is meant to stay compact");

struct CodecPlan {
    static constexpr int kDense = 128;
    static constexpr uint16_t kNone = 0xFFFF;

    std::vector<PlanEntry> entries;
    uint32_t has_bits_offset = 0;
    uint32_t has_words = 0;
    // number -> entry: [0, kDense) direct, above that sorted by number
    uint16_t dense[kDense];
    std::vector<std::pair<uint32_t, uint16_t>> sparse;
    // IsInitialized: nothing to do when false, else only these entries
    // (required ones and message fields flagged PF_SUB_NEEDS_INIT)
    bool needs_init_check = false;
    std::vector<uint16_t> init_entries;
    // Clear: has-bit -> entry, and the entries that have none
    std::vector<uint16_t> by_has_bit;
    std::vector<uint16_t> no_has_bit;

    const PlanEntry* Find(uint32_t number) const {
        if (number < (uint32_t)kDense) {
            const uint16_t i = dense[number];
            return i == kNone ? nullptr : &entries[i];
        }
        size_t lo = 0, hi = sparse.size();
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if (sparse[mid].first < number) lo = mid + 1;
            else hi = mid;
        }
        return lo < sparse.size() && sparse[lo].first == number ? &entries[sparse[lo].second] : nullptr;
    }
};

// Compiles d's plan on first use and publishes it on the descriptor; when
// two threads race, the loser deletes its copy. Not called from
// BuildIndex(): message_type pointers into other files may be linked later.
const CodecPlan* CompileCodecPlan(const Descriptor* d);
inline const CodecPlan* PlanOf(const Descriptor* d) {
    const CodecPlan* p = d->codec_plan.load(std::memory_order_acquire);
    return p ? p : CompileCodecPlan(d);
}
void DeleteCodecPlan(const CodecPlan* p);

}  // namespace pb
}  // namespace mrpc
