// The codec against its own earlier behaviour: seeded messages of generated
// and dynamic types are serialized, parsed (whole, truncated, mutated, with
// wrong wire types) and re-serialized, and every result is compared byte for
// byte with tests/golden/pb_plan/corpus.txt, which this same file recorded
// when built against the descriptor-walking codec (see pb_plan_corpus.h).
// Then the properties the golden file cannot hold: Clear() equals a fresh
// instance, parsing into a dirty message, IsInitialized over required fields
// at depth, the packed-run sink hook, and first use of one descriptor from
// eight threads. Only API that the earlier codec had is used.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mrpc/proto/echo.pb.h"
#include "mrpc/proto/rpc_meta.pb.h"
#include "pb/dynamic.h"
#include "pb/parser.h"
#include "pb/wire.h"
#include "tests/pb_plan_corpus.h"
#include "tests/test.h"

using namespace mrpc;
using namespace mrpc::pb;

namespace {

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    uint64_t below(uint64_t n) { return next() % n; }
    // numbers that sit on the encoding's edges, or anywhere
    uint64_t number() {
        static const uint64_t kEdges[] = {0, 1, 127, 128, 16383, 16384, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull,
                                          0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull};
        if (below(3) == 0) return kEdges[below(12)];
        return next() >> below(64);
    }
    std::string text() {
        static const size_t kLens[] = {0, 1, 2, 5, 11, 19};
        std::string t(kLens[below(6)], 'a');
        for (char& c : t) c = (char)below(256);
        return t;
    }
};

struct Types {
    Importer imp{{}};
    bool ok = false;
    Types() {
        std::string err;
        ok = imp.ImportFromString("t.proto", pb_plan::Proto2Text(), &err) != nullptr &&
             imp.ImportFromString("t3.proto", pb_plan::Proto3Text(), &err) != nullptr;
        if (!ok) fprintf(stderr, "proto import: %s\n", err.c_str());
    }
    const Descriptor* desc(const std::string& name) const {
        if (name == "mrpc.policy.RpcMeta") return policy::RpcMeta::descriptor();
        if (name == "example.EchoRequest") return example::EchoRequest::descriptor();
        if (name == "example.EchoResponse") return example::EchoResponse::descriptor();
        return imp.FindMessageTypeByName(name);
    }
    Message* make(const std::string& name) const {
        const Descriptor* d = desc(name);
        return d ? d->NewMessage() : nullptr;
    }
};

const char* const kTypeNames[] = {"mrpc.policy.RpcMeta", "example.EchoRequest", "example.EchoResponse", "t.All", "t.Req",
                                  "t.Rec",               "t.NoReq",             "t.Wide",               "t3.P3"};
const int kSeedsPerType = 8;

void fill(Message* m, Rng* r, int depth, int percent);

void fill_field(Message* m, const FieldDescriptor* f, Rng* r, int depth, int percent) {
    const bool rep = f->is_repeated();
    const int n = rep ? (int)r->below(4) : 1;
    for (int i = 0; i < n; ++i) {
        const uint64_t v = r->number();
        switch (f->cpp_type()) {
        case CppType::INT32: rep ? Reflection::AddInt32(m, f, (int32_t)v) : Reflection::SetInt32(m, f, (int32_t)v); break;
        case CppType::INT64: rep ? Reflection::AddInt64(m, f, (int64_t)v) : Reflection::SetInt64(m, f, (int64_t)v); break;
        case CppType::UINT32: rep ? Reflection::AddUInt32(m, f, (uint32_t)v) : Reflection::SetUInt32(m, f, (uint32_t)v); break;
        case CppType::UINT64: rep ? Reflection::AddUInt64(m, f, v) : Reflection::SetUInt64(m, f, v); break;
        case CppType::FLOAT: {
            const float x = (float)(int32_t)v / 8.0f;
            rep ? Reflection::AddFloat(m, f, x) : Reflection::SetFloat(m, f, x);
            break;
        }
        case CppType::DOUBLE: {
            const double x = (double)(int64_t)v / 1024.0;
            rep ? Reflection::AddDouble(m, f, x) : Reflection::SetDouble(m, f, x);
            break;
        }
        case CppType::BOOL: rep ? Reflection::AddBool(m, f, v & 1) : Reflection::SetBool(m, f, v & 1); break;
        case CppType::ENUM: {
            const auto& vals = f->enum_type->values;
            const int x = vals[r->below(vals.size())].number;
            rep ? Reflection::AddEnumValue(m, f, x) : Reflection::SetEnumValue(m, f, x);
            break;
        }
        case CppType::STRING: rep ? Reflection::AddString(m, f, r->text()) : Reflection::SetString(m, f, r->text()); break;
        case CppType::MESSAGE:
            if (depth >= 3) break;
            fill(rep ? Reflection::AddMessage(m, f) : Reflection::MutableMessage(m, f), r, depth + 1, percent);
            break;
        }
    }
}

void fill(Message* m, Rng* r, int depth, int percent) {
    const Descriptor* d = m->GetDescriptor();
    for (const FieldDescriptor& f : d->fields) {
        if ((int)r->below(100) < percent) fill_field(m, &f, r, depth, percent);
    }
}

// The message of (type, seed). Seeds 0..5 of t.All are the value edges:
// empty, packed runs of 0/1/127/128 payload bytes, negative int32, set empty
// strings, and a message of unknown fields only.
void build(const std::string& type, int seed, Message* m) {
    Rng r((uint64_t)seed * 131 + type.size() * 7 + (unsigned char)type.back());
    const Descriptor* d = m->GetDescriptor();
    if (type == "t.All" && seed <= 5) {
        if (seed >= 1 && seed <= 4) {
            const int n = seed == 1 ? 0 : seed == 2 ? 1 : seed == 3 ? 127 : 128;
            for (int i = 0; i < n; ++i) Reflection::AddInt64(m, d->FindFieldByName("p_i64"), i % 100);
            for (int i = 0; i < n; ++i) Reflection::AddBool(m, d->FindFieldByName("p_b"), i & 1);
            for (int i = 0; i < n; ++i) Reflection::AddInt32(m, d->FindFieldByName("p_far"), i % 60);
            Reflection::AddInt32(m, d->FindFieldByName("p_i32"), -1);
            Reflection::AddInt32(m, d->FindFieldByName("r_i32"), -2147483647 - 1);
            Reflection::SetInt32(m, d->FindFieldByName("i32"), -seed);
            Reflection::SetEnumValue(m, d->FindFieldByName("col"), -3);
            Reflection::SetString(m, d->FindFieldByName("str"), "");
            Reflection::SetString(m, d->FindFieldByName("byt"), "");
            Reflection::SetString(m, d->FindFieldByName("d_str"), "");
            Reflection::SetString(m, d->FindFieldByName("n2047"), std::string(seed == 3 ? 127 : 128, 'x'));
            Reflection::SetString(m, d->FindFieldByName("n2048"), "");
            Reflection::SetInt64(m, d->FindFieldByName("big"), -1);
            Reflection::SetInt32(m, d->FindFieldByName("n127"), 127);
            Reflection::SetInt32(m, d->FindFieldByName("n128"), 128);
            Reflection::AddString(m, d->FindFieldByName("r_str"), "");
        } else if (seed == 5) {
            // field 1000 varint 5, field 1001 "ab", field 1002 fixed32
            *m->mutable_unknown_fields() = std::string("\xc0\x3e\x05\xca\x3e\x02" "ab\xd5\x3e\x01\x02\x03\x04", 14);
        }
        return;
    }
    if (type == "example.EchoRequest" && seed == 0) {
        Reflection::SetString(m, d->FindFieldByName("message"), std::string(32, 'x'));
        return;
    }
    if (type == "mrpc.policy.RpcMeta" && seed <= 1) {
        policy::RpcMeta* meta = static_cast<policy::RpcMeta*>(m);
        if (seed == 0) {
            meta->mutable_request()->set_service_name("example.EchoService");
            meta->mutable_request()->set_method_name("Echo");
        } else {
            meta->mutable_response();
            meta->set_compress_type(0);
        }
        meta->set_correlation_id(0x100000001ll * 77);
        return;
    }
    fill(m, &r, 0, type == "t.All" ? 18 : 45);
}

// ParseFromArray of `in` into m, then what m holds: "<verdict> <hex>"
std::string parse_result(Message* m, const std::string& in) {
    const bool ok = m->ParseFromArray(in.data(), in.size());
    return std::string(ok ? "1 " : "0 ") + pb_plan::Hex(m->SerializeAsString());
}

void add_parse(const Types& t, const std::string& type, const std::string& in, std::vector<std::string>* out) {
    std::unique_ptr<Message> m(t.make(type));
    out->push_back("P " + type + " " + pb_plan::Hex(in) + " " + parse_result(m.get(), in));
}

std::string tag_bytes(uint32_t number, uint32_t wt) {
    uint8_t b[8];
    return std::string((const char*)b, write_varint(b, ((uint64_t)number << 3) | wt) - b);
}

struct RecordingSink : PackedRunSink {
    std::vector<PackedRun> runs;
    size_t min_elems() const override { return 4; }
    void Take(PackedRun&& run) override { runs.push_back(std::move(run)); }
};

std::vector<std::string> sink_lines() {
    std::vector<std::string> out;
    for (int n : {3, 4, 2047, 2048, 2049}) {
        example::EchoRequest req;
        req.set_message("m");
        for (int i = 0; i < n; ++i) req.add_ids(i % 97 == 0 ? -i : (int64_t)(i * 37) % 140);
        RecordingSink sink;
        PackedRunSink* prev = SetThreadPackedRunSink(&sink);
        std::string wire;
        wire.resize(req.ByteSizeLong());
        uint8_t* begin = (uint8_t*)&wire[0];
        uint8_t* end = req.SerializeWithCachedSizesToArray(begin);
        SetThreadPackedRunSink(prev);
        std::string line = "S " + std::to_string(n);
        if ((size_t)(end - begin) != wire.size()) line += " size-mismatch";
        line += " " + std::to_string(sink.runs.size());
        for (const PackedRun& run : sink.runs) {
            line += " " + std::to_string(run.n) + " " + std::to_string(run.elem_bytes) + " " + std::to_string((int)run.type) +
                    " " + std::to_string(run.bytes) + " " + std::to_string(run.dst - begin) + " ";
            for (size_t i = 0; i < run.chunk_bytes.size(); ++i) line += (i ? "," : "") + std::to_string(run.chunk_bytes[i]);
            if (run.values != req.ids().data()) line += " values-moved";
            EncodePackedRunOnHost(run);
        }
        out.push_back(line + " " + pb_plan::Hex(wire));
    }
    return out;
}

// Every line of the corpus, computed with the codec this binary links.
std::vector<std::string> compute_corpus(const Types& t) {
    std::vector<std::string> out;
    std::vector<std::pair<std::string, std::string>> wires;  // type, bytes
    for (const char* type : kTypeNames) {
        for (int seed = 0; seed < kSeedsPerType; ++seed) {
            std::unique_ptr<Message> m(t.make(type));
            build(type, seed, m.get());
            const std::string w = m->SerializeAsString();
            out.push_back(std::string("M ") + type + " " + std::to_string(seed) + " " + pb_plan::Hex(w) + " " +
                          (m->IsInitialized() ? "1" : "0"));
            wires.emplace_back(type, w);
        }
    }
    for (const auto& tw : wires) add_parse(t, tw.first, tw.second, &out);
    // truncations at every length of a few small messages of each type
    Rng r(4242);
    for (const char* type : kTypeNames) {
        int taken = 0;
        for (const auto& tw : wires) {
            if (tw.first != type || tw.second.size() < 4 || tw.second.size() > 40 || taken == 1) continue;
            ++taken;
            for (size_t n = 0; n < tw.second.size(); ++n) add_parse(t, type, tw.second.substr(0, n), &out);
        }
    }
    // single-byte mutations
    for (size_t i = 0; i < wires.size(); i += 3) {
        if (wires[i].second.empty() || wires[i].second.size() > 200) continue;
        for (int k = 0; k < 4; ++k) {
            std::string w = wires[i].second;
            w[r.below(w.size())] ^= (char)(1u << r.below(8));
            add_parse(t, wires[i].first, w, &out);
        }
    }
    // wrong wire types, both forms of packable fields, groups, bad tags
    const std::string A = "t.All";
    add_parse(t, A, tag_bytes(1, 2) + std::string("\x03" "abc", 4), &out);            // int32 as bytes
    add_parse(t, A, tag_bytes(14, 0) + std::string("\x05", 1), &out);                  // string as varint
    add_parse(t, A, tag_bytes(7, 1) + std::string(8, '\x01'), &out);                   // fixed32 as fixed64
    add_parse(t, A, tag_bytes(8, 5) + std::string(4, '\x01'), &out);                   // fixed64 as fixed32
    add_parse(t, A, tag_bytes(17, 0) + std::string("\x01", 1), &out);                  // message as varint
    add_parse(t, A, tag_bytes(41, 0) + "\x01" + tag_bytes(41, 0) + "\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01", &out);
    add_parse(t, A, tag_bytes(21, 2) + std::string("\x03\x01\x80\x01", 4), &out);      // unpacked field, packed form
    add_parse(t, A, tag_bytes(21, 2) + std::string("\x02\x01\x80", 3), &out);          // ... ending inside a varint
    add_parse(t, A, tag_bytes(47, 5) + std::string(4, '\x02'), &out);                  // packed fixed32, unpacked form
    add_parse(t, A, tag_bytes(47, 2) + std::string("\x05" "12345", 6), &out);          // ... 5 bytes: not a multiple of 4
    add_parse(t, A, tag_bytes(52, 2) + std::string("\x08" "12345678", 9), &out);
    add_parse(t, A, tag_bytes(53, 2) + std::string("\x03\x00\x02\x81\x00", 5), &out);  // bools, one over-long
    add_parse(t, A, tag_bytes(45, 2) + std::string("\x02\x03\x04", 3) + tag_bytes(46, 0) + "\x03", &out);
    add_parse(t, A, tag_bytes(34, 0) + "\x01", &out);                                   // repeated string as varint
    add_parse(t, A, tag_bytes(1, 3) + tag_bytes(2, 0) + "\x01" + tag_bytes(1, 4), &out);  // a group on a known number
    add_parse(t, A, tag_bytes(900, 3) + tag_bytes(2, 0) + "\x01" + tag_bytes(900, 4) + tag_bytes(1, 0) + "\x07", &out);
    add_parse(t, A, tag_bytes(900, 3) + tag_bytes(901, 4), &out);                       // group ended by another number
    add_parse(t, A, tag_bytes(900, 3) + tag_bytes(2, 0) + "\x01", &out);                // group never ended
    add_parse(t, A, tag_bytes(1, 4), &out);                                             // END_GROUP alone
    add_parse(t, A, std::string("\x00", 1), &out);                                      // tag 0
    add_parse(t, A, tag_bytes(1, 0) + "\x01" + std::string("\x00", 1), &out);           // tag 0 at the end
    add_parse(t, A, std::string("\x01\x00\x00\x00\x00\x00\x00\x00\x00", 9), &out);       // field number 0
    add_parse(t, A, tag_bytes(1, 6) + "\x01", &out);                                    // wire type 6
    add_parse(t, A, tag_bytes(1, 0) + std::string(11, '\xff'), &out);                   // varint that never ends
    add_parse(t, A, std::string("\xff\xff\xff\xff\x7f\x01", 6), &out);                  // tag above 32 bits
    add_parse(t, A, tag_bytes(14, 2) + "\x7f" + "short", &out);                         // length past the end
    add_parse(t, A, tag_bytes(71, 0) + "\x01" + tag_bytes(72, 2) + "\x01z" + tag_bytes(73, 2) + std::string("\x00", 1), &out);
    add_parse(t, A, tag_bytes(73, 2) + std::string("\x02\x08\x01", 3) + tag_bytes(71, 0) + "\x09", &out);  // oneof, last wins
    add_parse(t, A, tag_bytes(17, 2) + std::string("\x03\x08\x01\x08", 4), &out);       // sub-message ends inside a field
    add_parse(t, A, tag_bytes(17, 2) + "\x02\x08\x01" + tag_bytes(17, 2) + "\x02\x22\x00", &out);  // sub-message merged twice
    add_parse(t, A, tag_bytes(536870911, 0) + "\x01" + tag_bytes(536870910, 0) + "\x01", &out);
    add_parse(t, A, tag_bytes(2047, 2) + "\x01q" + tag_bytes(2048, 2) + "\x01r" + tag_bytes(2049, 0) + "\x05" +
                        tag_bytes(2050, 0) + "\x05", &out);
    add_parse(t, A, tag_bytes(127, 0) + "\x01" + tag_bytes(128, 0) + "\x02" + tag_bytes(129, 0) + "\x03", &out);
    add_parse(t, "t3.P3", tag_bytes(1, 0) + std::string("\x00", 1) + tag_bytes(2, 2) + std::string("\x00", 1) + tag_bytes(5, 0) + "\x07", &out);
    add_parse(t, "t.Wide", tag_bytes(33, 2) + "\x01w" + tag_bytes(40, 0) + "\x01" + tag_bytes(1, 0) + "\x02", &out);
    add_parse(t, "mrpc.policy.RpcMeta", tag_bytes(100, 2) + std::string("\x00", 1) + tag_bytes(101, 2) + std::string("\x00", 1) +
                                            tag_bytes(102, 0) + "\x01" + tag_bytes(103, 0) + "\x01", &out);
    // nesting at and past the depth limit (t.Rec.next = 2)
    for (int depth : {99, 100, 101}) {
        std::string w;
        for (int i = 0; i < depth; ++i) {
            uint8_t b[8];
            w = tag_bytes(2, 2) + std::string((const char*)b, write_varint(b, w.size()) - b) + w;
        }
        add_parse(t, "t.Rec", w, &out);
    }
    for (const std::string& l : sink_lines()) out.push_back(l);
    return out;
}

// m against a fresh instance of its type, through everything observable
void expect_same_as_fresh(const Message& m, const std::string& ctx) {
    const Descriptor* d = m.GetDescriptor();
    std::unique_ptr<Message> fresh(d->NewMessage());
    EXPECT_TRUE_M(m.SerializeAsString() == fresh->SerializeAsString(), ctx);
    EXPECT_TRUE_M(m.DebugString() == fresh->DebugString(), ctx);
    EXPECT_TRUE_M(m.unknown_fields().empty(), ctx);
    for (const FieldDescriptor& fd : d->fields) {
        const FieldDescriptor* f = &fd;
        const std::string c = ctx + " " + f->name;
        EXPECT_TRUE_M(Reflection::HasField(m, f) == Reflection::HasField(*fresh, f), c);
        EXPECT_TRUE_M(Reflection::FieldSize(m, f) == Reflection::FieldSize(*fresh, f), c);
        if (f->is_repeated()) continue;
        switch (f->cpp_type()) {
        case CppType::INT32: EXPECT_TRUE_M(Reflection::GetInt32(m, f) == Reflection::GetInt32(*fresh, f), c); break;
        case CppType::INT64: EXPECT_TRUE_M(Reflection::GetInt64(m, f) == Reflection::GetInt64(*fresh, f), c); break;
        case CppType::UINT32: EXPECT_TRUE_M(Reflection::GetUInt32(m, f) == Reflection::GetUInt32(*fresh, f), c); break;
        case CppType::UINT64: EXPECT_TRUE_M(Reflection::GetUInt64(m, f) == Reflection::GetUInt64(*fresh, f), c); break;
        case CppType::FLOAT: EXPECT_TRUE_M(Reflection::GetFloat(m, f) == Reflection::GetFloat(*fresh, f), c); break;
        case CppType::DOUBLE: EXPECT_TRUE_M(Reflection::GetDouble(m, f) == Reflection::GetDouble(*fresh, f), c); break;
        case CppType::BOOL: EXPECT_TRUE_M(Reflection::GetBool(m, f) == Reflection::GetBool(*fresh, f), c); break;
        case CppType::ENUM: EXPECT_TRUE_M(Reflection::GetEnumValue(m, f) == Reflection::GetEnumValue(*fresh, f), c); break;
        case CppType::STRING: EXPECT_TRUE_M(Reflection::GetString(m, f) == Reflection::GetString(*fresh, f), c); break;
        case CppType::MESSAGE: break;  // HasField above: the pointer is null again
        }
    }
}

}  // namespace

TEST(PbPlan, golden_differential) {
    Types t;
    ASSERT_TRUE(t.ok);
    const std::vector<std::string> now = compute_corpus(t);
    if (const char* rec = getenv("MRPC_PB_PLAN_RECORD")) {
        FILE* f = fopen(rec, "w");
        ASSERT_TRUE(f != nullptr);
        fprintf(f, "# recorded by pb_plan_unittest.cc (MRPC_PB_PLAN_RECORD) with the descriptor-walking codec; see pb_plan_corpus.h\n");
        for (const std::string& l : now) fprintf(f, "%s\n", l.c_str());
        fclose(f);
        return;
    }
    std::vector<std::string> golden;
    ASSERT_TRUE_M(pb_plan::ReadLines(pb_plan::CorpusPath(), &golden), pb_plan::CorpusPath());
    ASSERT_EQ(golden.size(), now.size());
    ASSERT_GT(golden.size(), (size_t)300);
    int shown = 0;
    for (size_t i = 0; i < golden.size(); ++i) {
        if (golden[i] == now[i]) continue;
        if (++shown <= 5) {
            EXPECT_TRUE_M(false, "line " + std::to_string(i + 1) + "\n  golden " + golden[i].substr(0, 300) + "\n  now    " +
                                     now[i].substr(0, 300));
        }
    }
    EXPECT_EQ(shown, 0);
}

// The value edges the issue names are really in what the corpus holds.
TEST(PbPlan, corpus_covers_the_edges) {
    Types t;
    ASSERT_TRUE(t.ok);
    const Descriptor* all = t.desc("t.All");
    int has_bits = 0;
    for (const FieldDescriptor& f : all->fields) has_bits += f.has_bit >= 0;
    EXPECT_GE(has_bits, 33);
    for (int seed = 1; seed <= 4; ++seed) {
        std::unique_ptr<Message> m(t.make("t.All"));
        build("t.All", seed, m.get());
        const std::string w = m->SerializeAsString();
        const int n = seed == 1 ? 0 : seed == 2 ? 1 : seed == 3 ? 127 : 128;
        // p_i64 = 42: tag d2 02, then the length varint (absent when the run is empty)
        std::string want = std::string("\xd2\x02", 2);
        if (n >= 128) want += std::string("\x80\x01", 2);
        else want += (char)n;
        EXPECT_TRUE_M((w.find(want) != std::string::npos) == (n > 0), "seed " + std::to_string(seed));
        // negative int32: ten bytes after the tag of field 1
        EXPECT_TRUE(w.compare(0, 1, "\x08") == 0 && (unsigned char)w[10] == 0x01 && (unsigned char)w[9] == 0xff);
        EXPECT_TRUE(Reflection::HasField(*m, all->FindFieldByName("str")));
        EXPECT_TRUE(w.find(std::string("\x72\x00", 2)) != std::string::npos);  // str = 14, set and empty
    }
    std::unique_ptr<Message> unk(t.make("t.All"));
    build("t.All", 5, unk.get());
    EXPECT_EQ(unk->SerializeAsString().size(), (size_t)14);
    EXPECT_EQ(unk->DebugString(), std::string());
}

TEST(PbPlan, clear_equals_fresh_and_parse_into_dirty) {
    Types t;
    ASSERT_TRUE(t.ok);
    for (const char* type : kTypeNames) {
        for (int seed = 0; seed < kSeedsPerType; ++seed) {
            const std::string ctx = std::string(type) + " seed " + std::to_string(seed);
            std::unique_ptr<Message> m(t.make(type));
            build(type, seed, m.get());
            const std::string wire = m->SerializeAsString();
            const std::string text = m->DebugString();
            m->Clear();
            expect_same_as_fresh(*m, ctx + " cleared");
            m->Clear();  // an already-clear message
            expect_same_as_fresh(*m, ctx + " cleared twice");
            // a message dirty with another seed's fields parses like a fresh one
            std::unique_ptr<Message> dirty(t.make(type));
            build(type, (seed + 3) % kSeedsPerType, dirty.get());
            std::unique_ptr<Message> fresh(t.make(type));
            const bool ok_dirty = dirty->ParseFromArray(wire.data(), wire.size());
            const bool ok_fresh = fresh->ParseFromArray(wire.data(), wire.size());
            EXPECT_TRUE_M(ok_dirty == ok_fresh, ctx);
            EXPECT_TRUE_M(dirty->SerializeAsString() == wire, ctx);
            EXPECT_TRUE_M(fresh->SerializeAsString() == wire, ctx);
            EXPECT_TRUE_M(dirty->DebugString() == text, ctx);
            EXPECT_TRUE_M(fresh->DebugString() == text, ctx);
        }
    }
}

TEST(PbPlan, explicit_defaults_come_back) {
    Types t;
    ASSERT_TRUE(t.ok);
    const Descriptor* d = t.desc("t.All");
    std::unique_ptr<Message> m(d->NewMessage());
    Reflection::SetInt32(m.get(), d->FindFieldByName("d_i32"), 5);
    Reflection::SetUInt64(m.get(), d->FindFieldByName("d_u64"), 0);
    Reflection::SetString(m.get(), d->FindFieldByName("d_str"), "");
    Reflection::SetDouble(m.get(), d->FindFieldByName("d_db"), 0);
    Reflection::SetBool(m.get(), d->FindFieldByName("d_b"), false);
    Reflection::SetEnumValue(m.get(), d->FindFieldByName("d_col"), 0);
    Reflection::SetFloat(m.get(), d->FindFieldByName("d_fl"), 0);
    Reflection::SetInt64(m.get(), d->FindFieldByName("d_s64"), 0);
    m->Clear();
    EXPECT_EQ(Reflection::GetInt32(*m, d->FindFieldByName("d_i32")), -7);
    EXPECT_EQ(Reflection::GetUInt64(*m, d->FindFieldByName("d_u64")), (uint64_t)1234567890123ull);
    EXPECT_EQ(Reflection::GetString(*m, d->FindFieldByName("d_str")), std::string("hello"));
    EXPECT_EQ(Reflection::GetDouble(*m, d->FindFieldByName("d_db")), 2.5);
    EXPECT_EQ(Reflection::GetBool(*m, d->FindFieldByName("d_b")), true);
    EXPECT_EQ(Reflection::GetEnumValue(*m, d->FindFieldByName("d_col")), 7);
    EXPECT_EQ(Reflection::GetFloat(*m, d->FindFieldByName("d_fl")), -1.5f);
    EXPECT_EQ(Reflection::GetInt64(*m, d->FindFieldByName("d_s64")), (int64_t)-9);
    EXPECT_FALSE(Reflection::HasField(*m, d->FindFieldByName("d_str")));
    // and a parse that does not mention them leaves them at their defaults
    Reflection::SetString(m.get(), d->FindFieldByName("d_str"), "other");
    EXPECT_TRUE(m->ParseFromArray("\x08\x01", 2));
    EXPECT_EQ(Reflection::GetString(*m, d->FindFieldByName("d_str")), std::string("hello"));
}

TEST(PbPlan, is_initialized) {
    Types t;
    ASSERT_TRUE(t.ok);
    // no required field anywhere, recursive types included: plan compilation ends
    std::unique_ptr<Message> none(t.make("t.NoReq"));
    EXPECT_TRUE(none->IsInitialized());
    const Descriptor* nd = none->GetDescriptor();
    Reflection::AddMessage(none.get(), nd->FindFieldByName("recs"));
    Reflection::MutableMessage(Reflection::MutableMessage(none.get(), nd->FindFieldByName("rec")),
                               t.desc("t.Rec")->FindFieldByName("next"));
    EXPECT_TRUE(none->IsInitialized());
    std::unique_ptr<Message> rec(t.make("t.Rec"));
    EXPECT_TRUE(rec->IsInitialized());

    const Descriptor* req = t.desc("t.Req");
    const Descriptor* mid = t.desc("t.Mid");
    const Descriptor* leaf = t.desc("t.Leaf");
    std::unique_ptr<Message> m(req->NewMessage());
    EXPECT_FALSE(m->IsInitialized());  // depth 0
    EXPECT_EQ(m->InitializationErrorString(), std::string("id"));
    Reflection::SetInt32(m.get(), req->FindFieldByName("id"), 1);
    EXPECT_TRUE(m->IsInitialized());
    // depth 2: mid.leaf.name
    Message* l = Reflection::MutableMessage(Reflection::MutableMessage(m.get(), req->FindFieldByName("mid")), mid->FindFieldByName("leaf"));
    EXPECT_FALSE(m->IsInitialized());
    EXPECT_EQ(m->InitializationErrorString(), std::string("mid.leaf.name"));
    Reflection::SetString(l, leaf->FindFieldByName("name"), "");
    EXPECT_TRUE(m->IsInitialized());
    // inside repeated messages: mids[1].leaves[0].name
    Reflection::AddMessage(m.get(), req->FindFieldByName("mids"));
    Message* m1 = Reflection::AddMessage(m.get(), req->FindFieldByName("mids"));
    EXPECT_TRUE(m->IsInitialized());
    Message* l1 = Reflection::AddMessage(m1, mid->FindFieldByName("leaves"));
    EXPECT_FALSE(m->IsInitialized());
    EXPECT_EQ(m->InitializationErrorString(), std::string("mids[1].leaves[0].name"));
    const std::string partial = m->SerializeAsString();
    std::unique_ptr<Message> back(req->NewMessage());
    EXPECT_FALSE(back->ParseFromArray(partial.data(), partial.size()));
    EXPECT_TRUE(back->ParsePartialFromArray(partial.data(), partial.size()));
    Reflection::SetString(l1, leaf->FindFieldByName("name"), "n");
    EXPECT_TRUE(m->IsInitialized());
    // the generated types of the small-RPC path
    policy::RpcMeta meta;
    EXPECT_TRUE(meta.IsInitialized());
    meta.mutable_request();
    EXPECT_FALSE(meta.IsInitialized());
    meta.mutable_request()->set_service_name("s");
    meta.mutable_request()->set_method_name("m");
    EXPECT_TRUE(meta.IsInitialized());
    example::EchoResponse res;
    EXPECT_FALSE(res.IsInitialized());
    res.set_message("");
    EXPECT_TRUE(res.IsInitialized());
}

TEST(PbPlan, sink_hook) {
    // below min_elems() the sink is not called and the bytes are plain
    example::EchoRequest req;
    req.set_message("m");
    for (int i = 0; i < 3; ++i) req.add_ids(i * 1000);
    const std::string plain = req.SerializeAsString();
    RecordingSink sink;
    PackedRunSink* prev = SetThreadPackedRunSink(&sink);
    const std::string with_sink = req.SerializeAsString();
    req.add_ids(4);
    std::string four;
    four.resize(req.ByteSizeLong());
    req.SerializeWithCachedSizesToArray((uint8_t*)&four[0]);
    SetThreadPackedRunSink(prev);
    EXPECT_TRUE(with_sink == plain);
    ASSERT_EQ(sink.runs.size(), (size_t)1);
    const PackedRun& run = sink.runs[0];
    EXPECT_EQ(run.n, (size_t)4);
    EXPECT_EQ(run.elem_bytes, (size_t)8);
    EXPECT_TRUE(run.type == FieldType::INT64);
    EXPECT_EQ(run.bytes, (size_t)(1 + 2 + 2 + 1));
    ASSERT_EQ(run.chunk_bytes.size(), (size_t)1);
    EXPECT_EQ(run.chunk_bytes[0], (uint32_t)6);
    // "m" field (3 bytes), tag 0x42, length 6
    EXPECT_EQ((size_t)(run.dst - (uint8_t*)&four[0]), (size_t)5);
    EncodePackedRunOnHost(run);
    EXPECT_TRUE(four == req.SerializeAsString());
    // runs of 3, 4, 2047, 2048 and 2049 elements are the S lines of the
    // golden file (sink_lines), compared in golden_differential
}

TEST(PbPlan, first_use_from_eight_threads) {
    // a descriptor no codec call has touched yet: every thread's first
    // serialize may be the one that compiles and publishes its plan
    Types t;
    ASSERT_TRUE(t.ok);
    const int kThreads = 8;
    std::vector<std::unique_ptr<Message>> msgs;
    for (int i = 0; i < kThreads; ++i) {
        msgs.emplace_back(t.make("t.All"));
        Rng r(99);
        fill(msgs.back().get(), &r, 0, 50);  // Reflection setters only: no codec use
    }
    std::vector<std::string> wires(kThreads);
    std::atomic<int> ready{0};
    std::vector<std::thread> threads;
    for (int i = 0; i < kThreads; ++i) {
        threads.emplace_back([&, i] {
            ready.fetch_add(1);
            while (ready.load() < kThreads) {
            }
            wires[i] = msgs[i]->SerializeAsString();
        });
    }
    for (auto& th : threads) th.join();
    EXPECT_GT(wires[0].size(), (size_t)50);
    for (int i = 1; i < kThreads; ++i) EXPECT_TRUE(wires[i] == wires[0]);
    std::unique_ptr<Message> back(t.make("t.All"));
    EXPECT_TRUE(back->ParseFromArray(wires[0].data(), wires[0].size()));
    EXPECT_TRUE(back->SerializeAsString() == wires[0]);
}
