// Shared by pb_plan_unittest.cc and standalone/pb_plan_sanitize_main.cc: the
// proto text of the dynamic test types, and the reading of
// tests/golden/pb_plan/corpus.txt. One record per line, fields separated by
// one space, "-" for an empty byte string:
//   M <type> <seed> <hex of the serialized message> <IsInitialized 0|1>
//   P <type> <hex input> <ParseFromArray 0|1> <hex of the message re-serialized after the parse>
//   S <elements> <n> <elem_bytes> <field type> <bytes> <dst offset> <chunk_bytes,...|-> <hex output>
// The file was written by pb_plan_unittest.cc built against the codec as it
// was before the CodecPlan (MRPC_PB_PLAN_RECORD=<path> records instead of
// comparing), so it is the old descriptor walk's behaviour, byte for byte.
#pragma once

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <unistd.h>

namespace pb_plan {

inline std::string Proto2Text() {
    std::string s = R"(
syntax = "proto2";
package t;
enum Color { RED = 0; GREEN = 1; BLUE = 7; }
message Leaf { optional int32 v = 1; required string name = 2; }
message Mid { optional Leaf leaf = 1; repeated Leaf leaves = 2; optional int32 x = 3; }
message Req { required int32 id = 1; optional Mid mid = 2; repeated Mid mids = 3; optional string note = 4; }
message Rec { optional int32 v = 1; optional Rec next = 2; repeated Rec kids = 3; optional string s = 4; }
message NoReq { optional int32 a = 1; optional Rec rec = 2; repeated Rec recs = 3; }
message All {
  optional int32 i32 = 1; optional int64 i64 = 2; optional uint32 u32 = 3; optional uint64 u64 = 4;
  optional sint32 s32 = 5; optional sint64 s64 = 6; optional fixed32 f32 = 7; optional fixed64 f64 = 8;
  optional sfixed32 sf32 = 9; optional sfixed64 sf64 = 10; optional float fl = 11; optional double db = 12;
  optional bool b = 13; optional string str = 14; optional bytes byt = 15; optional Color col = 16;
  optional Rec rec = 17;
  repeated int32 r_i32 = 21; repeated int64 r_i64 = 22; repeated uint32 r_u32 = 23; repeated uint64 r_u64 = 24;
  repeated sint32 r_s32 = 25; repeated sint64 r_s64 = 26; repeated fixed32 r_f32 = 27; repeated fixed64 r_f64 = 28;
  repeated sfixed32 r_sf32 = 29; repeated sfixed64 r_sf64 = 30; repeated float r_fl = 31; repeated double r_db = 32;
  repeated bool r_b = 33; repeated string r_str = 34; repeated bytes r_byt = 35; repeated Color r_col = 36;
  repeated Rec r_rec = 37;
  repeated int32 p_i32 = 41 [packed = true]; repeated int64 p_i64 = 42 [packed = true];
  repeated uint32 p_u32 = 43 [packed = true]; repeated uint64 p_u64 = 44 [packed = true];
  repeated sint32 p_s32 = 45 [packed = true]; repeated sint64 p_s64 = 46 [packed = true];
  repeated fixed32 p_f32 = 47 [packed = true]; repeated fixed64 p_f64 = 48 [packed = true];
  repeated sfixed32 p_sf32 = 49 [packed = true]; repeated sfixed64 p_sf64 = 50 [packed = true];
  repeated float p_fl = 51 [packed = true]; repeated double p_db = 52 [packed = true];
  repeated bool p_b = 53 [packed = true]; repeated Color p_col = 54 [packed = true];
  optional int32 d_i32 = 61 [default = -7]; optional uint64 d_u64 = 62 [default = 1234567890123];
  optional string d_str = 63 [default = "hello"]; optional double d_db = 64 [default = 2.5];
  optional bool d_b = 65 [default = true]; optional Color d_col = 66 [default = BLUE];
  optional float d_fl = 67 [default = -1.5]; optional sint64 d_s64 = 68 [default = -9];
  oneof pick { int32 o_i = 71; string o_s = 72; Rec o_m = 73; }
  optional int32 x1 = 81; optional string x2 = 82; optional bool x3 = 83;
  optional int32 n127 = 127; optional int32 n128 = 128;
  optional string n2047 = 2047; optional string n2048 = 2048; optional int64 big = 536870911;
  repeated sint32 p_far = 2049 [packed = true];
}
message Wide {
)";
    // 40 optional fields: a second has word
    for (int i = 1; i <= 40; ++i) {
        s += "  optional " + std::string(i % 3 == 0 ? "string" : i % 3 == 1 ? "int32" : "uint64") + " f" + std::to_string(i) +
             " = " + std::to_string(i) + ";\n";
    }
    s += "}\n";
    return s;
}

inline const char* Proto3Text() {
    return R"(
syntax = "proto3";
package t3;
message P3 {
  int32 a = 1; string s = 2; bool b = 3; double d = 4; repeated int32 r = 5; bytes y = 6; P3 sub = 7;
  sint64 z = 8; float f = 9; uint64 u = 10; fixed32 fx = 12; repeated string rs = 13; int64 far = 16;
}
)";
}

inline std::string Hex(const std::string& s) {
    static const char* d = "0123456789abcdef";
    if (s.empty()) return "-";
    std::string o;
    o.reserve(s.size() * 2);
    for (unsigned char c : s) {
        o += d[c >> 4];
        o += d[c & 15];
    }
    return o;
}

inline std::string Unhex(const std::string& h) {
    std::string o;
    if (h == "-") return o;
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)((nib(h[i]) << 4) | nib(h[i + 1])));
    return o;
}

inline std::vector<std::string> Split(const std::string& line) {
    std::vector<std::string> out;
    std::istringstream is(line);
    std::string w;
    while (is >> w) out.push_back(w);
    return out;
}

// <repository>/tests/golden/pb_plan/corpus.txt, found from the running
// binary (build/bin/<program>) unless MRPC_PB_PLAN_CORPUS names it.
inline std::string CorpusPath() {
    if (const char* e = getenv("MRPC_PB_PLAN_CORPUS")) return e;
    char buf[4096];
    const ssize_t n = readlink("/proc/self/exe", buf, sizeof(buf) - 1);
    if (n <= 0) return "tests/golden/pb_plan/corpus.txt";
    std::string p(buf, (size_t)n);
    for (int up = 0; up < 3; ++up) {
        const size_t slash = p.rfind('/');
        if (slash == std::string::npos) break;
        p.resize(slash);
    }
    return p + "/tests/golden/pb_plan/corpus.txt";
}

inline bool ReadLines(const std::string& path, std::vector<std::string>* lines) {
    std::ifstream in(path);
    if (!in) return false;
    std::string l;
    while (std::getline(in, l)) {
        if (!l.empty() && l[0] != '#') lines->push_back(l);
    }
    return true;
}

}  // namespace pb_plan
