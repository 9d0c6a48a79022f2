// The plan-driven parser (pb/codec.cc, pb/plan.cc) under AddressSanitizer and
// UBSan, as a program of its own: every parse input of
// tests/golden/pb_plan/corpus.txt (whole messages, truncations at every
// length, single-byte mutations, wrong wire types, both forms of packable
// fields, groups, nesting past the depth limit) is copied into a heap buffer
// of exactly its size, where one byte read too many is a report, parsed, and
// the verdict and the re-serialized message compared with the golden line.
// The generated types of the corpus (RpcMeta, EchoRequest, EchoResponse) are
// loaded from their .proto files as dynamic messages: same wire behaviour,
// and no generated code to link. Built by hand, on the CPU only, from the
// repository root (build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/pb_plan_sanitize_main.cc
//       brpc_amd/csrc/pb/*.cc brpc_amd/csrc/base/*.cc -lcrypto -ldl -o pb_plan_sanitize
//   ./pb_plan_sanitize [repository root, default .]
// Prints "ok <lines>" and returns 0 when every line agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pb/dynamic.h"
#include "pb/message.h"
#include "pb/parser.h"
#include "tests/pb_plan_corpus.h"

using namespace mrpc::pb;

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    Importer imp({root + "/brpc_amd/proto"});
    std::string err;
    if (!imp.ImportFromString("t.proto", pb_plan::Proto2Text(), &err) ||
        !imp.ImportFromString("t3.proto", pb_plan::Proto3Text(), &err) || !imp.Import("rpc_meta.proto", &err) ||
        !imp.Import("echo.proto", &err)) {
        printf("import failed: %s\n", err.c_str());
        return 2;
    }
    std::vector<std::string> lines;
    const std::string path = root + "/tests/golden/pb_plan/corpus.txt";
    if (!pb_plan::ReadLines(path, &lines)) {
        printf("cannot read %s\n", path.c_str());
        return 2;
    }
    int failures = 0, checked = 0;
    for (size_t i = 0; i < lines.size(); ++i) {
        const std::vector<std::string> w = pb_plan::Split(lines[i]);
        if (w.empty() || w[0] != "P") continue;
        if (w.size() != 5) {
            printf("line %zu: malformed\n", i + 1);
            ++failures;
            continue;
        }
        const Descriptor* d = imp.FindMessageTypeByName(w[1]);
        if (!d) {
            printf("line %zu: no type %s\n", i + 1, w[1].c_str());
            ++failures;
            continue;
        }
        const std::string in = pb_plan::Unhex(w[2]);
        // exact-size heap copy: malloc(0) may be null, which is fine for an empty input
        char* buf = static_cast<char*>(malloc(in.size()));
        if (!in.empty()) memcpy(buf, in.data(), in.size());
        std::unique_ptr<Message> m(d->NewMessage());
        const bool ok = m->ParseFromArray(buf, in.size());
        free(buf);
        const std::string back = pb_plan::Hex(m->SerializeAsString());
        if ((ok ? "1" : "0") != w[3] || back != w[4]) {
            printf("line %zu (%s): verdict %d, golden %s%s\n", i + 1, w[1].c_str(), (int)ok, w[3].c_str(),
                   back != w[4] ? ", re-serialized bytes differ" : "");
            ++failures;
        }
        // the same input into the now dirty message: Clear() then the same result
        const bool again = m->ParseFromArray(in.data(), in.size());
        if (again != ok || pb_plan::Hex(m->SerializeAsString()) != back) {
            printf("line %zu (%s): parse into a dirty message differs\n", i + 1, w[1].c_str());
            ++failures;
        }
        ++checked;
    }
    if (failures || checked == 0) {
        printf("%d failures over %d parse inputs\n", failures, checked);
        return 1;
    }
    printf("ok %d\n", checked);
    return 0;
}
