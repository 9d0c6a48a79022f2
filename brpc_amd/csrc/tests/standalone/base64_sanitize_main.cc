// The host base64 coder under AddressSanitizer and UBSan, as a program of
// its own: the fast loops of base/util.cc read and write whole words, so
// every length 0..64 is coded from and into heap buffers of exactly its size,
// where one byte too many is a report. Built by hand, on the CPU only, from
// this file and base/util.cc alone (build.py does not pick it up):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ibrpc_amd/csrc brpc_amd/csrc/tests/standalone/base64_sanitize_main.cc
//       brpc_amd/csrc/base/util.cc -lcrypto -lpthread
// Prints "ok" and returns 0 when every round trip is right.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "base/base64.h"
#include "base/util.h"

int main() {
    int failures = 0;
    for (size_t n = 0; n <= 64; ++n) {
        // exact-size heap buffers: malloc(0) may be null, which is fine for n 0
        unsigned char* data = static_cast<unsigned char*>(malloc(n));
        for (size_t i = 0; i < n; ++i) data[i] = (unsigned char)(i * 131 + n * 17 + 3);
        const size_t tn = (size_t)mrpc::base64::Base64EncodedBytes(n);
        char* text = static_cast<char*>(malloc(tn));
        mrpc::base64_encode_to(data, n, text);
        const std::string same = mrpc::base64_encode(data, n);
        if (same.size() != tn || memcmp(same.data(), text, tn) != 0) ++failures;
        std::string back;
        if (!mrpc::base64_decode(text, tn, &back) || back.size() != n || memcmp(back.data(), data, n) != 0) ++failures;
        // the same text cut short (unpadded forms, refused tails) and with a
        // byte of each odd kind, each from a buffer of its exact size
        for (size_t cut = 0; cut <= tn; ++cut) {
            char* part = static_cast<char*>(malloc(cut));
            memcpy(part, text, cut);
            std::string out;
            mrpc::base64_decode(part, cut, &out);
            if (out.size() > (size_t)mrpc::base64::Base64DecodedMaxBytes(cut)) ++failures;
            for (char odd : {'\n', '=', '!'}) {
                if (cut == 0) break;
                part[cut - 1] = odd;
                mrpc::base64_decode(part, cut, &out);
                part[cut / 2] = odd;
                mrpc::base64_decode(part, cut, &out);
                memcpy(part, text, cut);
            }
            free(part);
        }
        free(text);
        free(data);
    }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
