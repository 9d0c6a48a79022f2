// base/base64.h and the host coder on top of it (base64_encode /
// base64_decode, base/util.h) against the byte-wise coder they replaced,
// kept here as the oracle: return value and *out, the partial output of a
// refused text included. json2pb / pb2json over a large bytes field.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <string>

#include "base/base64.h"
#include "base/util.h"
#include "json/json2pb.h"
#include "mrpc/proto/test_services.pb.h"
#include "tests/test.h"

using namespace mrpc;

namespace {

const char* kAlphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

std::string oracle_encode(const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    std::string out;
    size_t i = 0;
    for (; i + 2 < n; i += 3) {
        uint32_t v = (p[i] << 16) | (p[i + 1] << 8) | p[i + 2];
        out.push_back(kAlphabet[v >> 18]);
        out.push_back(kAlphabet[(v >> 12) & 63]);
        out.push_back(kAlphabet[(v >> 6) & 63]);
        out.push_back(kAlphabet[v & 63]);
    }
    if (i < n) {
        uint32_t v = p[i] << 16;
        if (i + 1 < n) v |= p[i + 1] << 8;
        out.push_back(kAlphabet[v >> 18]);
        out.push_back(kAlphabet[(v >> 12) & 63]);
        out.push_back(i + 1 < n ? kAlphabet[(v >> 6) & 63] : '=');
        out.push_back('=');
    }
    return out;
}

bool oracle_decode(const std::string& in, std::string* out) {
    int8_t rev[256];
    memset(rev, -1, sizeof(rev));
    for (int i = 0; i < 64; ++i) rev[(uint8_t)kAlphabet[i]] = (int8_t)i;
    out->clear();
    uint32_t acc = 0;
    int bits = 0;
    size_t n = 0, pad = 0;
    for (char c : in) {
        if (c == '\n' || c == '\r' || c == ' ') continue;
        if (c == '=') {
            ++pad;
            continue;
        }
        if (pad) return false;
        int v = rev[(uint8_t)c];
        if (v < 0) return false;
        ++n;
        acc = (acc << 6) | (uint32_t)v;
        bits += 6;
        if (bits >= 8) {
            bits -= 8;
            out->push_back((char)((acc >> bits) & 0xff));
        }
    }
    if (n % 4 == 1 || pad > 2 || (pad && (n + pad) % 4 != 0)) return false;
    return true;
}

// both overloads against the oracle: verdict and output
bool same_as_oracle(const std::string& text) {
    std::string want, got = "stale", got2 = "stale";
    const bool w = oracle_decode(text, &want);
    const bool g = base64_decode(text, &got);
    const bool g2 = base64_decode(text.data(), text.size(), &got2);
    return w == g && want == got && w == g2 && want == got2;
}

std::string printable(const std::string& s) { return hex_dump(s.data(), s.size(), 256); }

}  // namespace

TEST(Base64, header_maps_every_value_and_every_byte) {
    for (uint32_t v = 0; v < 64; ++v) {
        EXPECT_EQ(base64::Symbol(v), kAlphabet[v]);
        EXPECT_EQ(base64::Value((uint8_t)kAlphabet[v]), (int)v);
    }
    int in_alphabet = 0;
    for (int c = 0; c < 256; ++c) in_alphabet += base64::Value((uint8_t)c) >= 0;
    EXPECT_EQ(in_alphabet, 64);
    // four symbols at once, every value in every position
    for (uint32_t v = 0; v < 64; ++v) {
        for (int pos = 0; pos < 4; ++pos) {
            const uint32_t w = 63 - v;  // the other three bytes
            uint32_t x = w | w << 8 | w << 16 | w << 24;
            x = (x & ~(0xFFu << (8 * pos))) | v << (8 * pos);
            const uint32_t s = base64::Symbols4(x);
            for (int b = 0; b < 4; ++b)
                EXPECT_EQ((char)(s >> (8 * b)), kAlphabet[b == pos ? v : w]);
        }
    }
    EXPECT_EQ(base64::Base64EncodedBytes(0), 0u);
    EXPECT_EQ(base64::Base64EncodedBytes(1), 4u);
    EXPECT_EQ(base64::Base64EncodedBytes(3), 4u);
    EXPECT_EQ(base64::Base64EncodedBytes(4), 8u);
    EXPECT_EQ(base64::Base64DecodedMaxBytes(4), 3u);
    EXPECT_EQ(base64::Base64DecodedMaxBytes(5), 3u);
    EXPECT_EQ(base64::Base64DecodedMaxBytes(6), 4u);
    EXPECT_EQ(base64::Base64DecodedMaxBytes(7), 5u);
}

TEST(Base64, encode3_and_decode4_invert_each_other) {
    std::mt19937 rng(7);
    for (int i = 0; i < 200000; ++i) {
        const uint32_t v = rng() & 0xFFFFFF;
        const uint32_t s = base64::Encode3(v);
        bool ok = false;
        EXPECT_EQ(base64::Decode4(s, &ok), v);
        EXPECT_TRUE(ok);
        const uint32_t le = base64::Bytes3LE(v);
        EXPECT_EQ(le, (v >> 16) | (v & 0xFF00) | (v & 0xFF) << 16);
        EXPECT_EQ(base64::Encode3LE(le | (rng() << 24)), s);
    }
    // one byte outside the alphabet in any position is seen
    const uint32_t good = base64::Encode3(0x123456);
    for (int pos = 0; pos < 4; ++pos) {
        for (int c = 0; c < 256; ++c) {
            const uint32_t s = (good & ~(0xFFu << (8 * pos))) | (uint32_t)c << (8 * pos);
            bool ok = true;
            base64::Decode4(s, &ok);
            EXPECT_EQ(ok, strchr(kAlphabet, c) != nullptr && c != 0);
        }
    }
}

TEST(Base64, encoder_equals_the_bytewise_coder) {
    std::mt19937 rng(11);
    std::string data(1 << 20, '\0');
    for (char& c : data) c = (char)rng();
    for (size_t n = 0; n <= 100; ++n) {
        EXPECT_TRUE_M(base64_encode(data.data(), n) == oracle_encode(data.data(), n), std::to_string(n));
        // into the caller's buffer: exactly the size promised, nothing after it
        std::string buf((size_t)base64::Base64EncodedBytes(n) + 8, '\x7f');
        base64_encode_to(data.data() + 1, n, &buf[0]);
        EXPECT_TRUE(buf.substr(0, buf.size() - 8) == oracle_encode(data.data() + 1, n));
        EXPECT_TRUE(buf.substr(buf.size() - 8) == std::string(8, '\x7f'));
    }
    std::string all(256, '\0');
    for (int i = 0; i < 256; ++i) all[i] = (char)i;
    for (int k = 1; k <= 5; ++k) {
        std::string rep;
        for (int i = 0; i < k; ++i) rep += all;
        EXPECT_TRUE(base64_encode(rep.data(), rep.size()) == oracle_encode(rep.data(), rep.size()));
    }
    for (size_t n : {(size_t)4095, (size_t)4096, (size_t)65537, data.size() - 1, data.size()})
        EXPECT_TRUE_M(base64_encode(data.data(), n) == oracle_encode(data.data(), n), std::to_string(n));
}

TEST(Base64, decoder_equals_the_scalar_loop_on_random_strings) {
    std::mt19937 rng(13);
    const std::string odd = "=\n\r ";
    const std::string junk = std::string("!-_.,*\t\x7f\x80\xff@[`{", 15) + std::string(1, '\0');
    int accepted = 0;
    for (int i = 0; i < 120000; ++i) {
        const size_t len = rng() % 201;
        // mostly alphabet, so that the fast loop runs before the first odd byte
        static const uint32_t kOdd[4] = {0, 2, 8, 40}, kJunk[4] = {0, 0, 1, 6};
        const uint32_t odd_in_256 = kOdd[rng() % 4], junk_in_256 = kJunk[rng() % 4];
        std::string t(len, 'A');
        for (char& c : t) {
            const uint32_t r = rng() & 255;
            if (r < odd_in_256) c = odd[rng() % odd.size()];
            else if (r < odd_in_256 + junk_in_256) c = junk[rng() % junk.size()];
            else c = kAlphabet[rng() % 64];
        }
        if (rng() % 3 == 0) {  // a padded tail, right or wrong
            t.resize(t.size() - std::min<size_t>(t.size(), rng() % 3));
            t.append(rng() % 4, '=');
        }
        std::string o;
        accepted += oracle_decode(t, &o);
        ASSERT_TRUE_M(same_as_oracle(t), printable(t));
    }
    EXPECT_GT(accepted, 10000);  // both verdicts are exercised
    EXPECT_LT(accepted, 110000);
}

TEST(Base64, decoder_equals_the_scalar_loop_with_one_byte_replaced) {
    std::string data(48, '\0');
    for (size_t i = 0; i < data.size(); ++i) data[i] = (char)(i * 37 + 5);
    const std::string text = oracle_encode(data.data(), data.size());
    ASSERT_EQ(text.size(), 64u);
    for (size_t pos = 0; pos < text.size(); ++pos) {
        for (int c = 0; c < 256; ++c) {
            std::string t = text;
            t[pos] = (char)c;
            ASSERT_TRUE_M(same_as_oracle(t), printable(t));
        }
    }
    // and with padded tails
    for (size_t n : {(size_t)46, (size_t)47}) {
        const std::string padded = oracle_encode(data.data(), n);
        for (size_t pos = 0; pos < padded.size(); ++pos) {
            for (int c = 0; c < 256; ++c) {
                std::string t = padded;
                t[pos] = (char)c;
                ASSERT_TRUE_M(same_as_oracle(t), printable(t));
            }
        }
    }
}

TEST(Base64, named_cases) {
    std::string out;
    EXPECT_TRUE(base64_decode("QR==", &out));  // trailing bits that are not zero are dropped
    EXPECT_EQ(out, std::string("A"));
    EXPECT_TRUE(base64_decode("QQ", &out));  // unpadded
    EXPECT_EQ(out, std::string("A"));
    EXPECT_FALSE(base64_decode("Q", &out));
    EXPECT_EQ(out, std::string());
    EXPECT_FALSE(base64_decode("=", &out));  // a pad that completes no group
    EXPECT_FALSE(base64_decode("====", &out));
    EXPECT_FALSE(base64_decode("QQ=Q", &out));
    EXPECT_EQ(out, std::string("A"));  // what was decoded before the refusal stays
    EXPECT_TRUE(base64_decode("QUJD\n", &out));
    EXPECT_EQ(out, std::string("ABC"));
    EXPECT_TRUE(base64_decode("QU JD", &out));
    EXPECT_EQ(out, std::string("ABC"));
    for (const char* t : {"QR==", "QQ", "Q", "=", "====", "QQ=Q", "QUJD\n", "QU JD", ""})
        EXPECT_TRUE_M(same_as_oracle(t), std::string(t));
}

TEST(Base64, json2pb_round_trip_of_a_large_bytes_field) {
    std::mt19937 rng(17);
    std::string raw(100000, '\0');
    for (char& c : raw) c = (char)rng();
    test::Rich r;
    r.set_must("m");
    r.set_raw(raw);
    std::string json, err;
    ASSERT_TRUE(json2pb::ProtoMessageToJson(r, &json, json2pb::Pb2JsonOptions(), &err));
    const std::string text = oracle_encode(raw.data(), raw.size());
    EXPECT_TRUE(json.find("\"raw\":\"" + text + "\"") != std::string::npos);
    test::Rich back;
    ASSERT_TRUE_M(json2pb::JsonToProtoMessage(json, &back, json2pb::Json2PbOptions(), &err), std::string(err));
    EXPECT_TRUE(back.raw() == raw);
    // a line break inside the text (the JSON escape of one) is skipped
    std::string broken = text;
    broken.insert(76, "\\n");
    test::Rich lax;
    ASSERT_TRUE_M(json2pb::JsonToProtoMessage("{\"must\":\"m\",\"raw\":\"" + broken + "\"}", &lax,
                                              json2pb::Json2PbOptions(), &err),
                  std::string(err));
    EXPECT_TRUE(lax.raw() == raw);
    // a symbol outside the alphabet is still the decoder's error
    test::Rich bad;
    err.clear();
    json2pb::JsonToProtoMessage("{\"must\":\"m\",\"raw\":\"QUJD!A==\"}", &bad, json2pb::Json2PbOptions(), &err);
    EXPECT_TRUE_M(err.find("Fail to decode base64 string=QUJD!A==") != std::string::npos, std::string(err));
}
