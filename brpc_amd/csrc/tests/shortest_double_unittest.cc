// base/shortest_double.h against its oracle, json::AppendShortestDouble /
// json::Value::write (snprintf + strtod rounds), byte for byte; and the
// pb2json host printer of float / double arrays built on it.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/shortest_double.h"
#include "base/time.h"
#include "gpu/json_offload.h"
#include "gpu/kernels.h"
#include "json/json.h"
#include "json/json2pb.h"
#include "mrpc/proto/json_arrays.pb.h"
#include "tests/test.h"

using namespace mrpc;
namespace sd = mrpc::shortest_double;

namespace {

double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, sizeof(d));
    return d;
}
uint64_t to_bits(double d) {
    uint64_t b;
    memcpy(&b, &d, sizeof(b));
    return b;
}

std::string oracle(double d) { return json::Value(d).ToString(); }

size_t g_longest = 0;

std::string ours(double d) {
    char buf[sd::kMaxJsonDoubleChars + 8];
    memset(buf, '#', sizeof(buf));
    const int n = sd::FormatJsonDouble(d, buf);
    if (n < 0 || n > sd::kMaxJsonDoubleChars) return "length " + std::to_string(n);
    for (size_t i = (size_t)n; i < sizeof(buf); ++i) {
        if (buf[i] != '#') return "wrote past its length";
    }
    if ((size_t)n > g_longest) g_longest = (size_t)n;
    const sd::Decimal dec = sd::ShortestDigits(to_bits(d));
    if (sd::JsonDecimalLength(dec) != n) return "JsonDecimalLength " + std::to_string(sd::JsonDecimalLength(dec));
    return std::string(buf, (size_t)n);
}

// d, -d and the neighbours of both
int check_around(double d) {
    int bad = 0;
    const double xs[] = {d, std::nextafter(d, INFINITY), std::nextafter(d, -INFINITY)};
    for (double x : xs) {
        for (double y : {x, -x}) {
            const std::string want = oracle(y), got = ours(y);
            if (want != got) {
                if (++bad < 5) EXPECT_EQ(got, want);
            }
        }
    }
    return bad;
}

}  // namespace

TEST(ShortestDouble, layouts_and_special_values) {
    EXPECT_EQ(ours(2.0), std::string("2.0"));
    EXPECT_EQ(ours(123.45), std::string("123.45"));
    EXPECT_EQ(ours(0.000123), std::string("0.000123"));
    EXPECT_EQ(ours(1.5e-7), std::string("1.5e-7"));
    EXPECT_EQ(ours(1e20), std::string("100000000000000000000.0"));
    EXPECT_EQ(ours(1e21), std::string("1e21"));
    EXPECT_EQ(ours(1e22), std::string("1e22"));
    EXPECT_EQ(ours(0.0), std::string("0.0"));
    EXPECT_EQ(ours(-0.0), std::string("-0.0"));
    EXPECT_EQ(ours(NAN), std::string("\"NaN\""));
    EXPECT_EQ(ours(-NAN), std::string("\"NaN\""));
    EXPECT_EQ(ours(INFINITY), std::string("\"Infinity\""));
    EXPECT_EQ(ours(-INFINITY), std::string("\"-Infinity\""));
    EXPECT_EQ(ours((double)0.1f), std::string("0.10000000149011612"));
    // not the shortest decimal in the interval: the oracle's rule
    EXPECT_EQ(ours(std::ldexp(1.0, -1017)), std::string("7.1202363472230444e-307"));
    for (double d : {0.0, -0.0, (double)NAN, (double)INFINITY, (double)-INFINITY}) EXPECT_EQ(ours(d), oracle(d));
}

TEST(ShortestDouble, powers_of_two_and_range_ends) {
    // a zero mantissa field: the interval below the value is half as wide,
    // where the oracle's rule and "shortest in the interval" part ways
    int bad = 0;
    for (uint64_t e = 1; e <= 2046; ++e) bad += check_around(from_bits(e << 52));
    EXPECT_EQ(bad, 0);
    bad = 0;
    const double ends[] = {from_bits(1), from_bits((1ull << 52) - 1), DBL_MIN, DBL_MAX};
    for (double d : ends) bad += check_around(d);
    EXPECT_EQ(ours(std::nextafter(DBL_MAX, INFINITY)), std::string("\"Infinity\""));
    EXPECT_EQ(bad, 0);
}

TEST(ShortestDouble, layout_thresholds_and_large_integers) {
    int bad = 0;
    for (double d : {1e-7, 1e-6, 1e-5, 1e21, 1e22, 1e20, 9.999999999999999e-7, 9.999999999999999e21, 1e-323, 1e300,
                     1e23, 5e-324, 1.7976931348623157e308, 123456789012345680000.0, 0.3, 2.5, 1e15, 1e16, 1e17}) {
        bad += check_around(d);
    }
    const double two53 = 9007199254740992.0;
    for (int k = -40; k <= 40; ++k) bad += check_around(two53 + 2.0 * k) + check_around(two53 / 2 + k);
    for (int p = -30; p <= 30; ++p) bad += check_around(std::pow(10.0, p));
    // every float power of two and the float range ends, widened
    for (uint32_t e = 0; e <= 254; ++e) {
        float f;
        const uint32_t b = e << 23;
        memcpy(&f, &b, sizeof(f));
        bad += check_around((double)f);
    }
    for (uint32_t b : {1u, 0x007FFFFFu, 0x00800000u, 0x7F7FFFFFu, 0x3DCCCCCDu}) {
        float f;
        memcpy(&f, &b, sizeof(f));
        bad += check_around((double)f);
        EXPECT_EQ(sd::WidenFloatBits(b), to_bits((double)f));
        EXPECT_EQ(sd::WidenFloatBits(b | 0x80000000u), to_bits(-(double)f));
    }
    EXPECT_EQ(bad, 0);
}

TEST(ShortestDouble, random_doubles_match_the_oracle) {
    const int64_t t0 = monotonic_us();
    std::mt19937_64 rng(20261019);
    int bad = 0;
    const int kN = 500000;
    for (int i = 0; i < kN; ++i) {
        const double d = from_bits(rng());  // non-finite patterns included
        const std::string want = oracle(d), got = ours(d);
        if (want != got && ++bad < 5) EXPECT_EQ(got, want);
    }
    // subnormals are 1/2048 of the patterns above
    for (int i = 0; i < 20000; ++i) {
        const double d = from_bits(rng() & ((1ull << 52) - 1));
        const std::string want = oracle(d), got = ours(d);
        if (want != got && ++bad < 5) EXPECT_EQ(got, want);
    }
    EXPECT_EQ(bad, 0);
    printf("    %d random doubles in %.1f s\n", kN + 20000, (double)(monotonic_us() - t0) / 1e6);
}

TEST(ShortestDouble, random_floats_widened_match_the_oracle) {
    const int64_t t0 = monotonic_us();
    std::mt19937 rng(950);
    int bad = 0;
    const int kN = 500000;
    for (int i = 0; i < kN; ++i) {
        const uint32_t b = rng();
        float f;
        memcpy(&f, &b, sizeof(f));
        const double d = (double)f;
        if (!std::isnan(f)) EXPECT_EQ(sd::WidenFloatBits(b), to_bits(d));
        const std::string want = oracle(d), got = ours(from_bits(sd::WidenFloatBits(b)));
        if (want != got && ++bad < 5) EXPECT_EQ(got, want);
    }
    EXPECT_EQ(bad, 0);
    printf("    %d random floats in %.1f s\n", kN, (double)(monotonic_us() - t0) / 1e6);
}

TEST(ShortestDouble, longest_element_is_reached_and_never_exceeded) {
    g_longest = 0;
    // -0.00000 + 17 digits
    const double d = -1.2345678901234567e-6;
    EXPECT_EQ(ours(d), oracle(d));
    EXPECT_EQ(oracle(d).size(), (size_t)sd::kMaxJsonDoubleChars);
    EXPECT_EQ(g_longest, (size_t)sd::kMaxJsonDoubleChars);
    // the other long layouts stay below it
    for (double x : {-1.2345678901234567e-308, -123456789012345678901.0, -1.2345678901234567e-7,
                     -12345.678901234567, -1.2345678901234567e+100}) {
        EXPECT_EQ(ours(x), oracle(x));
        EXPECT_LE(oracle(x).size(), (size_t)sd::kMaxJsonDoubleChars);
    }
    std::mt19937_64 rng(7);
    for (int i = 0; i < 20000; ++i) {  // ours() fails on anything longer
        const double x = from_bits((rng() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1003 + i % 3) << 52));  // around 1e-6
        const std::string got = ours(x);
        if (got != oracle(x)) EXPECT_EQ(got, oracle(x));
    }
    EXPECT_EQ(g_longest, (size_t)sd::kMaxJsonDoubleChars);
}

TEST(ShortestDouble, format_float_array_matches_value_printing) {
    const std::vector<double> ds = {1.0, -0.0, 0.1, 1e300, 5e-324, NAN, INFINITY, -INFINITY, 123.45, 1e22};
    std::vector<float> fs;
    for (double d : ds) fs.push_back((float)d);
    std::string want_d, want_f, got = "[";
    for (size_t i = 0; i < ds.size(); ++i) {
        if (i) {
            want_d += ',';
            want_f += ',';
        }
        want_d += oracle(ds[i]);
        want_f += oracle((double)fs[i]);
    }
    ASSERT_TRUE(json2pb::FormatFloatArray(ds.data(), ds.size(), json2pb::kArrayKindDouble, &got));
    EXPECT_EQ(got, "[" + want_d);  // appends
    got.clear();
    ASSERT_TRUE(json2pb::FormatFloatArray(fs.data(), fs.size(), json2pb::kArrayKindFloat, &got));
    EXPECT_EQ(got, want_f);
    got = "x";
    EXPECT_TRUE(json2pb::FormatFloatArray(nullptr, 0, json2pb::kArrayKindFloat, &got));
    EXPECT_EQ(got, std::string("x"));
    EXPECT_FALSE(json2pb::FormatFloatArray(ds.data(), ds.size(), 3, &got));
    EXPECT_FALSE(json2pb::FormatFloatArray(ds.data(), ds.size(), 7, &got));
}

namespace {
int g_standin_calls = 0, g_standin_float_calls = 0;
// a stand-in for the device printer: prints the float kinds with the oracle,
// declines every other kind
bool standin_offload(const void* values, size_t n, uint32_t kind, std::string* text) {
    ++g_standin_calls;
    if (kind != json2pb::kArrayKindFloat && kind != json2pb::kArrayKindDouble) return false;
    ++g_standin_float_calls;
    text->clear();
    for (size_t i = 0; i < n; ++i) {
        if (i) text->push_back(',');
        const double d = kind == json2pb::kArrayKindFloat ? (double)static_cast<const float*>(values)[i]
                                                           : static_cast<const double*>(values)[i];
        *text += oracle(d);
    }
    return true;
}
bool declining_offload(const void*, size_t, uint32_t, std::string*) {
    ++g_standin_calls;
    return false;
}
}  // namespace

TEST(ShortestDouble, pb2json_float_arrays_match_dom_output) {
    test::FloatArrays m;
    m.set_name("embedding");
    std::mt19937_64 rng(5000);
    std::normal_distribution<double> normal(0.0, 1.0);
    for (int i = 0; i < 5000; ++i) {
        m.add_fs((float)normal(rng));
        m.add_ds(i % 97 == 0 ? from_bits(rng()) : normal(rng));
        m.add_ids(i);
    }
    m.set_ds(17, -0.0);
    m.set_ds(18, 1e22);
    m.set_ds(19, std::ldexp(1.0, -1017));
    for (int i = 0; i < 5000; ++i) {
        if (std::isnan(m.ds(i))) m.set_ds(i, 0.5);  // a NaN's payload does not survive text
    }
    m.set_fs(3, INFINITY);
    m.set_ds(4, -INFINITY);
    // what the element-wise DOM printer gives: a Value per element
    std::string want = "{\"name\":\"embedding\",\"fs\":[";
    for (int i = 0; i < 5000; ++i) want += (i ? "," : "") + oracle((double)m.fs(i));
    want += "],\"ds\":[";
    for (int i = 0; i < 5000; ++i) want += (i ? "," : "") + oracle(m.ds(i));
    want += "],\"ids\":[";
    for (int i = 0; i < 5000; ++i) want += (i ? "," : "") + std::to_string(i);
    want += "]}";
    json2pb::Pb2JsonOptions opt;
    std::string host, with_standin, with_declining, err;
    ASSERT_TRUE(json2pb::ProtoMessageToJson(m, &host, opt, &err));
    EXPECT_TRUE(host == want);
    g_standin_calls = g_standin_float_calls = 0;
    json2pb::SetPb2JsonArrayOffload(standin_offload, 4096);
    ASSERT_TRUE(json2pb::ProtoMessageToJson(m, &with_standin, opt, &err));
    EXPECT_EQ(g_standin_float_calls, 2);
    json2pb::SetPb2JsonArrayOffload(declining_offload, 4096);
    g_standin_calls = 0;
    ASSERT_TRUE(json2pb::ProtoMessageToJson(m, &with_declining, opt, &err));
    EXPECT_EQ(g_standin_calls, 3);
    // pretty output never reaches an offload
    json2pb::Pb2JsonOptions popt;
    popt.pretty_json = true;
    std::string pretty_off, pretty_on;
    ASSERT_TRUE(json2pb::ProtoMessageToJson(m, &pretty_on, popt, &err));
    EXPECT_EQ(g_standin_calls, 3);
    json2pb::SetPb2JsonArrayOffload(nullptr, 0);
    ASSERT_TRUE(json2pb::ProtoMessageToJson(m, &pretty_off, popt, &err));
    EXPECT_TRUE(pretty_on == pretty_off);
    EXPECT_TRUE(with_standin == want);
    EXPECT_TRUE(with_declining == want);
    test::FloatArrays back;
    ASSERT_TRUE(json2pb::JsonToProtoMessage(host, &back, json2pb::Json2PbOptions(), &err));
    EXPECT_TRUE(back.SerializeAsString() == m.SerializeAsString());
}

// Host half of gpu::DevicePrintFloatArrays: a refused or empty job reaches no
// kernel and none of its pointers is dereferenced, so this runs without a
// device. The device half is tests/test_gpu_json_float_print.py.
TEST(ShortestDouble, device_print_refuses_bad_jobs_before_any_launch) {
    static char mem[64] __attribute__((aligned(16)));
    auto code = [](const void* src, uint64_t count, uint32_t kind, void* dst) {
        gpu::DeviceFloatPrintJob j;
        j.src = src;
        j.count = count;
        j.kind = kind;
        j.dst = dst;
        j.cap = sizeof(mem);
        j.err = -1;
        j.len = 99;
        EXPECT_EQ(gpu::DevicePrintFloatArrays(&j, 1, 0), 0);
        EXPECT_EQ(j.len, 0u);
        return j.err;
    };
    EXPECT_EQ(code(mem, 0, gpu::kJsonFloat64, mem), 0);      // empty: nothing to print
    EXPECT_EQ(code(nullptr, 0, gpu::kJsonFloat32, nullptr), 0);
    EXPECT_EQ(code(nullptr, 4, gpu::kJsonFloat64, mem), 2);  // null src
    EXPECT_EQ(code(mem, 4, gpu::kJsonFloat64, nullptr), 2);  // null dst
    EXPECT_EQ(code(mem + 4, 4, gpu::kJsonFloat64, mem), 2);  // a double at 4 (mod 8)
    EXPECT_EQ(code(mem + 2, 4, gpu::kJsonFloat32, mem), 2);  // a float at 2 (mod 4)
    EXPECT_EQ(code(mem, 4, 3, mem), 2);                      // an integer kind
    EXPECT_EQ(code(mem, 4, 7, mem), 2);                      // the codec's raw bytes
    EXPECT_EQ(code(mem, (1ull << 32) / 26 + 1, gpu::kJsonFloat32, mem), 2);  // worst case above 2^32 - 1
    EXPECT_EQ(gpu::FloatPrintWorstCaseBytes(0), 0u);
    EXPECT_EQ(gpu::FloatPrintWorstCaseBytes(1), (uint64_t)sd::kMaxJsonDoubleChars);
    EXPECT_EQ(gpu::FloatPrintWorstCaseBytes(1000), 1000u * (sd::kMaxJsonDoubleChars + 1) - 1);
    EXPECT_EQ((uint32_t)json2pb::kArrayKindFloat, gpu::kJsonFloat32);
    EXPECT_EQ((uint32_t)json2pb::kArrayKindDouble, gpu::kJsonFloat64);
    EXPECT_EQ(gpu::kJsonFloat32, gpu::JSON_FLOAT32);
    EXPECT_EQ(gpu::kJsonFloat64, gpu::JSON_FLOAT64);
}
