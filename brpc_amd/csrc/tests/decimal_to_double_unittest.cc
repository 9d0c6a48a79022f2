// base/decimal_to_double.h against its oracle strtod (std::from_chars must
// agree), bit for bit; the packed-number DOM of json::Reader against the
// element-wise route it replaced; json2pb over packed numbers.
#include <cerrno>
#include <cfloat>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "base/decimal_to_double.h"
#include "base/shortest_double.h"
#include "base/time.h"
#include "gpu/json_offload.h"
#include "gpu/kernels.h"
#include "json/json.h"
#include "json/json2pb.h"
#include "mrpc/proto/json_arrays.pb.h"
#include "tests/test.h"

using namespace mrpc;
namespace dd = mrpc::decimal_to_double;
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

dd::NumberResult ours(const std::string& t) {
    dd::NumberResult r;
    dd::ParseJsonNumber(t.data(), t.data() + t.size(), &r);
    return r;
}
int cls_of(const std::string& t) { return ours(t).cls; }

uint64_t strtod_bits(const std::string& t) { return to_bits(strtod(t.c_str(), nullptr)); }

// strtod and, where it gives a value, std::from_chars
bool oracles_agree(const std::string& t) {
    double d = 0;
    auto r = std::from_chars(t.data(), t.data() + t.size(), d);
    if (r.ec == std::errc::result_out_of_range) return true;  // Reader::number then takes strtod
    return r.ec == std::errc() && r.ptr == t.data() + t.size() && to_bits(d) == strtod_bits(t);
}

int significant_digits(const std::string& t) {
    int n = 0;
    bool lead = true;
    for (char c : t) {
        if (c == 'e' || c == 'E') break;
        if (c < '0' || c > '9') continue;
        if (lead && c == '0') continue;
        lead = false;
        ++n;
    }
    return n;
}

struct Tally {
    long texts = 0, wrong = 0, needs_exact = 0, needs_exact_short = 0, long_texts = 0, long_needs_exact = 0;
};

// One text of the RFC 8259 grammar against the oracle.
void check_text(const std::string& t, Tally* tally) {
    ++tally->texts;
    const dd::NumberResult r = ours(t);
    const int digits = significant_digits(t);
    if (digits >= 20) ++tally->long_texts;
    if (r.cls == dd::kNeedsExact) {
        ++tally->needs_exact;
        if (digits <= 19 && (int)t.size() <= dd::kMaxDeviceNumberChars) ++tally->needs_exact_short;
        if (digits >= 20) ++tally->long_needs_exact;
        return;
    }
    bool ok;
    const bool is_float = t.find_first_of(".eE") != std::string::npos;
    if (r.cls == dd::kInt64) {
        char* end = nullptr;
        errno = 0;
        const long long x = strtoll(t.c_str(), &end, 10);
        ok = !is_float && errno == 0 && *end == 0 && (uint64_t)x == r.bits;
    } else if (r.cls == dd::kUInt64) {
        char* end = nullptr;
        errno = 0;
        const unsigned long long x = strtoull(t.c_str(), &end, 10);
        ok = !is_float && t[0] != '-' && errno == 0 && *end == 0 && x == r.bits && x > (uint64_t)INT64_MAX;
    } else {
        ok = r.cls == dd::kDouble && r.bits == strtod_bits(t) && oracles_agree(t);
        if (ok && !is_float) {  // an integer literal is a double only out of both integer ranges
            errno = 0;
            if (t[0] == '-') ok = (strtoll(t.c_str(), nullptr, 10), errno == ERANGE);
            else ok = (strtoull(t.c_str(), nullptr, 10), errno == ERANGE);
        }
    }
    if (!ok && ++tally->wrong < 6) {
        char msg[256];
        snprintf(msg, sizeof(msg), "%s: class %d bits %016llx, strtod %016llx", t.c_str(), r.cls,
                 (unsigned long long)r.bits, (unsigned long long)strtod_bits(t));
        EXPECT_TRUE_M(ok, msg);
    }
}

// "d.ddde[+-]XX" -> the same digits with the exponent moved by `shift` and
// written in another of the legal spellings
std::string shifted(const std::string& e_form, int shift, int style) {
    const size_t e = e_form.find('e');
    const int x = atoi(e_form.c_str() + e + 1) + shift;
    char tail[16];
    snprintf(tail, sizeof(tail), style == 0 ? "E%+d" : style == 1 ? "e%d" : "e%+03d", x);
    return e_form.substr(0, e) + tail;
}

std::string e_form(double d, int digits) {
    char buf[80];
    snprintf(buf, sizeof(buf), "%.*e", digits - 1, d);
    return buf;
}

std::string g_form(double d, int digits) {
    char buf[80];
    snprintf(buf, sizeof(buf), "%.*g", digits, d);
    return buf;
}

std::string shortest(double d) {
    char buf[sd::kMaxJsonDoubleChars + 1];
    return std::string(buf, (size_t)sd::FormatJsonDouble(d, buf));
}

// the exact decimal expansion of the point halfway between d and the next
// double above it (one more bit than a double holds: exact in an x87 long
// double, and glibc prints every digit)
std::string halfway_above(double d) {
    const long double mid = ((long double)d + (long double)std::nextafter(d, INFINITY)) / 2;
    static char buf[1400];
    snprintf(buf, sizeof(buf), "%.1200Le", mid);
    std::string t = buf;
    // strip the zeros before the exponent
    const size_t e = t.find('e');
    size_t z = e;
    while (z > 2 && t[z - 1] == '0') --z;
    if (t[z - 1] == '.') --z;  // 10^23 is itself halfway between two doubles
    return t.substr(0, z) + t.substr(e);
}

}  // namespace

TEST(DecimalToDouble, random_doubles_in_every_spelling_match_strtod) {
    static_assert(sizeof(long double) > sizeof(double), "the halfway cases need a wider long double");
    const int64_t t0 = monotonic_us();
    std::mt19937_64 rng(20261019);
    Tally tally;
    const int kValues = 26000;
    for (int i = 0; i < kValues; ++i) {
        uint64_t bits = rng();
        if (i % 16 == 0) bits &= 0x800FFFFFFFFFFFFFull;  // subnormals are 1/2048 of the patterns
        const double d = from_bits(bits);
        if (!std::isfinite(d)) continue;
        check_text(g_form(d, 17), &tally);
        check_text(shortest(d), &tally);
        const int shift = (int)(rng() % 41) - 20;
        for (int digits = 1; digits <= 17; ++digits) {
            const std::string t = e_form(d, digits);
            check_text(t, &tally);
            check_text(shifted(t, shift, digits % 3), &tally);
        }
        check_text(g_form(d, 1 + (int)(rng() % 16)), &tally);
    }
    EXPECT_EQ(tally.wrong, 0);
    EXPECT_EQ(tally.needs_exact, 0);  // nothing here has more than 19 significant digits
    EXPECT_GT(tally.texts, 900000);
    printf("    %ld texts of %d doubles in %.1f s\n", tally.texts, kValues, (double)(monotonic_us() - t0) / 1e6);
}

TEST(DecimalToDouble, twenty_to_forty_digits_rarely_need_exact_arithmetic) {
    std::mt19937_64 rng(40);
    Tally tally;
    for (int i = 0; i < 60000; ++i) {
        const double d = from_bits(rng());
        if (!std::isfinite(d)) continue;
        check_text(e_form(d, 20 + (int)(rng() % 21)), &tally);  // the digits of a double: never undecided
    }
    // digits of no double in particular: undecided when the 19-digit
    // truncation and its successor straddle a rounding boundary, about
    // 10^-19 / 2^-53 of the time
    for (int i = 0; i < 60000; ++i) {
        std::string t;
        if (rng() & 1) t += '-';
        const int digits = 20 + (int)(rng() % 21);
        t += (char)('1' + rng() % 9);
        t += '.';
        for (int k = 1; k < digits; ++k) t += (char)('0' + rng() % 10);
        if (t.back() == '0') t.back() = '7';
        const int x = (int)(rng() % 640) - 320;
        if (t.size() + 5 <= (size_t)dd::kMaxDeviceNumberChars) t += "e" + std::to_string(x);
        check_text(t, &tally);
    }
    EXPECT_EQ(tally.wrong, 0);
    EXPECT_EQ(tally.needs_exact_short, 0);
    EXPECT_EQ(tally.long_texts, tally.texts);
    EXPECT_LT(tally.long_needs_exact * 20, tally.long_texts);  // under 5 %
    printf("    %ld of %ld texts with 20 to 40 digits need exact arithmetic\n", tally.long_needs_exact,
           tally.long_texts);
}

TEST(DecimalToDouble, hard_cases) {
    Tally tally;
    const char* texts[] = {
        // float and double boundaries
        "3.4028234663852886e38", "3.4028235677973366e38", "1.1754943508222875e-38", "1.401298464324817e-45",
        "7.006492321624085e-46", "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",
        "1.797693134862315807e308", "1.8e308", "179769313486231570000000000000000000000000e267",
        // around the smallest subnormal: below half of it, above half of it
        "2.4703282292062327e-324", "2.4703282292062328e-324", "2.4703282292062327208e-324", "4.9e-324", "5e-324",
        "4.9406564584124654e-324", "7.4109846876186981e-324", "7.4109846876186982e-324",
        // the largest subnormal and the smallest normal
        "2.2250738585072009e-308", "2.225073858507201e-308", "2.2250738585072011e-308", "2.2250738585072014e-308",
        "2.2250738585072012e-308", "2.2250738585072013e-308",
        // integers around 2^53 as doubles and as integers
        "9007199254740991.0", "9007199254740992.0", "9007199254740993.0", "9007199254740995.0", "9007199254740991",
        "9007199254740993", "9007199254740993e0", "9007199254740993.000000000000001",
        // around INT64_MAX and UINT64_MAX
        "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
        "9223372036854775806", "1000000000000000000", "9999999999999999999", "10000000000000000000",
        "18446744073709551615", "18446744073709551616", "18446744073709551614", "99999999999999999999",
        "100000000000000000000", "184467440737095516150", "-18446744073709551615", "-10000000000000000000",
        "123456789012345678901", "1000000000000000000000", "1000000000000000000001",
        // zeros and clamped exponents
        "0", "-0", "-0.0", "0.0", "0e0", "-0e-5", "0e999999999999", "-0e999999999999", "0.000e-999999999999",
        "1e-999999999999", "-1e-999999999999", "1e+400", "-1e+400", "1e999999999999", "1e309", "1e308", "1e-323",
        "1e-324", "1e-325", "123e-326", "0.00000000000000000000000000000000000001e350",
        // ties and near-ties with few digits
        "1e23", "8.41e21", "9.5e-5", "4.35", "0.3", "1e22", "1e-22", "5e-1", "0.000001", "1.5e-7",
        "100000000000000000000000", "8.5", "0.1e1", "2.5E+0", "6.02214076e23", "1.616255e-35",
    };
    for (const char* t : texts) check_text(t, &tally);
    EXPECT_EQ(tally.wrong, 0);
    EXPECT_EQ(tally.needs_exact_short, 0);
    EXPECT_EQ(cls_of("-0"), (int)dd::kInt64);
    EXPECT_EQ(ours("-0").bits, 0u);
    EXPECT_EQ(cls_of("-0.0"), (int)dd::kDouble);
    EXPECT_EQ(ours("-0.0").bits, 0x8000000000000000ull);
    EXPECT_EQ(cls_of("9223372036854775808"), (int)dd::kUInt64);
    EXPECT_EQ(cls_of("18446744073709551616"), (int)dd::kDouble);
    EXPECT_EQ(cls_of("-9223372036854775809"), (int)dd::kDouble);
    EXPECT_EQ(ours("1e+400").bits, 0x7FF0000000000000ull);
    EXPECT_EQ(ours("-1e400").bits, 0xFFF0000000000000ull);
    EXPECT_EQ(ours("1e-999999999999").bits, 0u);
    EXPECT_EQ(ours("2.4703282292062327e-324").bits, 0u);
    EXPECT_EQ(ours("2.4703282292062328e-324").bits, 1u);
    EXPECT_EQ(ours("9007199254740993.0").bits, to_bits(9007199254740992.0));  // ties to even
    EXPECT_EQ(ours("9007199254740995.0").bits, to_bits(9007199254740996.0));
}

TEST(DecimalToDouble, exact_halfway_points_written_in_full) {
    std::mt19937_64 rng(53);
    std::vector<double> ds = {1.0, 9007199254740992.0, DBL_MIN, from_bits(1), from_bits((1ull << 52) - 1),
                              std::nextafter(DBL_MAX, 0.0), 1e23, 0.1, 3.4028234663852886e38};
    for (int i = 0; i < 300; ++i) {
        const double d = std::fabs(from_bits(rng()));
        if (std::isfinite(d) && d < DBL_MAX) ds.push_back(d);
    }
    int wrong = 0, decided = 0;
    size_t longest = 0;
    for (double d : ds) {
        const std::string mid = halfway_above(d);
        longest = std::max(longest, mid.size());
        // ties to even: the neighbour with the even significand
        const double up = std::nextafter(d, INFINITY);
        const uint64_t even = (to_bits(d) & 1) == 0 ? to_bits(d) : to_bits(up);
        if (strtod_bits(mid) != even) {  // the construction itself
            if (++wrong < 4) EXPECT_EQ(strtod_bits(mid), even);
            continue;
        }
        for (const std::string& t : {mid, "-" + mid}) {
            const dd::NumberResult r = ours(t);
            if (r.cls == dd::kNeedsExact) continue;
            ++decided;
            if ((r.cls != dd::kDouble || r.bits != strtod_bits(t)) && ++wrong < 4) EXPECT_EQ(r.bits, strtod_bits(t));
        }
        // one digit changed at the end moves it off the tie: the exact route decides both ways
        for (const char* last : {"1", "9"}) {
            const size_t e = mid.find('e');
            if (mid.find('.') == std::string::npos) break;
            std::string above = mid.substr(0, e) + last + mid.substr(e);
            if (*last == '9') above[e - 1] = (char)(above[e - 1] - 1);  // ...(k-1)9 is below ...k
            uint64_t payload;
            uint8_t cls;
            ASSERT_TRUE(json::ParseNumberExact(above.data(), above.data() + above.size(), &payload, &cls));
            if (payload != (*last == '1' ? to_bits(up) : to_bits(d)) && ++wrong < 4) EXPECT_EQ(above, std::string());
        }
    }
    EXPECT_EQ(wrong, 0);
    EXPECT_GT(longest, (size_t)700);  // hundreds of digits
    printf("    %zu halfway points, the longest %zu characters, %d decided without exact arithmetic\n", ds.size(),
           longest, decided);
}

TEST(DecimalToDouble, long_texts_always_need_exact_arithmetic) {
    std::string t = "1.";
    while ((int)t.size() < dd::kMaxDeviceNumberChars) t += '0';
    EXPECT_EQ((int)t.size(), dd::kMaxDeviceNumberChars);
    EXPECT_EQ(cls_of(t), (int)dd::kDouble);  // the dropped digits are zeros: decided
    EXPECT_EQ(ours(t).bits, to_bits(1.0));
    t += '0';
    EXPECT_EQ(cls_of(t), (int)dd::kNeedsExact);
    EXPECT_EQ(cls_of(std::string(60, 'x')), (int)dd::kNeedsExact);  // unread: the exact route rejects it
    uint64_t payload;
    uint8_t cls;
    EXPECT_TRUE(json::ParseNumberExact(t.data(), t.data() + t.size(), &payload, &cls));
    EXPECT_EQ(payload, to_bits(1.0));
    const std::string junk(60, 'x');
    EXPECT_FALSE(json::ParseNumberExact(junk.data(), junk.data() + junk.size(), &payload, &cls));
    EXPECT_GE(dd::kMaxDeviceNumberChars, 40);
    EXPECT_LE(dd::kMaxDeviceNumberChars, 64);
}

TEST(DecimalToDouble, grammar) {
    for (const char* t : {"01", "1.", ".5", "+1", "1e", "1e+", "--1", "1.2.3", "0x10", "NaN", "Infinity", "", "-", "-.5",
                          "1e5.3", "1 2", " 1", "1 ", "1e-", "1.e3", "00", "-01.5", "1,2", "\"1\"", "1f", "1e+-2", "e5",
                          "-Infinity", "nan", "0.", "1.5e", "1..5"}) {
        EXPECT_EQ(cls_of(t), (int)dd::kMalformed);
    }
    for (const char* t : {"0", "-0", "10", "1.0", "0.5", "1e5", "1E5", "1e+5", "1e-5", "1.5E+05", "-1.25e-007", "0e0"}) {
        EXPECT_LE(cls_of(t), (int)dd::kDouble);
    }
}

namespace {
struct Recorded {
    const char* text;
    bool ok;
    const char* result;  // ToString() of the DOM, or the error
    const char* types;   // json::Value::Type of each element
};
// what json::Parse answered before packed numbers existed
const Recorded kRecorded[] = {
    {R"([01])", true, R"([1])", "2"},
    {R"([1.])", true, R"([1.0])", "4"},
    {R"([1.5,01,2])", true, R"([1.5,1,2])", "422"},
    {R"([-01.5])", true, R"([-1.5])", "4"},
    {R"([1.e3])", true, R"([1000.0])", "4"},
    {R"([00])", true, R"([0])", "2"},
    {R"([1,2.5,007])", true, R"([1,2.5,7])", "242"},
    {R"([1.5,1.])", true, R"([1.5,1.0])", "44"},
    {R"([0.5,1e5.3])", false, R"(invalid json at offset 10: bad number)", ""},
    {R"([1.5,1e])", false, R"(invalid json at offset 7: bad number)", ""},
    {R"([1.5,.5])", false, R"(invalid json at offset 5: bad number)", ""},
    {R"([1.5,+1])", false, R"(invalid json at offset 5: bad number)", ""},
    {R"([1.5,--1])", false, R"(invalid json at offset 6: bad number)", ""},
    {R"([1.5,1.2.3])", false, R"(invalid json at offset 10: bad number)", ""},
    {R"([1.5,0x10])", false, R"(invalid json at offset 6: expected , or ])", ""},
    {R"([1.5,NaN])", false, R"(invalid json at offset 5: bad number)", ""},
    {R"([2.5,-])", false, R"(invalid json at offset 6: bad number)", ""},
    {R"([1.5 2])", false, R"(invalid json at offset 5: expected , or ])", ""},
    {R"([1.5,])", false, R"(invalid json at offset 5: bad number)", ""},
    {R"([1.5,1e+])", false, R"(invalid json at offset 8: bad number)", ""},
    {R"([1.5,2)", false, R"(invalid json at offset 6: expected , or ])", ""},
    {R"([1.5,"a",2.5])", true, R"([1.5,"a",2.5])", "454"},
    {R"([1,2.5,[3.5,4],{"a":1.5}])", true, R"([1,2.5,[3.5,4],{"a":1.5}])", "2467"},
    {"[ 1.5 ,\t2 ,\n-3e2 ]", true, R"([1.5,2,-300.0])", "424"},
    {R"([1.0.0])", false, R"(invalid json at offset 6: bad number)", ""},
    {R"([1e5e5])", false, R"(invalid json at offset 6: bad number)", ""},
    {R"([1.5,-0,-0.0])", true, R"([1.5,0,-0.0])", "424"},
    {R"([18446744073709551615,1.5])", true, R"([18446744073709551615,1.5])", "34"},
    {R"([18446744073709551616,1])", true, R"([18446744073709552000.0,1])", "42"},
    {R"([-9223372036854775809,1])", true, R"([-9223372036854776000.0,1])", "42"},
    {R"([1,00000000000000000000001])", true, R"([1,1])", "22"},
    {R"([1.5,1-2])", false, R"(invalid json at offset 6: expected , or ])", ""},
    {R"([1.5,1e-])", false, R"(invalid json at offset 8: bad number)", ""},
    {R"([1.5e+-2])", false, R"(invalid json at offset 6: bad number)", ""},
};

std::string element_types(const json::Value& v) {
    std::string s;
    for (const json::Value& e : v.array()) s += std::to_string((int)e.type());
    return s;
}
}  // namespace

TEST(DecimalToDouble, lax_forms_and_errors_parse_as_they_always_did) {
    for (const Recorded& r : kRecorded) {
        json::Value v;
        std::string err;
        const bool ok = json::Parse(r.text, strlen(r.text), &v, &err);
        EXPECT_TRUE_M(ok == r.ok, r.text);
        if (ok != r.ok) continue;
        if (ok) {
            EXPECT_EQ(v.ToString(), std::string(r.result));
            EXPECT_EQ(element_types(v), std::string(r.types));
        } else {
            EXPECT_EQ(err, std::string(r.result));
        }
    }
}

TEST(DecimalToDouble, narrow_double_bits_matches_the_cast) {
    const int64_t t0 = monotonic_us();
    std::mt19937_64 rng(24);
    long wrong = 0, n = 0;
    auto check = [&](uint64_t b) {
        ++n;
        const volatile double d = from_bits(b);
        const float f = (float)d;
        uint32_t fb;
        memcpy(&fb, &f, sizeof(fb));
        if (dd::NarrowDoubleBits(b) != fb && ++wrong < 5) EXPECT_EQ(dd::NarrowDoubleBits(b), fb);
    };
    for (int i = 0; i < 400000; ++i) check(rng());  // mostly far out of float range, NaN payloads among them
    for (int i = 0; i < 400000; ++i) {               // the float range, subnormal floats included
        check((rng() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 160 + rng() % 300) << 52));
    }
    for (int i = 0; i < 200000; ++i) {  // exact halves and their neighbours at every cut a float makes
        const int cut = 29 + (int)(rng() % 26);
        uint64_t b = (rng() & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(1023 - 126 - (cut - 29)) << 52);
        b &= ~((1ull << (cut > 52 ? 52 : cut)) - 1);
        if (cut <= 52) b |= 1ull << (cut - 1);
        check(b);
        check(b + 1);
        check(b - 1);
    }
    // every float subnormal boundary: each float subnormal and the smallest
    // normals, the doubles halfway between neighbours and the doubles next
    // to those; the same around the largest floats
    auto boundary = [&](uint32_t fb) {
        const uint64_t w = sd::WidenFloatBits(fb);
        if (dd::NarrowDoubleBits(w) != fb && ++wrong < 5) EXPECT_EQ(dd::NarrowDoubleBits(w), fb);
        const uint64_t next = sd::WidenFloatBits(fb + 1);
        if ((next >> 52) == 0x7FF) return;
        const uint64_t mid = to_bits((from_bits(w) + from_bits(next)) / 2);  // exact: one more bit
        check(mid);
        check(mid - 1);
        check(mid + 1);
        check(mid | (1ull << 63));
    };
    for (uint32_t fb = 0; fb < 0x00800040u; ++fb) boundary(fb);
    for (uint32_t fb = 0x7F7FFFC0u; fb < 0x7F800000u; ++fb) boundary(fb);
    for (uint32_t e = 0; e < 23; ++e) {  // the subnormal floats 2^-149 .. 2^-127 and half of the smallest
        check(sd::WidenFloatBits(1u << e));
        check(to_bits(from_bits(sd::WidenFloatBits(1u << e)) / 2));
    }
    for (uint64_t payload : {1ull, 1ull << 28, 1ull << 29, 1ull << 51, (1ull << 52) - 1, 0x5555555555555ull}) {
        check(0x7FF0000000000000ull | payload);
        check(0xFFF0000000000000ull | payload);
    }
    for (uint64_t b : std::vector<uint64_t>{0ull, 1ull << 63, 0x7FF0000000000000ull, 0xFFF0000000000000ull, to_bits(DBL_MAX),
                       to_bits(3.4028235677973366e38), to_bits(3.4028235677973362e38), to_bits(DBL_MIN), 1ull}) {
        check(b);
    }
    EXPECT_EQ(wrong, 0);
    EXPECT_GT(n, 1000000);
    printf("    %ld patterns in %.1f s\n", n, (double)(monotonic_us() - t0) / 1e6);
}

TEST(DecimalToDouble, integer_classes_convert_as_the_cast) {
    std::mt19937_64 rng(63);
    for (int i = 0; i < 200000; ++i) {
        const uint64_t u = rng() >> (rng() % 64);
        dd::NumberResult r{u, (uint8_t)(u > (uint64_t)INT64_MAX ? dd::kUInt64 : dd::kInt64)};
        ASSERT_EQ(dd::NumberToDoubleBits(r), to_bits((double)u));
        const int64_t s = (int64_t)(rng() >> (1 + rng() % 63)) * (rng() & 1 ? 1 : -1);
        dd::NumberResult q{(uint64_t)s, dd::kInt64};
        ASSERT_EQ(dd::NumberToDoubleBits(q), to_bits((double)s));
    }
    dd::NumberResult m{(uint64_t)INT64_MIN, dd::kInt64};
    EXPECT_EQ(dd::NumberToDoubleBits(m), to_bits((double)INT64_MIN));
    dd::NumberResult z{0, dd::kInt64};
    EXPECT_EQ(dd::NumberToDoubleBits(z), 0u);  // "-0" is the integer 0: +0.0
}

namespace {
// The DOM of `text` by the packed route and by the element-wise route the
// reader had before (std::from_chars per element, a Value per element).
void expect_same_dom(const std::string& text, int want_packed) {
    json::Value packed, plain;
    std::string e1, e2;
    const bool ok1 = json::Parse(text, &packed, &e1);
    json::SetPackedNumberArrays(false);
    const bool ok2 = json::Parse(text, &plain, &e2);
    json::SetPackedNumberArrays(true);
    ASSERT_TRUE_M(ok1 == ok2, text);
    if (!ok1) {
        EXPECT_EQ(e1, e2);
        return;
    }
    EXPECT_TRUE(plain.packed_numbers() == nullptr);
    EXPECT_TRUE_M(packed.ToString() == plain.ToString(), text.substr(0, 200));
    EXPECT_TRUE(packed.ToString(true) == plain.ToString(true));
    ASSERT_EQ(packed.size(), plain.size());
    if (want_packed >= 0) EXPECT_TRUE_M((packed.packed_numbers() != nullptr) == (want_packed == 1), text.substr(0, 200));
    if (packed.packed_numbers()) EXPECT_TRUE(packed.packed_ints() == nullptr);
    const std::vector<json::Value>& a = packed.array();
    const std::vector<json::Value>& b = plain.array();
    ASSERT_EQ(a.size(), b.size());
    for (size_t i = 0; i < a.size(); ++i) {
        ASSERT_EQ((int)a[i].type(), (int)b[i].type());
        if (!a[i].is_number()) continue;
        ASSERT_EQ(a[i].as_int(), b[i].as_int());
        ASSERT_EQ(a[i].as_uint(), b[i].as_uint());
        ASSERT_EQ(to_bits(a[i].as_double()), to_bits(b[i].as_double()));
    }
    if (!packed.is_array()) return;
    // copies and the mutating accessors
    json::Value copy = packed;
    EXPECT_TRUE(copy.ToString() == plain.ToString());
    copy.push_back(json::Value("tail"));
    EXPECT_TRUE(copy.packed_numbers() == nullptr);
    EXPECT_EQ(copy.size(), plain.size() + 1);
    EXPECT_TRUE(packed.ToString() == plain.ToString());  // the original is untouched
    json::Value copy2 = packed;
    EXPECT_EQ(copy2.mutable_array().size(), plain.size());
    EXPECT_TRUE(copy2.ToString() == plain.ToString());
}

std::string random_number(std::mt19937_64& rng, int kind) {
    switch (kind) {
    case 0: return std::to_string((int64_t)(rng() >> (1 + rng() % 63)) * (rng() & 1 ? 1 : -1));
    case 1: return shortest(from_bits((rng() & 0x7FEFFFFFFFFFFFFFull) | (rng() & 1 ? 1ull << 63 : 0)));
    case 2: return std::to_string(rng() | (1ull << 63));  // above INT64_MAX
    case 3: return e_form(std::fabs(from_bits(rng() & 0x7FEFFFFFFFFFFFFFull)), 1 + (int)(rng() % 30));
    default: return "-0";
    }
}
}  // namespace

TEST(DecimalToDouble, packed_number_dom_equals_the_element_wise_dom) {
    std::mt19937_64 rng(2026);
    auto join = [&](int n, auto pick, bool spaces) {
        std::string t = spaces ? " [ " : "[";
        for (int i = 0; i < n; ++i) {
            if (i) t += spaces && (rng() & 1) ? " ,\n\t" : ",";
            t += pick(i);
            if (spaces && (rng() & 3) == 0) t += "  ";
        }
        return t + (spaces ? " ] " : "]");
    };
    for (int round = 0; round < 40; ++round) {
        const int n = 1 + (int)(rng() % 60);
        const bool spaces = round % 4 == 3;
        expect_same_dom(join(n, [&](int) { return random_number(rng, 0); }, spaces), 0);            // ints only
        expect_same_dom(join(n, [&](int) { return random_number(rng, 1); }, spaces), 1);            // floats only
        expect_same_dom(join(n, [&](int i) { return random_number(rng, i == n - 1 ? 1 : 0); }, spaces), 1);  // a float last
        expect_same_dom(join(n, [&](int i) { return random_number(rng, i == 0 ? 3 : 0); }, spaces), 1);      // a float first
        expect_same_dom(join(n + 1, [&](int i) { return random_number(rng, i == n / 2 ? 2 : (int)(rng() % 5)); }, spaces), 1);
        // a string, a literal, an object or a nested array in the middle: Values
        const char* odd[] = {"\"s\"", "null", "true", "{\"a\":1.5}", "[1.5,2]", "[]"};
        expect_same_dom(join(n + 2, [&](int i) { return i == n / 2 + 1 ? std::string(odd[round % 6]) : random_number(rng, (int)(rng() % 5)); }, spaces), 0);
    }
    expect_same_dom("[]", 0);
    expect_same_dom("[1.5]", 1);
    expect_same_dom("[-0]", 0);
    expect_same_dom("[-0,-0.0]", 1);
    expect_same_dom("[1,18446744073709551615]", 1);
    expect_same_dom("[1,18446744073709551616]", 1);
    expect_same_dom("[1,00000000000000000000001]", 0);  // lax, and every element an int64: packed ints
    expect_same_dom("{\"a\":[1.5,2],\"b\":[[0.25,1e400],[3]]}", -1);
    expect_same_dom("[1.5,2,\"x\"", -1);
    expect_same_dom("[1.5,2,", -1);
    expect_same_dom("[1.5,2,]", -1);
    expect_same_dom("[1.5,1e5.3]", -1);
    for (const Recorded& r : kRecorded) expect_same_dom(r.text, -1);
    // the packed form itself
    json::Value v;
    ASSERT_TRUE(json::Parse(std::string("[1,2.5,18446744073709551615,-0.0,1e400]"), &v));
    const json::Value::NumberArray* p = v.packed_numbers();
    ASSERT_TRUE(p != nullptr);
    EXPECT_TRUE(v.packed_ints() == nullptr);
    EXPECT_EQ(v.size(), 5u);
    ASSERT_EQ(p->payload.size(), 5u);
    EXPECT_TRUE(p->classes == (std::vector<uint8_t>{dd::kInt64, dd::kDouble, dd::kUInt64, dd::kDouble, dd::kDouble}));
    EXPECT_EQ(p->payload[0], 1u);
    EXPECT_EQ(p->payload[1], to_bits(2.5));
    EXPECT_EQ(p->payload[2], 18446744073709551615ull);
    EXPECT_EQ(p->payload[3], 1ull << 63);
    EXPECT_EQ(p->payload[4], to_bits(INFINITY));
    EXPECT_EQ(&v.array(), &v.array());  // one published view
    EXPECT_EQ(v.ToString(), std::string("[1,2.5,18446744073709551615,-0.0,\"Infinity\"]"));
}

TEST(DecimalToDouble, parse_number_array_is_the_twin_of_the_reader) {
    const std::string text = " [ 1, 2.5 ,-0,\t-0.0,18446744073709551615, 1.0000000000000000000000000000001e0 ,7e-1] ";
    std::vector<uint32_t> seps;
    json::NumberArraySeparators(text.data(), text.size(), &seps);
    ASSERT_EQ(seps.size(), 8u);
    uint64_t payload[7];
    uint8_t classes[7];
    ASSERT_TRUE(json::ParseNumberArray(text.data(), seps.data(), seps.size(), payload, classes));
    json::Value v;
    ASSERT_TRUE(json::Parse(text, &v));
    ASSERT_TRUE(v.packed_numbers() != nullptr);
    for (int i = 0; i < 7; ++i) {
        EXPECT_EQ(payload[i], v.packed_numbers()->payload[i]);
        EXPECT_EQ((int)classes[i], (int)v.packed_numbers()->classes[i]);
    }
    const std::string bare = "1.5,2, 3e2";
    json::NumberArraySeparators(bare.data(), bare.size(), &seps);
    ASSERT_EQ(seps.size(), 4u);
    EXPECT_EQ(seps[0], 0xFFFFFFFFu);
    ASSERT_TRUE(json::ParseNumberArray(bare.data(), seps.data(), seps.size(), payload, classes));
    EXPECT_EQ(payload[0], to_bits(1.5));
    EXPECT_EQ(payload[1], 2u);
    EXPECT_EQ(payload[2], to_bits(300.0));
    size_t bad = 99;
    for (const char* t : {"1.5,1.,2", "1.5,,2", "1.5,\"NaN\",2", "1.5,01,2"}) {
        json::NumberArraySeparators(t, strlen(t), &seps);
        EXPECT_FALSE(json::ParseNumberArray(t, seps.data(), seps.size(), payload, classes, true, &bad));
        EXPECT_EQ(bad, 1u);
    }
    // exact = false leaves what a device lane would hand back
    std::string longish = "1.5," + std::string(dd::kMaxDeviceNumberChars + 1, '7') + ",2";
    json::NumberArraySeparators(longish.data(), longish.size(), &seps);
    ASSERT_TRUE(json::ParseNumberArray(longish.data(), seps.data(), seps.size(), payload, classes, false));
    EXPECT_EQ((int)classes[1], (int)dd::kNeedsExact);
    ASSERT_TRUE(json::ParseNumberArray(longish.data(), seps.data(), seps.size(), payload, classes, true));
    EXPECT_EQ((int)classes[1], (int)dd::kDouble);
    EXPECT_EQ(payload[1], strtod_bits(std::string(dd::kMaxDeviceNumberChars + 1, '7')));
}

TEST(DecimalToDouble, json2pb_takes_packed_numbers_in_bulk) {
    std::mt19937_64 rng(77);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::string fs, ds;
    for (int i = 0; i < 5000; ++i) {
        if (i) {
            fs += ',';
            ds += ',';
        }
        fs += i % 50 == 0 ? std::to_string(i - 100) : i % 51 == 0 ? "3.5e38" : shortest(normal(rng));
        ds += i % 70 == 0 ? std::to_string(rng() | (1ull << 63))
                          : i % 71 == 0 ? "1e400" : i % 73 == 0 ? "-0" : shortest(from_bits(rng() & 0xFFEFFFFFFFFFFFFFull));
    }
    const std::string body = "{\"name\":\"e\",\"fs\":[" + fs + "],\"ds\":[" + ds + "],\"ids\":[1,2,3]}";
    json::Value dom;
    ASSERT_TRUE(json::Parse(body, &dom));
    ASSERT_TRUE(dom.find("fs")->packed_numbers() != nullptr);
    ASSERT_TRUE(dom.find("ds")->packed_numbers() != nullptr);
    ASSERT_TRUE(dom.find("ids")->packed_ints() != nullptr);
    test::FloatArrays packed, plain;
    std::string err;
    ASSERT_TRUE(json2pb::JsonToProtoMessage(body, &packed, json2pb::Json2PbOptions(), &err));
    json::SetPackedNumberArrays(false);
    const bool ok = json2pb::JsonToProtoMessage(body, &plain, json2pb::Json2PbOptions(), &err);
    json::SetPackedNumberArrays(true);
    ASSERT_TRUE(ok);
    EXPECT_EQ(packed.fs_size(), 5000);
    EXPECT_EQ(packed.ds_size(), 5000);
    EXPECT_TRUE(packed.SerializeAsString() == plain.SerializeAsString());
    EXPECT_TRUE(std::isinf(packed.fs(51)));  // 3.5e38 overflows a float
    EXPECT_EQ(to_bits(packed.ds(73)), 0u);   // "-0" is the integer 0
    // packed numbers into an integer field: the element loop reports it, in
    // the words recorded before packed numbers existed
    test::FloatArrays m;
    EXPECT_FALSE(json2pb::JsonToProtoMessage(std::string("{\"ids\":[1,2.5]}"), &m, json2pb::Json2PbOptions(), &err));
    EXPECT_EQ(err, std::string("Invalid value `2.500000' for field `mrpc.test.FloatArrays.ids' which SHOULD be INT32"));
    EXPECT_FALSE(json2pb::JsonToProtoMessage(std::string("{\"ids\":[1.5,2]}"), &m, json2pb::Json2PbOptions(), &err));
    EXPECT_EQ(err, std::string("Invalid value `1.500000' for field `mrpc.test.FloatArrays.ids' which SHOULD be INT32"));
}

namespace {
int g_int_calls = 0, g_number_calls = 0;
bool declining_ints(const char*, const uint32_t*, size_t, std::vector<int64_t>*) {
    ++g_int_calls;
    return false;
}
bool twin_numbers(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload, uint8_t* classes) {
    ++g_number_calls;
    return json::ParseNumberArray(base, seps, nseps, payload, classes);
}
// quotes and {}[]:, outside strings (no escapes in these tests)
std::vector<uint32_t> host_index(const std::string& t) {
    std::vector<uint32_t> idx;
    bool in = false;
    for (size_t i = 0; i < t.size(); ++i) {
        if (t[i] == '"') {
            in = !in;
            idx.push_back((uint32_t)i);
        } else if (!in && strchr("{}[]:,", t[i])) {
            idx.push_back((uint32_t)i);
        }
    }
    return idx;
}
}  // namespace

TEST(DecimalToDouble, reader_tries_the_int_offload_first_then_the_number_offload) {
    const std::string body = "{\"a\":[1.5, 2,3e0,4],\"b\":[1,2],\"c\":[1.5,\"NaN\",2,3],\"d\":[1.5,1.,2,3]}";
    const std::vector<uint32_t> idx = host_index(body);
    json::Value plain, v;
    ASSERT_TRUE(json::Parse(body, &plain));
    json::SetIntArrayOffload(declining_ints, 4);
    json::SetNumberArrayOffload(twin_numbers, 3);
    g_int_calls = g_number_calls = 0;
    const bool ok = json::ParseWithIndex(body.data(), body.size(), idx.data(), idx.size(), &v);
    json::SetIntArrayOffload(nullptr, 0);
    json::SetNumberArrayOffload(nullptr, 0);
    ASSERT_TRUE(ok);
    // a: both thresholds met, the int offload declines, the number offload
    // takes it. b: below both. c: a string, no plain run. d: 4 elements, the
    // int offload declines, the number offload declines ("1." is lax), the
    // element-wise path parses it
    EXPECT_EQ(g_int_calls, 2);
    EXPECT_EQ(g_number_calls, 2);
    EXPECT_TRUE(v.ToString() == plain.ToString());
    EXPECT_TRUE(v.find("a")->packed_numbers() != nullptr);
    EXPECT_TRUE(v.find("d")->packed_numbers() != nullptr);
    // the number offload's own threshold: three elements reach it alone
    const std::string three = "[1.5,2,3]";
    const std::vector<uint32_t> idx3 = host_index(three);
    json::SetIntArrayOffload(declining_ints, 4);
    json::SetNumberArrayOffload(twin_numbers, 3);
    g_int_calls = g_number_calls = 0;
    ASSERT_TRUE(json::ParseWithIndex(three.data(), three.size(), idx3.data(), idx3.size(), &v));
    json::SetIntArrayOffload(nullptr, 0);
    json::SetNumberArrayOffload(nullptr, 0);
    EXPECT_EQ(g_int_calls, 0);
    EXPECT_EQ(g_number_calls, 1);
    EXPECT_EQ(v.ToString(), std::string("[1.5,2,3]"));
}

// Host half of gpu::DeviceParseNumberArrays: a refused or empty job reaches
// no kernel and none of its pointers is dereferenced, so this runs without a
// device. The device half is tests/test_gpu_json_float_parse.py.
TEST(DecimalToDouble, device_parse_refuses_bad_jobs_before_any_launch) {
    static char mem[128] __attribute__((aligned(16)));
    auto code = [](const void* text, const void* seps, uint64_t count, uint32_t mode, void* out, void* classes,
                   void* redo, uint32_t redo_cap) {
        gpu::DeviceNumberParseJob j;
        j.text = static_cast<const char*>(text);
        j.seps = static_cast<const uint32_t*>(seps);
        j.count = count;
        j.mode = mode;
        j.out = out;
        j.classes = static_cast<uint8_t*>(classes);
        j.redo = static_cast<uint32_t*>(redo);
        j.redo_cap = redo_cap;
        j.err = -1;
        j.n_redo = 99;
        EXPECT_EQ(gpu::DeviceParseNumberArrays(&j, 1, 0), 0);
        EXPECT_EQ(j.n_redo, 0u);
        EXPECT_EQ(j.first_bad, 0xFFFFFFFFu);
        return j.err;
    };
    EXPECT_EQ(code(nullptr, nullptr, 0, gpu::kJsonParseFloat64, nullptr, nullptr, nullptr, 0), 0);  // empty
    EXPECT_EQ(code(nullptr, mem, 4, gpu::kJsonParseFloat64, mem, nullptr, nullptr, 0), 2);  // null text
    EXPECT_EQ(code(mem, nullptr, 4, gpu::kJsonParseFloat64, mem, nullptr, nullptr, 0), 2);  // null seps
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseFloat64, nullptr, nullptr, nullptr, 0), 2);  // null out
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseNumbers, mem, nullptr, nullptr, 0), 2);      // numbers without classes
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseFloat64, mem, nullptr, nullptr, 8), 2);      // redo_cap without redo
    EXPECT_EQ(code(mem, mem, 4, 3, mem, mem, nullptr, 0), 2);                               // bad mode
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseFloat64, mem + 4, nullptr, nullptr, 0), 2);  // a double at 4 (mod 8)
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseNumbers, mem + 4, mem, nullptr, 0), 2);
    EXPECT_EQ(code(mem, mem, 4, gpu::kJsonParseFloat32, mem + 2, nullptr, nullptr, 0), 2);  // a float at 2 (mod 4)
    EXPECT_EQ(code(mem, mem, 0xFFFFFFFFull, gpu::kJsonParseFloat64, mem, nullptr, nullptr, 0), 2);  // above 2^32 - 2
    EXPECT_EQ(gpu::kJsonParseNumbers, gpu::JSON_PARSE_NUMBERS);
    EXPECT_EQ(gpu::kJsonParseFloat64, gpu::JSON_PARSE_FLOAT64);
    EXPECT_EQ(gpu::kJsonParseFloat32, gpu::JSON_PARSE_FLOAT32);
}
