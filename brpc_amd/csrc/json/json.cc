#include "json/json.h"

#include <charconv>

#include <algorithm>
#include <atomic>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "base/base64_rows.h"
#include "base/decimal_to_double.h"
#include "base/json_records.h"
#include "base/json_string.h"
#include "base/json_string_rows.h"
#include "base/number_print.h"
#include "base/number_text.h"
#include "base/shortest_double.h"
#include "base/util.h"

namespace mrpc {
namespace json {

const std::vector<Value>& Value::packed_view() const {
    std::shared_ptr<const std::vector<Value>> v = std::atomic_load(&_view);
    if (v) return *v;
    auto built = std::make_shared<std::vector<Value>>();
    if (_nums) {
        built->reserve(_nums->payload.size());
        for (size_t i = 0; i < _nums->payload.size(); ++i)
            built->push_back(NumberElement(_nums->payload[i], _nums->classes[i]));
    } else {
        built->reserve(_ints.size());
        for (int64_t x : _ints) built->emplace_back(x);
    }
    std::shared_ptr<const std::vector<Value>> want = built;
    // first publisher wins; a loser's copy is dropped, every reader gets the
    // published one
    std::shared_ptr<const std::vector<Value>> expected;
    if (std::atomic_compare_exchange_strong(&_view, &expected, want)) return *want;
    return *expected;
}

Value Value::NumberElement(uint64_t payload, uint8_t cls) {
    if (cls == decimal_to_double::kInt64) return Value((int64_t)payload);
    if (cls == decimal_to_double::kUInt64) return Value(payload);
    double d;
    memcpy(&d, &payload, sizeof(d));
    return Value(d);
}

int64_t Value::as_int() const {
    switch (_type) {
    case INT: return _i;
    case UINT: return (int64_t)_u;
    case DOUBLE: return (int64_t)_d;
    case BOOL: return _b;
    case STRING: return strtoll(_s.c_str(), nullptr, 10);
    default: return 0;
    }
}

uint64_t Value::as_uint() const {
    switch (_type) {
    case INT: return (uint64_t)_i;
    case UINT: return _u;
    case DOUBLE: return (uint64_t)_d;
    case BOOL: return _b;
    case STRING: return strtoull(_s.c_str(), nullptr, 10);
    default: return 0;
    }
}

double Value::as_double() const {
    switch (_type) {
    case INT: return (double)_i;
    case UINT: return (double)_u;
    case DOUBLE: return _d;
    case BOOL: return _b;
    case STRING: return strtod(_s.c_str(), nullptr);
    default: return 0;
    }
}

const Value* Value::find(const std::string& key) const {
    if (_type != OBJECT) return nullptr;
    for (auto& kv : _obj) {
        if (kv.first == key) return &kv.second;
    }
    return nullptr;
}

Value* Value::find(const std::string& key) {
    if (_type != OBJECT) return nullptr;
    for (auto& kv : _obj) {
        if (kv.first == key) return &kv.second;
    }
    return nullptr;
}

Value& Value::set(const std::string& key, Value v) {
    _type = OBJECT;
    Value* e = find(key);
    if (e) {
        *e = std::move(v);
        return *e;
    }
    _obj.emplace_back(key, std::move(v));
    return _obj.back().second;
}

Value& Value::operator[](const std::string& key) {
    _type = OBJECT;
    Value* e = find(key);
    if (e) return *e;
    _obj.emplace_back(key, Value());
    return _obj.back().second;
}

// Bytes that need no escape are copied in runs: a word at a time while no
// byte of it is a control character, '"' or '\\' (per-byte push_back was
// 43% of an http echo of a 32 KiB string field). The rules are
// base/json_string.h, the code the device escaper runs.
void EscapeStringBody(const char* p, size_t n, std::string* out) {
    namespace js = json_string;
    const char* const end = p + n;
    while (p < end) {
        const char* run = p;
        while (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            if (!js::PlainWord8(w)) break;
            p += 8;
        }
        while (p < end && js::EscapedSize((uint8_t)*p) == 1) ++p;
        out->append(run, (size_t)(p - run));
        if (p >= end) break;
        char b[8];
        out->append(b, js::EscapeByte((uint8_t)*p++, b));
    }
}

void EscapeString(const std::string& s, std::string* out) {
    out->reserve(out->size() + s.size() + 2);
    out->push_back('"');
    EscapeStringBody(s.data(), s.size(), out);
    out->push_back('"');
}

bool EscapeStringRows(const char* bytes, const uint32_t* row_ends, size_t rows, std::string* out) {
    for (size_t r = 1; r < rows; ++r) {
        if (row_ends[r] < row_ends[r - 1]) return false;
    }
    if (rows) out->reserve(out->size() + row_ends[rows - 1] + 3 * rows);
    uint32_t at = 0;
    for (size_t r = 0; r < rows; ++r) {
        if (r) out->push_back(',');
        out->push_back('"');
        EscapeStringBody(bytes + at, row_ends[r] - at, out);
        out->push_back('"');
        at = row_ends[r];
    }
    return true;
}

int UnescapeStringBody(const char* body, size_t n, std::string* out, uint64_t* first_bad) {
    namespace js = json_string;
    const size_t mark = out->size();
    out->reserve(mark + n);
    size_t p = 0, last_escape = (size_t)-1;  // where the escape before this one began
    while (p < n) {
        const size_t run = p;
        // a word at a time while it holds neither a backslash nor a quote
        while (n - p >= 8) {
            uint64_t w;
            memcpy(&w, body + p, 8);
            if ((js::EqMask8(w, '\\') | js::EqMask8(w, '"')) != 0) break;
            p += 8;
        }
        while (p < n && body[p] != '\\' && body[p] != '"') ++p;
        out->append(body + run, p - run);
        if (p >= n) break;
        char b[4];
        uint32_t span = 0;
        int got = js::kEscapeBad;
        if (body[p] == '\\') {
            got = js::DecodeEscape([&](int k) { return (uint8_t)body[(ptrdiff_t)p + k]; }, p, n - p,
                                   [&] { return last_escape == p - 6; }, b, &span);
        }
        if (got < 0) {
            out->resize(mark);
            if (first_bad) *first_bad = p;
            return 1;
        }
        out->append(b, (size_t)got);
        last_escape = p;
        p += span;
    }
    return 0;
}

int UnescapeStringRows(const char* text, size_t n, StringRows* out) {
    out->bytes.clear();
    out->row_ends.clear();
    out->depth = 0;
    out->first_bad = 0;
    out->bytes.reserve(json_string_rows::JsonStringRowsMaxBytes(n));
    const int rc = json_string_rows::WalkStringRows(
        [&](uint64_t k) { return (uint8_t)text[k]; }, n, [&](uint64_t from, uint64_t len) { out->bytes.append(text + from, len); },
        [&](const char* p, uint32_t len) { out->bytes.append(p, len); },
        [&] { out->row_ends.push_back((uint32_t)out->bytes.size()); }, &out->depth, &out->first_bad);
    if (rc != 0) {
        out->bytes.clear();
        out->row_ends.clear();
        out->depth = 0;
    }
    return rc;
}

bool EncodeBase64Rows(const char* bytes, const uint32_t* row_ends, size_t rows, bool brackets, std::string* out) {
    for (size_t r = 1; r < rows; ++r) {
        if (row_ends[r] < row_ends[r - 1]) return false;
    }
    size_t at = out->size();
    out->resize(at + base64_rows::Base64RowsWorstCaseBytes(rows ? row_ends[rows - 1] : 0, rows, brackets));
    char* o = &(*out)[0];
    if (brackets) o[at++] = '[';
    uint32_t from = 0;
    for (size_t r = 0; r < rows; ++r) {
        if (r) o[at++] = ',';
        o[at++] = '"';
        base64_encode_to(bytes + from, row_ends[r] - from, o + at);
        at += base64::Base64EncodedBytes(row_ends[r] - from);
        o[at++] = '"';
        from = row_ends[r];
    }
    if (brackets) o[at++] = ']';
    out->resize(at);
    return true;
}

int DecodeBase64Rows(const char* text, size_t n, StringRows* out) {
    out->bytes.clear();
    out->row_ends.clear();
    out->depth = 0;
    out->first_bad = 0;
    out->bytes.reserve(base64_rows::Base64RowsMaxBytes(n));
    const int rc = base64_rows::WalkBase64Rows(
        [&](uint64_t k) { return (uint8_t)text[k]; }, n, [&](const char* p, uint32_t len) { out->bytes.append(p, len); },
        [&] { out->row_ends.push_back((uint32_t)out->bytes.size()); }, &out->depth, &out->first_bad);
    if (rc != 0) {
        out->bytes.clear();
        out->row_ends.clear();
        out->depth = 0;
    }
    return rc;
}

size_t Utf8FirstBad(const char* s, size_t n) {
    namespace js = json_string;
    const uint8_t* u = reinterpret_cast<const uint8_t*>(s);
    size_t p = 0;
    while (p < n) {
        while (n - p >= 8) {  // a word at a time while all of it is ASCII
            uint64_t w;
            memcpy(&w, u + p, 8);
            if (w & 0x8080808080808080ull) break;
            p += 8;
        }
        if (p >= n) break;
        const size_t left = n - p;
        const uint32_t len = js::Utf8SequenceLen(u[p], left > 1 ? u[p + 1] : 0, left > 2 ? u[p + 2] : 0,
                                                 left > 3 ? u[p + 3] : 0, left);
        if (len == 0) return p;
        p += len;
    }
    return n;
}

// Shortest round-tripping decimal form of a double, laid out the way the
// reference's rapidjson Writer does (Grisu digits + Prettify): integral
// values keep a ".0" ("2.0"), plain decimals up to 21 integer digits,
// "0.000ddd" down to 1e-6, exponent form otherwise ("1e22", "1.5e-7").
// Matches the expected strings of test/brpc_protobuf_json_unittest.cpp.
void AppendShortestDouble(double d, std::string* out) {
    if (d == 0) {
        *out += std::signbit(d) ? "-0.0" : "0.0";
        return;
    }
    char buf[40];
    int prec = 1;
    for (; prec <= 17; ++prec) {
        snprintf(buf, sizeof(buf), "%.*e", prec - 1, d);
        if (strtod(buf, nullptr) == d) break;
    }
    // buf: [-]d[.ddd]e(+|-)XX
    const char* p = buf;
    if (*p == '-') {
        out->push_back('-');
        ++p;
    }
    std::string digits;
    for (; *p && *p != 'e'; ++p)
        if (*p != '.') digits.push_back(*p);
    const int e10 = atoi(p + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int length = (int)digits.size();
    const int kk = e10 + 1;      // position of the decimal point
    const int k = kk - length;   // zeros after the digits
    if (k >= 0 && kk <= 21) {
        *out += digits;
        out->append((size_t)k, '0');
        *out += ".0";
    } else if (kk > 0 && kk <= 21) {
        out->append(digits, 0, (size_t)kk);
        out->push_back('.');
        out->append(digits, (size_t)kk, std::string::npos);
    } else if (kk > -6 && kk <= 0) {
        *out += "0.";
        out->append((size_t)(-kk), '0');
        *out += digits;
    } else {
        out->push_back(digits[0]);
        if (length > 1) {
            out->push_back('.');
            out->append(digits, 1, std::string::npos);
        }
        out->push_back('e');
        *out += std::to_string(kk - 1);
    }
}

void Value::write(std::string* out, bool pretty, int indent) const {
    char buf[64];
    auto nl = [&](int ind) {
        if (!pretty) return;
        out->push_back('\n');
        out->append(ind * 2, ' ');
    };
    switch (_type) {
    case NUL: *out += "null"; break;
    case BOOL: *out += _b ? "true" : "false"; break;
    case INT: snprintf(buf, sizeof(buf), "%lld", (long long)_i); *out += buf; break;
    case UINT: snprintf(buf, sizeof(buf), "%llu", (unsigned long long)_u); *out += buf; break;
    case DOUBLE:
        if (std::isnan(_d) || std::isinf(_d)) {
            *out += std::isnan(_d) ? "\"NaN\"" : (_d > 0 ? "\"Infinity\"" : "\"-Infinity\"");
        } else {
            AppendShortestDouble(_d, out);
        }
        break;
    case STRING: EscapeString(_s, out); break;
    case RAW: *out += _s; break;
    case ARRAY:
        if (_nums) {  // each element as its INT / UINT / DOUBLE Value prints
            out->push_back('[');
            for (size_t i = 0; i < _nums->payload.size(); ++i) {
                if (i) out->push_back(',');
                nl(indent + 1);
                const uint64_t x = _nums->payload[i];
                const uint8_t cls = _nums->classes[i];
                if (cls == decimal_to_double::kInt64) {
                    snprintf(buf, sizeof(buf), "%lld", (long long)x);
                    *out += buf;
                } else if (cls == decimal_to_double::kUInt64) {
                    snprintf(buf, sizeof(buf), "%llu", (unsigned long long)x);
                    *out += buf;
                } else {
                    NumberElement(x, cls).write(out, pretty, indent + 1);
                }
            }
            nl(indent);
            out->push_back(']');
            break;
        }
        if (!_ints.empty()) {
            out->push_back('[');
            for (size_t i = 0; i < _ints.size(); ++i) {
                if (i) out->push_back(',');
                nl(indent + 1);
                snprintf(buf, sizeof(buf), "%lld", (long long)_ints[i]);
                *out += buf;
            }
            nl(indent);
            out->push_back(']');
            break;
        }
        out->push_back('[');
        for (size_t i = 0; i < _arr.size(); ++i) {
            if (i) out->push_back(',');
            nl(indent + 1);
            _arr[i].write(out, pretty, indent + 1);
        }
        if (!_arr.empty()) nl(indent);
        out->push_back(']');
        break;
    case OBJECT:
        out->push_back('{');
        for (size_t i = 0; i < _obj.size(); ++i) {
            if (i) out->push_back(',');
            nl(indent + 1);
            EscapeString(_obj[i].first, out);
            out->push_back(':');
            if (pretty) out->push_back(' ');
            _obj[i].second.write(out, pretty, indent + 1);
        }
        if (!_obj.empty()) nl(indent);
        out->push_back('}');
        break;
    }
}

std::string Value::ToString(bool pretty) const {
    std::string s;
    write(&s, pretty, 0);
    return s;
}

namespace {
std::atomic<IntArrayOffload> g_int_array_offload{nullptr};
std::atomic<size_t> g_int_array_min{(size_t)-1};
}  // namespace

void SetIntArrayOffload(IntArrayOffload fn, size_t min_elems) {
    g_int_array_min.store(fn ? (min_elems ? min_elems : 1) : (size_t)-1, std::memory_order_relaxed);
    g_int_array_offload.store(fn, std::memory_order_release);
}

namespace {
std::atomic<NumberArrayOffload> g_number_array_offload{nullptr};
std::atomic<size_t> g_number_array_min{(size_t)-1};
std::atomic<bool> g_packed_numbers{true};

namespace dd = decimal_to_double;

inline bool json_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// A decimal int64 literal at [p, end): the end of its digits, or nullptr
// (no digits, more than 19 digits, or out of int64 range: the caller
// takes the general path). Up to 19 digits cannot overflow a uint64, so
// the loop has no per-digit overflow check.
const char* parse_int64(const char* p, const char* end, int64_t* out) {
    const bool neg = p < end && *p == '-';
    if (neg) ++p;
    const char* b = p;
    const char* lim = end - p > 19 ? p + 19 : end;
    uint64_t v = 0;
    while (p < lim && (unsigned)(*p - '0') < 10u) v = v * 10 + (unsigned)(*p++ - '0');
    if (p == b || (p < end && (unsigned)(*p - '0') < 10u)) return nullptr;
    if (neg) {
        if (v > (uint64_t)INT64_MAX + 1) return nullptr;
        *out = (int64_t)(0 - v);
    } else {
        if (v > (uint64_t)INT64_MAX) return nullptr;
        *out = (int64_t)v;
    }
    return p;
}

// The general number route (std::from_chars: no std::string per number, no
// errno/strtoll round trip) over text [b, e) made of digits, '.', 'e', 'E'
// and exponent signs after a leading -?digit: laxer than RFC 8259 ("01",
// "1."). is_float: the text holds '.', 'e' or 'E'. False: "bad number".
bool convert_number_general(const char* b, const char* e, bool is_float, uint64_t* payload, uint8_t* cls) {
    if (!is_float) {
        int64_t x;
        if (parse_int64(b, e, &x) == e) {
            *payload = (uint64_t)x;
            *cls = dd::kInt64;
            return true;
        }
        if (*b != '-') {
            uint64_t x;
            auto r = std::from_chars(b, e, x);
            if (r.ec == std::errc() && r.ptr == e) {
                *payload = x;
                *cls = x <= (uint64_t)INT64_MAX ? dd::kInt64 : dd::kUInt64;
                return true;
            }
        }
    }
    double d = 0;
    auto r = std::from_chars(b, e, d);
    if (r.ec == std::errc::result_out_of_range) {
        d = strtod(std::string(b, e - b).c_str(), nullptr);  // +-inf / denormal edge, as before
    } else if (r.ec != std::errc() || r.ptr != e) {
        return false;
    }
    memcpy(payload, &d, sizeof(d));
    *cls = dd::kDouble;
    return true;
}

// -? (0 | [1-9][0-9]*) (\.[0-9]+)? ([eE][+-]?[0-9]+)? over all of [p, e)
bool rfc8259_number(const char* p, const char* e, bool* is_float) {
    auto digit = [&](const char* q) { return q < e && (unsigned)(*q - '0') < 10u; };
    *is_float = false;
    if (p < e && *p == '-') ++p;
    if (!digit(p)) return false;
    if (*p == '0') {
        ++p;
    } else {
        while (digit(p)) ++p;
    }
    if (p < e && *p == '.') {
        *is_float = true;
        ++p;
        if (!digit(p)) return false;
        while (digit(p)) ++p;
    }
    if (p < e && (*p == 'e' || *p == 'E')) {
        *is_float = true;
        ++p;
        if (p < e && (*p == '+' || *p == '-')) ++p;
        if (!digit(p)) return false;
        while (digit(p)) ++p;
    }
    return p == e;
}
}  // namespace

void SetNumberArrayOffload(NumberArrayOffload fn, size_t min_elems) {
    g_number_array_min.store(fn ? (min_elems ? min_elems : 1) : (size_t)-1, std::memory_order_relaxed);
    g_number_array_offload.store(fn, std::memory_order_release);
}

void SetPackedNumberArrays(bool on) { g_packed_numbers.store(on, std::memory_order_relaxed); }

bool ParseNumberExact(const char* b, const char* e, uint64_t* payload, uint8_t* cls) {
    bool is_float;
    return rfc8259_number(b, e, &is_float) && convert_number_general(b, e, is_float, payload, cls);
}

void NumberArraySeparators(const char* text, size_t n, std::vector<uint32_t>* seps) {
    seps->clear();
    size_t b = 0, e = n;
    while (b < e && json_space(text[b])) ++b;
    while (e > b && json_space(text[e - 1])) --e;
    const bool bracketed = e - b >= 2 && text[b] == '[' && text[e - 1] == ']';
    seps->push_back(bracketed ? (uint32_t)b : 0xFFFFFFFFu);
    const size_t from = bracketed ? b + 1 : 0, to = bracketed ? e - 1 : n;
    for (size_t i = from; i < to; ++i) {
        if (text[i] == ',') seps->push_back((uint32_t)i);
    }
    seps->push_back((uint32_t)to);
}

bool ParseNumberArray(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload, uint8_t* classes,
                      bool exact, size_t* bad_index) {
    for (size_t i = 0; i + 1 < nseps; ++i) {
        const char* b = base + (uint32_t)(seps[i] + 1);  // 0xFFFFFFFF: before the first byte
        const char* e = base + seps[i + 1];
        while (b < e && json_space(*b)) ++b;
        while (e > b && json_space(e[-1])) --e;
        dd::NumberResult r;
        dd::ParseJsonNumber(b, e, &r);
        if (r.cls == dd::kNeedsExact && exact && !ParseNumberExact(b, e, &r.bits, &r.cls)) r.cls = dd::kMalformed;
        if (r.cls == dd::kMalformed) {
            if (bad_index) *bad_index = i;
            return false;
        }
        payload[i] = r.bits;
        classes[i] = r.cls;
    }
    return true;
}

bool ParseNumberText(const char* text, size_t n, uint32_t mode, NumberText* out, bool exact, bool nested_ok) {
    namespace nt = number_text;
    *out = NumberText();
    if (mode > 2 || n >= 0xFFFFFFFFull || (!text && n > 0)) {
        out->err = 2;
        return false;
    }
    if (n == 0) return true;
    const uint32_t N = (uint32_t)n;
    // the k-th ']' ends row k (the last one closes the outer array)
    uint32_t commas = 0, closes = 0;
    for (uint32_t i = 0; i < N; ++i) {
        if (text[i] == ',') ++commas;
        else if (text[i] == ']') {
            ++closes;
            if (nested_ok) out->row_ends.push_back(commas + 1);
        }
    }
    const dd::PointerAt at{text};
    const size_t width = mode == 2 ? 4 : 8;
    out->out.reserve(((size_t)commas + 1) * width);
    nt::TextState st{nt::kNone, nt::kNone, 0, 0, 0};
    uint32_t b = 0;
    // in index order, so the first piece found wanting is the lowest
    for (uint32_t idx = 0;; ++idx) {
        nt::Piece s;
        nt::ScanPiece(at, b, N, &s);
        const uint32_t verdict = nt::JudgePiece(s, idx, N, idx > 0 && nt::ClosesBefore(at, b - 1));
        if (verdict & nt::kPieceBad) {
            st.bad = idx;
            break;
        }
        if (idx == 0) st.lead0 = s.lead;
        if (s.end == N) st.trail_last = s.trail;
        if (verdict & nt::kPieceBlank) {
            st.blank = 1;
            break;
        }
        if ((verdict & nt::kPieceNested) && st.nested_min == nt::kNone) st.nested_min = idx;
        dd::NumberResult r;
        dd::ParseJsonNumber(text + s.nb, text + s.ne, &r);
        if (r.cls == dd::kNeedsExact) {
            if (!exact) {
                out->redo.push_back(idx);
                out->redo.push_back(b);
                r.bits = 0;
            } else if (!ParseNumberExact(text + s.nb, text + s.ne, &r.bits, &r.cls)) {
                r.cls = dd::kMalformed;
            }
        }
        if (r.cls == dd::kMalformed) {
            st.bad = idx;
            break;
        }
        if (mode == 0) {
            out->out.append(reinterpret_cast<const char*>(&r.bits), 8);
            out->classes.push_back((char)r.cls);
        } else {
            const uint64_t d = r.cls == dd::kNeedsExact ? 0 : dd::NumberToDoubleBits(r);
            if (mode == 1) {
                out->out.append(reinterpret_cast<const char*>(&d), 8);
            } else {
                const uint32_t f = dd::NarrowDoubleBits(d);
                out->out.append(reinterpret_cast<const char*>(&f), 4);
            }
        }
        if (s.end == N) break;
        b = s.end + 1;
    }
    const nt::TextVerdict v = nt::CombineNumberText(st, commas, closes, nested_ok);
    out->depth = v.depth;
    out->count = v.count;
    out->rows = v.rows;
    out->first_bad = v.first_bad;
    if (v.first_bad != nt::kNone) {
        out->err = 1;
        out->out.clear();
        out->classes.clear();
        out->row_ends.clear();
        out->redo.clear();
        return false;
    }
    out->row_ends.resize(v.rows);
    return true;
}

int FormatNumberRows(const void* values, uint64_t count, uint32_t kind, const uint32_t* row_ends, uint64_t rows,
                     bool brackets, std::string* out, uint32_t* first_bad) {
    namespace np = number_print;
    namespace sd = shortest_double;
    if (first_bad) *first_bad = np::kNone;
    if (!np::KindValid(kind) || (!values && count > 0) || ((uintptr_t)values & (np::ElemBytes(kind) - 1)) != 0 ||
        (row_ends == nullptr) != (rows == 0) || np::WorstCaseBytes(kind, count, rows) > 0xFFFFFFFFull)
        return 2;
    const uint32_t form = row_ends ? np::kNested : brackets ? np::kBracketed : np::kBare;
    uint32_t prev = 0;
    for (uint64_t r = 0; r < rows; ++r) {  // in row order, so the first row found wanting is the lowest
        if (np::RowEndBad(prev, row_ends[r], r, rows, count)) {
            if (first_bad) *first_bad = (uint32_t)r;
            return 1;
        }
        prev = row_ends[r];
    }
    if (count == 0) {
        if (form == np::kBracketed) out->append("[]");
        return 0;
    }
    const size_t before = out->size();
    size_t used = before;
    uint64_t next_row = 0;  // the row whose end is looked for
    for (uint64_t i = 0; i < count; ++i) {
        if (out->size() - used < np::kMaxLead + np::kMaxElemChars + np::kMaxTrail)
            out->resize(used + std::max<size_t>(4096, (count - i) * 8) + np::kMaxLead + np::kMaxElemChars + np::kMaxTrail);
        char* o = &(*out)[used];
        bool row_start = false;
        if (form == np::kNested && i > 0 && row_ends[next_row] == i) {
            row_start = true;
            ++next_row;
        }
        o += np::FormatLead(form, i == 0, row_start, o);
        if (kind == np::kBool) {
            o += np::FormatBool(static_cast<const uint8_t*>(values)[i] != 0, o);
        } else if (kind == np::kFloat32) {
            o += sd::FormatJsonDoubleBits(sd::WidenFloatBits(static_cast<const uint32_t*>(values)[i]), o);
        } else if (kind == np::kFloat64) {
            o += sd::FormatJsonDoubleBits(static_cast<const uint64_t*>(values)[i], o);
        } else {
            o += np::FormatInteger(np::LoadInteger(values, i, kind), o);
        }
        o += np::FormatTrail(form, i + 1 == count, o);
        used = (size_t)(o - out->data());
    }
    out->resize(used);
    return 0;
}

bool RecordObjectPrefixes(const json_records::Job& job, std::vector<std::string>* prefixes) {
    namespace jr = json_records;
    prefixes->clear();
    if (!job.columns || job.ncols < 1 || job.ncols > jr::kMaxColumns) return false;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const jr::Column& col = job.columns[c];
        if (!col.key && col.key_len > 0) return false;
        for (uint32_t d = 0; d < c; ++d) {
            const jr::Column& other = job.columns[d];
            if (other.key_len == col.key_len && (col.key_len == 0 || memcmp(other.key, col.key, col.key_len) == 0))
                return false;
        }
        std::string escaped;
        EscapeStringBody(static_cast<const char*>(col.key), col.key_len, &escaped);
        if (escaped.size() > jr::kMaxEscapedKey) return false;
        uint8_t buf[jr::kMaxPrefixBytes];
        const uint32_t n = jr::PutPrefix(c, escaped.data(), (uint32_t)escaped.size(), buf);
        prefixes->emplace_back(reinterpret_cast<const char*>(buf), n);
    }
    return true;
}

int FormatRecordObjects(const json_records::Job& job, std::string* out, uint32_t* first_bad, uint32_t* bad_column) {
    namespace jr = json_records;
    if (first_bad) *first_bad = jr::kNone;
    if (bad_column) *bad_column = jr::kNone;
    std::vector<std::string> prefixes;
    if (!jr::FieldsOk(job) || !RecordObjectPrefixes(job, &prefixes)) return 2;
    uint64_t prefix_bytes = 0;
    for (const std::string& p : prefixes) prefix_bytes += p.size();
    if (jr::WorstCaseBytes(job, prefix_bytes) > 0xFFFFFFFFull) return 2;
    for (uint32_t c = 0; c < job.ncols; ++c) {
        const jr::Column& col = job.columns[c];
        if ((!col.src && col.count > 0) || ((uintptr_t)col.src & (jr::ElemBytes(col.kind) - 1)) != 0 ||
            ((uintptr_t)col.row_ends & 3) != 0)
            return 2;
    }
    if (job.rows == 0) {
        if (job.brackets) out->append("[]");
        return 0;
    }
    const size_t before = out->size();
    char num[number_print::kMaxElemChars];
    for (uint64_t r = 0; r < job.rows; ++r) {  // in row order, columns inside: the first offender is the lowest
        if (jr::LeadBytes(r, job.brackets)) out->push_back(r > 0 ? ',' : '[');
        for (uint32_t c = 0; c < job.ncols; ++c) {
            const jr::Column& col = job.columns[c];
            out->append(prefixes[c]);
            if (!col.row_ends) {
                out->append(num, jr::FormatElem(col.src, r, col.kind, num));
                continue;
            }
            const uint32_t s = r ? col.row_ends[r - 1] : 0u, e = col.row_ends[r];
            if (jr::RowEndBad(s, e, r, job.rows, col.count)) {
                out->resize(before);
                if (first_bad) *first_bad = (uint32_t)r;
                if (bad_column) *bad_column = c;
                return 1;
            }
            if (col.text == jr::kBase64) {
                out->push_back('"');
                for (uint32_t k = 0; k < e - s; k += 3) {
                    const uint32_t sym = jr::Base64Group(static_cast<const uint8_t*>(col.src) + s, k, e - s);
                    for (int b = 0; b < 4; ++b) out->push_back((char)(sym >> (8 * b)));
                }
                out->push_back('"');
                continue;
            }
            const bool str = col.text == jr::kString;
            out->push_back(str ? '"' : '[');
            for (uint32_t i = s; i < e; ++i) {
                if (!str && i > s) out->push_back(',');
                out->append(num, jr::FormatElem(col.src, i, col.kind, num));
            }
            out->push_back(str ? '"' : ']');
        }
        out->push_back('}');
        if (jr::TrailBytes(r, job.rows, job.brackets)) out->push_back(']');
    }
    return 0;
}

namespace {
class Reader {
public:
    Reader(const char* p, size_t n) : _p(p), _end(p + n), _begin(p) {}
    // A structural index (offsets of unescaped quotes and of {}[]:, outside
    // strings, ascending — gpu/json_kernels.hip): strings end at the next
    // indexed quote instead of a byte scan. An index that disagrees with the
    // text is ignored from that point on.
    void set_index(const uint32_t* idx, size_t n) {
        _idx = idx;
        _nidx = n;
        _k = 0;
    }
    bool parse(Value* v, std::string* err) {
        skip();
        if (!value(v, 0)) {
            if (err) *err = "invalid json at offset " + std::to_string(_p - _begin) + ": " + _err;
            return false;
        }
        skip();
        if (_p != _end) {
            if (err) *err = "trailing characters at offset " + std::to_string(_p - _begin);
            return false;
        }
        return true;
    }

private:
    void skip() {
        while (_p < _end && (*_p == ' ' || *_p == '\t' || *_p == '\n' || *_p == '\r')) ++_p;
    }
    bool fail(const char* m) {
        _err = m;
        return false;
    }
    bool value(Value* v, int depth) {
        if (depth > 200) return fail("nesting too deep");
        if (_p >= _end) return fail("unexpected end");
        switch (*_p) {
        case '{': return object(v, depth);
        case '[': return array(v, depth);
        case '"': {
            std::string s;
            if (!string(&s)) return false;
            *v = Value(s);
            return true;
        }
        case 't':
            if (_end - _p >= 4 && memcmp(_p, "true", 4) == 0) {
                _p += 4;
                *v = Value(true);
                return true;
            }
            return fail("bad literal");
        case 'f':
            if (_end - _p >= 5 && memcmp(_p, "false", 5) == 0) {
                _p += 5;
                *v = Value(false);
                return true;
            }
            return fail("bad literal");
        case 'n':
            if (_end - _p >= 4 && memcmp(_p, "null", 4) == 0) {
                _p += 4;
                *v = Value();
                return true;
            }
            return fail("bad literal");
        default: return number(v);
        }
    }
    // Numbers are converted in place from the text: base/decimal_to_double.h
    // when the text is of the RFC 8259 grammar and it decides the rounding,
    // the general route (std::from_chars) for everything else, so laxness
    // and error text are what they always were.
    bool number(Value* v) {
        uint64_t payload;
        uint8_t cls;
        if (!number_raw(&payload, &cls)) return false;
        if (cls == dd::kInt64) {
            *v = Value((int64_t)payload);
        } else if (cls == dd::kUInt64) {
            *v = Value(payload);
        } else {
            double d;
            memcpy(&d, &payload, sizeof(d));
            *v = Value(d);
        }
        return true;
    }
    bool number_raw(uint64_t* payload, uint8_t* cls) {
        const char* b = _p;
        if (_p < _end && *_p == '-') ++_p;
        if (_p >= _end || !isdigit((unsigned char)*_p)) return fail("bad number");
        bool is_float = false;
        while (_p < _end && (isdigit((unsigned char)*_p) || *_p == '.' || *_p == 'e' || *_p == 'E' ||
                             ((*_p == '+' || *_p == '-') && (_p[-1] == 'e' || _p[-1] == 'E')))) {
            if (*_p == '.' || *_p == 'e' || *_p == 'E') is_float = true;
            ++_p;
        }
        if (g_packed_numbers.load(std::memory_order_relaxed)) {
            dd::NumberResult r;
            dd::ParseJsonNumber(b, _p, &r);
            if (r.cls <= dd::kDouble) {
                *payload = r.bits;
                *cls = r.cls;
                return true;
            }
        }
        if (!convert_number_general(b, _p, is_float, payload, cls)) return fail("bad number");
        return true;
    }
    // An integer element of an int array, converted in place: true with *x
    // when the next value is a plain int64 literal followed by ',' or ']'
    // (after spaces); false (nothing consumed) otherwise.
    bool int_element(int64_t* x) {
        const char* e = parse_int64(_p, _end, x);
        if (!e) return false;
        if (e < _end && (*e == '.' || *e == 'e' || *e == 'E')) return false;
        _p = e;
        return true;
    }
    static void put_utf8(std::string* s, uint32_t cp) {
        if (cp < 0x80) {
            s->push_back((char)cp);
        } else if (cp < 0x800) {
            s->push_back((char)(0xC0 | (cp >> 6)));
            s->push_back((char)(0x80 | (cp & 0x3F)));
        } else if (cp < 0x10000) {
            s->push_back((char)(0xE0 | (cp >> 12)));
            s->push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            s->push_back((char)(0x80 | (cp & 0x3F)));
        } else {
            s->push_back((char)(0xF0 | (cp >> 18)));
            s->push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
            s->push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            s->push_back((char)(0x80 | (cp & 0x3F)));
        }
    }
    bool hex4(uint32_t* out) {
        if (_end - _p < 4) return fail("bad unicode escape");
        uint32_t v = 0;
        for (int i = 0; i < 4; ++i) {
            char c = _p[i];
            v <<= 4;
            if (c >= '0' && c <= '9') v |= c - '0';
            else if (c >= 'a' && c <= 'f') v |= c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') v |= c - 'A' + 10;
            else return fail("bad unicode escape");
        }
        _p += 4;
        *out = v;
        return true;
    }
    // Closing quote of the string opening at _p from the index, or nullptr.
    const char* indexed_close() {
        if (!_idx) return nullptr;
        const size_t at = (size_t)(_p - _begin);
        while (_k < _nidx && _idx[_k] < at) ++_k;
        if (_k + 1 >= _nidx || _idx[_k] != at || _idx[_k + 1] >= (size_t)(_end - _begin) ||
            _begin[_idx[_k + 1]] != '"') {
            _idx = nullptr;  // stale or foreign index: scan from here on
            return nullptr;
        }
        const char* close = _begin + _idx[_k + 1];
        _k += 2;
        return close;
    }
    bool string(std::string* s) {
        if (const char* close = indexed_close()) {
            const char* b = _p + 1;
            // only trusted when the range holds no quote or backslash: then
            // `close` is certainly this string's end
            if (!memchr(b, '\\', (size_t)(close - b)) && !memchr(b, '"', (size_t)(close - b))) {
                s->append(b, (size_t)(close - b));
                _p = close + 1;
                return true;
            }
        }
        ++_p;  // opening quote
        for (;;) {  // runs without escapes or quotes go in one append
            const char* q = _p;
            // the closing quote, then any backslash before it (both memchr)
            const char* quote = (const char*)memchr(q, '"', (size_t)(_end - q));
            if (!quote) quote = _end;
            const char* bs = (const char*)memchr(q, '\\', (size_t)(quote - q));
            q = bs ? bs : quote;
            s->append(_p, (size_t)(q - _p));
            _p = q;
            if (_p >= _end || *_p == '"') break;
            ++_p;  // backslash
            if (_p >= _end) return fail("bad escape");
            if (!escape(s)) return false;
        }
        if (_p >= _end) return fail("unterminated string");
        ++_p;
        return true;
    }
    bool escape(std::string* s) {
        char e = *_p++;
        switch (e) {
        case '"': s->push_back('"'); break;
        case '\\': s->push_back('\\'); break;
        case '/': s->push_back('/'); break;
        case 'b': s->push_back('\b'); break;
        case 'f': s->push_back('\f'); break;
        case 'n': s->push_back('\n'); break;
        case 'r': s->push_back('\r'); break;
        case 't': s->push_back('\t'); break;
        case 'u': {
            uint32_t cp;
            if (!hex4(&cp)) return false;
            if (cp >= 0xD800 && cp < 0xDC00 && _end - _p >= 6 && _p[0] == '\\' && _p[1] == 'u') {
                _p += 2;
                uint32_t lo;
                if (!hex4(&lo)) return false;
                cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
            }
            put_utf8(s, cp);
            break;
        }
        default: return fail("bad escape");
        }
        return true;
    }
    // The index shows an array of plain elements (only ',' between the
    // brackets): one bulk parse instead of a Value per element. The integer
    // offload is tried first when the run meets its minimum, then the number
    // offload when the run meets its own; false leaves the array to the
    // element-wise path.
    bool bulk_array(Value* v) {
        if (!_idx) return false;
        IntArrayOffload fn = g_int_array_offload.load(std::memory_order_acquire);
        NumberArrayOffload nfn = g_number_array_offload.load(std::memory_order_acquire);
        if (!fn && !nfn) return false;
        const size_t at = (size_t)(_p - _begin);
        while (_k < _nidx && _idx[_k] < at) ++_k;
        if (_k >= _nidx || _idx[_k] != at) return false;
        size_t j = _k + 1;
        const size_t len = (size_t)(_end - _begin);
        while (j < _nidx && _idx[j] < len && _begin[_idx[j]] == ',') ++j;
        if (j >= _nidx || _idx[j] >= len || _begin[_idx[j]] != ']') return false;
        const size_t n = j - _k;
        bool done = false;
        if (fn && n >= g_int_array_min.load(std::memory_order_relaxed)) {
            std::vector<int64_t> ints;
            if (fn(_begin, _idx + _k, n + 1, &ints) && ints.size() == n) {
                *v = Value::PackedInts(std::move(ints));
                done = true;
            }
        }
        if (!done && nfn && n >= g_number_array_min.load(std::memory_order_relaxed) &&
            g_packed_numbers.load(std::memory_order_relaxed)) {
            Value::NumberArray nums;
            nums.payload.resize(n);
            nums.classes.resize(n);
            if (nfn(_begin, _idx + _k, n + 1, nums.payload.data(), nums.classes.data())) {
                *v = packed(std::move(nums));
                done = true;
            }
        }
        if (!done) return false;
        _p = _begin + _idx[j] + 1;
        _k = j + 1;
        return true;
    }
    // Packed numbers; packed ints when every element turned out an int64
    static Value packed(Value::NumberArray nums) {
        for (uint8_t c : nums.classes) {
            if (c != dd::kInt64) return Value::PackedNumbers(std::move(nums));
        }
        std::vector<int64_t> ints(nums.payload.size());
        if (!ints.empty()) memcpy(ints.data(), nums.payload.data(), ints.size() * sizeof(int64_t));
        return Value::PackedInts(std::move(ints));
    }
    bool array(Value* v, int depth) {
        if (bulk_array(v)) return true;
        ++_p;
        *v = Value::Array();
        skip();
        if (_p < _end && *_p == ']') {
            ++_p;
            return true;
        }
        // Integer arrays stay packed (one int64 per element, no Value per
        // element; json2pb takes them in bulk, the way rapidjson's in-situ
        // numbers feed the reference's json_to_pb.cpp). The first element
        // that is not a plain int64 but is a number carries the array on in
        // packed-number form (8 bytes and a class byte per element); the
        // first element that is no number turns it into Values.
        std::vector<int64_t> ints;
        for (;;) {
            int64_t x;
            skip();
            if (!int_element(&x)) break;
            ints.push_back(x);
            skip();
            if (_p < _end && *_p == ',') {
                ++_p;
                continue;
            }
            if (_p < _end && *_p == ']') {
                ++_p;
                *v = Value::PackedInts(std::move(ints));
                return true;
            }
            return fail("expected , or ]");
        }
        auto starts_number = [&] { return _p < _end && (*_p == '-' || isdigit((unsigned char)*_p)); };
        if (g_packed_numbers.load(std::memory_order_relaxed) && starts_number()) {
            Value::NumberArray nums;
            nums.payload.assign(ints.begin(), ints.end());
            nums.classes.assign(ints.size(), (uint8_t)dd::kInt64);
            while (starts_number()) {
                uint64_t payload;
                uint8_t cls;
                if (!number_raw(&payload, &cls)) return false;
                nums.payload.push_back(payload);
                nums.classes.push_back(cls);
                skip();
                if (_p < _end && *_p == ',') {
                    ++_p;
                    skip();
                    continue;
                }
                if (_p < _end && *_p == ']') {
                    ++_p;
                    *v = packed(std::move(nums));
                    return true;
                }
                return fail("expected , or ]");
            }
            // no number: the element-wise loop takes over where this one stands
            for (size_t i = 0; i < nums.payload.size(); ++i)
                v->push_back(Value::NumberElement(nums.payload[i], nums.classes[i]));
        } else {
            for (int64_t x : ints) v->push_back(Value(x));
        }
        for (;;) {
            Value e;
            skip();
            if (!value(&e, depth + 1)) return false;
            v->push_back(std::move(e));
            skip();
            if (_p < _end && *_p == ',') {
                ++_p;
                continue;
            }
            if (_p < _end && *_p == ']') {
                ++_p;
                return true;
            }
            return fail("expected , or ]");
        }
    }
    bool object(Value* v, int depth) {
        ++_p;
        *v = Value::Object();
        skip();
        if (_p < _end && *_p == '}') {
            ++_p;
            return true;
        }
        for (;;) {
            skip();
            if (_p >= _end || *_p != '"') return fail("expected key");
            std::string key;
            if (!string(&key)) return false;
            skip();
            if (_p >= _end || *_p != ':') return fail("expected :");
            ++_p;
            skip();
            Value e;
            if (!value(&e, depth + 1)) return false;
            v->set(key, std::move(e));
            skip();
            if (_p < _end && *_p == ',') {
                ++_p;
                continue;
            }
            if (_p < _end && *_p == '}') {
                ++_p;
                return true;
            }
            return fail("expected , or }");
        }
    }
    const char* _p;
    const char* _end;
    const char* _begin;
    std::string _err;
    const uint32_t* _idx = nullptr;
    size_t _nidx = 0, _k = 0;
};
}  // namespace

bool Parse(const char* data, size_t n, Value* out, std::string* error) {
    Reader r(data, n);
    return r.parse(out, error);
}

bool ParseWithIndex(const char* data, size_t n, const uint32_t* index, size_t nindex, Value* out,
                    std::string* error) {
    Reader r(data, n);
    r.set_index(index, nindex);
    return r.parse(out, error);
}

bool Parse(const std::string& text, Value* out, std::string* error) { return Parse(text.data(), text.size(), out, error); }

}  // namespace json
}  // namespace mrpc
