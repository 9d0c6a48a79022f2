// Small JSON DOM: parse / serialize (rapidjson is not available; the
// reference's json2pb builds on rapidjson, src/json2pb). Used by json2pb,
// naming services and builtin pages.
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace mrpc {
namespace json_records {
struct Job;  // base/json_records.h
}
namespace json {

class Value {
public:
    // RAW: pre-rendered JSON text written verbatim (an array of numbers
    // printed by the device, json2pb's SetPb2JsonArrayOffload)
    enum Type { NUL, BOOL, INT, UINT, DOUBLE, STRING, ARRAY, OBJECT, RAW };
    Value() : _type(NUL) {}
    // copies never share the packed view (it is rebuilt on demand), so a
    // copy never reads _view non-atomically while a reader publishes it
    Value(const Value& o)
        : _type(o._type), _b(o._b), _i(o._i), _u(o._u), _d(o._d), _s(o._s), _arr(o._arr), _ints(o._ints),
          _nums(o._nums), _obj(o._obj) {}
    Value(Value&&) = default;
    Value& operator=(const Value& o) {
        if (this != &o) *this = Value(o);
        return *this;
    }
    Value& operator=(Value&&) = default;
    explicit Value(bool b) : _type(BOOL), _b(b) {}
    explicit Value(int64_t i) : _type(INT), _i(i) {}
    explicit Value(uint64_t u) : _type(UINT), _u(u) {}
    explicit Value(int i) : _type(INT), _i(i) {}
    explicit Value(double d) : _type(DOUBLE), _d(d) {}
    explicit Value(const std::string& s) : _type(STRING), _s(s) {}
    explicit Value(const char* s) : _type(STRING), _s(s) {}
    static Value Array() { Value v; v._type = ARRAY; return v; }
    static Value Object() { Value v; v._type = OBJECT; return v; }
    static Value Raw(std::string text) { Value v; v._type = RAW; v._s = std::move(text); return v; }

    Type type() const { return _type; }
    bool is_null() const { return _type == NUL; }
    bool is_bool() const { return _type == BOOL; }
    bool is_number() const { return _type == INT || _type == UINT || _type == DOUBLE; }
    bool is_int() const { return _type == INT || _type == UINT; }
    bool is_string() const { return _type == STRING; }
    bool is_array() const { return _type == ARRAY; }
    bool is_object() const { return _type == OBJECT; }

    bool as_bool() const { return _type == BOOL ? _b : (is_number() && as_double() != 0); }
    int64_t as_int() const;
    uint64_t as_uint() const;
    double as_double() const;
    const std::string& as_string() const { return _s; }
    std::string& mutable_string() { return _s; }
    bool uint_overflows_int() const { return _type == UINT && _u > (uint64_t)INT64_MAX; }

    // arrays. An array of integers parsed in bulk (the device parser of
    // SetIntArrayOffload) keeps them packed; packed_ints() lets json2pb take
    // them as they are. The const array() of a packed array builds a Value
    // view once (published atomically, so concurrent readers of one parsed
    // Value are safe; the packed form itself never changes); the mutating
    // accessors convert the array to Values in place.
    static Value PackedInts(std::vector<int64_t> v) {
        Value a;
        a._type = ARRAY;
        a._ints = std::move(v);
        return a;
    }
    const std::vector<int64_t>* packed_ints() const { return _ints.empty() ? nullptr : &_ints; }
    // An array of numbers of which at least one is not an int64 (floats, or
    // integers above INT64_MAX) stays packed too: 8 bytes of payload and a
    // class byte per element, so int64 and uint64 elements stay exact. The
    // classes are those of base/decimal_to_double.h: 0 the payload is the
    // int64 (an INT Value), 1 a uint64 above INT64_MAX (UINT), 2 the bits of
    // the double (DOUBLE). packed_ints() is nullptr for such an array; the
    // accessors behave as for packed ints. The packed form never changes, so
    // copies share it.
    struct NumberArray {
        std::vector<uint64_t> payload;
        std::vector<uint8_t> classes;
    };
    static Value PackedNumbers(NumberArray nums) {
        Value a;
        a._type = ARRAY;
        if (!nums.payload.empty()) a._nums = std::make_shared<const NumberArray>(std::move(nums));
        return a;
    }
    const NumberArray* packed_numbers() const { return _nums.get(); }
    // the Value of element i of a packed-number array
    static Value NumberElement(uint64_t payload, uint8_t cls);
    const std::vector<Value>& array() const {
        if (_ints.empty() && !_nums) return _arr;
        return packed_view();
    }
    std::vector<Value>& mutable_array() {
        materialize();
        _type = ARRAY;
        return _arr;
    }
    Value& push_back(Value v) {
        materialize();
        _type = ARRAY;
        _arr.push_back(std::move(v));
        return _arr.back();
    }
    size_t size() const {
        if (_type != ARRAY) return _obj.size();
        if (_nums) return _nums->payload.size();
        return _ints.empty() ? _arr.size() : _ints.size();
    }

    // objects (insertion ordered)
    const std::vector<std::pair<std::string, Value>>& members() const { return _obj; }
    const Value* find(const std::string& key) const;
    Value* find(const std::string& key);
    Value& set(const std::string& key, Value v);
    Value& operator[](const std::string& key);

    std::string ToString(bool pretty = false) const;

private:
    void write(std::string* out, bool pretty, int indent) const;
    void materialize() {
        if (_nums) {
            _arr.reserve(_nums->payload.size());
            for (size_t i = 0; i < _nums->payload.size(); ++i)
                _arr.push_back(NumberElement(_nums->payload[i], _nums->classes[i]));
            _nums.reset();
            _view.reset();
            return;
        }
        if (_ints.empty()) return;
        _arr.reserve(_ints.size());
        for (int64_t x : _ints) _arr.emplace_back(x);
        _ints.clear();
        _view.reset();
    }
    const std::vector<Value>& packed_view() const;
    Type _type;
    bool _b = false;
    int64_t _i = 0;
    uint64_t _u = 0;
    double _d = 0;
    std::string _s;
    std::vector<Value> _arr;
    std::vector<int64_t> _ints;
    std::shared_ptr<const NumberArray> _nums;
    // Values of a packed array for const readers (std::atomic_load/store)
    mutable std::shared_ptr<const std::vector<Value>> _view;
    std::vector<std::pair<std::string, Value>> _obj;
};

// Bulk parse of a large integer array (gpu/json_offload.cc): the
// reader, when it has a structural index, hands an array whose index shows
// only ',' between its brackets (no strings, objects or nested arrays) and
// at least min_elems elements to `fn` with the text base and the n + 1
// separator offsets; fn returns false unless every element is an int64,
// and the reader then parses the array itself.
typedef bool (*IntArrayOffload)(const char* base, const uint32_t* seps, size_t nseps, std::vector<int64_t>* out);
void SetIntArrayOffload(IntArrayOffload fn, size_t min_elems);

// The same for arrays of numbers that are not all int64 (floats): tried on
// the same separator run when the integer offload declined or its threshold
// is not met, if the run has at least this offload's min_elems elements. fn
// fills payload[n] and classes[n] (n = nseps - 1; the classes of
// Value::NumberArray) and returns false unless every element is a number of
// the RFC 8259 grammar; the reader then parses the array itself.
typedef bool (*NumberArrayOffload)(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload,
                                   uint8_t* classes);
void SetNumberArrayOffload(NumberArrayOffload fn, size_t min_elems);

// The host twin of the device number parser (gpu/json_kernels.hip
// json_number_array_kernel): element i is the text between separators
// seps[i] and seps[i+1] (exclusive), trimmed of JSON whitespace and
// converted with base/decimal_to_double.h. An element that needs exact
// arithmetic (more than 19 significant digits whose truncation does not
// decide the rounding, or a text too long for a device lane) is converted
// as Reader::number always did (std::from_chars / strtod) when `exact` is
// set, and left as class 3 with payload 0 otherwise. Returns false, with
// *bad_index (if given) the first offending element, when an element is not
// a number of the RFC 8259 grammar.
bool ParseNumberArray(const char* base, const uint32_t* seps, size_t nseps, uint64_t* payload, uint8_t* classes,
                      bool exact = true, size_t* bad_index = nullptr);
// One trimmed number of the RFC 8259 grammar, of any length, by the exact
// route alone; false when the text is not in the grammar.
bool ParseNumberExact(const char* b, const char* e, uint64_t* payload, uint8_t* cls);
// Separator offsets of a flat number array for ParseNumberArray and the
// device parser: of "[v,v,...]" (spaces around the brackets allowed) the
// '[', every ',' and the ']'; of bare "v,v,...,v" every ',' between
// 0xFFFFFFFF (a separator before the first byte) and n. Text below 4 GiB.
void NumberArraySeparators(const char* text, size_t n, std::vector<uint32_t>* seps);
// The host twin of gpu::DeviceParseNumberText (gpu/json_offload.h): number
// text with no separator table, bare "v,v,...,v" (depth 0), "[v,v,...,v]"
// (depth 1) or "[[v,..],[v,..],..]" (depth 2, rows of any lengths), JSON
// whitespace wherever JSON allows it. One scanner, base/number_text.h, gives
// the device and this function the same verdict on every text. mode: 0 eight
// bytes of payload per element in `out` and a class byte in `classes` (as
// ParseNumberArray), 1 doubles, 2 floats (the narrowed double).
struct NumberText {
    int err = 0;  // 0 parsed; 1 malformed (first_bad set, out / classes / row_ends empty); 2 bad mode or n >= 2^32 - 1
    uint32_t depth = 0;
    uint32_t count = 0;  // elements; with err 1 the pieces (commas + 1)
    uint32_t rows = 0;   // depth 2 only
    uint32_t first_bad = 0xFFFFFFFFu;  // lowest index of a piece (the text between commas) that does not fit
    std::string out, classes;
    std::vector<uint32_t> row_ends;  // rows entries: the elements in rows 0..r
    // exact == false only: the elements a device lane hands back (class 3 /
    // a zero in out), as pairs {index, offset of the byte after the comma
    // before the element}
    std::vector<uint32_t> redo;
};
// Empty text, whitespace and "[ ]" are count 0. nested_ok == false refuses
// depth 2 (first_bad 0), as the device does without a row_ends buffer.
// Returns err == 0.
bool ParseNumberText(const char* text, size_t n, uint32_t mode, NumberText* out, bool exact = true,
                     bool nested_ok = true);
// The host twin of gpu::DevicePrintNumbers (gpu/json_offload.h), the inverse
// of ParseNumberText: `count` elements of one kind (gpu::PbRunKind 0..6: the
// integers as the decimal number of their type, a bool byte as true / false;
// 8 / 9: a float / double as FormatFloatArray prints it) appended to *out as
//   row_ends null, brackets false   v,v,...,v
//   row_ends null, brackets true    [v,v,...,v]          ("[]" for count 0)
//   row_ends given (rows entries)   [[v,..],[v,..],..]   brackets ignored
// with no whitespace; the rules are base/number_print.h for both. Returns the
// device's codes: 0 printed; 1 a malformed table of row ends, *first_bad (if
// given) the lowest row r with row_ends[r] <= row_ends[r - 1], row_ends[r] >
// count, or r the last row and row_ends[r] != count; 2 refused (a kind there
// is not, null values with count > 0, values not naturally aligned, rows
// without row_ends or row_ends without rows, a worst case above 2^32 - 1).
// Nothing is appended on a code other than 0.
int FormatNumberRows(const void* values, uint64_t count, uint32_t kind, const uint32_t* row_ends, uint64_t rows,
                     bool brackets, std::string* out, uint32_t* first_bad = nullptr);
// Test and benchmark hook: false makes the reader parse number arrays element
// by element with std::from_chars, as it did before packed numbers (the DOM
// is the same either way; only storage and speed differ). Default true.
void SetPackedNumberArrays(bool on);

// Returns false and sets *error on malformed input.
bool Parse(const std::string& text, Value* out, std::string* error = nullptr);
bool Parse(const char* data, size_t n, Value* out, std::string* error = nullptr);
// Same result as Parse, with a structural index of `data` (ascending
// offsets of every unescaped quote and every {}[]:, outside strings, as
// gpu::LaunchJsonIndex produces): strings are cut at indexed quotes instead
// of scanned. A wrong index only costs speed, never correctness.
bool ParseWithIndex(const char* data, size_t n, const uint32_t* index, size_t nindex, Value* out,
                    std::string* error = nullptr);
void EscapeString(const std::string& s, std::string* out);
// The host twins of the device string entries (gpu/json_string_offload.h);
// the rules are base/json_string.h for both.
// What EscapeString writes between its quotes, appended to *out.
void EscapeStringBody(const char* s, size_t n, std::string* out);
// "r0","r1",...,"r(rows-1)" appended to *out: row r is bytes[row_ends[r - 1],
// row_ends[r]) (row_ends[-1] = 0), the pair pb::SplitRows gives a repeated
// string. False, with nothing appended, when row_ends decreases.
bool EscapeStringRows(const char* bytes, const uint32_t* row_ends, size_t rows, std::string* out);
// The body between the quotes -> its bytes, appended to *out. 0: done, and the
// bytes are what the reader makes of '"' + body + '"'. 1: not decided here
// (the reader is looser there, or refuses): *first_bad (if given) is the offset
// of the offending backslash or quote and *out is as it was.
int UnescapeStringBody(const char* body, size_t n, std::string* out, uint64_t* first_bad = nullptr);
// The host twin of gpu::DeviceUnescapeJsonStringRows: the inverse of
// EscapeStringRows. `text` is "r0","r1",... (depth 0) or ["r0","r1",...]
// (depth 1), JSON whitespace wherever JSON allows it; the grammar and the
// offsets of refusal are base/json_string_rows.h, one sequential walk. 0: done,
// bytes holds the decoded strings one after the other, row_ends[r] the bytes
// in strings 0..r (empty text, whitespace and "[ ]": no row). 1: not decided
// here (json::Reader decides): first_bad is set, everything else empty and 0.
struct StringRows {
    std::string bytes;
    std::vector<uint32_t> row_ends;
    uint32_t depth = 0;
    uint64_t first_bad = 0;
};
int UnescapeStringRows(const char* text, size_t n, StringRows* out);
// The host twins of gpu::DeviceBase64EncodeRows / DeviceBase64DecodeRows
// (gpu/base64_offload.h); the rules are base/base64_rows.h for both.
// "b0","b1",... appended to *out, wrapped in '[' ']' with brackets: row r, cut
// from bytes as above, as its '='-padded base64. False, with nothing appended,
// when row_ends decreases.
bool EncodeBase64Rows(const char* bytes, const uint32_t* row_ends, size_t rows, bool brackets, std::string* out);
// The inverse: the text of an array of base64 strings, depth 0 or 1 as above,
// bodies canonical base64 only. 0: done, filled like UnescapeStringRows. 1:
// not decided here (json::Reader and base64_decode are laxer): first_bad is
// set, everything else empty and 0. One sequential walk.
int DecodeBase64Rows(const char* text, size_t n, StringRows* out);
// The host twin of gpu::DevicePrintRecordObjects (gpu/json_offload.h): the
// job's columns as [{"k0":cell,"k1":cell,...},...] appended to *out, every key
// in every record (this is not pb2json's omission rule), no whitespace; without
// brackets the records are only joined by ','. No row: "[]" or nothing. The
// rules are base/json_records.h for both; one sequential walk. Returns the
// device's codes: 0 printed; 1 a bad table of row ends, *first_bad the lowest
// offending row over all columns and *bad_column the lowest column that
// offends there; 2 refused (a column count, kind, text form or shape there is
// not, a null or misaligned source, a key whose escaped form is above 255
// bytes, two equal keys, a worst case above 2^32 - 1). Nothing is appended on
// a code other than 0.
int FormatRecordObjects(const json_records::Job& job, std::string* out, uint32_t* first_bad = nullptr,
                        uint32_t* bad_column = nullptr);
// The fixed per-column prefixes of such a job ({"k": for column 0, ,"k":
// behind it), the keys escaped with EscapeStringBody. False when a key is
// missing, its escaped form is above 255 bytes, or two keys are equal.
bool RecordObjectPrefixes(const json_records::Job& job, std::vector<std::string>* prefixes);
// The first offset at which no well-formed UTF-8 sequence starts on the walk
// from 0 (what Python reports as UnicodeDecodeError.start), n when the text
// is well-formed.
size_t Utf8FirstBad(const char* s, size_t n);
// Shortest round-tripping form of d in the reference rapidjson layout ("2.0", "0.1", "1e22").
void AppendShortestDouble(double d, std::string* out);

}  // namespace json
}  // namespace mrpc
