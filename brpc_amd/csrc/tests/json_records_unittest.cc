// json::FormatRecordObjects, the host twin of gpu::DevicePrintRecordObjects,
// against a naive printer that builds every record with std::string appends
// from json::Value, json::EscapeString and base64_encode: random jobs of every
// column count, kind and shape with empty rows and keys that need escaping,
// every position of a bad table, the worst case as a cap, and what the twin
// and the device entry refuse before any launch.
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "base/json_records.h"
#include "base/util.h"
#include "gpu/json_offload.h"
#include "json/json.h"
#include "tests/test.h"

using namespace mrpc;
namespace jr = mrpc::json_records;

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
const uint32_t kNumberKinds[] = {0, 1, 2, 3, 4, 5, 6, 8, 9};

// A column that owns its memory.
struct Col {
    std::string key;
    uint32_t kind = 0, text = 0;
    std::vector<uint64_t> image;  // aligned for every kind, never null
    uint64_t count = 0;
    bool ragged = false;
    std::vector<uint32_t> ends;  // rows entries and one spare
};

struct Batch {
    std::vector<Col> cols;
    uint64_t rows = 0;
    bool brackets = true;
    std::vector<jr::Column> view;
    jr::Job job() {
        view.assign(cols.size(), jr::Column());
        for (size_t c = 0; c < cols.size(); ++c) {
            view[c].key = cols[c].key.data();
            view[c].key_len = (uint32_t)cols[c].key.size();
            view[c].kind = cols[c].kind;
            view[c].text = cols[c].text;
            view[c].src = cols[c].image.data();
            view[c].count = cols[c].count;
            view[c].row_ends = cols[c].ragged ? cols[c].ends.data() : nullptr;
        }
        jr::Job j;
        j.columns = view.data();
        j.ncols = (uint32_t)view.size();
        j.rows = rows;
        j.brackets = brackets;
        return j;
    }
};

// Element i of a memory image, printed without the code under test.
std::string naive_elem(const Col& col, size_t i) {
    const char* p = reinterpret_cast<const char*>(col.image.data());
    switch (col.kind) {
    case 0:
    case 2: {
        int32_t v;
        memcpy(&v, p + 4 * i, 4);
        return json::Value((int64_t)v).ToString();
    }
    case 1: {
        uint32_t v;
        memcpy(&v, p + 4 * i, 4);
        return json::Value((uint64_t)v).ToString();
    }
    case 3:
    case 5: {
        int64_t v;
        memcpy(&v, p + 8 * i, 8);
        return json::Value(v).ToString();
    }
    case 4: {
        uint64_t v;
        memcpy(&v, p + 8 * i, 8);
        return json::Value(v).ToString();
    }
    case 6: return json::Value(p[i] != 0).ToString();
    case 8: {
        float v;
        memcpy(&v, p + 4 * i, 4);
        return json::Value((double)v).ToString();
    }
    default: {
        double v;
        memcpy(&v, p + 8 * i, 8);
        return json::Value(v).ToString();
    }
    }
}

std::string naive(const Batch& b) {
    if (b.rows == 0) return b.brackets ? "[]" : "";
    std::string s = b.brackets ? "[" : "";
    for (uint64_t r = 0; r < b.rows; ++r) {
        if (r) s += ",";
        s += "{";
        for (size_t c = 0; c < b.cols.size(); ++c) {
            const Col& col = b.cols[c];
            if (c) s += ",";
            json::EscapeString(col.key, &s);
            s += ":";
            if (!col.ragged) {
                s += naive_elem(col, r);
                continue;
            }
            const uint32_t from = r ? col.ends[r - 1] : 0, to = col.ends[r];
            const char* bytes = reinterpret_cast<const char*>(col.image.data());
            if (col.text == jr::kString) {
                json::EscapeString(std::string(bytes + from, to - from), &s);
            } else if (col.text == jr::kBase64) {
                s += "\"" + base64_encode(bytes + from, to - from) + "\"";
            } else {
                s += "[";
                for (uint32_t i = from; i < to; ++i) s += (i > from ? "," : "") + naive_elem(col, i);
                s += "]";
            }
        }
        s += "}";
    }
    return b.brackets ? s + "]" : s;
}

void fill(std::mt19937_64& rng, Col* col) {
    const size_t eb = jr::ElemBytes(col->kind);
    col->image.assign(col->count * eb / 8 + 1, 0);
    char* p = reinterpret_cast<char*>(col->image.data());
    for (size_t i = 0; i < col->count; ++i) {
        const uint64_t bits = rng() >> (rng() % 64);  // every width
        uint64_t v = (rng() & 1) ? bits : 0 - bits;
        if (col->kind == 8 && rng() % 16 == 0) v = 0x7F800000u | (uint32_t)(rng() % 3 == 0 ? 1 : 0) | (uint32_t)(rng() & 1) << 31;
        if (col->kind == 9 && rng() % 16 == 0) v = 0x7FF0000000000000ull | (rng() % 3 == 0 ? 1 : 0) | (rng() & 1) << 63;
        switch (eb) {
        case 1:
            if (col->kind == 6) p[i] = (char)((rng() & 1) ? (v | 1) : 0);
            else p[i] = (char)(rng() % 4 == 0 ? "\"\\\n\x01\x1f/\x7f\x80\xff"[rng() % 9] : (char)(rng() % 256));
            break;
        case 4: memcpy(p + 4 * i, &v, 4); break;
        default: memcpy(p + 8 * i, &v, 8); break;
        }
    }
}

std::string random_key(std::mt19937_64& rng, size_t c) {
    std::string k(1, (char)('a' + c));  // distinct whatever follows
    const size_t n = rng() % 6;
    for (size_t i = 0; i < n; ++i) k.push_back(rng() % 3 == 0 ? "\"\\\t\x02\xc3\xa9 "[rng() % 7] : (char)('A' + rng() % 26));
    return k;
}

// 1..8 columns of any kind and shape over 0..40 rows, rows of 0..5 elements.
Batch random_batch(std::mt19937_64& rng) {
    Batch b;
    b.rows = rng() % 41;
    b.brackets = rng() & 1;
    const size_t ncols = 1 + rng() % 8;
    for (size_t c = 0; c < ncols; ++c) {
        Col col;
        col.key = random_key(rng, c);
        const unsigned pick = (unsigned)(rng() % 11);
        if (pick < 9) {
            col.kind = kNumberKinds[pick];
            col.ragged = rng() % 3 != 0;
        } else {
            col.kind = jr::kKindBytes;
            col.text = pick == 9 ? jr::kString : jr::kBase64;
            col.ragged = true;
        }
        if (col.ragged) {
            uint32_t at = 0;
            for (uint64_t r = 0; r < b.rows; ++r) {
                if (rng() % 3) at += (uint32_t)(rng() % 6);
                col.ends.push_back(at);
            }
            col.count = at;
        } else {
            col.count = b.rows;
        }
        col.ends.push_back(0);  // data() of an empty table is still a table
        fill(rng, &col);
        b.cols.push_back(col);
    }
    return b;
}

struct Got {
    int err;
    uint32_t first_bad, bad_column;
    std::string text;
};

Got format(Batch& b) {
    Got g;
    g.text = "kept";
    g.first_bad = g.bad_column = 77;
    g.err = json::FormatRecordObjects(b.job(), &g.text, &g.first_bad, &g.bad_column);
    EXPECT_TRUE(g.text.compare(0, 4, "kept") == 0);  // appended, never assigned
    if (g.err != 0) EXPECT_EQ(g.text, std::string("kept"));
    g.text.erase(0, 4);
    return g;
}

uint64_t worst(Batch& b) {
    const jr::Job j = b.job();
    std::vector<std::string> prefixes;
    EXPECT_TRUE(json::RecordObjectPrefixes(j, &prefixes));
    uint64_t bytes = 0;
    for (const std::string& p : prefixes) bytes += p.size();
    return jr::WorstCaseBytes(j, bytes);
}

// The lowest offender of the tables as they are, by the rule spelled out
// (not base/json_records.h's), walked column by column (not the twin's order).
bool naive_bad(const Batch& b, uint32_t* row, uint32_t* column) {
    uint64_t best = ~0ull;
    for (size_t c = 0; c < b.cols.size(); ++c) {
        const Col& col = b.cols[c];
        if (!col.ragged) continue;
        for (uint64_t r = 0; r < b.rows; ++r) {
            const uint32_t prev = r ? col.ends[r - 1] : 0, end = col.ends[r];
            if (end < prev || end > col.count || (r + 1 == b.rows && end != col.count)) {
                if ((r << 4 | c) < best) best = r << 4 | c;
                break;
            }
        }
    }
    if (best == ~0ull) return false;
    *row = (uint32_t)(best >> 4);
    *column = (uint32_t)(best & 15);
    return true;
}

Batch one_column(uint32_t kind, uint32_t text, std::vector<uint32_t> ends, uint64_t count) {
    Batch b;
    Col col;
    col.key = "k";
    col.kind = kind;
    col.text = text;
    col.ragged = true;
    col.count = count;
    b.rows = ends.size();
    col.ends = ends;
    col.ends.push_back(0);
    col.image.assign(count + 1, 0);
    b.cols.push_back(col);
    return b;
}

}  // namespace

TEST(JsonRecords, random_jobs_equal_the_naive_printer) {
    std::mt19937_64 rng(20250722);
    for (int round = 0; round < 20000; ++round) {
        Batch b = random_batch(rng);
        const Got g = format(b);
        EXPECT_EQ(g.err, 0);
        EXPECT_EQ(g.first_bad, kNone);
        EXPECT_EQ(g.bad_column, kNone);
        EXPECT_EQ(g.text, naive(b));
        EXPECT_LE((uint64_t)g.text.size(), worst(b));
        if (g.err != 0 || g.text != naive(b)) break;  // one report is enough
    }
}

TEST(JsonRecords, every_bad_table_position) {
    std::mt19937_64 rng(7);
    int seen = 0;
    for (int round = 0; round < 4000; ++round) {
        Batch b = random_batch(rng);
        std::vector<size_t> ragged;
        for (size_t c = 0; c < b.cols.size(); ++c) {
            if (b.cols[c].ragged) ragged.push_back(c);
        }
        if (b.rows == 0 || ragged.empty()) continue;
        // one or two columns hurt at a row each: the first, one inside, the last
        for (int hurt = 0; hurt < 1 + (int)(rng() % 2); ++hurt) {
            Col& col = b.cols[ragged[rng() % ragged.size()]];
            const uint64_t r = round % 3 == 0 ? 0 : round % 3 == 1 ? b.rows - 1 : rng() % b.rows;
            switch (rng() % 3) {
            case 0: col.ends[r] = (uint32_t)col.count + 1 + (uint32_t)(rng() % 3); break;  // above count
            case 1: col.ends[r] = (r ? col.ends[r - 1] : 1) - 1; break;  // below its predecessor (or 2^32 - 1)
            default: col.ends[b.rows - 1] += 1; break;                    // the last is not count
            }
        }
        uint32_t row = 0, column = 0;
        const bool bad = naive_bad(b, &row, &column);
        const Got g = format(b);
        EXPECT_EQ(g.err, bad ? 1 : 0);
        if (bad) {
            ++seen;
            EXPECT_EQ(g.first_bad, row);
            EXPECT_EQ(g.bad_column, column);
        }
    }
    EXPECT_GT(seen, 1000);  // the generator does hurt tables
}

TEST(JsonRecords, fixed_texts) {
    Batch b;
    b.rows = 2;
    Col label;
    label.key = "label";
    label.kind = 0;
    label.count = 2;
    const int32_t labels[] = {3, -2147483647 - 1};
    label.image.assign(2, 0);
    memcpy(label.image.data(), labels, sizeof(labels));
    label.ends.push_back(0);
    Col ids;
    ids.key = "ids";
    ids.kind = 4;
    ids.ragged = true;
    ids.count = 2;
    ids.image = {1, std::numeric_limits<uint64_t>::max(), 0};
    ids.ends = {2, 2, 0};
    Col scores;
    scores.key = "sc\"ores";
    scores.kind = 9;
    scores.ragged = true;
    scores.count = 3;
    const double ds[] = {0.5, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::quiet_NaN()};
    scores.image.assign(4, 0);
    memcpy(scores.image.data(), ds, sizeof(ds));
    scores.ends = {1, 3, 0};
    Col text;
    text.key = "text";
    text.kind = 7;
    text.text = jr::kString;
    text.ragged = true;
    text.count = 4;
    text.image.assign(2, 0);
    memcpy(text.image.data(), "a\"\n\x01", 4);
    text.ends = {0, 4, 0};
    Col blob = text;
    blob.key = "blob";
    blob.text = jr::kBase64;
    blob.ends = {1, 4, 0};
    b.cols = {label, ids, scores, text, blob};
    Got g = format(b);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text, std::string("[{\"label\":3,\"ids\":[1,18446744073709551615],\"sc\\\"ores\":[0.5],\"text\":\"\","
                                  "\"blob\":\"YQ==\"},{\"label\":-2147483648,\"ids\":[],\"sc\\\"ores\":[\"Infinity\","
                                  "\"NaN\"],\"text\":\"a\\\"\\n\\u0001\",\"blob\":\"Igo" "B\"}]"));
    b.brackets = false;
    const std::string inner = g.text.substr(1, g.text.size() - 2);
    g = format(b);
    EXPECT_EQ(g.text, inner);
    // no row: "[]" or nothing, whatever the columns hold
    Batch none = one_column(3, 0, {}, 0);
    g = format(none);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text, std::string("[]"));
    EXPECT_EQ(worst(none), 2u);
    none.brackets = false;
    g = format(none);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text, std::string());
    EXPECT_EQ(worst(none), 0u);
    // base64 cell sizes need no element pass
    for (uint32_t len = 0; len < 20; ++len) {
        EXPECT_EQ((size_t)jr::Base64CellBytes(len), 2 + base64_encode(std::string(len, 'x').data(), len).size());
    }
}

TEST(JsonRecords, a_255_byte_escaped_key_is_the_longest) {
    Batch b = one_column(0, 0, {0}, 0);
    b.cols[0].key = std::string(255, 'k');
    EXPECT_EQ(format(b).err, 0);
    b.cols[0].key = std::string(125, 'k') + std::string(65, '"');  // 125 + 130
    const Got g = format(b);
    EXPECT_EQ(g.err, 0);
    EXPECT_EQ(g.text.size(), (size_t)(1 + 2 + 255 + 2 + 2 + 1 + 1));
    b.cols[0].key = std::string(256, 'k');
    EXPECT_EQ(format(b).err, 2);
    b.cols[0].key = std::string(250, 'k') + "\x01";  // 250 + 6
    EXPECT_EQ(format(b).err, 2);
    b.cols[0].key = "";
    EXPECT_EQ(format(b).err, 0);
}

TEST(JsonRecords, what_is_refused) {
    auto base = [] {
        Batch b = one_column(3, 0, {1, 2}, 2);
        Col scalar;
        scalar.key = "s";
        scalar.kind = 0;
        scalar.count = 2;
        scalar.image.assign(2, 0);
        scalar.ends.push_back(0);
        b.cols.push_back(scalar);
        return b;
    };
    Batch b = base();
    EXPECT_EQ(format(b).err, 0);
    b.cols[0].kind = 7;  // a text form is missing
    EXPECT_EQ(format(b).err, 2);
    b.cols[0].text = 3;  // a text form there is not
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols[0].kind = 10;  // a kind there is not
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols[0].text = jr::kString;  // a text form on a number kind
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols[1].kind = 7;  // bytes without row ends
    b.cols[1].text = jr::kBase64;
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols[1].count = 3;  // a scalar column of another length
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols[1].key = "k";  // two equal keys
    EXPECT_EQ(format(b).err, 2);
    b = base();
    b.cols.clear();  // no column
    EXPECT_EQ(format(b).err, 2);
    b = base();
    for (int c = 2; c < 9; ++c) {
        b.cols.push_back(b.cols[1]);
        b.cols.back().key = std::string(1, (char)('a' + c));
    }
    EXPECT_EQ(format(b).err, 2);  // nine columns
    b.cols.pop_back();
    EXPECT_EQ(format(b).err, 0);  // eight
    // pointers: a null source with elements, a misaligned source or table, a null key with a length
    b = base();
    jr::Job j = b.job();
    std::string out;
    b.view[0].src = nullptr;
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    j = b.job();
    b.view[0].src = reinterpret_cast<const char*>(b.cols[0].image.data()) + 4;  // an int64 at 4 (mod 8)
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    j = b.job();
    b.view[0].row_ends = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(b.cols[0].ends.data()) + 2);
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    j = b.job();
    b.view[1].key = nullptr;
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    j = b.job();
    j.columns = nullptr;
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    EXPECT_EQ(out, std::string());
    // a worst case above 2^32 - 1: nothing is read before the refusal
    b = base();
    j = b.job();
    b.view[0].count = 1ull << 28;  // 2^28 * 21
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
    b.view[0].count = 1ull << 33;
    EXPECT_EQ(json::FormatRecordObjects(j, &out), 2);
}

// The device entry refuses the same jobs, and a few more that only it can
// see, before it touches a device: these run without one.
TEST(JsonRecords, the_device_entry_refuses_before_any_launch) {
    alignas(16) static char mem[256];
    const char key[] = "k", key2[] = "q";
    auto job_of = [&](gpu::DeviceRecordPrintColumn* cols, uint32_t ncols) {
        gpu::DeviceRecordPrintJob j;
        j.columns = cols;
        j.ncols = ncols;
        j.rows = 2;
        j.brackets = true;
        j.dst = mem + 128;
        j.cap = 64;
        return j;
    };
    auto good = [&] {
        gpu::DeviceRecordPrintColumn c;
        c.key = key;
        c.key_len = 1;
        c.kind = 3;
        c.src = mem;
        c.count = 2;
        c.row_ends = reinterpret_cast<const uint32_t*>(mem + 64);
        return c;
    };
    auto refused = [&](gpu::DeviceRecordPrintJob j) {
        EXPECT_EQ(gpu::DevicePrintRecordObjects(&j, 1, 0), 0);
        EXPECT_EQ(j.len, 0u);
        return j.err == 2;
    };
    gpu::DeviceRecordPrintColumn c[9];
    c[0] = good();
    EXPECT_GT(gpu::RecordObjectsWorstCaseBytes(job_of(c, 1)), 0u);
    gpu::DeviceRecordPrintJob j = job_of(c, 1);
    j.dst = nullptr;  // a null dst with a cap
    EXPECT_TRUE(refused(j));
    j = job_of(c, 1);
    j.dst = mem + 8;  // dst over the source
    EXPECT_TRUE(refused(j));
    j = job_of(c, 1);
    j.dst = mem + 60;  // dst over the table
    EXPECT_TRUE(refused(j));
    EXPECT_TRUE(refused(job_of(c, 0)));
    EXPECT_TRUE(refused(job_of(nullptr, 1)));
    c[0].src = nullptr;
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].src = mem + 4;
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].row_ends = reinterpret_cast<const uint32_t*>(mem + 66);
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].kind = 11;
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].text = gpu::kJsonRecordBase64;  // a text form on a number kind
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].kind = 7;  // bytes without a text form
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0].text = gpu::kJsonRecordString;
    c[0].row_ends = nullptr;  // bytes without row ends
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].row_ends = nullptr;
    c[0].count = 3;  // a scalar column whose count is not rows
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[0].key = nullptr;  // a null key with a length
    EXPECT_TRUE(refused(job_of(c, 1)));
    const std::string long_key(256, 'k');
    c[0] = good();
    c[0].key = long_key.data();
    c[0].key_len = 256;
    EXPECT_TRUE(refused(job_of(c, 1)));
    c[0] = good();
    c[1] = good();  // two equal keys
    EXPECT_TRUE(refused(job_of(c, 2)));
    c[1].key = key2;
    c[0].count = 1ull << 28;  // a worst case above 2^32 - 1
    EXPECT_TRUE(refused(job_of(c, 2)));
    EXPECT_EQ(gpu::RecordObjectsWorstCaseBytes(job_of(c, 2)), ~0ull);
    for (int k = 0; k < 9; ++k) c[k] = good();
    EXPECT_TRUE(refused(job_of(c, 9)));
    EXPECT_EQ(gpu::RecordObjectsWorstCaseBytes(job_of(c, 9)), 0u);
    // no row and no brackets: nothing to do, and nothing refused
    c[0] = good();
    c[0].count = 0;
    j = job_of(c, 1);
    j.rows = 0;
    j.brackets = false;
    EXPECT_EQ(gpu::DevicePrintRecordObjects(&j, 1, 0), 0);
    EXPECT_EQ(j.err, 0);
    EXPECT_EQ(j.len, 0u);
    // "[]" does not fit
    j.brackets = true;
    j.cap = 1;
    EXPECT_EQ(gpu::DevicePrintRecordObjects(&j, 1, 0), 0);
    EXPECT_EQ(j.err, 3);
    EXPECT_EQ(j.len, 2u);
    EXPECT_EQ(gpu::JsonRecordsChunkElems() % 64, 0u);
    EXPECT_GT(gpu::JsonRecordsBlockRows(), 0u);
}
