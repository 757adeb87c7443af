// Stand-alone sanitizer check of the host form of the JSON Lines passes (csrc/json_fields_host.h and
// csrc/json_text_host.h, the code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/json_fields_host_check.cpp -o build/json_fields_host_check \
//       && build/json_fields_host_check
//
// Every data buffer is a heap allocation of exactly data_bytes, so a read one byte outside it is an
// AddressSanitizer error.  The cases are the CPU edge cases of tests/test_json_fields.py and
// tests/test_json_text.py (row states, keys, numbers, literals, nesting, backslash runs, every
// escape, bad escapes at the start, the middle and the end of a value, windows that disagree with
// the data) and rows and values whose spans lie outside the buffer; jf_escaped16 is compared with
// a byte walk for every mask and carry.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "json_fields_host.h"
#include "json_text_host.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

struct Heap {
  std::unique_ptr<uint8_t[]> p;                     // exactly n bytes
  uint64_t n = 0;
  explicit Heap(const std::string& s) : p(new uint8_t[s.size()]), n(s.size()) { std::memcpy(p.get(), s.data(), n); }
};

struct Cell {
  uint8_t st;
  int64_t i;       // the value, or the span's start relative to the row
  int32_t len;
  double f;
};

// One row, one column: key `key` as `type`.
static Cell one(const std::string& row, const std::string& key, uint32_t type, size_t lead = 3, uint32_t term = '\n') {
  const std::string all = std::string(lead, '{') + row;
  Heap data(all), names(key);
  int64_t off = (int64_t)lead, len = (int64_t)row.size();
  uint64_t value = 0x1111111111111111ull;
  int32_t length = -7;
  uint8_t status = 9;
  JsonFieldsArgs a{};
  a.data = data.p.get();
  a.data_bytes = data.n;
  a.off = &off;
  a.len = &len;
  a.len_is_64 = 1;
  a.nrows = 1;
  a.names = names.p.get();
  a.names_bytes = (uint32_t)names.n;
  a.terminator = term;
  a.ncols = 1;
  a.cols[0] = JsonFieldsCol{0, (uint32_t)key.size(), type, 0, &value, &length, &status};
  CHECK(json_fields_scalars_ok(a));
  json_fields_host(a);
  Cell c{};
  c.st = status;
  c.len = length;
  if (type == kFpInt32) c.i = (int32_t)(uint32_t)value;
  else if (type == kJfBool) c.i = (uint8_t)value;
  else if (type == kFpSpan || type == kJfString) c.i = (int64_t)value - (status == 0 ? (int64_t)lead : 0);
  else c.i = (int64_t)value;
  if (type == kFpFloat64) std::memcpy(&c.f, &value, 8);
  if (type == kFpFloat32) {
    float f;
    std::memcpy(&f, &value, 4);
    c.f = f;
  }
  return c;
}

static uint8_t st(const std::string& row, const std::string& key = "a", uint32_t type = kFpInt64) {
  return one(row, key, type).st;
}

static std::string span(const std::string& row, const std::string& key, uint32_t type = kFpSpan) {
  const Cell c = one(row, key, type);
  return c.st == 0 ? row.substr((size_t)c.i, (size_t)c.len) : "<" + std::to_string(c.st) + ">";
}

static void check_locate() {
  // row states
  CHECK(st("") == 1 && st("  \t\r ") == 1 && st("\n") == 1);
  CHECK(st("[1]") == 2 && st("x{\"a\":1}") == 2 && st("\"a\"") == 2);
  CHECK(st("{\"a\":1]") == 2 && st("{\"a\":1") == 2 && st("{\"a\":[1}") == 2 && st("{\"a\":{}") == 2);
  CHECK(st("{\"a\":1} x") == 2 && st("{\"a\":1}{") == 2 && st("{\"a\":1}\"") == 2);
  CHECK(st("{\"a\":\"1}") == 2 && st("{\"a\":1,\"b\":\"}") == 2);
  CHECK(st(" \t{\"a\":1} \r\n") == 0 && st("{\"a\":1}\r\n") == 0 && st("{\"a\":1}\n") == 0);
  CHECK(one("{\"a\":1}\r", "a", kFpInt64).st == 0 && one("{\"a\":1};", "a", kFpInt64, 3, ';').st == 0);
  CHECK(st("{}") == 1 && st("{ }") == 1 && st("{\"b\":1}") == 1);
  // a row outside the buffer is not read
  {
    Heap data("{\"a\":1}"), names("a");
    int64_t off[4] = {-1, 0, 1, 0}, len[4] = {3, 8, 7, -1};
    int64_t v[4];
    uint8_t s[4];
    JsonFieldsArgs a{};
    a.data = data.p.get();
    a.data_bytes = data.n;
    a.off = off;
    a.len = len;
    a.len_is_64 = 1;
    a.nrows = 4;
    a.names = names.p.get();
    a.names_bytes = 1;
    a.terminator = '\n';
    a.ncols = 1;
    a.cols[0] = JsonFieldsCol{0, 1, kFpInt64, 0, v, nullptr, s};
    json_fields_host(a);
    CHECK(s[0] == 2 && s[1] == 2 && s[2] == 2 && s[3] == 2);
  }
  // keys
  CHECK(one("{\"a\":1,\"a\":2}", "a", kFpInt64).i == 2 && one("{\"a\":1,\"a\":null}", "a", kFpInt64).st == 1);
  CHECK(one("{\"ab\":1,\"a\":2}", "a", kFpInt64).i == 2 && one("{\"ab\":1,\"a\":2}", "ab", kFpInt64).i == 1);
  CHECK(st("{\"b\":{\"a\":1}}") == 1 && st("{\"b\":[{\"a\":1}],\"c\":\"\\\"a\\\":1\"}") == 1);
  CHECK(st("{\"\\u0061\":1}") == 1 && st("{a:1}") == 1 && st("{\"a\" x:1}") == 1);
  CHECK(one("{ \"a\" \t:\r 5 \n, \"b\":6}", "a", kFpInt64).i == 5);
  CHECK(span("{\"a\":1:2}", "a") == "1:2" && span("{\"k\":{\"x\":[1,2,{\"y\":\"}\"}]} ,\"z\":0}", "k") == "{\"x\":[1,2,{\"y\":\"}\"}]}");
  for (size_t nl : {1u, 15u, 16u, 17u, 255u}) {
    const std::string k(nl, 'k');
    CHECK(one("{\"" + k + "\":7}", k, kFpInt64).i == 7);
    CHECK(st("{\"" + k + "x\":7}", k) == 1);
  }
  // strings that hold structure, backslash runs
  CHECK(span("{\"s\":\"{}[],:\",\"a\":1}", "s") == "\"{}[],:\"" && one("{\"s\":\"{}[],:\",\"a\":1}", "a", kFpInt64).i == 1);
  for (int k = 1; k <= 35; ++k) {
    const std::string row = "{\"s\":\"x" + std::string((size_t)k, '\\') + "\",\"a\":1}\"}";
    // an odd run escapes the quote: the string runs on to the next quote
    if (k % 2) CHECK(span(row, "s") == "\"x" + std::string((size_t)k, '\\') + "\",\"a\":1}\"");
    else CHECK(st(row) == 2);                       // the object closes and a quote follows
  }
  CHECK(st("{\"s\":\"" + std::string(300, '\\') + "\"}") == 1 && st("{\"s\":\"" + std::string(301, '\\') + "\"}") == 2);
  // nesting
  for (int d : {1, 2, 63, 64, 65, 300}) {
    const std::string v = std::string((size_t)d, '[') + std::string((size_t)d, ']');
    CHECK(span("{\"n\":" + v + ",\"a\":3}", "n") == v && one("{\"n\":" + v + ",\"a\":3}", "a", kFpInt64).i == 3);
  }
  // numbers
  for (const char* s : {"0", "-0", "7", "-12", "9223372036854775807", "-9223372036854775808"})
    CHECK(st(std::string("{\"a\":") + s + "}") == 0);
  for (const char* s : {"+1", "01", "1.0", "1e3", "-", "--1", "1 2", "0x1", "9223372036854775808", "-9223372036854775809",
                        "12345678901234567890", "\"1\"", "true", ""})
    CHECK(st(std::string("{\"a\":") + s + "}") == 2);
  CHECK(one("{\"a\":2147483647}", "a", kFpInt32).i == 2147483647 && one("{\"a\":2147483648}", "a", kFpInt32).st == 2);
  CHECK(one("{\"a\":-2147483648}", "a", kFpInt32).i == -2147483648ll && one("{\"a\":-2147483649}", "a", kFpInt32).st == 2);
  for (const char* s : {"0", "-0", "1.5", "-2.25e2", "1E+2", "1e-2", "0.000", "12.50"})
    CHECK(st(std::string("{\"a\":") + s + "}", "a", kFpFloat64) == 0);
  for (const char* s : {"NaN", "Infinity", "-Infinity", "+1", "01", "1.", ".5", "1e", "1e+", "1.e2", "-.5", "0x1p3", "1f", "inf"})
    CHECK(st(std::string("{\"a\":") + s + "}", "a", kFpFloat64) == 2);
  CHECK(one("{\"a\":-2.25e2}", "a", kFpFloat64).f == -225.0 && one("{\"a\":0.5}", "a", kFpFloat32).f == 0.5);
  CHECK(st("{\"a\":1e400}", "a", kFpFloat64) == 3 && st("{\"a\":0.1234567890123456789012}", "a", kFpFloat64) == 3);
  // literals
  CHECK(one("{\"a\":true}", "a", kJfBool).i == 1 && one("{\"a\": false }", "a", kJfBool).st == 0);
  CHECK(one("{\"a\":false}", "a", kJfBool).i == 0 && st("{\"a\":True}", "a", kJfBool) == 2 && st("{\"a\":1}", "a", kJfBool) == 2);
  for (uint32_t t = 0; t <= kJfString; ++t) CHECK(st("{\"a\":null}", "a", t) == 1 && st("{\"a\": }", "a", t) == 2);
  CHECK(st("{\"a\":Null}", "a", kFpSpan) == 0);
  // strings
  CHECK(span("{\"a\":\"\"}", "a", kJfString) == "" && span("{\"a\": \"x\\\"y\" }", "a", kJfString) == "x\\\"y");
  CHECK(st("{\"a\":\"}", "a", kJfString) == 2 && st("{\"a\":5}", "a", kJfString) == 2 && st("{\"a\":\"x\"y}", "a", kJfString) == 2);
  // scalars
  {
    JsonFieldsArgs a{};
    a.terminator = '\n';
    a.ncols = 1;
    a.names_bytes = 4;
    a.cols[0] = JsonFieldsCol{0, 4, kFpSpan, 0, nullptr, nullptr, nullptr};
    CHECK(json_fields_scalars_ok(a));
    a.terminator = 256;
    CHECK(!json_fields_scalars_ok(a));
    a.terminator = '\n';
    a.ncols = 0;
    CHECK(!json_fields_scalars_ok(a));
    a.ncols = 33;
    CHECK(!json_fields_scalars_ok(a));
    a.ncols = 1;
    a.cols[0].type = 7;
    CHECK(!json_fields_scalars_ok(a));
    a.cols[0].type = 0;
    a.cols[0].name_len = 0;
    CHECK(!json_fields_scalars_ok(a));
    a.cols[0].name_len = 256;
    CHECK(!json_fields_scalars_ok(a));
    a.cols[0].name_len = 4;
    a.cols[0].name_off = 1;
    CHECK(!json_fields_scalars_ok(a));
  }
  // 32 columns, long rows
  {
    std::string row = "{", keys;
    for (int j = 0; j < 32; ++j) row += (j ? ",\"k" : "\"k") + std::to_string(j) + "\":" + std::to_string(j * j) + std::string((size_t)j * 9, ' ');
    row += "}\n";
    Heap data(row);
    int64_t off = 0, len = (int64_t)row.size();
    int64_t v[32];
    uint8_t s[32];
    JsonFieldsArgs a{};
    a.data = data.p.get();
    a.data_bytes = data.n;
    a.off = &off;
    a.len = &len;
    a.len_is_64 = 1;
    a.nrows = 1;
    a.terminator = '\n';
    a.ncols = 32;
    for (int j = 0; j < 32; ++j) {
      const std::string k = "k" + std::to_string(31 - j);
      a.cols[j] = JsonFieldsCol{(uint32_t)keys.size(), (uint32_t)k.size(), kFpInt64, 0, &v[j], nullptr, &s[j]};
      keys += k;
    }
    Heap names(keys);
    a.names = names.p.get();
    a.names_bytes = (uint32_t)names.n;
    CHECK(json_fields_scalars_ok(a));
    json_fields_host(a);
    for (int j = 0; j < 32; ++j) CHECK(s[j] == 0 && v[j] == (31 - j) * (31 - j));
  }
}

static void check_escaped16() {
  for (uint32_t cin = 0; cin < 2; ++cin)
    for (uint32_t bm = 0; bm < 65536; ++bm) {
      uint32_t want = 0, esc = cin;
      for (int j = 0; j < 16; ++j) {
        const bool code = esc != 0;
        if (code) want |= 1u << j;
        esc = !code && ((bm >> j) & 1u);
      }
      uint32_t cout;
      const uint32_t got = jf_escaped16(bm, cin, &cout);
      if (got != want || cout != esc) {
        CHECK(got == want && cout == esc);
        return;
      }
    }
}

struct Text {
  std::vector<int32_t> len;
  std::vector<uint8_t> st;
  std::string out;
};

static Text unescape(const std::vector<std::string>& values, const std::vector<uint8_t>* status = nullptr,
                     const std::vector<int64_t>* offsets = nullptr, uint64_t out_bytes = 0) {
  std::string all;
  std::vector<int64_t> start;
  std::vector<int32_t> length;
  for (auto& v : values) {
    all += "\\";                                    // a byte that belongs to no value
    start.push_back((int64_t)all.size());
    length.push_back((int32_t)v.size());
    all += v;
  }
  Heap data(all);
  const size_t n = values.size();
  Text t;
  t.len.assign(n, 77);
  t.st.assign(n, 9);
  JsonTextArgs a{};
  a.t.data = data.p.get();
  a.t.data_bytes = data.n;
  a.t.start = start.data();
  a.t.length = length.data();
  a.t.status = status ? status->data() : nullptr;
  a.t.n = n;
  a.t.quote = -1;
  a.t.out_len = t.len.data();
  a.out_status = t.st.data();
  json_text_measure_host(a);
  std::vector<int64_t> off(n + 1, 0);
  for (size_t r = 0; r < n; ++r) off[r + 1] = off[r] + t.len[r];
  if (offsets) off = *offsets;
  else out_bytes = (uint64_t)off[n];
  std::unique_ptr<uint8_t[]> out(new uint8_t[out_bytes]);   // exactly out_bytes
  std::memset(out.get(), 0xEE, out_bytes);
  a.t.status = t.st.data();
  a.t.offsets = off.data();
  a.t.out = out.get();
  a.t.out_bytes = out_bytes;
  json_text_emit_host(a);
  t.out.assign(reinterpret_cast<char*>(out.get()), out_bytes);
  return t;
}

static std::string un1(const std::string& v) {
  const Text t = unescape({v});
  return t.st[0] == 0 ? t.out : "<bad>";
}

static void check_unescape() {
  CHECK(un1("") == "" && un1("abc") == "abc" && un1("a\\\"b\\\\c\\/d") == "a\"b\\c/d");
  CHECK(un1("\\b\\f\\n\\r\\t") == "\x08\x0C\x0A\x0D\x09");
  CHECK(un1("\\u0041\\u00e9\\u20AC") == "A\xC3\xA9\xE2\x82\xAC" && un1("\\u0000") == std::string(1, '\0'));
  CHECK(un1("\\ud83d\\ude00") == "\xF0\x9F\x98\x80" && un1("\\uD83D\\uDE00x") == "\xF0\x9F\x98\x80x");
  CHECK(un1("\\ud800") == "\xED\xA0\x80" && un1("\\udc00") == "\xED\xB0\x80");
  CHECK(un1("\\ude00\\ud83d") == "\xED\xB8\x80\xED\xA0\xBD");
  CHECK(un1("\\ud83d\\ud83d\\ude00") == "\xED\xA0\xBD\xF0\x9F\x98\x80" && un1("\\ud83dx\\ude00") == "\xED\xA0\xBDx\xED\xB8\x80");
  CHECK(un1("\\ud83d\\n") == "\xED\xA0\xBD\n" && un1("\\ud83d\\u00e9") == "\xED\xA0\xBD\xC3\xA9");
  for (const char* s : {"\\", "a\\", "\\x", "\\a", "\\U0041", "\\u", "\\u0", "\\u00", "\\u004", "\\u004g", "ab\\u12", "\\ud83d\\u",
                        "\\ud83d\\ude0", "\\'", "\\0", "x\\ y"})
    CHECK(un1(s) == "<bad>");
  CHECK(un1("\\\\") == "\\" && un1("\\\\\\") == "<bad>" && un1("\\\\n") == "\\n");
  for (size_t n : {0u, 1u, 2u, 15u, 16u, 17u, 255u, 256u, 257u, 511u, 512u, 513u, 4099u}) {
    std::string v, w;
    for (size_t i = 0; v.size() + 2 <= n; ++i) {
      if (i % 5 == 4) {
        v += "\\n";
        w += "\n";
      } else {
        v += (char)('a' + i % 7);
        w += (char)('a' + i % 7);
      }
    }
    CHECK(un1(v) == w);
  }
  // a bad value is empty and its neighbours are untouched
  {
    const Text t = unescape({"ab", "c\\qd", "e\\tf", "\\u12", "g"});
    CHECK(t.out == "abe\tfg" && t.len == (std::vector<int32_t>{2, 0, 3, 0, 1}));
    CHECK(t.st == (std::vector<uint8_t>{0, 2, 0, 2, 0}));
  }
  // liveness
  {
    const std::vector<uint8_t> status{0, 1, 2, 3, 0};
    const Text t = unescape({"a\\nb", "zz", "zz", "zz", "c"}, &status);
    CHECK(t.out == "a\nbc" && t.st == status);
  }
  {
    Heap data("abcdef");
    int64_t start[5] = {-1, 0, 3, 7, 1};
    int32_t length[5] = {2, 7, 4, 0, -1};
    int32_t len[5];
    uint8_t s[5];
    JsonTextArgs a{};
    a.t.data = data.p.get();
    a.t.data_bytes = data.n;
    a.t.start = start;
    a.t.length = length;
    a.t.n = 5;
    a.t.quote = -1;
    a.t.out_len = len;
    a.out_status = s;
    json_text_measure_host(a);
    for (int r = 0; r < 5; ++r) CHECK(len[r] == 0 && s[r] == 2);
  }
  // windows that disagree with the data
  {
    const std::vector<std::string> vals{"abcdefgh", "i\\nj", "\\u00e9", "k\\q"};
    const std::vector<int64_t> offsets{-3, 4, 5, 9, 14};
    const Text t = unescape(vals, nullptr, &offsets, 12);
    std::string want(12, '\xEE');
    want.replace(0, 4, "defg");
    want[4] = 'i';
    want.replace(5, 2, "\xC3\xA9");
    CHECK(t.out == want);
    const std::vector<int64_t> far{INT64_MIN, -5, 0, 0, INT64_MAX};
    CHECK(unescape(vals, nullptr, &far, 12).out == std::string(12, '\xEE'));
  }
}

int main() {
  check_escaped16();
  check_locate();
  check_unescape();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
