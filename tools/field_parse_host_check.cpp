// Stand-alone sanitizer check of the host form of the field parser (csrc/field_parse_host.h, the
// code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/field_parse_host_check.cpp -o build/field_parse_host_check \
//       && build/field_parse_host_check
//
// Every data buffer is a heap allocation of exactly data_bytes, so a read one byte outside it is an
// AddressSanitizer error.  The cases are the edge cases of tests/test_field_parse.py (row ends,
// missing and empty fields, quoting, integer and float limits, the deferred rule, long rows, 32
// columns) and rows whose off / len lie outside the buffer.  Exit status 0 and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "field_parse_host.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

struct Out {
  std::vector<int64_t> i64;
  std::vector<int32_t> i32, len;
  std::vector<double> f64;
  std::vector<float> f32;
  std::vector<uint8_t> st;
};

struct Table {
  std::unique_ptr<uint8_t[]> data;                  // exactly data_bytes
  uint64_t data_bytes = 0;
  std::vector<int64_t> off, len;
  void rows(const std::vector<std::string>& rs, size_t lead = 0) {
    std::string all(lead, '5');
    for (auto& r : rs) {
      off.push_back((int64_t)all.size());
      len.push_back((int64_t)r.size());
      all += r;
    }
    data_bytes = all.size();
    data.reset(new uint8_t[all.size()]);
    std::memcpy(data.get(), all.data(), all.size());
  }
};

static std::vector<Out> run(const Table& t, const std::vector<std::pair<uint32_t, uint32_t>>& cols, int quote = -1,
                            uint32_t sep = ',', uint32_t term = '\n', bool len64 = true) {
  const size_t n = t.off.size();
  std::vector<Out> outs(cols.size());
  std::vector<int32_t> len32(t.len.begin(), t.len.end());
  FieldParseArgs a{};
  a.data = t.data.get();
  a.data_bytes = t.data_bytes;
  a.off = t.off.data();
  a.len = len64 ? (const void*)t.len.data() : (const void*)len32.data();
  a.len_is_64 = len64;
  a.nrows = n;
  a.sep = sep;
  a.quote = quote;
  a.terminator = term;
  a.ncols = (uint32_t)cols.size();
  for (size_t j = 0; j < cols.size(); ++j) {
    Out& o = outs[j];
    o.i64.assign(n, 77);
    o.i32.assign(n, 77);
    o.len.assign(n, 77);
    o.f64.assign(n, 77);
    o.f32.assign(n, 77);
    o.st.assign(n, 77);
    FieldParseCol& c = a.cols[j];
    c.field = cols[j].first;
    c.type = cols[j].second;
    c.status = o.st.data();
    c.length = o.len.data();
    switch (c.type) {
      case kFpSpan:
      case kFpInt64: c.values = o.i64.data(); break;
      case kFpInt32: c.values = o.i32.data(); break;
      case kFpFloat64: c.values = o.f64.data(); break;
      default: c.values = o.f32.data(); break;
    }
    if (c.field > a.max_field) a.max_field = c.field;
  }
  if (!field_parse_scalars_ok(a)) {
    std::printf("FAILED: scalars rejected\n");
    ++g_failed;
    return outs;
  }
  field_parse_host(a);
  return outs;
}

static uint64_t bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

int main() {
  {  // row ends, missing and empty fields
    Table t;
    t.rows({"\n", "\r\n", "1,2\r\n", "1,2\r", "", ",\n", " , \t\n", "9,10"}, 3);
    auto o = run(t, {{0, kFpInt64}, {1, kFpInt64}, {2, kFpFloat64}, {1, kFpSpan}, {65535, kFpFloat32}});
    const uint8_t st0[] = {1, 1, 0, 0, 1, 1, 1, 0}, st1[] = {1, 1, 0, 2, 1, 1, 1, 0};
    for (int r = 0; r < 8; ++r) {
      CHECK(o[0].st[r] == st0[r]);
      CHECK(o[1].st[r] == st1[r]);
      CHECK(o[2].st[r] == 1 && std::isnan(o[2].f64[r]));
      CHECK(o[4].st[r] == 1 && std::isnan(o[4].f32[r]));
    }
    CHECK(o[0].i64[2] == 1 && o[1].i64[2] == 2 && o[1].i64[7] == 10);
    CHECK(o[3].st[0] == 1 && o[3].i64[0] == 0 && o[3].len[0] == 0);
    CHECK(o[3].st[3] == 0 && o[3].len[3] == 2);     // "2\r": no \n, so the \r stays
    CHECK(o[3].st[7] == 0 && o[3].i64[7] == t.off[7] + 2 && o[3].len[7] == 2);
    run(t, {{0, kFpInt64}, {1, kFpSpan}}, '"', ',', '\n', false);
  }
  {  // quoting
    Table t;
    t.rows({"x,\"12\"\n", "x,\" 12 \"\n", "x,\"1\"\"2\"\n", "x,\"\n", "\"a,b\n\"\"c\"\",\",17,0.25\n", "\"", "\"open,1"});
    auto o = run(t, {{1, kFpInt64}, {1, kFpSpan}, {2, kFpFloat64}, {0, kFpSpan}}, '"');
    CHECK(o[0].st[0] == 0 && o[0].i64[0] == 12 && o[0].st[1] == 0 && o[0].i64[1] == 12);
    CHECK(o[0].st[2] == 2 && o[1].len[2] == 4);
    CHECK(o[0].st[3] == 2 && o[1].st[3] == 0 && o[1].len[3] == 1);      // a lone quote is its own content
    CHECK(o[0].st[4] == 0 && o[0].i64[4] == 17 && o[2].st[4] == 0 && o[2].f64[4] == 0.25 && o[3].len[4] == 10);
    CHECK(o[3].st[5] == 0 && o[3].len[5] == 1 && o[0].st[5] == 1);
    CHECK(o[0].st[6] == 1 && o[3].len[6] == 7);
  }
  {  // integers
    Table t;
    t.rows({"0\n", "-0\n", "+7\n", "000000000000000000000000012\n", "9223372036854775807\n", "-9223372036854775808\n",
            "9223372036854775808\n", "123456789012345678901234567890\n", "2147483647\n", "2147483648\n", "-2147483648\n",
            "-2147483649\n", "1.0\n", "1e3\n", "+\n", "-\n", "1 2\n", "18446744073709551616\n"});
    auto o = run(t, {{0, kFpInt64}, {0, kFpInt32}});
    const uint8_t s64[] = {0, 0, 0, 0, 0, 0, 2, 2, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2};
    const uint8_t s32[] = {0, 0, 0, 0, 2, 2, 2, 2, 0, 2, 0, 2, 2, 2, 2, 2, 2, 2};
    for (int r = 0; r < 18; ++r) {
      CHECK(o[0].st[r] == s64[r]);
      CHECK(o[1].st[r] == s32[r]);
    }
    CHECK(o[0].i64[2] == 7 && o[0].i64[3] == 12 && o[0].i64[4] == INT64_MAX && o[0].i64[5] == INT64_MIN);
    CHECK(o[1].i32[8] == INT32_MAX && o[1].i32[10] == INT32_MIN && o[0].i64[6] == 0);
  }
  {  // floats and the deferred rule
    Table t;
    t.rows({".5\n", "5.\n", ".\n", "e5\n", "1e\n", "1e+\n", "-0.0\n", "0e999999999999999999999\n", "1e22\n", "1e23\n",
            "9007199254740992\n", "9007199254740993\n", "0.100000000000000000000\n", "1e-22\n", "123456789012345e-37\n",
            "nan\n", "-Inf\n", "INFINITY\n", "infinit\n", "1e99999999999999999999999999\n", "4.35\n", "2.5e-3\n"});
    auto o = run(t, {{0, kFpFloat64}, {0, kFpFloat32}});
    const uint8_t st[] = {0, 0, 2, 2, 2, 2, 0, 0, 0, 3, 0, 3, 3, 0, 3, 0, 0, 0, 2, 3, 0, 0};
    for (int r = 0; r < 22; ++r) {
      CHECK(o[0].st[r] == st[r]);
      CHECK(o[1].st[r] == st[r]);
      if (st[r] != 0) CHECK(std::isnan(o[0].f64[r]) && std::isnan(o[1].f32[r]));
    }
    CHECK(o[0].f64[0] == 0.5 && o[0].f64[1] == 5.0 && bits(o[0].f64[6]) == 0x8000000000000000ull && bits(o[0].f64[7]) == 0);
    CHECK(o[0].f64[8] == 1e22 && o[0].f64[10] == 9007199254740992.0 && o[0].f64[13] == 1e-22);
    CHECK(std::isnan(o[0].f64[15]) && o[0].f64[16] == -INFINITY && o[0].f64[17] == INFINITY && o[1].f32[16] == -INFINITY);
    CHECK(o[0].f64[20] == 4.35 && o[0].f64[21] == 2.5e-3 && o[1].f32[20] == (float)4.35);
    CHECK(o[0].f64[20] == std::strtod("4.35", nullptr) && o[0].f64[21] == std::strtod("2.5e-3", nullptr));
  }
  {  // long rows, column 300 of 400, 32 columns
    std::string row;
    for (int i = 0; i < 400; ++i) row += std::to_string(i * 3) + (i + 1 < 400 ? "," : "\n");
    std::string big;
    while (big.size() < 70000) big += "12,\"a,b\",";
    big += "5";                                     // no terminator: the buffer ends with the row
    Table t;
    t.rows({row, row.substr(0, row.size() - 1), big});
    auto o = run(t, {{300, kFpInt64}, {399, kFpInt32}, {400, kFpInt64}}, '"');
    CHECK(o[0].st[0] == 0 && o[0].i64[0] == 900 && o[1].i32[1] == 1197 && o[2].st[0] == 1 && o[2].st[1] == 1);
    CHECK(o[0].st[2] == 0 && o[0].i64[2] == 12);    // field 300 of 12,"a,b",... is a 12
    std::vector<std::pair<uint32_t, uint32_t>> cols;
    for (uint32_t k = 0; k < 32; ++k) cols.push_back({k * 7, k % 5});
    auto w = run(t, cols, '"');
    for (uint32_t k = 0; k < 32; ++k) CHECK(w[k].st[0] == 0 && w[k].st[1] == 0);
    CHECK(w[1].i64[0] == 21 && w[2].i32[0] == 42 && w[3].f64[0] == 63.0 && w[4].f32[0] == 84.0f && w[0].len[0] == 1);
  }
  {  // rows outside the buffer are not read; their neighbours are
    Table t;
    t.rows({"1,2.5,a\n", "3,4.5,b\n", "5,6.5,c\n"});
    t.off = {0, -1, 8, 16, 16, 25, 8, (int64_t)1 << 62, 24, 23};
    t.len = {8, 8, -1, 8, 9, 0, ((int64_t)1 << 31) - 1, 8, 0, 1};
    for (int len64 = 0; len64 < 2; ++len64) {
      auto o = run(t, {{0, kFpInt64}, {1, kFpFloat64}, {2, kFpSpan}}, -1, ',', '\n', len64 != 0);
      const uint8_t st[] = {0, 2, 2, 0, 2, 2, 2, 2, 1, 1};
      for (int r = 0; r < 10; ++r) {
        CHECK(o[0].st[r] == st[r]);
        if (st[r] == 2) CHECK(o[0].i64[r] == 0 && std::isnan(o[1].f64[r]) && o[2].st[r] == 2 && o[2].len[r] == 0);
      }
      CHECK(o[0].i64[0] == 1 && o[0].i64[3] == 5 && o[1].f64[3] == 6.5 && o[2].i64[3] == 22 && o[2].len[3] == 1);
    }
    t.len[0] = (int64_t)1 << 40;
    auto o = run(t, {{0, kFpInt64}});
    CHECK(o[0].st[0] == 2 && o[0].st[3] == 0);
  }
  {  // scalars
    FieldParseArgs a{};
    a.sep = ',';
    a.quote = '"';
    a.terminator = '\n';
    a.ncols = 1;
    CHECK(field_parse_scalars_ok(a));
    a.quote = ',';
    CHECK(!field_parse_scalars_ok(a));
    a.quote = '\n';
    CHECK(!field_parse_scalars_ok(a));
    a.quote = -1;
    a.ncols = 33;
    CHECK(!field_parse_scalars_ok(a));
    a.ncols = 0;
    CHECK(!field_parse_scalars_ok(a));
    a.ncols = 1;
    a.cols[0].field = 65536;
    a.max_field = 65536;
    CHECK(!field_parse_scalars_ok(a));
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
