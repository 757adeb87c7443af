// Stand-alone sanitizer check of the host form of the text column (csrc/text_column_host.h, the
// code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/text_column_host_check.cpp -o build/text_column_host_check \
//       && build/text_column_host_check
//
// Every buffer (data, spans, lengths, offsets, output) is a heap allocation of its exact size, so a
// read or write one byte outside it is an AddressSanitizer error.  The cases are those of
// tests/test_text_column.py: the value lengths and start phases around the 16-byte vector and the
// 256-byte step, quote runs that end at and straddle those edges, values of quotes only, values
// that are not live, offsets that disagree with the data.  tc_drop16 is compared with the serial
// rule for all 2^17 inputs, and the way kernel variant 1 hands the run parity from vector to
// vector (nearest lower vector that is not all quotes: lg_carry_in and lg_carry_next of
// csrc/lane_group.h, the functions the kernel calls) is replayed here against the serial walk.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "lane_group.h"
#include "text_column_host.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

// The rule, written a second time and differently: runs of k quotes become (k + 1) / 2.
static std::string collapse(const std::string& s, int quote) {
  if (quote < 0) return s;
  std::string out;
  for (size_t i = 0; i < s.size();) {
    if ((uint8_t)s[i] != (uint8_t)quote) {
      out += s[i++];
      continue;
    }
    size_t k = 0;
    while (i < s.size() && (uint8_t)s[i] == (uint8_t)quote) ++i, ++k;
    out.append((k + 1) / 2, (char)quote);
  }
  return out;
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

struct Case {
  std::string data;
  std::vector<int64_t> start;
  std::vector<int32_t> length;
  std::vector<uint8_t> status;
  void add(const std::string& v, size_t lead = 0) {
    data.append(lead, '"');                         // bytes that belong to no value are quotes
    start.push_back((int64_t)data.size());
    length.push_back((int32_t)v.size());
    status.push_back(0);
    data += v;
  }
};

// measure, scan, emit with guard bytes; returns the packed bytes and fills lens.
static std::string run(const Case& c, int quote, std::vector<int32_t>* lens, bool with_status = true) {
  const size_t n = c.start.size();
  auto data = exact(std::vector<uint8_t>(c.data.begin(), c.data.end()));
  auto start = exact(c.start);
  auto length = exact(c.length);
  auto status = exact(c.status);
  std::unique_ptr<int32_t[]> out_len(new int32_t[n]);
  TextColumnArgs a{};
  a.data = data.get();
  a.data_bytes = c.data.size();
  a.start = start.get();
  a.length = length.get();
  a.status = with_status ? status.get() : nullptr;
  a.n = n;
  a.quote = quote;
  a.out_len = out_len.get();
  CHECK(text_column_scalars_ok(a));
  text_measure_host(a);
  std::unique_ptr<int64_t[]> offsets(new int64_t[n + 1]);
  offsets[0] = 0;
  for (size_t r = 0; r < n; ++r) offsets[r + 1] = offsets[r] + out_len[r];
  const size_t total = (size_t)offsets[n];
  std::unique_ptr<uint8_t[]> out(new uint8_t[total]);
  std::memset(out.get(), 0xEE, total);
  a.offsets = offsets.get();
  a.out = out.get();
  a.out_bytes = total;
  text_emit_host(a);
  lens->assign(out_len.get(), out_len.get() + n);
  return std::string(reinterpret_cast<char*>(out.get()), total);
}

static void check_values(const std::vector<std::string>& values, int quote, size_t lead) {
  Case c;
  for (auto& v : values) c.add(v, lead);
  std::vector<int32_t> lens;
  const std::string got = run(c, quote, &lens);
  std::string want;
  for (size_t r = 0; r < values.size(); ++r) {
    const std::string w = collapse(values[r], quote);
    CHECK(lens[r] == (int32_t)w.size());
    want += w;
  }
  CHECK(got == want);
}

// Kernel variant 1 on the host: vectors of 16 bytes in steps of 16 lanes, the incoming parity of a
// lane taken from the nearest lower lane that is not all quotes by the kernel's own two functions.
static std::string coop(const std::string& v, int quote) {
  std::string out;
  uint32_t carry = 0;
  for (size_t base = 0; base < v.size(); base += 256) {
    uint32_t qm[16], valid[16], ga = 0, gb = 0;
    for (uint32_t l = 0; l < 16; ++l) {
      const size_t pos = base + 16 * l;
      const size_t rem = pos < v.size() ? v.size() - pos : 0;
      valid[l] = rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
      qm[l] = 0;
      for (size_t j = 0; j < 16 && j < rem; ++j)
        if (quote >= 0 && (uint8_t)v[pos + j] == (uint8_t)quote) qm[l] |= 1u << j;
      if (qm[l] != 0xFFFFu) ga |= 1u << l;
      if (tc_carry_out16(qm[l], tc_drop16(qm[l], 0))) gb |= 1u << l;
    }
    for (uint32_t l = 0; l < 16; ++l) {
      const uint32_t keep = valid[l] & ~tc_drop16(qm[l], lg_carry_in(ga, gb, l, carry));
      for (uint32_t j = 0; j < 16; ++j)
        if ((keep >> j) & 1u) out += v[base + 16 * l + j];
    }
    carry = lg_carry_next(ga, gb, carry);
  }
  return out;
}

int main() {
  {  // tc_drop16 against the serial rule, every mask and both carries
    for (uint32_t carry = 0; carry < 2; ++carry)
      for (uint32_t qm = 0; qm < 0x10000u; ++qm) {
        uint32_t want = 0;
        bool odd = carry != 0;
        for (uint32_t j = 0; j < 16; ++j) {
          const bool q = (qm >> j) & 1u;
          if (q && odd) want |= 1u << j;
          odd = q && !odd;
        }
        if (tc_drop16(qm, carry) != want) {
          std::printf("FAILED: tc_drop16(%#x, %u)\n", qm, carry);
          ++g_failed;
          carry = 2;
          break;
        }
        if (qm != 0xFFFFu) CHECK(tc_carry_out16(qm, tc_drop16(qm, 0)) == tc_carry_out16(qm, want));
      }
  }
  const size_t lengths[] = {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 4099};
  const size_t runs[] = {1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 35};
  {  // plain lengths at four start phases, with and without quotes in them
    for (size_t lead : {0u, 1u, 7u, 15u}) {
      std::vector<std::string> plain, quoted;
      for (size_t n : lengths) {
        std::string v(n, 'a');
        for (size_t i = 0; i < n; ++i) v[i] = (char)('a' + i % 23);
        plain.push_back(v);
        for (size_t i = 3; i + 1 < n; i += 11) v[i] = v[i + 1] = '"';
        if (n) v[n - 1] = '"';
        quoted.push_back(v);
      }
      check_values(plain, '"', lead);
      check_values(plain, -1, lead);
      check_values(quoted, '"', lead);
      check_values(quoted, -1, lead);
      check_values(quoted, 'a', lead);
    }
  }
  {  // runs that end at and straddle a vector edge (16) and a step edge (256); quotes only; cut runs
    std::vector<std::string> vs;
    for (size_t edge : {16u, 256u})
      for (size_t k : runs)
        for (size_t before : std::vector<size_t>{0, 1, k / 2, k - 1, k}) {
          if (before > edge) continue;
          std::string v(edge + 40, 'x');
          for (size_t i = 0; i < k; ++i) v[edge - before + i] = '"';
          vs.push_back(v);
          vs.push_back(v.substr(0, edge - before + (k + 1) / 2));      // the run is cut by the end
        }
    for (size_t k : {16u, 32u, 33u, 256u, 257u, 512u, 513u}) vs.push_back(std::string(k, '"'));
    check_values(vs, '"', 0);
    check_values(vs, '"', 5);
    for (auto& v : vs) CHECK(coop(v, '"') == collapse(v, '"'));
  }
  {  // random values over {quote, a, comma}: the host loop and the replay of variant 1
    uint64_t s = 12345;
    auto next = [&s] {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      return (uint32_t)(s >> 33);
    };
    std::vector<std::string> vs;
    for (int r = 0; r < 2000; ++r) {
      size_t n = next() % 40;
      if (next() % 8 == 0) n = next() % 1200;
      const uint32_t qbias = next() % 4;            // 0: mostly quotes
      std::string v(n, 'a');
      for (auto& ch : v) {
        const uint32_t x = next() % 8;
        ch = qbias == 0 ? (x < 6 ? '"' : 'a') : (x < 3 ? '"' : (x < 6 ? 'a' : ','));
      }
      vs.push_back(v);
      CHECK(coop(v, '"') == collapse(v, '"'));
    }
    check_values(vs, '"', 1);
    check_values(vs, -1, 1);
  }
  {  // values that are not live: length 0, nothing read, the neighbours as usual
    Case c;
    c.add("a\"\"b");
    c.add("zzzz");
    c.add("zzzz");
    c.add("zzzz");
    c.add("zzzz");
    c.add("c\"\"d");
    c.add("zzzz");
    c.status[1] = 1;
    c.status[2] = 2;
    c.start[3] = -1;
    c.length[4] = -1;
    c.start[6] = (int64_t)c.data.size() - 3;        // start + length = data_bytes + 1
    std::vector<int32_t> lens;
    CHECK(run(c, '"', &lens) == "a\"bc\"d");
    CHECK(lens == (std::vector<int32_t>{3, 0, 0, 0, 0, 3, 0}));
    c.status.assign(7, 0);
    c.start[1] = INT64_MAX;
    c.length[2] = INT32_MAX;
    CHECK(run(c, '"', &lens, false) == "a\"bc\"d");
    c.start[6] = (int64_t)c.data.size() - 4;        // the value that ends with the buffer is live
    CHECK(run(c, '"', &lens, false) == "a\"bc\"dzzzz");
  }
  {  // emit with offsets that disagree: nothing outside the value's window and the buffer
    Case c;
    c.add("abcdefgh");
    c.add("ij\"\"kl");
    c.add("mnop");
    auto data = exact(std::vector<uint8_t>(c.data.begin(), c.data.end()));
    auto start = exact(c.start);
    auto length = exact(c.length);
    TextColumnArgs a{};
    a.data = data.get();
    a.data_bytes = c.data.size();
    a.start = start.get();
    a.length = length.get();
    a.n = 3;
    a.quote = '"';
    const std::vector<std::vector<int64_t>> offs = {
        {0, 3, 8, 12},                              // too small for value 0: it is cut to 3 bytes
        {-5, 3, 5, 40},                             // starts before the buffer, ends past it
        {20, 30, 40, 50},                           // past out_bytes altogether
        {9, 4, 0, 0},                               // decreasing: empty windows
        {INT64_MIN, INT64_MAX, INT64_MIN, INT64_MAX},
    };
    const std::vector<std::string> want = {"abcij\"klmnop", "fghijmnop\xEE\xEE\xEE", std::string(12, '\xEE'),
                                           std::string(12, '\xEE'), std::string(12, '\xEE')};
    for (size_t t = 0; t < offs.size(); ++t) {
      auto offsets = exact(offs[t]);
      std::unique_ptr<uint8_t[]> out(new uint8_t[12]);
      std::memset(out.get(), 0xEE, 12);
      a.offsets = offsets.get();
      a.out = out.get();
      a.out_bytes = 12;
      text_emit_host(a);
      CHECK(std::string(reinterpret_cast<char*>(out.get()), 12) == want[t]);
    }
    std::unique_ptr<uint8_t[]> none(new uint8_t[0]);   // an output of no bytes takes nothing
    auto offsets = exact(offs[0]);
    a.offsets = offsets.get();
    a.out = none.get();
    a.out_bytes = 0;
    text_emit_host(a);
  }
  {  // scalars
    TextColumnArgs a{};
    a.quote = -1;
    CHECK(text_column_scalars_ok(a));
    a.quote = 255;
    CHECK(text_column_scalars_ok(a));
    a.quote = 256;
    CHECK(!text_column_scalars_ok(a));
    a.quote = -2;
    CHECK(!text_column_scalars_ok(a));
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
