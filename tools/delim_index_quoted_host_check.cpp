// Stand-alone check of the quoted host delimiter-index loop (delim_index_host_quoted in
// alluxio_amd/csrc/delim_index_host.h), meant for a sanitizer build on the CPU:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/delim_index_quoted_host_check.cpp -o build/delim_index_quoted_host_check
// Every page of the arena is its own heap allocation of exactly one page, so a read past a page
// (or before it) is a heap-buffer-overflow for the sanitizer.  The loop takes one arena base and
// page numbers, so the lowest allocation is the base and the others are numbered by their
// distance from it.  Cases: the edge cases of tests/test_delim_index_quoted.py; the expected cuts
// come from a byte-by-byte count of the quote bytes before each delimiter.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "delim_index_host.h"

namespace {

constexpr uint32_t kShift = 12;
constexpr uint64_t kPage = 1ull << kShift;
constexpr int kPages = 64;
constexpr uint8_t kD = 0x0A, kQ = '"';

struct Arena {
  std::vector<uint8_t*> mem;
  std::vector<int64_t> vtab;
  const uint8_t* base = nullptr;
  Arena() {
    for (int i = 0; i < kPages; ++i) {
      uint8_t* p = static_cast<uint8_t*>(std::aligned_alloc(kPage, kPage));
      if (!p) std::abort();
      mem.push_back(p);
      if (!base || p < base) base = p;
    }
    for (uint8_t* p : mem) vtab.push_back((int64_t)((uint64_t)(p - base) >> kShift));
  }
  ~Arena() {
    for (uint8_t* p : mem) std::free(p);
  }
  uint8_t& at(uint64_t va) { return mem[va >> kShift][va & (kPage - 1)]; }
  void fill(uint8_t v) {
    for (uint8_t* p : mem) std::memset(p, v, kPage);
  }
  void put(uint64_t va, const char* s) {
    for (; *s; ++s) at(va++) = (uint8_t)*s;
  }
};

int failures = 0;

void check(Arena& a, uint64_t vstart, uint64_t bytes, uint8_t d, uint8_t q, bool in_quote, const char* what) {
  std::vector<uint64_t> want, got;
  uint64_t quotes = in_quote ? 1 : 0;
  for (uint64_t i = 0; i < bytes; ++i) {
    const uint8_t b = a.at(vstart + i);
    if (b == d && quotes % 2 == 0) want.push_back(5 + i + 1);
    if (b == q) ++quotes;
  }
  const bool end = amdx::delim_index_host_quoted(a.base, a.vtab.data(), kShift, vstart, bytes, d, q, in_quote, 5, &got);
  if (got != want || end != (quotes % 2 == 1)) {
    std::printf("FAIL %s: vstart %llu bytes %llu in_quote %d: %zu cuts, expected %zu; end state %d, expected %d\n", what,
                (unsigned long long)vstart, (unsigned long long)bytes, (int)in_quote, got.size(), want.size(), (int)end,
                (int)(quotes % 2));
    ++failures;
  }
}

void check2(Arena& a, uint64_t vstart, uint64_t bytes, uint8_t d, uint8_t q, const char* what) {
  check(a, vstart, bytes, d, q, false, what);
  check(a, vstart, bytes, d, q, true, what);
}

void random_text(Arena& a, uint64_t vstart, uint64_t bytes, uint8_t d, uint8_t q, uint32_t seed, int d_in, int q_in) {
  std::mt19937 rng(seed);
  for (uint64_t i = 0; i < bytes; ++i) {
    uint8_t b = (uint8_t)rng();
    while (b == d || b == q) b += 0x11;
    if (rng() % d_in == 0) b = d;
    if (rng() % q_in == 0) b = q;
    a.at(vstart + i) = b;
  }
}

}  // namespace

int main() {
  Arena a;
  const uint64_t flen = 39 * kPage + 1000;
  for (int q_in : {20, 200, 1 << 30}) {
    a.fill(kQ);
    random_text(a, 0, flen, kD, kQ, 1, 40, q_in);
    if (q_in == 1 << 30) a.at(flen / 3) = kQ;     // one single quote
    check2(a, 0, flen, kD, kQ, "file ending inside its last page");
  }
  const uint64_t sizes[] = {0, 1, 15, 16, 17, 4095, 4096, 4097};
  for (uint8_t fill : {kQ, kD})
    for (int ph = 0; ph < 16; ++ph)
      for (uint64_t n : sizes) {
        const uint64_t vstart = 5 * kPage - 32 + ph;
        a.fill(fill);
        random_text(a, vstart, n, kD, kQ, 100 * ph + (uint32_t)n, 6, 9);
        check2(a, vstart, n, kD, kQ, "phases and short ranges");
      }
  {
    // a quoted field and a doubled quote at the page edges and at the two ends of the range
    const uint64_t vstart = 3 * kPage + 83, n = 50 * kPage + 77;
    const uint64_t edges[] = {vstart, vstart + 1, 5 * kPage, 17 * kPage, vstart + n - 1, vstart + n};
    for (uint8_t fill : {kQ, kD})
      for (uint64_t e : edges)
        for (int shift = 0; shift < 12; ++shift) {
          a.fill(fill);
          random_text(a, vstart, n, kD, kQ, 3, 1 << 30, 1 << 30);
          a.put(e - shift, "\n\"\nab\n\"\"\ncd\n\"\n");   // may stick out of the range: those bytes do not count
          check2(a, vstart, n, kD, kQ, "quoted field at range and page edges");
        }
  }
  {
    // a quoted field over several whole pages that hold delimiters and no quote
    const uint64_t vstart = kPage + 7, n = 20 * kPage;
    a.fill(kQ);
    random_text(a, vstart, n, kD, kQ, 9, 30, 1 << 30);
    a.at(vstart + kPage + 100) = kQ;
    a.at(vstart + 14 * kPage + 200) = kQ;
    check2(a, vstart, n, kD, kQ, "quoted field over whole pages");
  }
  a.fill(kQ);
  check2(a, 7 * kPage, 3 * kPage, kD, kQ, "every byte a quote, even length");
  check2(a, 7 * kPage + 5, 3 * kPage + 1, kD, kQ, "every byte a quote, odd length");
  a.fill(kD);
  check2(a, 7 * kPage + 5, 3 * kPage, kD, kQ, "every byte a delimiter");
  a.at(7 * kPage + 5) = kQ;
  check2(a, 7 * kPage + 5, 3 * kPage, kD, kQ, "every byte a delimiter after one quote");
  for (int q : {0x00, 0xFF}) {
    a.fill((uint8_t)q);
    random_text(a, 2 * kPage + 11, 9 * kPage + 123, (uint8_t)(0xFF - q), (uint8_t)q, 6, 40, 50);
    check2(a, 2 * kPage + 11, 9 * kPage + 123, (uint8_t)(0xFF - q), (uint8_t)q, "quote 0x00 / 0xFF");
  }
  a.fill(kQ);
  check2(a, (uint64_t)kPages * kPage - 100, 100, kD, kQ, "range ending with the page table");
  a.fill(kD);
  check2(a, (uint64_t)kPages * kPage - 100, 100, kD, kQ, "range ending with the page table");
  if (failures) return 1;
  std::printf("delim_index_quoted_host_check ok\n");
  return 0;
}
