// Stand-alone check of the host delimiter-index loop (alluxio_amd/csrc/delim_index_host.h), meant
// for a sanitizer build on the CPU:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/delim_index_host_check.cpp -o build/delim_index_host_check
// Every page of the arena is its own heap allocation of exactly one page, so a read past a page
// (or before it) is a heap-buffer-overflow for the sanitizer.  The loop takes one arena base and
// page numbers, so the lowest allocation is the base and the others are numbered by their
// distance from it.  Cases: the edge cases of tests/test_delim_index.py, and the page walk under the
// loop (for_each_page_run in paged_view_host.h) on its own.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "delim_index_host.h"

namespace {

constexpr uint32_t kShift = 12;
constexpr uint64_t kPage = 1ull << kShift;
constexpr int kPages = 64;

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
};

int failures = 0;

void check(Arena& a, uint64_t vstart, uint64_t bytes, uint8_t d, const char* what) {
  std::vector<uint64_t> want, got;
  for (uint64_t i = 0; i < bytes; ++i)
    if (a.at(vstart + i) == d) want.push_back(i + 1);
  amdx::delim_index_host(a.base, a.vtab.data(), kShift, vstart, bytes, d, 0, &got);
  if (got != want) {
    std::printf("FAIL %s: vstart %llu bytes %llu: %zu cuts, expected %zu\n", what, (unsigned long long)vstart,
                (unsigned long long)bytes, got.size(), want.size());
    ++failures;
  }
}

void random_text(Arena& a, uint64_t vstart, uint64_t bytes, uint8_t d, uint32_t seed, int one_in) {
  std::mt19937 rng(seed);
  for (uint64_t i = 0; i < bytes; ++i) {
    uint8_t b = (uint8_t)rng();
    if (b == d) b ^= 0x55;
    if (rng() % one_in == 0) b = d;
    a.at(vstart + i) = b;
  }
}

// The pieces must tile [va, va + len) in order, each inside one page, and every byte of them is read.
void check_runs(Arena& a, uint64_t va, uint64_t len, const char* what) {
  uint64_t next = 0, sum = 0, want = 0;
  bool ok = true;
  for (uint64_t i = 0; i < len; ++i) want += a.at(va + i);
  amdx::for_each_page_run(a.base, a.vtab.data(), kShift, va, len, [&](const uint8_t* p, uint64_t n, uint64_t done) {
    const uint64_t first = va + done, last = first + n - 1;
    ok = ok && done == next && n > 0 && p == &a.at(first) && (first >> kShift) == (last >> kShift);
    for (uint64_t i = 0; i < n; ++i) sum += p[i];
    next = done + n;
  });
  if (!ok || next != len || sum != want) {
    std::printf("FAIL page runs, %s: va %llu len %llu\n", what, (unsigned long long)va, (unsigned long long)len);
    ++failures;
  }
}

}  // namespace

int main() {
  Arena a;
  const uint64_t flen = 39 * kPage + 1000;
  a.fill(0x0A);
  random_text(a, 0, flen, 0x0A, 1, 40);
  check(a, 0, flen, 0x0A, "file ending inside its last page");
  const uint64_t sizes[] = {0, 1, 15, 16, 17, 4095, 4096, 4097};
  for (int ph = 0; ph < 16; ++ph)
    for (uint64_t n : sizes) {
      const uint64_t vstart = 5 * kPage - 32 + ph;
      a.fill(0x0A);
      random_text(a, vstart, n, 0x0A, 100 * ph + (uint32_t)n, 8);
      check(a, vstart, n, 0x0A, "phases and short ranges");
    }
  {
    const uint64_t vstart = 3 * kPage + 83, n = 50 * kPage + 77;
    a.fill(',');
    random_text(a, vstart, n, ',', 3, 1 << 30);
    const uint64_t spots[] = {vstart, vstart + n - 1, 5 * kPage - 1, 5 * kPage};
    for (uint64_t s : spots) a.at(s) = ',';
    check(a, vstart, n, ',', "delimiters at range and page edges");
  }
  a.fill(0x0A);
  random_text(a, kPage + 9, 3 * kPage + 5, 0x0A, 4, 1 << 30);
  check(a, kPage + 9, 3 * kPage + 5, 0x0A, "no delimiter");
  a.fill(0x0A);
  check(a, 7 * kPage + 5, 3 * kPage, 0x0A, "every byte a delimiter");
  for (int d : {0x00, 0xFF}) {
    a.fill((uint8_t)d);
    random_text(a, 2 * kPage + 11, 9 * kPage + 123, (uint8_t)d, 6, 40);
    check(a, 2 * kPage + 11, 9 * kPage + 123, (uint8_t)d, "delimiter 0x00 / 0xFF");
  }
  check(a, (uint64_t)kPages * kPage - 100, 100, 0xFF, "range ending with the page table");
  random_text(a, 0, (uint64_t)kPages * kPage, 0x0A, 9, 40);
  check_runs(a, 3 * kPage + 100, 4 * kPage + 17, "starts and ends mid-page");
  check_runs(a, 6 * kPage + 4095, 1, "one byte, the last of its page");
  check_runs(a, 9 * kPage, 1, "one byte, the first of its page");
  check_runs(a, 11 * kPage + 7, 2 * kPage - 7, "ends on a page's last byte");
  check_runs(a, 13 * kPage, 0, "empty");
  if (failures) return 1;
  std::printf("delim_index_host_check ok\n");
  return 0;
}
