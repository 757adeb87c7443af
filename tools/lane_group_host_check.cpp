// Stand-alone sanitizer check of the pure part of csrc/lane_group.h (the bit functions that also
// run on the device) against the obvious serial code.  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/lane_group_host_check.cpp -o build/lane_group_host_check \
//       && build/lane_group_host_check
//
// lg_mask16 against a byte loop: every target byte t, with t, t - 1, t + 1, t ^ 0x80, 0x00 and 0xFF
// as each other's neighbours in every byte position (what "exact: no carry between bytes" claims),
// and seeded random vectors.  lg_inside16 and lg_compact for all 65,536 masks.  lg_carry_in and
// lg_carry_next against a chain that walks the lanes one by one: every ga, both carries, all 16
// lanes, gb all zero, all one and seeded.  Every buffer is a heap allocation of its exact size, so
// a read or write one byte outside it is an AddressSanitizer error.  Exit status 0 and "ok" when
// all hold.
#include <cstdio>
#include <cstring>
#include <memory>

#include "lane_group.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static uint64_t g_seed = 0x5EEDull;
static uint32_t next() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_seed >> 33);
}

// lg_mask16 of the 16 bytes at b against the byte loop.
static bool mask_ok(const uint8_t* b, uint8_t t) {
  uint32_t w[4], want = 0;
  std::memcpy(w, b, 16);                            // lowest address in the lowest byte, as on the device
  for (uint32_t j = 0; j < 16; ++j)
    if (b[j] == t) want |= 1u << j;
  return lg_mask16(w[0], w[1], w[2], w[3], (uint32_t)t * 0x01010101u) == want;
}

static void check_mask16() {
  std::unique_ptr<uint8_t[]> b(new uint8_t[16]);
  for (uint32_t t = 0; t < 256; ++t) {
    const uint8_t near[6] = {(uint8_t)t, (uint8_t)(t - 1), (uint8_t)(t + 1), (uint8_t)(t ^ 0x80u), 0x00, 0xFF};
    bool ok = true;
    // byte j holds near[(j * s + r) % 6]: the six values in every stride and rotation
    for (uint32_t s = 0; s < 6; ++s)
      for (uint32_t r = 0; r < 6; ++r) {
        for (uint32_t j = 0; j < 16; ++j) b[j] = near[(j * s + r) % 6];
        ok = ok && mask_ok(b.get(), (uint8_t)t);
      }
    // each value in each position with each value on all sides of it: every pair of neighbours in
    // every byte position of a word, across the words too
    for (uint32_t pos = 0; pos < 16; ++pos)
      for (uint32_t x = 0; x < 6; ++x)
        for (uint32_t y = 0; y < 6; ++y) {
          for (uint32_t j = 0; j < 16; ++j) b[j] = near[y];
          b[pos] = near[x];
          ok = ok && mask_ok(b.get(), (uint8_t)t);
        }
    if (!ok) {
      std::printf("FAILED: lg_mask16, target %#x\n", t);
      ++g_failed;
      return;
    }
  }
  for (int i = 0; i < 4096; ++i) {
    const uint8_t t = (uint8_t)next();
    const uint32_t density = next() % 4;            // 0: about half of the bytes match
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t x = next();
      b[j] = (density == 0 ? (x & 1u) : (x % 8 == 0)) ? t : (uint8_t)(x >> 8);
    }
    if (!mask_ok(b.get(), t)) {
      CHECK(mask_ok(b.get(), t));
      return;
    }
  }
}

static void check_inside16() {
  for (uint32_t qm = 0; qm < 0x10000u; ++qm) {
    uint32_t want = 0, par = 0;
    for (uint32_t j = 0; j < 16; ++j) {
      if (par) want |= 1u << j;
      par ^= (qm >> j) & 1u;
    }
    if (lg_inside16(qm) != want) {
      std::printf("FAILED: lg_inside16(%#x)\n", qm);
      ++g_failed;
      return;
    }
  }
}

static void check_compact() {
  std::unique_ptr<uint8_t[]> in(new uint8_t[16]), got(new uint8_t[16]), want(new uint8_t[16]);
  for (uint32_t j = 0; j < 16; ++j) in[j] = (uint8_t)(0x91u + 7u * j);   // distinct per position, none zero
  uint64_t vlo, vhi;
  std::memcpy(&vlo, in.get(), 8);
  std::memcpy(&vhi, in.get() + 8, 8);
  for (uint32_t keep = 0; keep < 0x10000u; ++keep) {
    std::memset(want.get(), 0, 16);
    uint32_t k = 0;
    for (uint32_t j = 0; j < 16; ++j)
      if ((keep >> j) & 1u) want[k++] = in[j];
    uint64_t clo = ~0ull, chi = ~0ull;
    lg_compact(vlo, vhi, keep, &clo, &chi);
    std::memcpy(got.get(), &clo, 8);
    std::memcpy(got.get() + 8, &chi, 8);
    if (std::memcmp(got.get(), want.get(), 16) != 0) {
      std::printf("FAILED: lg_compact, keep %#x\n", keep);
      ++g_failed;
      return;
    }
  }
  // in place, as lg_place calls it
  uint64_t a = vlo, b = vhi;
  lg_compact(a, b, 0xFF00u, &a, &b);
  CHECK(a == vhi && b == 0);
}

// The chain: lane l hands on its own bit when its vector is not all set, and what it got otherwise.
static void check_carry() {
  for (uint32_t ga = 0; ga < 0x10000u; ++ga) {
    const uint32_t gbs[8] = {0u, 0xFFFFu, next(), next(), next(), next(), ~ga, ga};
    for (uint32_t gb : gbs)
      for (uint32_t carry = 0; carry < 2; ++carry) {
        uint32_t state = carry;
        bool ok = true;
        for (uint32_t l = 0; l < 16; ++l) {
          ok = ok && lg_carry_in(ga, gb & 0xFFFFu, l, carry) == state;
          if ((ga >> l) & 1u) state = (gb >> l) & 1u;
        }
        ok = ok && lg_carry_next(ga, gb & 0xFFFFu, carry) == state;
        if (!ok) {
          std::printf("FAILED: carry hand-off, ga %#x gb %#x carry %u\n", ga, gb & 0xFFFFu, carry);
          ++g_failed;
          return;
        }
      }
  }
}

int main() {
  check_mask16();
  check_inside16();
  check_compact();
  check_carry();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
