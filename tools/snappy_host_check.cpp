// Stand-alone sanitizer check of the host form of the Snappy raw decoder (csrc/snappy_host.h: the
// header rules that also run on the device, and the decode loop).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/snappy_host_check.cpp \
//       -o build/snappy_host_check && build/snappy_host_check
//
// Every stream and every output is a heap allocation of exactly its size, so an access one byte
// outside is an AddressSanitizer error.  Well-formed streams are built element by element next to
// the bytes they must give (byte i of a copy is out[op - offset + i % offset]): all four kinds, the
// literal tags 60..63 with 1..4 length bytes, a 70,000-byte literal, kind 3 with a small and a
// large offset, overlapping copies of 64 bytes at offsets 1, 2, 3, 7 and 63, a copy that reaches
// byte 0, a copy of one byte, the empty stream, and 2,000 random sequences of elements.  Malformed
// streams (offset 0, an offset one past the output, a copy and a literal one byte past the
// capacity, a literal and a header cut short, a stream one byte short of its preamble, a preamble
// that is not the capacity, a 6-byte preamble, a preamble above 2^31-1, no bytes at all) must give a
// negative code, and so must every prefix of a well-formed stream; 20,000 streams of random bytes
// must give the capacity or a negative code.  Exit status 0 and "ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cpu_codecs.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_failed < 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

struct Builder {                                      // the elements (without preamble) and what they give
  std::string body, out;
  void literal(const std::string& s, int len_bytes = 0) {   // len_bytes 0: the shortest form
    const uint32_t m = (uint32_t)s.size() - 1;
    if (len_bytes == 0) len_bytes = m < 60 ? -1 : (m < 256 ? 1 : (m < 65536 ? 2 : (m < (1u << 24) ? 3 : 4)));
    if (len_bytes < 0) {
      body += (char)(m << 2);
    } else {
      body += (char)((59 + len_bytes) << 2);
      for (int i = 0; i < len_bytes; ++i) body += (char)((m >> (8 * i)) & 255);
    }
    body += s;
    out += s;
  }
  void random_literal(uint32_t n, int len_bytes = 0) {
    std::string s(n, '\0');
    for (auto& c : s) c = (char)rnd();
    literal(s, len_bytes);
  }
  void copy(int kind, uint32_t len, uint32_t off, bool apply = true) {
    if (kind == 1) {
      body += (char)(1 | ((len - 4) << 2) | ((off >> 8) << 5));
      body += (char)(off & 255);
    } else {
      body += (char)(kind | ((len - 1) << 2));
      for (int i = 0; i < (kind == 2 ? 2 : 4); ++i) body += (char)((off >> (8 * i)) & 255);
    }
    if (apply) {
      const size_t op = out.size();
      for (uint32_t i = 0; i < len; ++i) out += out[op - off + i % off];
    }
  }
  std::string stream(int64_t preamble = -1) const {
    uint64_t v = preamble < 0 ? out.size() : (uint64_t)preamble;
    std::string s;
    while (v >= 128) {
      s += (char)(128 | (v & 127));
      v >>= 7;
    }
    s += (char)v;
    return s + body;
  }
};

// The decoder on exactly sized heap buffers; the bytes come back in *got.
static int64_t run(const std::string& stream, uint64_t cap, std::string* got = nullptr) {
  std::unique_ptr<uint8_t[]> src(new uint8_t[stream.size()]), dst(new uint8_t[cap]);
  std::memcpy(src.get(), stream.data(), stream.size());
  std::memset(dst.get(), 0xEE, cap);
  const int64_t r = snappy_decompress_block(src.get(), stream.size(), dst.get(), cap);
  if (got) got->assign((const char*)dst.get(), cap);
  return r;
}

static void good(const Builder& b) {
  std::string got;
  const std::string s = b.stream();
  CHECK(run(s, b.out.size(), &got) == (int64_t)b.out.size());
  CHECK(got == b.out);
  for (size_t cut = 0; cut < s.size() && cut < 200; ++cut) CHECK(run(s.substr(0, cut), b.out.size()) < 0);
  if (s.size() > 200) CHECK(run(s.substr(0, s.size() - 1), b.out.size()) < 0);
  CHECK(run(s, b.out.size() + 1) == kSnLength);
  if (!b.out.empty()) CHECK(run(s, b.out.size() - 1) == kSnLength);
}

int main() {
  {
    Builder b;                                        // the empty stream
    good(b);
    CHECK(b.stream() == std::string(1, '\0'));
  }
  {
    Builder b;                                        // all four kinds
    b.literal("abcdefghijklmnop");
    b.copy(1, 7, 5);
    b.copy(2, 33, 16);
    b.copy(3, 64, 23);
    b.literal("z");
    good(b);
  }
  for (int lb = 1; lb <= 4; ++lb) {                   // tags 60..63
    Builder b;
    b.random_literal(lb == 3 ? 70000 : 61 + lb, lb);
    b.copy(2, 10, 3);
    good(b);
  }
  {
    Builder b;                                        // kind 3, small and large offsets; a copy to byte 0
    b.random_literal(70000);
    b.copy(3, 64, 9);
    b.copy(3, 50, 66000);
    b.copy(3, 64, (uint32_t)b.out.size());
    b.copy(2, 1, 1);
    good(b);
  }
  for (uint32_t off : {1u, 2u, 3u, 7u, 63u}) {          // overlapping copies
    Builder b;
    b.random_literal(off);
    b.copy(2, 64, off);
    b.copy(2, 64, off);
    b.copy(1, 11, off);
    good(b);
  }
  for (int round = 0; round < 2000; ++round) {        // random sequences
    Builder b;
    const uint32_t elements = 1 + rnd() % 40;
    for (uint32_t e = 0; e < elements; ++e) {
      const uint32_t k = b.out.empty() ? 0 : rnd() % 4;
      if (k == 0) {
        const uint32_t len = 1 + rnd() % (rnd() % 8 ? 70 : 700);
        b.random_literal(len, rnd() % 3 ? 0 : (len > 256 ? 2 : 1) + rnd() % 3);   // also longer forms than needed
      } else {
        const uint32_t max_off = (uint32_t)std::min<size_t>(b.out.size(), k == 1 ? 2047 : 65535);
        const uint32_t off = 1 + rnd() % max_off;
        b.copy((int)k, k == 1 ? 4 + rnd() % 8 : 1 + rnd() % 64, off);
      }
    }
    good(b);
  }
  // malformed
  auto refused = [](const Builder& b, uint64_t cap, int64_t preamble = -1) { return run(b.stream(preamble), cap) < 0; };
  {
    Builder b;
    b.literal("abcd");
    b.copy(2, 4, 0, false);
    CHECK(run(b.stream(8), 8) == kSnOffset);
  }
  {
    Builder b;
    b.literal("abcd");
    b.copy(2, 4, 5, false);
    CHECK(run(b.stream(8), 8) == kSnOffset);
  }
  {
    Builder b;                                        // a copy one byte past the capacity
    b.literal("abcd");
    b.copy(2, 5, 4, false);
    CHECK(run(b.stream(8), 8) == kSnOutput);
  }
  {
    Builder b;                                        // a literal one byte past the capacity
    b.literal("abcde");
    CHECK(run(b.stream(4), 4) == kSnOutput);
  }
  {
    Builder b;                                        // a literal cut short
    b.literal("abcdefgh");
    std::string s = b.stream();
    CHECK(run(s.substr(0, s.size() - 1), 8) == kSnInput);
  }
  for (int kind = 1; kind <= 3; ++kind) {             // a header cut short
    Builder b;
    b.literal("abcdefgh");
    b.copy(kind, 4, 2, false);
    std::string s = b.stream(12);
    CHECK(run(s.substr(0, s.size() - 1), 12) == kSnInput);
  }
  {
    Builder b;                                        // one byte short of the preamble
    b.literal("abcdefgh");
    CHECK(run(b.stream(9), 9) == kSnShort);
    CHECK(refused(b, 7, 7));
  }
  {
    Builder b;
    b.literal("abcd");
    CHECK(run(std::string("\x84\x80\x80\x80\x80\x00", 6) + b.body, 4) == kSnPreamble);   // six bytes
    CHECK(run(std::string("\x84\x80\x80\x80\x10", 5) + b.body, 4) == kSnPreamble);       // above 2^31-1
    CHECK(run(std::string("\x84\x80\x80\x80\x00", 5) + b.body, 4) == 4);                 // five bytes, padded: fine
    CHECK(run(std::string(), 0) == kSnPreamble);
    CHECK(run(std::string("\x84", 1), 4) == kSnPreamble);
    CHECK(run(std::string("\xFC\xFF\xFF\xFF\xFF", 5), 0) < 0);
    // a literal of 2^32 bytes
    CHECK(run(std::string("\x04\xFC\xFF\xFF\xFF\xFF", 6) + "abcd", 4) < 0);
  }
  for (int round = 0; round < 20000; ++round) {       // random bytes behind a true preamble
    const uint32_t cap = rnd() % 300, n = rnd() % 64;
    Builder b;
    for (uint32_t i = 0; i < n; ++i) b.body += (char)(rnd() % 5 ? rnd() : (rnd() % 4) << 2 | (rnd() & 3));
    const int64_t r = run(b.stream(cap), cap);
    CHECK(r < 0 || r == (int64_t)cap);
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
