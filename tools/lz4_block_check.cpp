// Stand-alone sanitizer check of the host form of the page-sized LZ4 block encoder
// (csrc/lz4_block_host.h: the segment rules, link and merge plan that also run on the device, and
// the scalar segment parser).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/lz4_block_check.cpp alluxio_amd/csrc/cpu_codecs.cpp \
//       -o build/lz4_block_check && build/lz4_block_check
//
// The source, the tables, the scratch buffer and the output are heap allocations of exactly their
// sizes, so an access one byte outside is an AddressSanitizer error.  Bodies of 0, 1, 12, 13, 4095,
// S-1, S, S+1, 2S+1 and 10S+7 bytes (S: the 32 KiB segment; also cut at 16 KiB and 60 KiB) with
// constant, random, random-then-repetitive, repetitive-then-random, period-3, words and CSV-like
// content lie at odd offsets of one source buffer and go through parse, link and merge; every block
// must decode with lz4_decompress_block (cpu_codecs.cpp) to its body, be no larger than LZ4's bound,
// and obey the end rules of the format (the last five bytes literals, which the decoder of the
// reference library insists on).  A constant body of 4 KiB or more must come out under 1 % of its
// size and words and CSV smaller than they went in.  With an output buffer one byte too small the
// merge must refuse the last page and write nothing outside.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cpu_codecs.h"
#include "lz4_block_host.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_failed < 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

template <typename T>
struct Heap {                                         // exactly n elements
  std::unique_ptr<T[]> p;
  uint64_t n;
  explicit Heap(uint64_t n_) : p(new T[n_]()), n(n_) {}
  T* get() const { return p.get(); }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

static const char* kWords[] = {"the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "alluxio", "page",
                               "cache", "tier", "block", "worker", "master", "parquet"};

enum { kConstant, kRandom, kRandomThenRep, kRepThenRandom, kPeriod3, kWordsText, kCsv, kContents };

static std::string content(int kind, uint64_t n, uint64_t segment) {
  std::string s;
  s.reserve(n + 64);
  uint64_t row = 0;
  while (s.size() < n) {
    const uint64_t i = s.size();
    switch (kind) {
      case kConstant: s.push_back('a'); break;
      case kRandom: s.push_back((char)rnd()); break;
      case kRandomThenRep: s.push_back(i < 2 * segment ? (char)rnd() : (char)('a' + i % 7)); break;
      case kRepThenRandom: s.push_back(i + segment < n ? (char)('a' + i % 7) : (char)rnd()); break;
      case kPeriod3: s.push_back("xyz"[i % 3]); break;
      case kWordsText: s += kWords[rnd() % 16]; s.push_back(' '); break;
      default:
        s += std::to_string(row++) + "," + kWords[rnd() % 16] + "," + std::to_string(rnd() % 1000) + ".5\n";
    }
  }
  s.resize(n);
  return s;
}

// The block's sequences, walked as a decoder would: the last one has literals only, and unless the
// block is that one sequence the last match ends at least 5 bytes before the end.
static bool end_rules(const uint8_t* b, uint64_t n, uint64_t body) {
  uint64_t ip = 0, op = 0;
  while (ip < n) {
    const uint32_t tok = b[ip++];
    uint64_t lit = tok >> 4;
    if (lit == 15) {
      uint32_t x;
      do { if (ip >= n) return false; x = b[ip++]; lit += x; } while (x == 255);
    }
    ip += lit;
    op += lit;
    if (ip == n) return op == body;
    if (ip + 2 > n) return false;
    ip += 2;
    uint64_t ml = tok & 15;
    if (ml == 15) {
      uint32_t x;
      do { if (ip >= n) return false; x = b[ip++]; ml += x; } while (x == 255);
    }
    op += ml + 4;
    if (op + kLbLastLiterals > body) return false;
  }
  return false;
}

static void run(uint64_t segment, bool starve) {
  const uint64_t S = kLbSegment;
  const uint64_t sizes[] = {0, 1, 12, 13, 4095, S - 1, S, S + 1, 2 * S + 1, 10 * S + 7};
  std::vector<std::string> bodies;
  std::vector<int> kinds;
  for (uint64_t n : sizes)
    for (int k = 0; k < kContents; ++k) {
      bodies.push_back(content(k, n, S));
      kinds.push_back(k);
    }
  const uint64_t npages = bodies.size();
  uint64_t nsegs = 0, src_bytes = 0;
  for (uint64_t p = 0; p < npages; ++p) {
    nsegs += lb_segments(bodies[p].size(), segment);
    src_bytes += 1 + p % 3 + bodies[p].size();          // a gap of 1 to 3 bytes: every byte phase
  }
  Heap<uint8_t> src(src_bytes);
  Heap<int64_t> pages(npages * kLbPageCols), segs(nsegs * kLbSegCols), result(npages * kLbResCols), dst(npages);
  uint64_t at = 0, s = 0, sc = lb_scratch_head(nsegs);
  for (uint64_t p = 0; p < npages; ++p) {
    at += 1 + p % 3;
    const uint64_t n = bodies[p].size(), k = lb_segments(n, segment);
    std::memcpy(src.get() + at, bodies[p].data(), n);
    int64_t* pg = pages.get() + p * kLbPageCols;
    pg[kLbPageOff] = (int64_t)at;
    pg[kLbPageLen] = (int64_t)n;
    pg[kLbPageSeg] = (int64_t)s;
    pg[kLbPageSegs] = (int64_t)k;
    for (uint64_t i = 0; i < k; ++i, ++s) {
      int64_t* sg = segs.get() + s * kLbSegCols;
      const uint64_t b = i * segment < n ? i * segment : n, e = (i + 1) * segment < n ? (i + 1) * segment : n;
      sg[kLbSegPage] = (int64_t)p;
      sg[kLbSegSrc] = (int64_t)at;
      sg[kLbSegBegin] = (int64_t)b;
      sg[kLbSegEnd] = (int64_t)e;
      sg[kLbSegLast] = i + 1 == k;
      sg[kLbSegScratch] = (int64_t)sc;
      sc += lb_bound(e - b);
    }
    at += n;
  }
  CHECK(at == src_bytes && s == nsegs);
  Heap<uint32_t> scratch((sc + 3) / 4);                 // 4-byte aligned; the last word may be partly unused
  LbArgs a{};
  a.src = src.get();
  a.src_bytes = src_bytes;
  a.pages = pages.get();
  a.npages = npages;
  a.segs = segs.get();
  a.nsegs = nsegs;
  a.scratch = reinterpret_cast<uint8_t*>(scratch.get());
  a.scratch_bytes = sc;
  a.result = result.get();
  a.segment = (uint32_t)segment;
  a.warm = segment + kLbWarm <= 65535 ? kLbWarm : 65535 - (uint32_t)segment;
  for (uint64_t i = 0; i < nsegs; ++i) CHECK(lb_seg_ok(a, segs.get() + i * kLbSegCols));
  lz4_block_parse_host(a);
  lz4_block_link_host(a);
  uint64_t total = 0;
  for (uint64_t p = 0; p < npages; ++p) {
    const int64_t* res = result.get() + p * kLbResCols;
    CHECK(res[kLbStatus] == 0 && res[kLbSize] >= 1 && (uint64_t)res[kLbSize] <= lb_bound(bodies[p].size()));
    CHECK((uint64_t)res[kLbSize] <= lz4_compress_bound(bodies[p].size()));
    dst.get()[p] = (int64_t)total;
    total += (uint64_t)(res[kLbSize] > 0 ? res[kLbSize] : 0);
  }
  if (g_failed) return;
  const uint64_t out_bytes = starve ? total - 1 : total;
  Heap<uint8_t> out(out_bytes);
  a.dst = dst.get();
  a.out = out.get();
  a.out_bytes = out_bytes;
  lz4_block_merge_host(a);
  for (uint64_t p = 0; p < npages; ++p) {
    const int64_t* res = result.get() + p * kLbResCols;
    const uint64_t n = bodies[p].size(), size = (uint64_t)res[kLbSize];
    if (starve && p + 1 == npages) {
      CHECK(res[kLbStatus] == 3);                       // refused, and the sanitizer saw no write outside
      continue;
    }
    CHECK(res[kLbStatus] == 0);
    Heap<uint8_t> back(n);
    const uint8_t* block = out.get() + dst.get()[p];
    CHECK(lz4_decompress_block(block, size, back.get(), n) == (int64_t)n);
    CHECK(std::memcmp(back.get(), bodies[p].data(), n) == 0);
    CHECK(end_rules(block, size, n));
    if (n == 0) CHECK(size == 1 && block[0] == 0);
    if (kinds[p] == kConstant && n >= 4096) CHECK(size * 100 < n);
    if ((kinds[p] == kWordsText || kinds[p] == kCsv) && n >= 4095) CHECK(size < n);
  }
}

int main() {
  run(kLbSegment, false);
  run(kLbSegment, true);
  run(16 * 1024, false);
  run(60 * 1024, false);
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
