// Stand-alone sanitizer check of the host form of the Parquet passes (csrc/parquet_host.h, the code
// that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/parquet_host_check.cpp -o build/parquet_host_check \
//       && build/parquet_host_check
//
// Every data buffer is a heap allocation of exactly data_bytes, so a read one byte outside it is an
// AddressSanitizer error, and every output is an exact allocation too.  The inputs are valid page
// headers (V1, V2, dictionary, with statistics), hybrid streams and byte-array pages written here,
// each of them cut at every length, and hostile ones: lengths, counts and nesting that lie, and
// pseudo-random bytes.  The serial decode and the run-table form must agree on every stream.  Exit
// status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parquet_host.h"

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

static std::string varint(uint64_t v) {
  std::string s;
  while (v >= 0x80) {
    s.push_back((char)((v & 0x7F) | 0x80));
    v >>= 7;
  }
  s.push_back((char)v);
  return s;
}
static std::string zz(int64_t v) { return varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
static std::string le32(uint32_t v) {
  std::string s(4, '\0');
  for (int i = 0; i < 4; ++i) s[i] = (char)(v >> (8 * i));
  return s;
}

// Statistics{max, min, null_count, distinct_count, max_value, min_value}: binaries of `n` bytes.
static std::string stats(size_t n) {
  const std::string b = varint(n) + std::string(n, 's');
  return "\x18" + b + "\x18" + b + "\x16" + zz(3) + "\x16" + zz(9) + "\x18" + b + "\x18" + b + std::string(1, '\0');
}
static std::string header_v1(int64_t unc, int64_t comp, int64_t nv, size_t stat) {
  std::string h = "\x15" + zz(0) + "\x15" + zz(unc) + "\x15" + zz(comp) + "\x15" + zz(77);          // with a crc
  h += "\x1c\x15" + zz(nv) + "\x15" + zz(0) + "\x15" + zz(3) + "\x15" + zz(3);
  if (stat) h += "\x1c" + stats(stat);
  return h + std::string(2, '\0');
}
static std::string header_dict(int64_t unc, int64_t comp, int64_t nv) {
  return "\x15" + zz(2) + "\x15" + zz(unc) + "\x15" + zz(comp) + "\x4c\x15" + zz(nv) + "\x15" + zz(2) + "\x11" +
         std::string(2, '\0');
}
static std::string header_v2(int64_t unc, int64_t comp, int64_t nv, int64_t nulls, int64_t dl, bool packed, size_t stat) {
  std::string h = "\x15" + zz(3) + "\x15" + zz(unc) + "\x15" + zz(comp);
  h += "\x5c\x15" + zz(nv) + "\x15" + zz(nulls) + "\x15" + zz(nv) + "\x15" + zz(8) + "\x15" + zz(dl) + "\x15" + zz(0);
  h += packed ? "\x11" : "\x12";
  if (stat) h += "\x1c" + stats(stat);
  return h + std::string(2, '\0');
}

struct Walk {
  std::vector<int64_t> table;
  int32_t count = -1, err = -1;
};

// One chunk that is the whole of `bytes` after `lead` bytes: count, then fill into an exact table.
static Walk walk(const std::string& bytes, size_t lead = 0, int64_t len_override = -1, uint64_t cap_rows = ~0ull) {
  Heap data(std::string(lead, '\x15') + bytes);
  int64_t off = (int64_t)lead, len = len_override >= 0 ? len_override : (int64_t)bytes.size();
  Walk w;
  PqWalkArgs a{};
  a.data = data.p.get();
  a.data_bytes = data.n;
  a.chunk_off = &off;
  a.chunk_len = &len;
  a.nchunks = 1;
  a.counts = &w.count;
  a.errors = &w.err;
  parquet_walk_host(a);
  const uint64_t rows = cap_rows == ~0ull ? (uint64_t)w.count : cap_rows;
  std::unique_ptr<int64_t[]> table(new int64_t[rows * kPqCols + 0]);
  int64_t base[2] = {0, w.count};
  int32_t c2 = -1, e2 = -1;
  a.counts = &c2;
  a.errors = &e2;
  a.page_base = base;
  a.table = rows ? table.get() : nullptr;
  a.table_rows = rows;
  if (rows) parquet_walk_host(a);
  if (rows) CHECK(c2 == w.count && e2 == w.err);
  w.table.assign(table.get(), table.get() + rows * kPqCols);
  return w;
}

static void check_walk() {
  const std::string p1 = header_v1(40, 40, 10, 300) + std::string(40, 'p');
  const std::string pd = header_dict(16, 16, 4) + std::string(16, 'd');
  const std::string p2 = header_v2(30, 30, 9, 2, 5, false, 7) + std::string(30, 'q');
  const std::string idx = "\x15" + zz(1) + "\x15" + zz(3) + "\x15" + zz(3) + std::string(1, '\0') + "iii";
  const std::string chunk = pd + p1 + idx + p2 + header_v1(0, 0, 0, 0);
  Walk w = walk(chunk, 5);
  CHECK(w.err == kPqOk && w.count == 4);
  if (w.count == 4) {
    const int64_t* t = w.table.data();
    CHECK(t[kPqType] == 2 && t[kPqNumValues] == 4 && t[kPqEncoding] == 2 && t[kPqCompressed] == 16);
    CHECK(t[kPqPayload] == 5 + (int64_t)(pd.size() - 16));
    t += kPqCols;
    CHECK(t[kPqType] == 0 && t[kPqNumValues] == 10 && t[kPqEncoding] == 0 && t[kPqDefEncoding] == 3 && t[kPqNumNulls] == -1);
    CHECK(t[kPqPayload] == 5 + (int64_t)(pd.size() + p1.size() - 40));
    t += kPqCols;
    CHECK(t[kPqType] == 3 && t[kPqNumValues] == 9 && t[kPqNumNulls] == 2 && t[kPqDefLen] == 5 && t[kPqRepLen] == 0 &&
          t[kPqIsCompressed] == 0 && t[kPqEncoding] == 8 && t[kPqChunk] == 0);
    t += kPqCols;
    CHECK(t[kPqType] == 0 && t[kPqCompressed] == 0);
  }
  // cut at every length: never a read outside, always an error unless the cut falls between pages
  for (size_t cut = 0; cut < chunk.size(); ++cut) {
    Walk c = walk(chunk.substr(0, cut), cut % 3);
    const bool between = cut == 0 || cut == pd.size() || cut == pd.size() + p1.size() ||
                         cut == pd.size() + p1.size() + idx.size() || cut == pd.size() + p1.size() + idx.size() + p2.size();
    CHECK((c.err == kPqOk) == between);
    CHECK(c.err == kPqOk || c.err == kPqErrHeader || c.err == kPqErrPayload);
    CHECK(c.count <= 3);
  }
  // a table with fewer rows than pages; a chunk longer than the buffer; negative numbers
  CHECK(walk(chunk, 0, -1, 2).table.size() == 2 * kPqCols);
  CHECK(walk(chunk, 0, (int64_t)chunk.size() + 1).err == kPqErrChunk);
  CHECK(walk(header_v1(-1, 4, 1, 0) + "abcd").err == kPqErrSize);
  CHECK(walk(header_v1(4, -4, 1, 0) + "abcd").err == kPqErrSize);
  CHECK(walk(header_v1(4, 4, -1, 0) + "abcd").err == kPqErrSize);
  CHECK(walk(header_v1(4, 5, 1, 0) + "abcd").err == kPqErrPayload);
  CHECK(walk(header_v2(4, 4, 1, 0, 5, true, 0) + "abcd").err == kPqErrSize);       // levels longer than the page
  CHECK(walk("\x15" + zz(6) + "\x15" + zz(0) + "\x15" + zz(0) + std::string(1, '\0')).err == kPqErrPageType);
  CHECK(walk(std::string("\x15\x00\x15\x00\x15\x00\x19\xff\xff\xff\xff\x0f\x00", 13)).err == kPqErrHeader);   // a list of 2^32
  CHECK(walk(std::string("\x15\x00\x15\x00\x15\x00\x18\xff\xff\xff\xff\xff\xff\xff\xff\xff\x01zz", 19)).err == kPqErrHeader);
  CHECK(walk("\x15" + zz(0) + "\x15" + zz(0) + "\x15" + zz(0) + std::string(12, '\x1c') + std::string(13, '\0')).err ==
        kPqErrHeader);                              // nested deeper than the skip stack
  CHECK(walk("\x15" + zz(0) + "\x15" + zz(0) + "\x15" + zz(0) + std::string(7, '\x1c') + std::string(8, '\0')).err == kPqOk);
  CHECK(walk("\x15" + zz(0) + "\x15" + zz(0) + "\x15" + zz(0) + "\x1b\x02\x88" "\x01" "a\x01" "b\x01" "c\x01" "d" + std::string(1, '\0')).err ==
        kPqOk);                                     // a map of two binaries each way
  for (int i = 0; i < 4000; ++i) {                  // noise: any outcome, no access outside
    std::string s(rnd() % 60, '\0');
    for (auto& ch : s) ch = (char)(rnd() % 7 ? rnd() % 0x30 : rnd());
    Walk r = walk(s, rnd() % 4);
    CHECK(r.err >= 0 && r.err <= kPqErrChunk);
  }
}

struct Decoded {
  std::vector<int32_t> out;
  int32_t err = -1;
};

// One stream over an exact buffer, serially and through the run table; both must agree.
static Decoded decode(const std::string& bytes, int64_t kind, int64_t skip, int64_t width, int64_t n, uint64_t out_n,
                      int64_t off = 0, int64_t len = -1) {
  Heap data(bytes);
  int64_t row[kPqStreamCols] = {off, len < 0 ? (int64_t)bytes.size() : len, kind, skip, width, n, 1, 0};
  Decoded d[2];
  for (int form = 0; form < 2; ++form) {
    std::unique_ptr<int32_t[]> out(new int32_t[out_n]);
    for (uint64_t i = 0; i < out_n; ++i) out[i] = -7;
    PqStreamArgs a{};
    a.data = data.p.get();
    a.data_bytes = data.n;
    a.streams = row;
    a.nstreams = 1;
    a.out = out.get();
    a.out_n = out_n;
    a.errors = &d[form].err;
    if (form == 0) {
      parquet_hybrid_host(a);
    } else {
      int32_t runs_n = -1;
      a.run_counts = &runs_n;
      pq_stream_runs(a, 0);
      std::unique_ptr<int64_t[]> runs(new int64_t[(size_t)runs_n * 4 + 0]);
      int64_t base[2] = {0, runs_n};
      a.run_base = base;
      a.runs = runs.get();
      a.runs_rows = (uint64_t)runs_n;
      if (runs_n) pq_stream_runs(a, 0);
      for (uint64_t t = 0; t < out_n; ++t) pq_stream_value(a, t);
    }
    d[form].out.assign(out.get(), out.get() + out_n);
  }
  CHECK(d[0].err == d[1].err && d[0].out == d[1].out);
  return d[0];
}

static std::string pack(const std::vector<uint32_t>& v, uint32_t bw) {       // whole groups of 8
  std::string s((v.size() / 8) * bw, '\0');
  for (size_t k = 0; k < v.size(); ++k)
    for (uint32_t b = 0; b < bw; ++b)
      if ((v[k] >> b) & 1) s[(k * bw + b) / 8] |= (char)(1 << ((k * bw + b) % 8));
  return s;
}

static void check_hybrid() {
  for (uint32_t bw : {0u, 1u, 2u, 3u, 5u, 8u, 11u, 16u, 17u, 24u, 31u, 32u}) {
    const uint32_t top = bw == 32 ? 0xFFFFFFFFu : (1u << bw) - 1u;
    std::vector<uint32_t> vals, grp;
    std::string s = varint(5 << 1);                 // five times `top`
    for (uint32_t i = 0; i < (bw + 7) / 8; ++i) s.push_back((char)(top >> (8 * i)));
    for (int i = 0; i < 5; ++i) vals.push_back(top);
    for (int i = 0; i < 24; ++i) grp.push_back(rnd() & top);
    s += varint((3 << 1) | 1) + pack(grp, bw);
    vals.insert(vals.end(), grp.begin(), grp.end());
    std::vector<uint32_t> one(8, top);              // a single group of which 3 values count
    one[0] = 0;
    s += varint((1 << 1) | 1) + pack(one, bw);
    for (int i = 0; i < 3; ++i) vals.push_back(one[i]);
    const int64_t n = (int64_t)vals.size();
    Decoded d = decode(s, 0, 0, bw, n, (uint64_t)n + 2);
    CHECK(d.err == 0 && d.out.front() == -7 && d.out.back() == -7);
    for (int64_t i = 0; i < n; ++i) CHECK((uint32_t)d.out[1 + i] == vals[i]);
    // behind a length prefix, behind a width byte after a skipped block
    d = decode(le32((uint32_t)s.size()) + s + "junk", 1, 0, bw, n, (uint64_t)n + 2);
    CHECK(d.err == 0 && (uint32_t)d.out[n] == vals[n - 1]);
    d = decode(le32(3) + "abc" + std::string(1, (char)bw) + s, 2, 1, 0, n, (uint64_t)n + 2);
    CHECK(d.err == 0 && (uint32_t)d.out[n] == vals[n - 1]);
    // cut at every length; one value more than the runs hold; an output shorter than the values
    for (size_t cut = 0; cut < s.size(); ++cut) {
      d = decode(s.substr(0, cut), 0, 0, bw, n, (uint64_t)n + 2);
      CHECK(d.err == kPqErrRun || (bw == 0 && d.err == 0));
      CHECK(d.out.front() == -7 && d.out.back() == -7);
    }
    CHECK(decode(s, 0, 0, bw, n + 6, (uint64_t)n + 8).err == kPqErrRun);
    CHECK(decode(s, 0, 0, bw, n + 5, (uint64_t)n + 7).err == 0);          // the padding of the last group is there to read
    CHECK(decode(s, 0, 0, bw, n, 4).out[3] == (int32_t)top);
  }
  CHECK(decode(le32(9) + "ab", 1, 0, 1, 4, 8).err == kPqErrStream);
  CHECK(decode("ab", 1, 0, 1, 4, 8).err == kPqErrStream);
  CHECK(decode(le32(90) + "ab", 0, 1, 1, 4, 8).err == kPqErrStream);
  CHECK(decode(std::string(1, '\x21') + "ab", 2, 0, 0, 4, 8).err == kPqErrStream);
  CHECK(decode("ab", 0, 0, 33, 4, 8).err == kPqErrStream);
  CHECK(decode("ab", 7, 0, 1, 4, 8).err == kPqErrStream);
  CHECK(decode("ab", 0, 0, 1, 4, 8, 1, 2).err == kPqErrStream);
  CHECK(decode("ab", 0, 0, 1, 4, 8, -1, 2).err == kPqErrStream);
  CHECK(decode(varint(((1ull << 62) << 1) | 1), 0, 0, 0, 6, 8).err == 0);
  CHECK(decode(varint(((1ull << 62) << 1) | 1) + "abcdefgh", 0, 0, 1, 6, 8).err == kPqErrRun);
  CHECK(decode(std::string(11, '\xff'), 0, 0, 1, 6, 8).err == kPqErrRun);
  for (int i = 0; i < 4000; ++i) {
    std::string s(rnd() % 40, '\0');
    for (auto& ch : s) ch = (char)(rnd() % 3 ? rnd() % 8 : rnd());
    Decoded d = decode(s, rnd() % 3, rnd() % 2, rnd() % 34, rnd() % 70, 64);
    CHECK(d.err == 0 || d.err == kPqErrStream || d.err == kPqErrRun);
    CHECK(d.out[0] == -7);
  }
}

static void check_place_and_bytes() {
  // a byte-array page: lengths 0, 1, 17, then a negative one; and one that runs past the page
  const std::string good = le32(0) + le32(1) + "a" + le32(17) + std::string(17, 'b');
  for (int hostile = 0; hostile < 3; ++hostile) {
    const std::string page = good + (hostile == 1 ? le32(0xFFFFFFF0u) + "cccc" : hostile == 2 ? le32(5) + "cccc" : le32(4) + "cccc");
    for (size_t cut = 0; cut <= page.size(); ++cut) {
      Heap data(page.substr(0, cut));
      int64_t pg[kPqPageCols] = {0, 4, 0, 0, (int64_t)cut, 0, 0, -1, -1, 0};
      std::unique_ptr<int64_t[]> start(new int64_t[4]);
      std::unique_ptr<int32_t[]> length(new int32_t[4]);
      std::unique_ptr<uint8_t[]> status(new uint8_t[4]);
      PqBytesArgs a{};
      a.data = data.p.get();
      a.data_bytes = data.n;
      a.pages = pg;
      a.npages = 1;
      a.rows = 4;
      a.start = start.get();
      a.length = length.get();
      a.status = status.get();
      a.nvalues = 4;
      parquet_bytes_host(a);
      bool bad = false;
      for (int k = 0; k < 4; ++k) {
        if (status[k] != 0) bad = true;
        CHECK(bad ? (status[k] == 2 && length[k] == 0) : (start[k] >= 0 && (uint64_t)(start[k] + length[k]) <= cut));
      }
      if (cut == page.size()) CHECK(bad == (hostile != 0) && status[2] == 0 && length[2] == 17);
      // the same page read as PLAIN values of 8 bytes behind a level block that may lie about its length
      std::unique_ptr<uint8_t[]> values(new uint8_t[5 * 8]);
      std::unique_ptr<uint8_t[]> st(new uint8_t[5]);
      int64_t pp[kPqPageCols] = {0, 5, 0, 0, (int64_t)cut, 1, 0, -1, -1, 0};
      PqPlaceArgs p{};
      p.data = data.p.get();
      p.data_bytes = data.n;
      p.pages = pp;
      p.npages = 1;
      p.width = 8;
      p.values = values.get();
      p.status = st.get();
      p.rows = 5;
      parquet_place_host(p);
      for (int r = 0; r < 5; ++r) CHECK(st[r] == 0 || st[r] == 2);
      p.width = 1;
      p.is_bool = 1;
      parquet_place_host(p);
    }
  }
  // dictionary indices out of range, an index array shorter than the rows
  Heap data(std::string(8, 'x'));
  const int32_t idx[4] = {0, 2, 3, -1};
  const uint8_t dict[12] = {1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0};
  int64_t pp[kPqPageCols] = {0, 6, 1, 0, 0, 0, 0, -1, -1, 0};
  std::unique_ptr<uint8_t[]> values(new uint8_t[6 * 4]);
  std::unique_ptr<uint8_t[]> st(new uint8_t[6]);
  PqPlaceArgs p{};
  p.data = data.p.get();
  p.data_bytes = data.n;
  p.pages = pp;
  p.npages = 1;
  p.idx = idx;
  p.idx_n = 4;
  p.dict = dict;
  p.dict_size = 3;
  p.width = 4;
  p.values = values.get();
  p.status = st.get();
  p.rows = 6;
  parquet_place_host(p);
  CHECK(st[0] == 0 && st[1] == 0 && st[2] == 2 && st[3] == 2 && st[4] == 2 && st[5] == 2);
  CHECK(values[0] == 1 && values[4] == 3 && values[8] == 0);
  // an LZ4 plan over pages that lie about their sizes
  int64_t table[2 * kPqCols] = {0, 2, 6, 40, 1, 0, 0, 0, -1, 1, 0, 3, 3, 4, 8, 8, 1, 0, 9, 9, 0, 1, 0, 3};
  int64_t dst[2] = {0, 40};
  std::unique_ptr<uint8_t[]> out(new uint8_t[48]);
  PqLz4Chunk chunks[2];
  int32_t expect[2];
  PqLz4Args l{};
  l.data = data.p.get();
  l.data_bytes = data.n;
  l.table = table;
  l.npages = 2;
  l.dst_off = dst;
  l.out = out.get();
  l.out_bytes = 48;
  l.chunks = chunks;
  l.expect = expect;
  parquet_lz4_plan_host(l);
  CHECK(expect[0] == 40 && chunks[0].src_bytes == 6 && expect[1] == -1 && chunks[1].src_bytes == 0);
}

int main() {
  check_walk();
  check_hybrid();
  check_place_and_bytes();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
