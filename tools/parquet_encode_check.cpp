// Stand-alone sanitizer check of the host form of the Parquet encode passes
// (csrc/parquet_encode_host.h, the code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/parquet_encode_check.cpp -o build/parquet_encode_check \
//       && build/parquet_encode_check
//
// Every column array, flat array and row-group buffer is a heap allocation of exactly its size, so
// an access one byte outside is an AddressSanitizer error.  For row counts 1, 7, 8, 9, 63, 64, 65
// and 1000, pages of 64 and 100 rows and of the whole chunk, five null patterns (none, all, the
// first row of a page, the last row of a page, scattered) and dictionaries of 1, 2, 3, 256 and 257
// entries, one column of every kind is measured, ranked, laid out and emitted, and each page is
// decoded again with the loops of parquet_host.h: the levels, the values of the valid rows, the
// text bytes and the dictionary indices must come back.  A buffer that is too small must not be
// written outside.  Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "parquet_encode_host.h"

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
  int64_t addr() const { return (int64_t)(uintptr_t)p.get(); }
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
static std::string le32(uint32_t v) {
  std::string s(4, '\0');
  for (int i = 0; i < 4; ++i) s[i] = (char)(v >> (8 * i));
  return s;
}

static bool is_null(int pattern, uint64_t i, uint64_t page_rows) {
  switch (pattern) {
    case 0: return false;
    case 1: return true;
    case 2: return i % page_rows == 0;
    case 3: return i % page_rows == page_rows - 1;
    default: return rnd() % 3 == 0;
  }
}

// One column of `rows` rows as one chunk of pages of `page_rows`: measured, laid out as a writer
// would (a stand-in header of `phase` bytes before each page moves the byte phase), emitted and
// decoded again.  kind: kPe*; width: bytes (fixed) or dictionary entries (index).
static void run(int kind, uint64_t width, uint64_t rows, uint64_t page_rows, int pattern, uint64_t phase, bool starve) {
  const uint64_t dict_n = kind == kPeIndex ? width : 0;
  const uint64_t vw = kind == kPeFixed ? width : kind == kPeIndex ? 4 : 1;
  Heap<uint8_t> status(rows), values(kind == kPeText ? 0 : rows * vw);
  Heap<int64_t> offsets(kind == kPeText ? rows + 1 : 0);
  std::string text;
  std::vector<std::string> strings(rows);
  for (uint64_t i = 0; i < rows; ++i) {
    const bool null = is_null(pattern, i, page_rows);
    status.get()[i] = null ? 1 : 0;
    if (kind == kPeText) {
      offsets.get()[i] = (int64_t)text.size();
      if (!null && pattern != 3) {                    // pattern 3: every value is empty
        const uint32_t len = rnd() % 41;
        for (uint32_t j = 0; j < len; ++j) strings[i].push_back((char)rnd());
        text += strings[i];
      }
    } else if (kind == kPeIndex) {
      const int32_t code = null ? -1 : (int32_t)(i % 3 == 0 ? dict_n - 1 : rnd() % dict_n);
      std::memcpy(values.get() + i * 4, &code, 4);
    } else if (kind == kPeBool) {
      values.get()[i] = null ? 0 : (uint8_t)(rnd() & 1);
    } else {
      for (uint64_t j = 0; j < vw; ++j) values.get()[i * vw + j] = null ? 0 : (i % 5 == 0 ? 0xFF : (uint8_t)rnd());
    }
  }
  if (kind == kPeText) offsets.get()[rows] = (int64_t)text.size();
  Heap<uint8_t> data(text.size());
  std::memcpy(data.get(), text.data(), text.size());

  const uint64_t npages = (rows + page_rows - 1) / page_rows;
  Heap<int64_t> table(npages * kPeCols), measure(npages * kPmCols);
  for (uint64_t p = 0; p < npages; ++p) {
    int64_t* pg = table.get() + p * kPeCols;
    pg[kPeKind] = kind;
    pg[kPeWidth] = kind == kPeFixed ? (int64_t)width : 1;
    pg[kPeValues] = kind == kPeText ? data.addr() : values.addr();
    pg[kPeStatus] = status.addr();
    pg[kPeOffsets] = kind == kPeText ? offsets.addr() : 0;
    pg[kPeAux] = kind == kPeText ? (int64_t)text.size() : (int64_t)dict_n;
    pg[kPeRow] = (int64_t)(p * page_rows);
    pg[kPeRows] = (int64_t)(rows - p * page_rows < page_rows ? rows - p * page_rows : page_rows);
    pg[kPeFlat] = pg[kPeRow];
    pg[kPeLevelOff] = -1;
    measure.get()[p * kPmCols + kPmMaxCode] = -1;
  }
  Heap<uint8_t> flags(rows);
  Heap<int32_t> text_bytes(kind == kPeText ? rows : 0), scratch(rows);
  PeArgs a{};
  a.pages = table.get();
  a.npages = npages;
  a.first = 0;
  a.last = npages;
  a.flags = flags.get();
  a.text_bytes = kind == kPeText ? text_bytes.get() : nullptr;
  a.flat_n = rows;
  a.measure = measure.get();
  parquet_encode_measure_host(a);
  Heap<int64_t> rank(rows + 1), text_at(rows + 1);
  for (uint64_t i = 0; i < rows; ++i) {
    rank.get()[i + 1] = rank.get()[i] + flags.get()[i];
    text_at.get()[i + 1] = text_at.get()[i] + (kind == kPeText ? text_bytes.get()[i] : 0);
    CHECK(flags.get()[i] == (status.get()[i] == 0));
  }
  // layout
  int64_t top = -1;
  for (uint64_t p = 0; p < npages; ++p) {
    const int64_t code = measure.get()[p * kPmCols + kPmMaxCode];
    top = code > top ? code : top;
  }
  uint32_t bits = 1;
  while (top > 0 && (1ll << bits) <= top) ++bits;
  std::string blob;
  std::vector<int64_t> segs;
  std::vector<uint64_t> body_at(npages), body_len(npages);
  uint64_t pos = 0;
  for (uint64_t p = 0; p < npages; ++p) {
    int64_t* pg = table.get() + p * kPeCols;
    const int64_t* m = measure.get() + p * kPmCols;
    const uint64_t prow = (uint64_t)pg[kPeRows], valid = (uint64_t)m[kPmValid];
    CHECK(m[kPmBad] == 0 && m[kPmOutside] == 0);
    CHECK(valid == (uint64_t)(rank.get()[pg[kPeRow] + prow] - rank.get()[pg[kPeRow]]));
    std::string head(phase, 'H'), pre;
    uint64_t lev_bits = 0;
    if (valid == prow) {
      const std::string runs = varint(prow << 1) + std::string(1, '\x01');
      head += le32((uint32_t)runs.size()) + runs;
    } else {
      lev_bits = (prow + 7) / 8;
      const std::string runs = varint((lev_bits << 1) | 1);
      head += le32((uint32_t)(runs.size() + lev_bits)) + runs;
    }
    uint64_t vb = 0;
    if (kind == kPeFixed) vb = valid * width;
    else if (kind == kPeBool) vb = (valid + 7) / 8;
    else if (kind == kPeText) vb = (uint64_t)m[kPmTextBytes];
    else {
      const uint64_t groups = (valid + 7) / 8;
      pre = std::string(1, (char)bits) + (valid ? varint((groups << 1) | 1) : std::string());
      vb = groups * bits;
      pg[kPeWidth] = bits;
    }
    segs.insert(segs.end(), {(int64_t)blob.size(), (int64_t)pos, (int64_t)head.size()});
    blob += head;
    body_at[p] = pos + phase;
    pos += head.size();
    pg[kPeLevelOff] = lev_bits ? (int64_t)pos : -1;
    pos += lev_bits;
    if (!pre.empty()) {
      segs.insert(segs.end(), {(int64_t)blob.size(), (int64_t)pos, (int64_t)pre.size()});
      blob += pre;
      pos += pre.size();
    }
    pg[kPeValOff] = (int64_t)pos;
    pg[kPeValBytes] = (int64_t)vb;
    pg[kPeNumValid] = (int64_t)valid;
    pos += vb;
    body_len[p] = pos - body_at[p];
  }
  const uint64_t out_bytes = starve ? pos / 2 : pos;
  Heap<uint8_t> out(out_bytes), hblob(blob.size());
  Heap<int64_t> hsegs(segs.size());
  std::memcpy(hblob.get(), blob.data(), blob.size());
  std::memcpy(hsegs.get(), segs.data(), segs.size() * 8);
  std::memset(out.get(), 0xAA, out_bytes);
  a.rank = rank.get();
  a.text_at = text_at.get();
  a.scratch = scratch.get();
  a.out = out.get();
  a.out_bytes = out_bytes;
  a.blob = hblob.get();
  a.blob_bytes = blob.size();
  a.segs = hsegs.get();
  a.nsegs = segs.size() / 3;
  parquet_encode_copy_host(a);
  parquet_encode_rows_host(a);
  parquet_encode_text_host(a);
  parquet_encode_pack_host(a);
  if (starve) return;                                 // the sanitizer is the check

  // decode again, page by page
  for (uint64_t p = 0; p < npages; ++p) {
    const int64_t* pg = table.get() + p * kPeCols;
    const uint64_t prow = (uint64_t)pg[kPeRows], r0 = (uint64_t)pg[kPeRow], valid = (uint64_t)pg[kPeNumValid];
    Heap<int64_t> st(2 * kPqStreamCols);
    Heap<int32_t> levels(prow), errs(2), idx(valid);
    int64_t* s = st.get();
    s[kPsOff] = (int64_t)body_at[p];
    s[kPsLen] = (int64_t)body_len[p];
    s[kPsKind] = 1;
    s[kPsWidth] = 1;
    s[kPsCount] = (int64_t)prow;
    PqStreamArgs sa{};
    sa.data = out.get();
    sa.data_bytes = out_bytes;
    sa.streams = s;
    sa.nstreams = 1;
    sa.out = levels.get();
    sa.out_n = prow;
    sa.errors = errs.get();
    parquet_hybrid_host(sa);
    CHECK(errs.get()[0] == 0);
    Heap<int64_t> excl(prow + 1);
    for (uint64_t i = 0; i < prow; ++i) {
      CHECK(levels.get()[i] == (status.get()[r0 + i] == 0 ? 1 : 0));
      excl.get()[i + 1] = excl.get()[i] + (levels.get()[i] == 1);
    }
    Heap<int64_t> pp(kPqPageCols);
    int64_t* q = pp.get();
    q[kPpNumValues] = (int64_t)prow;
    q[kPpOff] = (int64_t)body_at[p];
    q[kPpLen] = (int64_t)body_len[p];
    q[kPpSkip] = 1;
    q[kPpDefStream] = q[kPpValStream] = -1;
    if (kind == kPeFixed || kind == kPeBool) {
      Heap<uint8_t> got(prow * vw), gst(prow);
      PqPlaceArgs pa{};
      pa.data = out.get();
      pa.data_bytes = out_bytes;
      pa.pages = q;
      pa.npages = 1;
      pa.excl = excl.get();
      pa.width = (uint32_t)vw;
      pa.is_bool = kind == kPeBool;
      pa.values = got.get();
      pa.status = gst.get();
      pa.rows = prow;
      parquet_place_host(pa);
      for (uint64_t i = 0; i < prow; ++i) {
        CHECK(gst.get()[i] == status.get()[r0 + i]);
        if (status.get()[r0 + i] == 0) CHECK(std::memcmp(got.get() + i * vw, values.get() + (r0 + i) * vw, vw) == 0);
      }
    } else if (kind == kPeText) {
      Heap<int64_t> start(valid);
      Heap<int32_t> length(valid);
      Heap<uint8_t> vst(valid);
      PqBytesArgs ba{};
      ba.data = out.get();
      ba.data_bytes = out_bytes;
      ba.pages = q;
      ba.npages = 1;
      ba.excl = excl.get();
      ba.rows = prow;
      ba.start = start.get();
      ba.length = length.get();
      ba.status = vst.get();
      ba.nvalues = valid;
      if (valid) parquet_bytes_host(ba);
      uint64_t k = 0, used = 0;
      for (uint64_t i = 0; i < prow; ++i) {
        if (status.get()[r0 + i]) continue;
        CHECK(vst.get()[k] == 0 && (uint64_t)length.get()[k] == strings[r0 + i].size());
        if (vst.get()[k] == 0 && (uint64_t)length.get()[k] == strings[r0 + i].size())
          CHECK(std::memcmp(out.get() + start.get()[k], strings[r0 + i].data(), strings[r0 + i].size()) == 0);
        used += 4 + strings[r0 + i].size();
        ++k;
      }
      CHECK(k == valid && used == (uint64_t)pg[kPeValBytes]);
    } else {
      s[kPsKind] = 2;
      s[kPsSkip] = 1;
      s[kPsCount] = (int64_t)valid;
      sa.out = idx.get();
      sa.out_n = valid;
      if (valid) parquet_hybrid_host(sa);
      CHECK(!valid || errs.get()[0] == 0);
      CHECK(out.get()[body_at[p] + 4 + pq_le32(out.get() + body_at[p])] == bits);
      uint64_t k = 0;
      for (uint64_t i = 0; i < prow; ++i) {
        if (status.get()[r0 + i]) continue;
        int32_t code;
        std::memcpy(&code, values.get() + (r0 + i) * 4, 4);
        CHECK(idx.get()[k] == code);
        ++k;
      }
      // zero padding bits after the last index
      const uint64_t used_bits = valid * bits, total_bits = (uint64_t)pg[kPeValBytes] * 8;
      for (uint64_t b = used_bits; b < total_bits; ++b)
        CHECK(((out.get()[(uint64_t)pg[kPeValOff] + b / 8] >> (b % 8)) & 1) == 0);
    }
  }
}

int main() {
  const uint64_t row_counts[] = {1, 7, 8, 9, 63, 64, 65, 1000};
  const uint64_t dict_sizes[] = {1, 2, 3, 256, 257};
  for (uint64_t rows : row_counts) {
    std::vector<uint64_t> page_rows = {rows};
    if (rows > 65) {
      page_rows.push_back(64);
      page_rows.push_back(100);
    }
    for (uint64_t pr : page_rows)
      for (int pattern = 0; pattern < 5; ++pattern)
        for (uint64_t phase = 0; phase < 2; ++phase) {
          run(kPeFixed, 8, rows, pr, pattern, phase, false);
          run(kPeFixed, 4, rows, pr, pattern, phase, false);
          run(kPeBool, 1, rows, pr, pattern, phase, false);
          run(kPeText, 0, rows, pr, pattern, phase, false);
          for (uint64_t d : dict_sizes) run(kPeIndex, d, rows, pr, pattern, phase, false);
          run(kPeFixed, 8, rows, pr, pattern, phase, true);
          run(kPeText, 0, rows, pr, pattern, phase, true);
          run(kPeIndex, 257, rows, pr, pattern, phase, true);
          run(kPeBool, 1, rows, pr, pattern, phase, true);
        }
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
