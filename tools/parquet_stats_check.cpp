// Stand-alone sanitizer check of the host form of the Parquet statistics passes
// (csrc/parquet_stats_host.h, the code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/parquet_stats_check.cpp -o build/parquet_stats_check \
//       && build/parquet_stats_check
//
// Every column array, mark array, alive array and table is a heap allocation of exactly its size, so
// an access one byte outside is an AddressSanitizer error.  Segments of 0, 1, 63, 64, 65, 255, 256,
// 257 and 1025 rows of every kind (INT32, INT64, FLOAT, DOUBLE, BOOLEAN, text, category), cut out
// of longer columns so that a neighbour's rows lie next to them, with random values, nulls, NaNs of
// both signs, zeros of both signs, infinities and denormals, text of 0 to 70 bytes over a small
// alphabet with long common prefixes, and dictionaries with entries that no row uses, go through
// mark, first and the rounds; the null count and the bounds that ps_finish gives must be those of
// serial code that compares the values themselves.  Then the edge cases by name: the key functions
// on the type limits, "" against "\0", a value and its prefix, 0x7f against 0x80, pairs that differ
// at byte 6, 7, 8, 13, 14, 62 and 63, the cap at 64 and 65 bytes.  Exit status 0 and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "parquet_stats_host.h"

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
  int64_t addr() const { return n ? (int64_t)(uintptr_t)p.get() : 0; }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

static bool bytes_less(const std::string& a, const std::string& b) {      // unsigned, a proper prefix first
  const size_t n = a.size() < b.size() ? a.size() : b.size();
  const int c = std::memcmp(a.data(), b.data(), n);
  return c < 0 || (c == 0 && a.size() < b.size());
}

struct Want {
  int64_t nulls = 0;
  bool has = false;
  std::string lo, hi;
};

static void want_text(Want& w, const std::vector<std::string>& live) {
  size_t longest = 0;
  for (const auto& v : live) longest = v.size() > longest ? v.size() : longest;
  if (live.empty() || longest > kPsTextCap) return;
  w.has = true;
  w.lo = w.hi = live[0];
  for (const auto& v : live) {
    if (bytes_less(v, w.lo)) w.lo = v;
    if (bytes_less(w.hi, v)) w.hi = v;
  }
}

template <typename T>
static std::string plain(T v) {
  std::string s(sizeof(T), '\0');
  std::memcpy(&s[0], &v, sizeof(T));
  return s;
}

template <typename T>
static void want_number(Want& w, const std::vector<T>& live) {
  bool any = false;
  T lo = 0, hi = 0;
  for (T v : live) {
    if (v != v) continue;                             // a NaN takes no part
    if (!any || v < lo) lo = v;
    if (!any || v > hi) hi = v;
    any = true;
  }
  if (!any) return;
  if (std::is_floating_point<T>::value) {
    if (lo == 0) lo = (T)-0.0;
    if (hi == 0) hi = (T)0.0;
  }
  w.has = true;
  w.lo = plain(lo);
  w.hi = plain(hi);
}

// One table of segments, run through all passes the way parquet_stats.cpp runs them.
struct Run {
  std::vector<int64_t> rows;                          // kPeCols each
  std::vector<Want> want;                             // per segment; a dictionary's segment has none
  std::vector<int> finish_from;                       // the segment whose result row holds the bounds
  std::vector<std::unique_ptr<Heap<uint8_t>>> bytes;
  std::vector<std::unique_ptr<Heap<int64_t>>> words;
  uint64_t flat = 0;

  int64_t* add() {
    rows.resize(rows.size() + kPeCols, 0);
    int64_t* r = &rows[rows.size() - kPeCols];
    r[kPeLevelOff] = -1;
    return r;
  }
  template <typename T>
  int64_t keep(const std::vector<T>& v) {
    bytes.emplace_back(new Heap<uint8_t>(v.size() * sizeof(T)));
    if (!v.empty()) std::memcpy(bytes.back()->get(), v.data(), v.size() * sizeof(T));
    return bytes.back()->addr();
  }
  // packed text: returns (data, offsets, bytes)
  void keep_text(const std::vector<std::string>& v, int64_t* data, int64_t* off, int64_t* n) {
    std::vector<uint8_t> d;
    words.emplace_back(new Heap<int64_t>(v.size() + 1));
    for (size_t i = 0; i < v.size(); ++i) {
      d.insert(d.end(), v[i].begin(), v[i].end());
      words.back()->get()[i + 1] = (int64_t)d.size();
    }
    *data = keep(d);
    *off = words.back()->addr();
    *n = (int64_t)d.size();
  }
};

static void run_and_check(Run& R, int line) {
  // the order the caller keeps: numbers, dictionary indices, text; here the rows come in any order, so
  // the ranges are the whole table and the passes skip what is not theirs
  const uint64_t nsegs = R.rows.size() / kPeCols;
  Heap<int64_t> table(R.rows.size()), results(nsegs * kPsCols);
  Heap<uint8_t> alive(R.flat);
  std::memcpy(table.get(), R.rows.data(), R.rows.size() * sizeof(int64_t));
  for (uint64_t s = 0; s < nsegs; ++s) {
    int64_t* r = results.get() + s * kPsCols;
    r[kPsMin] = INT64_MAX;
    r[kPsMax] = INT64_MIN;
    for (int k = 0; k < kPsRounds; ++k) r[kPsRoundMin + k] = -1;
  }
  PsArgs a{};
  a.segs = table.get();
  a.nsegs = nsegs;
  a.first = 0;
  a.last = nsegs;
  a.alive = alive.get();
  a.flat_n = R.flat;
  a.results = results.get();
  parquet_stats_host(a, kPsPassMark);
  parquet_stats_host(a, kPsPassFirst);
  for (uint32_t r = 1; r < kPsRounds; ++r) {
    a.round = r;
    parquet_stats_host(a, kPsPassRound);
  }
  for (uint64_t s = 0; s < R.want.size(); ++s) {
    if (R.finish_from[s] < 0) continue;
    const int64_t* sg = table.get() + s * kPeCols;
    const int64_t* from = table.get() + (uint64_t)R.finish_from[s] * kPeCols;
    uint8_t mn[kPsTextCap], mx[kPsTextCap];
    uint32_t nmin = 0, nmax = 0;
    const bool has = ps_finish(results.get() + (uint64_t)R.finish_from[s] * kPsCols, from[kPeKind], (uint32_t)from[kPeWidth],
                               from[kPsIsFloat] != 0, mn, &nmin, mx, &nmax);
    const Want& w = R.want[s];
    const bool ok = results.get()[s * kPsCols + kPsNulls] == w.nulls && has == w.has &&
                    (!has || (std::string((char*)mn, nmin) == w.lo && std::string((char*)mx, nmax) == w.hi));
    if (!ok && g_failed < 20)
      std::printf("segment %llu (kind %lld, rows %lld) of the table built at line %d\n", (unsigned long long)s,
                  (long long)sg[kPeKind], (long long)sg[kPeRows], line);
    CHECK(ok);
  }
}

template <typename T>
static T special(uint32_t r);
template <>
int32_t special<int32_t>(uint32_t r) { return r % 3 == 0 ? INT32_MIN : r % 3 == 1 ? INT32_MAX : 0; }
template <>
int64_t special<int64_t>(uint32_t r) { return r % 3 == 0 ? INT64_MIN : r % 3 == 1 ? INT64_MAX : -1; }
template <>
uint8_t special<uint8_t>(uint32_t) { return 1; }
template <typename F, typename U>
static F special_float(uint32_t r, U neg_nan_bits) {
  switch (r % 8) {
    case 0: return std::numeric_limits<F>::quiet_NaN();
    case 1: {
      F f;
      std::memcpy(&f, &neg_nan_bits, sizeof(F));
      return f;
    }
    case 2: return (F)0.0;
    case 3: return (F)-0.0;
    case 4: return std::numeric_limits<F>::infinity();
    case 5: return -std::numeric_limits<F>::infinity();
    case 6: return std::numeric_limits<F>::denorm_min();
    default: return -std::numeric_limits<F>::denorm_min();
  }
}
template <>
float special<float>(uint32_t r) { return special_float<float, uint32_t>(r, 0xFFC00001u); }
template <>
double special<double>(uint32_t r) { return special_float<double, uint64_t>(r, 0xFFF8000000000001ull); }

static const uint64_t kSizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 1025};

// A column of `total` rows of T and segments of every size inside it.  mode 0: random values; 1: many
// special values; 2: only zeros and NaNs (floats) or one value (integers).
template <typename T>
static void number_segments(Run& R, int kind, bool is_float, int mode, int null_every) {
  const uint64_t total = 1025 + 64;
  std::vector<T> vals(total);
  std::vector<uint8_t> status(total);
  for (uint64_t i = 0; i < total; ++i) {
    const uint32_t r = rnd();
    if (kind == kPeBool) vals[i] = (T)(mode == 2 ? 1 : r % 3);          // any byte but 0 is true
    else if (mode == 2) vals[i] = special<T>(is_float ? r % 4 : 2);
    else if (mode == 1 && r % 4 == 0) vals[i] = special<T>(r >> 8);
    else vals[i] = (T)((int32_t)(r >> 4) % 2001 - 1000) / (T)(is_float ? 7 : 1);
    status[i] = null_every == 1 ? 1 : (null_every && r % null_every == 0) ? (uint8_t)(1 + r % 2) : 0;
  }
  const int64_t v = R.keep(vals), st = R.keep(status);
  for (uint64_t n : kSizes) {
    const uint64_t r0 = n == 1025 ? 32 : rnd() % (total - n);
    int64_t* row = R.add();
    row[kPeKind] = kind;
    row[kPeWidth] = kind == kPeBool ? 1 : (int64_t)sizeof(T);
    row[kPeValues] = v;
    row[kPeStatus] = st;
    row[kPeRow] = (int64_t)r0;
    row[kPeRows] = (int64_t)n;
    row[kPsIsFloat] = is_float;
    Want w;
    std::vector<T> live;
    for (uint64_t i = r0; i < r0 + n; ++i) {
      if (status[i]) ++w.nulls;
      else live.push_back(kind == kPeBool ? (T)(vals[i] != 0) : vals[i]);
    }
    want_number(w, live);
    R.want.push_back(w);
    R.finish_from.push_back((int)R.want.size() - 1);
  }
}

static std::string random_text(int mode) {
  // a small alphabet and long shared prefixes, so that winners are decided late and often tie
  static const char* const heads[] = {"", "abcdefg", "abcdefgabcdefg", "abcdefgabcdefgabcdefgabcdefgabcdefgabcdefgabcdefgabcdefgabcdefg"};
  std::string s = heads[rnd() % 4];
  const uint32_t more = mode == 1 ? rnd() % 8 : rnd() % 3;
  static const char alphabet[] = {'\0', 'a', '\x7f', '\x80', '\xff'};
  for (uint32_t j = 0; j < more; ++j) s.push_back(alphabet[rnd() % 5]);
  if (s.size() > (mode == 2 ? 70u : 64u)) s.resize(mode == 2 ? 70 : 64);
  return s;
}

static void text_segments(Run& R, int mode, int null_every) {
  const uint64_t total = 1025 + 64;
  std::vector<std::string> vals(total);
  std::vector<uint8_t> status(total);
  for (uint64_t i = 0; i < total; ++i) {
    vals[i] = random_text(mode);
    const uint32_t r = rnd();
    status[i] = null_every == 1 ? 1 : (null_every && r % null_every == 0) ? 1 : 0;
  }
  int64_t data = 0, off = 0, nbytes = 0;
  R.keep_text(vals, &data, &off, &nbytes);
  const int64_t st = R.keep(status);
  for (uint64_t n : kSizes) {
    const uint64_t r0 = n == 1025 ? 32 : rnd() % (total - n);
    int64_t* row = R.add();
    row[kPeKind] = kPeText;
    row[kPeValues] = data;
    row[kPeOffsets] = off;
    row[kPeAux] = nbytes;
    row[kPeStatus] = st;
    row[kPeRow] = (int64_t)r0;
    row[kPeRows] = (int64_t)n;
    row[kPeFlat] = (int64_t)R.flat;
    R.flat += n;
    Want w;
    std::vector<std::string> live;
    for (uint64_t i = r0; i < r0 + n; ++i) {
      if (status[i]) ++w.nulls;
      else live.push_back(vals[i]);
    }
    want_text(w, live);
    R.want.push_back(w);
    R.finish_from.push_back((int)R.want.size() - 1);
  }
}

// Category segments: the dictionary's smallest and largest entries are used by no row.
static void category_segments(Run& R, int mode) {
  const uint64_t total = 1025 + 64;
  std::vector<std::string> vocab = {std::string("\0", 1), "zzzz-unused", ""};
  for (int k = 0; k < 40; ++k) vocab.push_back("e" + random_text(mode) + std::to_string(k));
  vocab.push_back("\xff\xff");                         // never used: codes stay in [3, size - 1)
  if (mode == 2) vocab.push_back(std::string(65, 'q'));
  std::vector<int32_t> codes(total);
  std::vector<uint8_t> status(total);
  for (uint64_t i = 0; i < total; ++i) {
    const uint32_t r = rnd();
    const uint32_t span = mode == 2 ? (uint32_t)vocab.size() - 3 : 40;
    codes[i] = r % 11 == 0 ? -1 : r % 13 == 0 ? (int32_t)vocab.size() + (int32_t)(r % 5) : 3 + (int32_t)((r >> 8) % span);
    if (mode == 2 && codes[i] == (int32_t)vocab.size() - 2) codes[i] = 3;
    status[i] = r % 7 == 0 ? 1 : 0;
  }
  const int64_t cv = R.keep(codes), st = R.keep(status);
  struct Pending { int seg; int64_t mark; };
  std::vector<Pending> pending;
  for (uint64_t n : kSizes) {
    const uint64_t r0 = n == 1025 ? 32 : rnd() % (total - n);
    int64_t* row = R.add();
    const int64_t mark = R.keep(std::vector<uint8_t>(vocab.size(), 1));
    row[kPeKind] = kPeIndex;
    row[kPeValues] = cv;
    row[kPeStatus] = st;
    row[kPeAux] = (int64_t)vocab.size();
    row[kPeRow] = (int64_t)r0;
    row[kPeRows] = (int64_t)n;
    row[kPsMark] = mark;
    Want w;
    std::vector<std::string> live;
    for (uint64_t i = r0; i < r0 + n; ++i) {
      if (status[i] || codes[i] < 0 || codes[i] >= (int32_t)vocab.size()) ++w.nulls;
      else live.push_back(vocab[codes[i]]);
    }
    want_text(w, live);
    R.want.push_back(w);
    R.finish_from.push_back(-1);
    pending.push_back({(int)R.want.size() - 1, mark});
  }
  for (const Pending& p : pending) {                  // the dictionaries' segments, after all others
    int64_t data = 0, off = 0, nbytes = 0;
    R.keep_text(vocab, &data, &off, &nbytes);
    int64_t* row = R.add();
    row[kPeKind] = kPeText;
    row[kPeValues] = data;
    row[kPeOffsets] = off;
    row[kPeAux] = nbytes;
    row[kPeStatus] = p.mark;
    row[kPeRows] = (int64_t)vocab.size();
    row[kPeFlat] = (int64_t)R.flat;
    R.flat += vocab.size();
    R.finish_from[p.seg] = (int)(R.rows.size() / kPeCols) - 1;
    R.want.push_back(Want());                         // nothing is asked of the dictionary's own row
    R.finish_from.push_back(-1);
  }
}

static void one_text_segment(Run& R, const std::vector<std::string>& vals) {
  int64_t data = 0, off = 0, nbytes = 0;
  R.keep_text(vals, &data, &off, &nbytes);
  int64_t* row = R.add();
  row[kPeKind] = kPeText;
  row[kPeValues] = data;
  row[kPeOffsets] = off;
  row[kPeAux] = nbytes;
  row[kPeRows] = (int64_t)vals.size();
  row[kPeFlat] = (int64_t)R.flat;
  R.flat += vals.size();
  Want w;
  want_text(w, vals);
  R.want.push_back(w);
  R.finish_from.push_back((int)R.want.size() - 1);
}

static void named_cases() {
  // the keys keep the order, and come back as the bits they were made from
  const int64_t ints[] = {INT64_MIN, -1, 0, 1, INT64_MAX};
  bool nan = false;
  for (int i = 0; i + 1 < 5; ++i) CHECK(ps_key((uint64_t)ints[i], 8, false, &nan) < ps_key((uint64_t)ints[i + 1], 8, false, &nan));
  const int32_t ints32[] = {INT32_MIN, -1, 0, 1, INT32_MAX};
  for (int i = 0; i + 1 < 5; ++i)
    CHECK(ps_key((uint32_t)ints32[i], 4, false, &nan) < ps_key((uint32_t)ints32[i + 1], 4, false, &nan));
  for (int i = 0; i < 5; ++i) {
    CHECK(ps_unkey(ps_key((uint64_t)ints[i], 8, false, &nan), 8, false, false) == (uint64_t)ints[i]);
    CHECK(ps_unkey(ps_key((uint32_t)ints32[i], 4, false, &nan), 4, false, true) == (uint32_t)ints32[i]);
  }
  const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
  const double ds[] = {-inf, -1e300, -1.0, -den, -0.0, 0.0, den, 1.0, 1e300, inf};
  for (int i = 0; i < 10; ++i) {
    uint64_t b, b2;
    std::memcpy(&b, &ds[i], 8);
    const int64_t k = ps_key(b, 8, true, &nan);
    CHECK(!nan);
    if (i + 1 < 10) {
      std::memcpy(&b2, &ds[i + 1], 8);
      CHECK(k < ps_key(b2, 8, true, &nan));
    }
    if (ds[i] != 0) CHECK(ps_unkey(k, 8, true, false) == b && ps_unkey(k, 8, true, true) == b);
    else CHECK(ps_unkey(k, 8, true, false) == 0x8000000000000000ull && ps_unkey(k, 8, true, true) == 0);
    const float f = (float)ds[i];
    uint32_t c;
    std::memcpy(&c, &f, 4);
    const int64_t k4 = ps_key(c, 4, true, &nan);
    CHECK(!nan && k4 >= 0 && k4 <= 0xFFFFFFFFll);
    if (f != 0) CHECK(ps_unkey(k4, 4, true, false) == c);
    else CHECK(ps_unkey(k4, 4, true, false) == 0x80000000u && ps_unkey(k4, 4, true, true) == 0);
  }
  for (uint64_t b : {0x7FF8000000000000ull, 0xFFF8000000000001ull, 0x7FF0000000000001ull}) {
    ps_key(b, 8, true, &nan);
    CHECK(nan);
  }
  for (uint32_t b : {0x7FC00000u, 0xFFC00001u, 0x7F800001u}) {
    ps_key(b, 4, true, &nan);
    CHECK(nan);
  }
  Run R;
  one_text_segment(R, {"", std::string("\0", 1)});
  one_text_segment(R, {std::string("\0", 1), ""});
  one_text_segment(R, {"abc", "ab", "abcd"});
  one_text_segment(R, {std::string("\x7f\0", 2), "\x80"});
  one_text_segment(R, {"abcdefg", std::string("abcdefg\0", 8), "abcdefg"});
  for (int k : {6, 7, 8, 13, 14, 62, 63}) {
    std::string head;
    for (int j = 0; j < k; ++j) head.push_back((char)((7 * j + 1) % 251));
    one_text_segment(R, {head + "\x02", head + "\x01", head + "\x02"});
    one_text_segment(R, {head + "\x01", head + "\x02"});
    one_text_segment(R, {head + "\x01" + std::string(64 - k - 1, 'x'), head});
  }
  one_text_segment(R, {"zz", "a", "zz", "a", "m"});
  one_text_segment(R, {std::string(64, 'x'), std::string(63, 'x'), std::string(64, 'x')});
  one_text_segment(R, {std::string(65, 'x'), "a"});
  one_text_segment(R, {std::string(70, 'a'), std::string(71, 'a')});
  one_text_segment(R, {});
  CHECK(R.want[R.want.size() - 4].has && R.want[R.want.size() - 4].hi.size() == 64);
  CHECK(!R.want[R.want.size() - 3].has && !R.want[R.want.size() - 2].has && !R.want.back().has);
  run_and_check(R, __LINE__);
  // a text value that does not lie inside its data counts as a null
  Run B;
  one_text_segment(B, {"b", "a", "c"});
  B.rows[kPeAux] = 2;                                   // the last value now ends outside
  B.want[0] = Want();
  B.want[0].nulls = 1;
  want_text(B.want[0], {"b", "a"});
  run_and_check(B, __LINE__);
}

int main() {
  named_cases();
  for (int mode = 0; mode < 3; ++mode) {
    for (int null_every : {0, 1, 2, 5}) {
      Run R;
      number_segments<int32_t>(R, kPeFixed, false, mode, null_every);
      number_segments<int64_t>(R, kPeFixed, false, mode, null_every);
      number_segments<float>(R, kPeFixed, true, mode, null_every);
      number_segments<double>(R, kPeFixed, true, mode, null_every);
      number_segments<uint8_t>(R, kPeBool, false, mode, null_every);
      category_segments(R, mode);
      text_segments(R, mode, null_every);
      run_and_check(R, __LINE__);
    }
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
