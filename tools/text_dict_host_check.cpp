// Stand-alone sanitizer check of the host form of the text dictionary (csrc/text_dict_host.h, the
// code that also runs on the device).  Build and run on the CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ialluxio_amd/csrc tools/text_dict_host_check.cpp -o build/text_dict_host_check \
//       && build/text_dict_host_check
//
// Every buffer (data, spans, the table, the entries' bytes, offsets and hashes, the per-row
// outputs) is a heap allocation of its exact size, so a read or write one element outside it is an
// AddressSanitizer error.  The cases are the CPU shapes of tests/test_text_dict.py: value lengths
// around the 8-byte word, the 16-byte vector and the 256-byte step as pairs that differ in one
// byte, prefix chains, zero-padding traps, the row counts under three mixes, forced collisions
// (hash bits 0 and 2), three batches into a table that starts with 8 slots and is rehashed, lookup,
// values that are not live.  The yardstick is a std::map filled in row order.  The way kernel
// variant 1 adds the hash up (two words per lane, sixteen lanes per step, any order) is replayed
// in plain C++ against the serial hash.  Exit status 0 and "ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "text_dict_host.h"

using namespace amdx;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// A dictionary whose arrays are reallocated at their exact size on every call.
struct Dict {
  std::vector<uint64_t> table;
  std::vector<uint64_t> ent_hash;
  std::vector<int64_t> ent_off{0};
  std::vector<uint8_t> ent_data;
  uint64_t D = 0;
  int bits = 64;
  explicit Dict(size_t capacity) : table(capacity, kTdEmpty) {}

  void reserve(uint64_t need) {
    if (table.size() >= need) return;
    size_t cap = table.size();
    while (cap < need) cap *= 2;
    auto t = exact(std::vector<uint64_t>(cap, kTdEmpty));
    auto h = exact(ent_hash);
    TextDictArgs a{};
    a.table = t.get();
    a.capacity = cap;
    a.ent_hash = h.get();
    a.D = D;
    a.hash_bits = bits;
    CHECK(text_dict_scalars_ok(a));
    text_dict_rehash_host(a);
    table.assign(t.get(), t.get() + cap);
  }

  // One encode (insert) or lookup of the spans; returns the codes.
  std::vector<int32_t> run(const std::string& data, const std::vector<int64_t>& start, const std::vector<int32_t>& length,
                           const std::vector<uint8_t>* status, bool insert) {
    const size_t n = start.size();
    if (insert) reserve(2 * (D + n));
    auto d = exact(std::vector<uint8_t>(data.begin(), data.end()));
    auto st = exact(start);
    auto ln = exact(length);
    auto ss = exact(status ? *status : std::vector<uint8_t>());
    auto t = exact(table);
    auto ed = exact(ent_data);
    auto eo = exact(ent_off);
    std::unique_ptr<int32_t[]> slot_of(new int32_t[n]), first(new int32_t[n]), first_len(new int32_t[n]), codes(new int32_t[n]);
    std::unique_ptr<uint64_t[]> hash(new uint64_t[n]);
    TextDictArgs a{};
    a.in.data = d.get();
    a.in.data_bytes = data.size();
    a.in.start = st.get();
    a.in.length = ln.get();
    a.in.status = status ? ss.get() : nullptr;
    a.in.n = n;
    a.in.quote = -1;
    a.ent_data = ed.get();
    a.ent_bytes = ent_data.size();
    a.ent_off = eo.get();
    a.ent_cap = D;
    a.D = D;
    a.table = t.get();
    a.capacity = table.size();
    a.hash_bits = bits;
    a.insert = insert ? 1 : 0;
    a.slot_of = slot_of.get();
    a.hash = hash.get();
    a.first = first.get();
    a.first_len = first_len.get();
    a.codes = codes.get();
    CHECK(text_dict_scalars_ok(a) && text_dict_probe_fits(a));
    text_dict_probe_host(a);
    std::unique_ptr<int64_t[]> rank(new int64_t[n]), byte_off(new int64_t[n + 1]);
    byte_off[0] = 0;
    if (insert) {
      text_dict_first_host(a);
      int64_t k = 0;
      for (size_t r = 0; r < n; ++r) {
        rank[r] = (k += first[r]);
        byte_off[r + 1] = byte_off[r] + first_len[r];
      }
      a.rank = rank.get();
    }
    text_dict_codes_host(a);
    std::vector<int32_t> out(codes.get(), codes.get() + n);
    if (insert && n) {
      const uint64_t fresh = (uint64_t)rank[n - 1], nb = (uint64_t)byte_off[n];
      std::unique_ptr<uint64_t[]> eh(new uint64_t[D + fresh]);
      std::unique_ptr<int64_t[]> eo2(new int64_t[D + fresh + 1]);
      std::copy(ent_hash.begin(), ent_hash.end(), eh.get());
      std::copy(ent_off.begin(), ent_off.end(), eo2.get());
      a.ent_hash = eh.get();
      a.ent_off = eo2.get();
      a.ent_cap = D + fresh;
      a.byte_off = byte_off.get();
      a.old_bytes = ent_data.size();
      text_dict_commit_host(a);
      std::unique_ptr<uint8_t[]> bytes(new uint8_t[nb]);      // the append: text_emit with quote -1
      TextColumnArgs e = a.in;
      e.offsets = byte_off.get();
      e.out = bytes.get();
      e.out_bytes = nb;
      text_emit_host(e);
      ent_data.insert(ent_data.end(), bytes.get(), bytes.get() + nb);
      ent_hash.assign(eh.get(), eh.get() + D + fresh);
      ent_off.assign(eo2.get(), eo2.get() + D + fresh + 1);
      D += fresh;
      table.assign(t.get(), t.get() + table.size());
    } else {
      CHECK(std::equal(table.begin(), table.end(), t.get()));   // a lookup writes nothing to the table
    }
    return out;
  }

  std::vector<int32_t> encode(const std::vector<std::string>& values, bool insert = true) {
    std::string data;
    std::vector<int64_t> start;
    std::vector<int32_t> length;
    for (auto& v : values) {
      data += "\"";                                 // a byte that belongs to no value
      start.push_back((int64_t)data.size());
      length.push_back((int32_t)v.size());
      data += v;
    }
    return run(data, start, length, nullptr, insert);
  }

  std::vector<std::string> entries() const {
    std::vector<std::string> out;
    for (uint64_t e = 0; e < D; ++e)
      out.emplace_back(ent_data.begin() + ent_off[e], ent_data.begin() + ent_off[e + 1]);
    return out;
  }
};

struct Yardstick {
  std::map<std::string, int32_t> codes;
  std::vector<std::string> order;
  int32_t code(const std::string& v) {
    auto it = codes.find(v);
    if (it != codes.end()) return it->second;
    order.push_back(v);
    return codes[v] = (int32_t)order.size() - 1;
  }
};

static void check(Dict& d, Yardstick& y, const std::vector<std::string>& values) {
  std::vector<int32_t> want;
  for (auto& v : values) want.push_back(y.code(v));
  CHECK(d.encode(values) == want);
  CHECK(d.entries() == y.order);
  CHECK(d.table.size() >= 2 * d.D);
}

static std::string letters(size_t n, size_t seed) {
  std::string v(n, 'a');
  for (size_t i = 0; i < n; ++i) v[i] = (char)('a' + (i * 7 + seed) % 23);
  return v;
}

// The hash as kernel variant 1 adds it up: lanes take 16 bytes each, in descending lane order here.
static uint64_t coop_hash(const std::string& v, int bits) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
  const uint64_t n = v.size();
  uint64_t lane_sum[16] = {0};
  for (uint64_t base = 0; base < n; base += 256)
    for (int l = 15; l >= 0; --l) {
      const uint64_t pos = base + 16 * (uint64_t)l;
      if (pos >= n) continue;
      const uint64_t rem = n - pos;
      lane_sum[l] += td_term(pos / 8, td_word(p + pos, rem));
      if (rem > 8) lane_sum[l] += td_term(pos / 8 + 1, td_word(p + pos + 8, rem - 8));
    }
  uint64_t sum = 0;
  for (int l = 15; l >= 0; --l) sum += lane_sum[l];
  return td_finish(sum, n, bits);
}

int main() {
  const size_t lengths[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, 4099};
  {  // lengths, as pairs that differ in one byte; the hash replayed; equality one byte short of a word
    std::vector<std::string> vs;
    for (size_t n : lengths) {
      const std::string v = letters(n, n);
      vs.push_back(v);
      for (size_t i : {n - 1, (size_t)15, (size_t)16, (size_t)255, (size_t)256})
        if (i < n) {
          std::string w = v;
          w[i] ^= 0x20;
          vs.push_back(w);
          CHECK(!td_equal((const uint8_t*)v.data(), (const uint8_t*)w.data(), n));
        }
    }
    for (auto& v : vs)
      for (int bits : {64, 2, 0}) CHECK(coop_hash(v, bits) == td_hash((const uint8_t*)v.data(), v.size(), bits));
    std::vector<std::string> rows = vs;
    rows.insert(rows.end(), vs.rbegin(), vs.rend());
    Dict d(1024);
    Yardstick y;
    check(d, y, rows);
    CHECK(d.D == y.order.size() && d.D > 3 * (sizeof(lengths) / sizeof(lengths[0])));
    check(d, y, rows);
  }
  {  // prefix chains and zero padding: all distinct keys, and distinct hashes by design
    std::vector<std::string> vs;
    for (size_t k = 0; k <= 40; ++k) vs.push_back(std::string(k, 'a'));
    for (size_t k : {1u, 2u, 7u, 8u, 9u, 16u, 17u}) vs.push_back(std::string(k, '\0'));
    vs.push_back(std::string("a\0", 2));
    vs.push_back(std::string("a\0\0", 3));
    vs.push_back(std::string("aaaaaaaa\0", 9));
    Dict d(8);
    Yardstick y;
    check(d, y, vs);
    CHECK(d.D == vs.size());
    const std::string a1("a"), a2("a\0", 2);
    CHECK(td_hash((const uint8_t*)a1.data(), 1, 64) != td_hash((const uint8_t*)a2.data(), 2, 64));
    CHECK(td_hash(nullptr, 0, 64) != td_hash((const uint8_t*)a2.data() + 1, 1, 64));
  }
  {  // row counts under three mixes
    for (size_t n : {0u, 1u, 15u, 16u, 17u, 255u, 256u, 257u, 4096u})
      for (int mix = 0; mix < 3; ++mix) {
        std::vector<std::string> vs;
        for (size_t r = 0; r < n; ++r)
          vs.push_back(mix == 0 ? "the same value" : mix == 1 ? (r & 1 ? "right, and longer than sixteen bytes" : "left")
                                                              : "v" + std::to_string(r * 7919 % 100003));
        Dict d(2);
        Yardstick y;
        check(d, y, vs);
        CHECK(d.D == (mix == 0 ? std::min<size_t>(n, 1) : mix == 1 ? std::min<size_t>(n, 2) : n));
      }
  }
  for (int bits : {0, 2}) {  // forced collisions: every value walks one chain (four with two bits)
    std::vector<std::string> vs;
    for (int i = 0; i < 300; ++i) vs.push_back("key-" + std::to_string(i) + std::string(i % 40, 'x'));
    for (int i = 0; i < 400; ++i) vs.push_back(vs[(size_t)(i * 37) % 300]);
    Dict d(8);
    d.bits = bits;
    Yardstick y;
    check(d, y, vs);
    std::vector<std::string> more(vs.begin() + 250, vs.begin() + 350);
    for (int i = 0; i < 20; ++i) more.push_back("new-" + std::to_string(i));
    check(d, y, more);
    CHECK(d.D == 320);
  }
  {  // three batches into a table of 8 slots; lookup; a second dictionary gives the same bytes
    Dict d(8), e(4096);
    Yardstick y, z;
    for (int b = 0; b < 3; ++b) {
      std::vector<std::string> vs;
      for (int i = 25 * b; i < 25 * b + 50; ++i) vs.push_back("item " + std::to_string(i) + std::string(i % 19, '.'));
      for (int i = 0; i < 10; ++i) vs.push_back(vs[(size_t)(i * 13) % 50]);
      check(d, y, vs);
      check(e, z, vs);
    }
    CHECK(d.D == 100 && d.table.size() == 512 && d.ent_data == e.ent_data && d.ent_off == e.ent_off);
    std::vector<std::string> q = {"item 3...", "item 3..", "nope", "", "item 99" + std::string(99 % 19, '.')};
    CHECK(d.encode(q, false) == (std::vector<int32_t>{3, -1, -1, -1, 99}));
    CHECK(d.D == 100);
  }
  {  // values that are not live: code -1, no entry, nothing read
    const std::vector<std::string> vals = {"keep", "zzzz", "zzzz", "zzzz", "zzzz", "keep", "zzzz", "other", "zzzz"};
    std::string data;
    std::vector<int64_t> start;
    std::vector<int32_t> length;
    for (auto& v : vals) {
      start.push_back((int64_t)data.size());
      length.push_back((int32_t)v.size());
      data += v;
    }
    std::vector<uint8_t> status(vals.size(), 0);
    status[1] = 1;
    status[2] = 2;
    start[3] = -1;
    length[4] = -1;
    start[8] = (int64_t)data.size() - 3;            // start + length = data_bytes + 1
    Dict d(64);
    CHECK(d.run(data, start, length, &status, true) == (std::vector<int32_t>{0, -1, -1, -1, -1, 0, 1, 2, -1}));
    CHECK(d.entries() == (std::vector<std::string>{"keep", "zzzz", "other"}));
    start[1] = INT64_MAX;
    length[2] = INT32_MAX;
    CHECK(d.run(data, start, length, nullptr, true) == (std::vector<int32_t>{0, -1, -1, -1, -1, 0, 1, 2, -1}));
    start[8] = (int64_t)data.size() - 4;            // the value that ends with the buffer is live
    CHECK(d.run(data, start, length, nullptr, false)[8] == 1);
    CHECK(d.D == 3);
  }
  {  // scalars
    TextDictArgs a{};
    a.capacity = 8;
    a.hash_bits = 64;
    CHECK(text_dict_scalars_ok(a) && text_dict_probe_fits(a));
    a.in.n = 5;
    a.insert = 1;
    CHECK(!text_dict_probe_fits(a));
    a.insert = 0;
    CHECK(text_dict_probe_fits(a));
    a.capacity = 12;
    CHECK(!text_dict_scalars_ok(a));
    a.capacity = 1ull << 32;
    CHECK(!text_dict_scalars_ok(a));
    a.capacity = 1ull << 31;
    a.in.n = (1ull << 30) + 1;
    CHECK(!text_dict_scalars_ok(a));
    a.in.n = 1;
    a.hash_bits = 65;
    CHECK(!text_dict_scalars_ok(a));
    CHECK(td_mask(~0ull, 0) == 0 && td_mask(~0ull, 2) == 3 && td_mask(~0ull, 64) == ~0ull && td_mask(~0ull, 63) == (~0ull >> 1));
  }
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
