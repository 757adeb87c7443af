// Dictionary encoding of text values: the rule, as plain C++.  The codes are those of
//
//   codes = [d.setdefault(v, len(d)) for v in values]        # d persists across calls
//
// over the live values in row order (first-occurrence order); a value that is not live (status not
// 0, or not inside the data: tc_live of text_column_host.h) has code -1, is not read and is not
// inserted.  Keys are compared byte for byte; the empty value is an ordinary key.
//
// State, all in arrays the caller owns: the table, open addressing with linear probing over
// `capacity` (a power of two) uint64 slots, all ones = empty, otherwise (tag << 32) | id with tag
// the high half of the value's hash; an id with bit 31 clear is a committed code, one with bit 31
// set is the pending row r of the call under way.  Rows per call are at most 2^30, so a slot never
// equals the empty pattern.  Entry e of the dictionary is ent_data[ent_off[e], ent_off[e + 1]) and
// ent_hash[e] its hash.
//
// One encode is five passes, each a loop over the rows here and a launch on the device:
//   probe   walk the chain of the value: claim an empty slot for row r (compare-and-swap), or stop
//           at a slot whose tag and bytes equal the value's; on a pending slot the smallest row
//           stays (atomic min; every candidate has equal bytes).  slot_of[r], hash[r].
//   first   first[r] = slot_of[r] still holds pending row r; first_len[r] = its length, else 0.
//           The caller scans first (rank, inclusive) and first_len (byte_off, exclusive, n + 1).
//   codes   the committed id, or D + rank[representative row] - 1, or -1.
//   commit  (after codes, never fused with it) each first row writes tag | code into its slot,
//           its hash into ent_hash[code] and the end of its bytes into ent_off[code + 1].
//   append  text_emit_raw with quote -1 over the rows with byte_off as offsets: only first rows
//           have a window, so the new entries' bytes land in code order.
// lookup is probe without the claim, then codes.  The result depends on neither the hash, the
// capacity nor the order in which rows run: a slot only ever goes empty -> pending -> pending with
// a smaller row of equal bytes, so all rows of one key stop at one slot, and ranks are by row.
//
// The hash is a sum of per-word terms (8-byte little-endian words, the last one zero padded, each
// mixed with its index) plus a finaliser that takes the length in, so that a group of lanes can add
// the terms in any order and b"a" and b"a\0" differ.  td_mask cuts it to its low `bits` bits before
// any use (a test hook: 0 sends every value down one chain).
//
// Written once and compiled twice, as text_column_host.h is.  No HIP include; the atomics of the
// device pass are HIP's global atomics, the host pass is serial and uses plain loads and stores.
#pragma once
#include <cstdint>

#include "text_column_host.h"

namespace amdx {

constexpr uint64_t kTdEmpty = ~0ull;
constexpr uint64_t kTdTagMask = 0xFFFFFFFF00000000ull;
constexpr uint32_t kTdPending = 0x80000000u;
constexpr uint64_t kTdMaxRows = 1ull << 30;
constexpr uint64_t kTdMaxCapacity = 1ull << 31;     // slot numbers are int32

struct TextDictArgs {
  TextColumnArgs in;         // data, data_bytes, start, length, status, n: the values (tc_live)
  const uint8_t* ent_data;   // the entries' bytes, packed in code order
  uint64_t ent_bytes;
  int64_t* ent_off;          // [ent_cap + 1]; read up to [D], commit writes (D, D + new]
  uint64_t* ent_hash;        // [ent_cap]
  uint64_t ent_cap;
  uint64_t D;                // entries before the call
  uint64_t* table;           // [capacity]
  uint64_t capacity;
  int32_t hash_bits;         // 0..64
  int32_t insert;            // probe: 1 encode, 0 lookup
  int32_t* slot_of;          // [n] the slot the value stopped at, -1: none
  uint64_t* hash;            // [n]
  int32_t* first;            // [n]
  int32_t* first_len;        // [n]
  const int64_t* rank;       // [n] inclusive scan of first (codes: may be null in a lookup)
  const int64_t* byte_off;   // [n + 1] exclusive scan of first_len (commit)
  uint64_t old_bytes;        // commit: bytes of the entries before the call
  int32_t* codes;            // [n]
};

TC_HD inline uint64_t td_mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

// The term of word i (bytes 8 i .. 8 i + 7 of the value, little endian, zero padded past the end).
TC_HD inline uint64_t td_term(uint64_t i, uint64_t w) { return td_mix(w + (i + 1) * 0x9E3779B97F4A7C15ull); }

TC_HD inline uint64_t td_mask(uint64_t h, int32_t bits) { return bits >= 64 ? h : (bits <= 0 ? 0 : h & ((1ull << bits) - 1ull)); }

TC_HD inline uint64_t td_finish(uint64_t sum, uint64_t n, int32_t bits) {
  return td_mask(td_mix(sum ^ (n * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull)), bits);
}

// The first k <= 8 bytes at p as a little-endian word; nothing else is read.
TC_HD inline uint64_t td_word(const uint8_t* p, uint64_t k) {
  uint64_t w = 0;
  if (k >= 8) {
    __builtin_memcpy(&w, p, 8);                     // any byte phase
  } else {
    for (uint64_t j = 0; j < k; ++j) w |= (uint64_t)p[j] << (8 * j);
  }
  return w;
}

TC_HD inline uint64_t td_hash(const uint8_t* p, uint64_t n, int32_t bits) {
  uint64_t sum = 0;
  for (uint64_t i = 0; 8 * i < n; ++i) sum += td_term(i, td_word(p + 8 * i, n - 8 * i));
  return td_finish(sum, n, bits);
}

TC_HD inline bool td_equal(const uint8_t* p, const uint8_t* q, uint64_t n) {
  uint64_t i = 0;
  for (; i + 8 <= n; i += 8)
    if (td_word(p + i, 8) != td_word(q + i, 8)) return false;
  return td_word(p + i, n - i) == td_word(q + i, n - i);
}

// The bytes a non-empty slot stands for: an entry, or a pending row of this call.  False for a slot
// that names neither (it is then no match for anything, and nothing is read).
TC_HD inline bool td_candidate(const TextDictArgs& a, uint64_t v, const uint8_t** q, uint64_t* qn) {
  const uint32_t id = (uint32_t)v;
  if (id & kTdPending) {
    const uint64_t rr = id & ~kTdPending;
    uint64_t s, l;
    if (rr >= a.in.n || !tc_live(a.in, rr, &s, &l)) return false;
    *q = a.in.data + s;
    *qn = l;
    return true;
  }
  if (id >= a.D) return false;
  const int64_t b = a.ent_off[id], e = a.ent_off[id + 1];
  if (b < 0 || e < b || (uint64_t)e > a.ent_bytes) return false;
  *q = a.ent_data + b;
  *qn = (uint64_t)(e - b);
  return true;
}

// The three operations on a slot: atomic in the device pass (slots are read with relaxed atomic
// loads, so no read is hoisted out of a walk), plain in the serial host pass.
TC_HD inline uint64_t td_load(const uint64_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
TC_HD inline uint64_t td_cas(uint64_t* p, uint64_t expect, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS((unsigned long long*)p, (unsigned long long)expect, (unsigned long long)v);
#else
  const uint64_t old = *p;
  if (old == expect) *p = v;
  return old;
#endif
}
TC_HD inline void td_min(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin((unsigned long long*)p, (unsigned long long)v);
#else
  if (v < *p) *p = v;
#endif
}

// Probe for row r: the host loop, and one lane's work in kernel variant 0.
TC_HD inline void td_probe_one(const TextDictArgs& a, uint64_t r) {
  uint64_t s, n, h = 0;
  int32_t found = -1;
  if (tc_live(a.in, r, &s, &n)) {
    const uint8_t* p = a.in.data + s;
    h = td_hash(p, n, a.hash_bits);
    const uint64_t mask = a.capacity - 1, tag = h & kTdTagMask;
    const uint64_t mine = tag | kTdPending | r;
    uint64_t i = h & mask;
    for (uint64_t step = 0; step < a.capacity; ++step, i = (i + 1) & mask) {
      uint64_t v = td_load(&a.table[i]);
      if (v == kTdEmpty) {
        if (!a.insert) break;                       // a lookup: the value is not in the dictionary
        v = td_cas(&a.table[i], kTdEmpty, mine);
        if (v == kTdEmpty) {                        // claimed
          found = (int32_t)i;
          break;
        }
      }                                             // a lost race: v is what stands there now
      if ((v & kTdTagMask) != tag) continue;
      const uint8_t* q;
      uint64_t qn;
      if (!td_candidate(a, v, &q, &qn) || qn != n || !td_equal(p, q, n)) continue;
      if (((uint32_t)v & kTdPending) && a.insert) td_min(&a.table[i], mine);
      found = (int32_t)i;
      break;
    }
  }
  a.slot_of[r] = found;
  a.hash[r] = h;
}

TC_HD inline bool td_slot_ok(const TextDictArgs& a, int32_t s) { return s >= 0 && (uint64_t)s < a.capacity; }

TC_HD inline void td_first_one(const TextDictArgs& a, uint64_t r) {
  const int32_t s = a.slot_of[r];
  const bool f = td_slot_ok(a, s) && (uint32_t)a.table[s] == (kTdPending | (uint32_t)r);
  a.first[r] = f ? 1 : 0;
  a.first_len[r] = f ? a.in.length[r] : 0;          // a first row is live: its length is valid
}

TC_HD inline void td_codes_one(const TextDictArgs& a, uint64_t r) {
  const int32_t s = a.slot_of[r];
  int32_t code = -1;
  if (td_slot_ok(a, s)) {
    const uint64_t v = a.table[s];
    const uint32_t id = (uint32_t)v;
    if (v == kTdEmpty) {
    } else if (!(id & kTdPending)) {
      code = (int32_t)id;
    } else if (a.rank && (id & ~kTdPending) < a.in.n) {
      code = (int32_t)(a.D + (uint64_t)a.rank[id & ~kTdPending] - 1);
    }
  }
  a.codes[r] = code;
}

TC_HD inline void td_commit_one(const TextDictArgs& a, uint64_t r) {
  if (!a.first[r]) return;
  const int32_t s = a.slot_of[r];
  const uint64_t k = a.D + (uint64_t)a.rank[r] - 1;
  if (!td_slot_ok(a, s) || k >= a.ent_cap) return;
  a.table[s] = (a.hash[r] & kTdTagMask) | k;
  a.ent_hash[k] = a.hash[r];
  a.ent_off[k + 1] = (int64_t)a.old_bytes + a.byte_off[r + 1];
}

// Entry e into a table that holds none of the entries' keys twice: the first empty slot of its
// chain, no byte compares (the entries are distinct).
TC_HD inline void td_rehash_one(const TextDictArgs& a, uint64_t e) {
  const uint64_t h = td_mask(a.ent_hash[e], a.hash_bits), mask = a.capacity - 1;
  uint64_t i = h & mask;
  for (uint64_t step = 0; step < a.capacity; ++step, i = (i + 1) & mask)
    if (td_cas(&a.table[i], kTdEmpty, (h & kTdTagMask) | e) == kTdEmpty) return;
}

inline bool td_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// What every pass checks: the table, the counts and the quote-free scalars.
inline bool text_dict_scalars_ok(const TextDictArgs& a) {
  return td_pow2(a.capacity) && a.capacity <= kTdMaxCapacity && a.in.n <= kTdMaxRows && a.D < (1ull << 31) &&
         a.D + a.in.n < (1ull << 31) && a.hash_bits >= 0 && a.hash_bits <= 64;
}
// The bounded walk of probe always meets an empty slot when the table is at most half full.
inline bool text_dict_probe_fits(const TextDictArgs& a) {
  return a.capacity >= 2 * (a.D + (a.insert ? a.in.n : 0)) && a.D <= a.ent_cap;
}

// The host loops.  The caller has checked the scalars and the pointers.
inline void text_dict_probe_host(const TextDictArgs& a) {
  for (uint64_t r = 0; r < a.in.n; ++r) td_probe_one(a, r);
}
inline void text_dict_first_host(const TextDictArgs& a) {
  for (uint64_t r = 0; r < a.in.n; ++r) td_first_one(a, r);
}
inline void text_dict_codes_host(const TextDictArgs& a) {
  for (uint64_t r = 0; r < a.in.n; ++r) td_codes_one(a, r);
}
inline void text_dict_commit_host(const TextDictArgs& a) {
  for (uint64_t r = 0; r < a.in.n; ++r) td_commit_one(a, r);
}
inline void text_dict_rehash_host(const TextDictArgs& a) {
  for (uint64_t e = 0; e < a.D; ++e) td_rehash_one(a, e);
}

}  // namespace amdx
