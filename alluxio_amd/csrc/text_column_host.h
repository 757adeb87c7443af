// Text columns from spans: the rule, as plain C++.  A value is data[start, start + length), the
// content of a field as a span column of field_parse_host.h describes it (enclosing quotes and
// blanks already off).  Its output is the same bytes with every maximal run of k consecutive quote
// bytes shortened to ceil(k / 2) of them, which is content.replace(qq, q) in Python and the reading
// of an RFC 4180 field of a well-formed file.  The rule is applied whether or not the field was
// enclosed in quotes; a lone quote stays and is not an error.  quote = -1: the bytes unchanged.
//
// A value is live when its status is 0 (or there is no status array) and it lies inside
// [0, data_bytes); every other value has output length 0 and none of its bytes is read.
//
// Two passes: measure (out_len[r]) and, after the caller's exclusive scan of out_len into
// offsets[n + 1], emit, which recomputes the collapse and writes value r at out[offsets[r] ...].
// Emit trusts no offset: a byte goes out only inside [offsets[r], offsets[r + 1]) cut to
// [0, out_bytes), so offsets that disagree with the data lose bytes and never write elsewhere.
//
// Written once and compiled twice, as field_parse_host.h is: the host loop (CPU batches, CPU-only
// use, the stand-alone check program) and, through TC_HD, the device code of text_column.hip.  No
// HIP include.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define TC_HD __attribute__((host)) __attribute__((device))
#else
#define TC_HD
#endif

namespace amdx {

struct TextColumnArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* start;      // [n] offset of the value in data
  const int32_t* length;     // [n] bytes
  const uint8_t* status;     // [n], or null: every value inside the buffer is live
  uint64_t n;
  int32_t quote;             // one byte, or -1: none
  int32_t* out_len;          // measure: [n]
  const int64_t* offsets;    // emit: [n + 1]
  uint8_t* out;              // emit: [out_bytes]
  uint64_t out_bytes;
};

// The bytes of value r, or false when it is not live (it is not read then).
TC_HD inline bool tc_live(const TextColumnArgs& a, uint64_t r, uint64_t* start, uint64_t* len) {
  if (a.status && a.status[r] != 0) return false;
  const int64_t s = a.start[r];
  const int64_t l = (int64_t)a.length[r];
  if (s < 0 || l < 0 || (uint64_t)s > a.data_bytes || (uint64_t)l > a.data_bytes - (uint64_t)s) return false;
  *start = (uint64_t)s;
  *len = (uint64_t)l;
  return true;
}

// The output bytes [*jlo, *jhi) of value r that emit may write, byte j at out[offsets[r] + j]:
// the window [offsets[r], offsets[r + 1]) cut to [0, out_bytes).  False: nothing may be written.
TC_HD inline bool tc_window(const TextColumnArgs& a, uint64_t r, int64_t* lo, uint64_t* jlo, uint64_t* jhi) {
  const int64_t b = a.offsets[r];
  int64_t e = a.offsets[r + 1];
  if (a.out_bytes < (uint64_t)INT64_MAX && e > (int64_t)a.out_bytes) e = (int64_t)a.out_bytes;
  if (e <= b || e <= 0) return false;
  *lo = b;
  *jlo = b < 0 ? 0 - (uint64_t)b : 0;               // the bytes that would land before the buffer
  *jhi = (uint64_t)e - (uint64_t)b;                 // no overflow: e > b and e > 0
  return true;
}

// The collapse of one value, byte by byte: the host loop, and one lane's work in kernel variant 0.
// Returns the output length; with out != null, output byte j in [jlo, jhi) is written to
// out[lo + j] (lo + j >= 0 there: see tc_window).
TC_HD inline uint32_t tc_value(const uint8_t* p, uint64_t n, int32_t quote, uint8_t* out, int64_t lo, uint64_t jlo,
                               uint64_t jhi) {
  uint32_t k = 0;
  bool odd = false;                                 // the run that ends at the previous byte has odd length
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t c = p[i];
    const bool q = quote >= 0 && c == (uint8_t)quote;
    const bool drop = q && odd;                     // the 2nd, 4th, ... of a run
    odd = q && !odd;
    if (drop) continue;
    if (out && k >= jlo && k < jhi) out[lo + (int64_t)k] = c;
    ++k;
  }
  return k;
}

TC_HD inline void tc_measure_one(const TextColumnArgs& a, uint64_t r) {
  uint64_t s, n;
  if (!tc_live(a, r, &s, &n)) {
    a.out_len[r] = 0;
    return;
  }
  a.out_len[r] = a.quote < 0 ? (int32_t)n : (int32_t)tc_value(a.data + s, n, a.quote, nullptr, 0, 0, 0);
}

TC_HD inline void tc_emit_one(const TextColumnArgs& a, uint64_t r) {
  uint64_t s, n, jlo, jhi;
  int64_t lo;
  if (!tc_live(a, r, &s, &n) || !tc_window(a, r, &lo, &jlo, &jhi)) return;
  tc_value(a.data + s, n, a.quote, a.out, lo, jlo, jhi);
}

// Kernel variant 1 takes a value in vectors of 16 bytes.  qm: bit j set where byte j of the vector
// is a quote; carry: the run that ends at the byte before the vector has odd length.  Returns the
// bits of the quotes to drop: those at an odd place (from 0) in their run, the run at bit 0 counted
// from the place the carry gives it.  p marks the quotes whose run starts at an odd position (a run
// at bit 0 with the carry starts "at -1"); it is filled along the runs in four doubling steps.
TC_HD inline uint32_t tc_drop16(uint32_t qm, uint32_t carry) {
  const uint32_t st = qm & ~(qm << 1);              // the first quote of every run
  uint32_t p = (st & 0xAAAAu) | (st & carry & 1u);
  uint32_t m = qm;
  p |= (p << 1) & m;
  m &= m << 1;
  p |= (p << 2) & m;
  m &= m << 2;
  p |= (p << 4) & m;
  m &= m << 4;
  p |= (p << 8) & m;
  return qm & (p ^ 0xAAAAu) & 0xFFFFu;
}

// The carry after a full vector that is not all quotes (such a vector hands its own carry on,
// because 16 is even): its last byte is a quote that is kept.
TC_HD inline uint32_t tc_carry_out16(uint32_t qm, uint32_t drop) { return ((qm & ~drop) >> 15) & 1u; }

inline bool text_column_scalars_ok(const TextColumnArgs& a) { return a.quote >= -1 && a.quote <= 255; }

// The host loops.  The caller has checked the scalars and the pointers.
inline void text_measure_host(const TextColumnArgs& a) {
  for (uint64_t r = 0; r < a.n; ++r) tc_measure_one(a, r);
}
inline void text_emit_host(const TextColumnArgs& a) {
  for (uint64_t r = 0; r < a.n; ++r) tc_emit_one(a, r);
}

}  // namespace amdx
