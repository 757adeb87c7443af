// Column statistics for Parquet (null_count, min_value, max_value): the rules, as plain C++.  The
// segments of all columns are rows of one table of int64 laid out like the writer's page table
// (parquet_encode_host.h: kind, width, the addresses of values, status and offsets, the first row
// and the rows), with three columns of their own, and every segment has one result row (kPsCols).
//
// A row is a value under the writer's rule: its status is 0, for text its bytes lie inside the data
// (pe_text_window), for a category its code is inside the dictionary.  Every other row counts
// toward kPsNulls.
//
//   INT32, INT64  signed order.  BOOLEAN: false < true.
//   FLOAT, DOUBLE NaNs take no part (they are values: they count neither as nulls nor toward
//                 kPsValues).  A minimum that equals zero is -0.0, a maximum that equals zero +0.0.
//   text          unsigned bytewise lexicographic order, a proper prefix first.  A segment with a
//                 value longer than kPsTextCap bytes has a null count and no bounds.
//   category      the bounds are taken over the dictionary's entries whose code occurs in a value row:
//                 a mark pass clears mark[code] (the caller filled the array with 1), and the
//                 dictionary is a text segment of its own whose status array is that mark array.
//
// Every number becomes an int64 key whose signed order is the type's order (ps_key), so one pair of
// 64-bit atomics serves all widths; a float's key is its bits with all bits flipped if negative and
// the sign bit flipped if not, an order-preserving unsigned number that is then moved into the
// signed range.  Minimum and maximum do not depend on the order of the rows, so the host loops and
// the kernels give the same result rows.
//
// Text takes kPsRounds rounds over the same rows.  In round r every row still alive for the minimum
// (and, separately, for the maximum) forms a 64-bit key: bytes [7r, 7r + 7) of the value big-endian
// in the upper 56 bits, zero padded, and min(remaining, 7) in the low byte, which puts "ab" before
// "ab\0".  The segment's winner is the unsigned minimum (maximum) of the keys, and a row stays alive
// only if its key equals the winner, which it checks at the start of the next round.  Ten rounds
// cover 70 bytes, more than the cap.  The winners of the rounds, put together, are the bound.
//
// Written once and compiled twice, as parquet_encode_host.h is: the host loops (CPU columns, the
// stand-alone check program) and, through PQ_HD, the device code of parquet_stats.hip.
#pragma once
#include <cstdint>

#include "parquet_encode_host.h"

namespace amdx {

// Segment row: the columns of the page row (kPeKind .. kPeFlat), and
enum {
  kPsIsFloat = 13,  // fixed width: 1 when the values are IEEE floats of that width
  kPsMark = 14,     // dictionary index: address of the mark bytes (kPeAux of them), cleared for every code in use
};
// Result row.
enum {
  kPsNulls = 0,     // rows that are not values
  kPsValues = 1,    // values that take part in the bounds (a NaN does not)
  kPsMin = 2,       // numbers: the smallest key (the caller sets INT64_MAX)
  kPsMax = 3,       // numbers: the largest key (the caller sets INT64_MIN)
  kPsMaxLen = 4,    // text: the most bytes of a value
  kPsRoundMin = 8,  // text: the winner of each round, unsigned (the caller sets all bits)
  kPsRoundMax = 18, // text: the same for the maximum (the caller sets 0)
  kPsCols = 28
};
enum { kPsRounds = 10, kPsTextCap = 64 };
enum { kPsPassMark = 0, kPsPassFirst = 1, kPsPassRound = 2 };
enum { kPsAliveMin = 1, kPsAliveMax = 2 };

struct PsArgs {
  const int64_t* segs;    // [nsegs][kPeCols]
  uint64_t nsegs;
  uint64_t first;         // the launch covers segments [first, last)
  uint64_t last;
  uint64_t tiles;         // workgroups per segment
  uint32_t round;         // kPsPassRound: 1 .. kPsRounds - 1
  uint8_t* alive;         // [flat_n] text rows: kPsAliveMin | kPsAliveMax (null: no text segment)
  uint64_t flat_n;
  int64_t* results;       // [nsegs][kPsCols]
};

struct PsAcc {
  int64_t nulls, values, mn, mx, maxlen;
  uint64_t kmin, kmax;
};
PQ_HD inline PsAcc ps_acc() { return PsAcc{0, 0, INT64_MAX, INT64_MIN, 0, ~0ull, 0}; }

// The key of a number: v holds its bits, zero extended.  *nan: a float that is one.
PQ_HD inline int64_t ps_key(uint64_t v, uint32_t width, bool is_float, bool* nan) {
  *nan = false;
  if (!is_float) return width == 4 ? (int64_t)(int32_t)(uint32_t)v : (int64_t)v;
  if (width == 4) {
    const uint32_t b = (uint32_t)v;
    *nan = (b & 0x7FFFFFFFu) > 0x7F800000u;
    return (int64_t)((b & 0x80000000u) ? ~b : (b ^ 0x80000000u));     // 0 .. 2^32 - 1
  }
  *nan = (v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
  const uint64_t u = (v >> 63) ? ~v : (v ^ 0x8000000000000000ull);
  return (int64_t)(u ^ 0x8000000000000000ull);
}

// The bits of the number whose key is `key`, with the zero rule for a bound: -0.0 as a minimum,
// +0.0 as a maximum.
PQ_HD inline uint64_t ps_unkey(int64_t key, uint32_t width, bool is_float, bool is_max) {
  if (!is_float) return width == 4 ? (uint64_t)(uint32_t)(int32_t)key : (uint64_t)key;
  if (width == 4) {
    const uint32_t u = (uint32_t)key;
    const uint32_t b = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
    if ((b & 0x7FFFFFFFu) == 0) return is_max ? 0u : 0x80000000u;
    return b;
  }
  const uint64_t u = (uint64_t)key ^ 0x8000000000000000ull;
  const uint64_t b = (u >> 63) ? (u ^ 0x8000000000000000ull) : ~u;
  if ((b & 0x7FFFFFFFFFFFFFFFull) == 0) return is_max ? 0ull : 0x8000000000000000ull;
  return b;
}

// The key of round `round` of the text value p[0, len).
PQ_HD inline uint64_t ps_text_key(const uint8_t* p, int64_t len, uint32_t round) {
  const int64_t pos = 7 * (int64_t)round;
  const int64_t rem = len > pos ? len - pos : 0;
  const uint32_t cnt = rem < 7 ? (uint32_t)rem : 7u;
  uint64_t key = cnt;
  for (uint32_t j = 0; j < cnt; ++j) key |= (uint64_t)p[pos + j] << (56 - 8 * j);
  return key;
}

// Whether row r of the segment's column is a value; for text its window.
PQ_HD inline bool ps_is_value(const int64_t* sg, uint64_t r, int64_t* off, int64_t* len) {
  const uint8_t* status = pe_ptr<const uint8_t>(sg[kPeStatus]);
  if (status && status[r] != 0) return false;
  if (sg[kPeKind] == kPeText) return pe_text_window(sg, r, off, len);
  if (sg[kPeKind] == kPeIndex) {
    const int64_t code = pe_ptr<const int32_t>(sg[kPeValues])[r];
    return code >= 0 && code < sg[kPeAux];
  }
  return true;
}

// mark: row i of a dictionary-index segment clears the mark of its code.
PQ_HD inline void ps_mark_row(const int64_t* sg, uint64_t i) {
  if (sg[kPeKind] != kPeIndex || !sg[kPsMark]) return;
  const uint64_t r = (uint64_t)sg[kPeRow] + i;
  int64_t off = 0, len = 0;
  if (!ps_is_value(sg, r, &off, &len)) return;
  pe_ptr<uint8_t>(sg[kPsMark])[pe_ptr<const int32_t>(sg[kPeValues])[r]] = 0;
}

// first: row i of any segment.  Numbers: their key into the bounds.  Text: round 0.
PQ_HD inline void ps_first_row(const PsArgs& a, const int64_t* sg, uint64_t i, PsAcc& c) {
  const uint64_t r = (uint64_t)sg[kPeRow] + i, f = (uint64_t)sg[kPeFlat] + i;
  const int64_t kind = sg[kPeKind];
  int64_t off = 0, len = 0;
  const bool value = ps_is_value(sg, r, &off, &len);
  if (kind == kPeText && a.alive && f < a.flat_n) a.alive[f] = value ? (kPsAliveMin | kPsAliveMax) : 0;
  if (!value) {
    ++c.nulls;
    return;
  }
  if (kind == kPeText) {
    if (!a.alive || f >= a.flat_n) return;
    ++c.values;
    if (len > c.maxlen) c.maxlen = len;
    const uint64_t key = ps_text_key(pe_ptr<const uint8_t>(sg[kPeValues]) + off, len, 0);
    if (key < c.kmin) c.kmin = key;
    if (key > c.kmax) c.kmax = key;
    return;
  }
  if (kind == kPeIndex) {
    ++c.values;
    return;
  }
  const uint32_t w = (uint32_t)sg[kPeWidth];
  uint64_t v;
  if (kind == kPeBool) v = pe_ptr<const uint8_t>(sg[kPeValues])[r] != 0;
  else if (w == 8) v = pe_ptr<const uint64_t>(sg[kPeValues])[r];
  else if (w == 4) v = pe_ptr<const uint32_t>(sg[kPeValues])[r];
  else return;
  bool nan = false;
  const int64_t key = ps_key(v, kind == kPeBool ? 8 : w, kind == kPeFixed && sg[kPsIsFloat] != 0, &nan);
  if (nan) return;
  ++c.values;
  if (key < c.mn) c.mn = key;
  if (key > c.mx) c.mx = key;
}

// round: row i of a text segment in round a.round >= 1.  res: the segment's result row, whose
// winners of round a.round - 1 are final.
PQ_HD inline void ps_round_row(const PsArgs& a, const int64_t* sg, const int64_t* res, uint64_t i, PsAcc& c) {
  const uint64_t r = (uint64_t)sg[kPeRow] + i, f = (uint64_t)sg[kPeFlat] + i;
  if (sg[kPeKind] != kPeText || !a.alive || f >= a.flat_n || a.round < 1 || a.round >= kPsRounds) return;
  const uint8_t was = a.alive[f];
  if (!was) return;
  int64_t off = 0, len = 0;
  if (!pe_text_window(sg, r, &off, &len)) return;
  const uint8_t* p = pe_ptr<const uint8_t>(sg[kPeValues]) + off;
  const uint64_t prev = ps_text_key(p, len, a.round - 1);
  uint8_t now = was;
  if ((now & kPsAliveMin) && prev != (uint64_t)res[kPsRoundMin + a.round - 1]) now &= (uint8_t)~kPsAliveMin;
  if ((now & kPsAliveMax) && prev != (uint64_t)res[kPsRoundMax + a.round - 1]) now &= (uint8_t)~kPsAliveMax;
  if (now != was) a.alive[f] = now;
  if (!now) return;
  const uint64_t key = ps_text_key(p, len, a.round);
  if ((now & kPsAliveMin) && key < c.kmin) c.kmin = key;
  if ((now & kPsAliveMax) && key > c.kmax) c.kmax = key;
}

// A bound of a text segment from the winners of its rounds (k: kPsRoundMin or kPsRoundMax) into
// out[kPsTextCap]; returns its length.  Only for a segment with values, none above the cap.
inline uint32_t ps_text_bound(const int64_t* res, int k, uint8_t* out) {
  uint32_t n = 0;
  for (uint32_t r = 0; r < kPsRounds; ++r) {
    const uint64_t key = (uint64_t)res[k + r];
    const uint32_t cnt = (uint32_t)(key & 0xFF) > 7 ? 7 : (uint32_t)(key & 0xFF);
    for (uint32_t j = 0; j < cnt && n < kPsTextCap; ++j) out[n++] = (uint8_t)(key >> (56 - 8 * j));
    if (cnt < 7) break;
  }
  return n;
}

// What a segment's result row says, as the format stores it.  Returns false when there are no
// bounds (no value, only NaNs, or text above the cap); else mn / mx hold the PLAIN bytes of the
// bounds (no length prefix for text, one byte for a boolean) and *nmin / *nmax their lengths.
// A dictionary-index segment has no bounds of its own: its dictionary's segment has them.
inline bool ps_finish(const int64_t* res, int64_t kind, uint32_t width, bool is_float, uint8_t* mn, uint32_t* nmin,
                      uint8_t* mx, uint32_t* nmax) {
  *nmin = *nmax = 0;
  if (res[kPsValues] <= 0 || kind == kPeIndex) return false;
  if (kind == kPeText) {
    if (res[kPsMaxLen] > kPsTextCap) return false;
    *nmin = ps_text_bound(res, kPsRoundMin, mn);
    *nmax = ps_text_bound(res, kPsRoundMax, mx);
    return true;
  }
  if (res[kPsMin] > res[kPsMax]) return false;
  if (kind == kPeBool) {
    mn[0] = res[kPsMin] != 0;
    mx[0] = res[kPsMax] != 0;
    *nmin = *nmax = 1;
    return true;
  }
  if (width != 4 && width != 8) return false;
  const uint64_t lo = ps_unkey(res[kPsMin], width, is_float, false), hi = ps_unkey(res[kPsMax], width, is_float, true);
  for (uint32_t j = 0; j < width; ++j) {
    mn[j] = (uint8_t)(lo >> (8 * j));
    mx[j] = (uint8_t)(hi >> (8 * j));
  }
  *nmin = *nmax = width;
  return true;
}

// One pass's sums of a segment into its result row (the host form; the kernels use atomics).
inline void ps_fold(int64_t* res, const PsAcc& c, int pass, uint32_t round) {
  if (pass == kPsPassFirst) {
    res[kPsNulls] += c.nulls;
    res[kPsValues] += c.values;
    if (c.mn < res[kPsMin]) res[kPsMin] = c.mn;
    if (c.mx > res[kPsMax]) res[kPsMax] = c.mx;
    if (c.maxlen > res[kPsMaxLen]) res[kPsMaxLen] = c.maxlen;
  }
  if (c.kmin < (uint64_t)res[kPsRoundMin + round]) res[kPsRoundMin + round] = (int64_t)c.kmin;
  if (c.kmax > (uint64_t)res[kPsRoundMax + round]) res[kPsRoundMax + round] = (int64_t)c.kmax;
}

// ---- the host loops ---------------------------------------------------------------------------------
inline void parquet_stats_host(const PsArgs& a, int pass) {
  for (uint64_t s = a.first; s < a.last; ++s) {
    const int64_t* sg = a.segs + s * kPeCols;
    int64_t* res = a.results + s * kPsCols;
    const uint64_t rows = (uint64_t)sg[kPeRows];
    if (pass == kPsPassMark) {
      for (uint64_t i = 0; i < rows; ++i) ps_mark_row(sg, i);
      continue;
    }
    PsAcc c = ps_acc();
    if (pass == kPsPassFirst) {
      for (uint64_t i = 0; i < rows; ++i) ps_first_row(a, sg, i, c);
      ps_fold(res, c, pass, 0);
    } else if (sg[kPeKind] == kPeText) {
      for (uint64_t i = 0; i < rows; ++i) ps_round_row(a, sg, res, i, c);
      ps_fold(res, c, pass, a.round);
    }
  }
}

}  // namespace amdx
