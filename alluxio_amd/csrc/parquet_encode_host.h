// Typed columns into Parquet pages: the rules, as plain C++.  The write side of parquet_host.h.  All
// pages of all columns of a row group are rows of one table of int64 (kPeCols each) that the caller
// lays out, and everything is written into one row-group buffer at offsets that the caller chose:
//
//   measure  one row per lane: a flag per row (1: a value) into a flat array that the caller scans
//            into ranks, for a text row its 4 + length, and per page the valid rows, the rows whose
//            status is above 1 (or whose text does not lie inside its data), the text bytes, the
//            largest live code and the live codes outside the dictionary.
//   rows     one row per lane: the level bits of the page (bit i of the stream is row i of the
//            page, least significant first, zero bits after the last row), a fixed-width value to
//            slot `rank` of the page's PLAIN area at any byte phase, a boolean or a dictionary
//            index to slot `rank` of the page's part of a scratch array of int32.
//   text     a PLAIN BYTE_ARRAY value per group of lanes: the 4-byte little-endian length, then the
//            bytes.  A page without a status array is a dictionary page: every row is a value.
//   pack     one output byte per lane: the scratch values that overlap the byte, `width` bits each,
//            least significant first (PLAIN booleans: width 1; a bit-packed run of indices).
//   copy     the bytes the host built (Thrift PageHeaders, level lengths, run headers, width bytes)
//            from one blob to their places.
//
// A row is a value when its status is 0 (and, for text, its bytes lie inside the data).  rank is the
// exclusive prefix sum of the flags, taken relative to the page's first row.  Every store is checked
// against the area the table names and against the buffer's size; what does not fit is not written.
//
// Written once and compiled twice, as parquet_host.h is: the host loops (CPU columns, the
// stand-alone check program) and, through PQ_HD, the device code of parquet_encode.hip.
#pragma once
#include <cstdint>

#include "parquet_host.h"

namespace amdx {

// Page row.
enum {
  kPeKind = 0,      // 0 fixed width, 1 boolean, 2 text, 3 dictionary index
  kPeWidth = 1,     // fixed: bytes of a value (4 or 8); index: bits of a value (1 to 32); boolean: 1
  kPeValues = 2,    // address of the column's values (fixed), bytes (boolean: one each), packed text
                    // data (text) or int32 codes (index)
  kPeStatus = 3,    // address of the column's status bytes; 0: every row is a value
  kPeOffsets = 4,   // text: address of the int64 offsets (value r is data[offsets[r], offsets[r + 1]))
  kPeAux = 5,       // text: bytes of the data; index: entries of the dictionary
  kPeRow = 6,       // the page's first row in the column's arrays
  kPeRows = 7,      // rows of the page
  kPeFlat = 8,      // the page's first slot in the flat arrays (flags, ranks, text sizes, scratch)
  kPeLevelOff = 9,  // where the page's level bits go in the buffer; -1: none are written
  kPeValOff = 10,   // the page's value area in the buffer
  kPeValBytes = 11,
  kPeNumValid = 12, // pack: the values of the page
  kPeCols = 16
};
enum { kPeFixed = 0, kPeBool = 1, kPeText = 2, kPeIndex = 3 };
// Measure row.
enum { kPmValid = 0, kPmBad = 1, kPmTextBytes = 2, kPmMaxCode = 3, kPmOutside = 4, kPmCols = 8 };
// Copy row.
enum { kPcSrc = 0, kPcDst = 1, kPcLen = 2, kPcCols = 3 };
enum { kPePassMeasure = 0, kPePassRows = 1, kPePassText = 2, kPePassPack = 3, kPePassCopy = 4 };

struct PeArgs {
  const int64_t* pages;   // [npages][kPeCols]
  uint64_t npages;
  uint64_t first;         // the launch covers pages [first, last)
  uint64_t last;
  uint64_t tiles;         // workgroups per page
  uint8_t* flags;         // [flat_n] 1: the row is a value
  int32_t* text_bytes;    // [flat_n] 4 + length of a text value, 0 for any other row (null: no text column)
  const int64_t* rank;    // [flat_n + 1] exclusive scan of flags
  const int64_t* text_at; // [flat_n + 1] exclusive scan of text_bytes
  int32_t* scratch;       // [flat_n] booleans and indices by rank
  uint64_t flat_n;
  int64_t* measure;       // [npages][kPmCols]
  uint8_t* out;           // the row-group buffer
  uint64_t out_bytes;
  const uint8_t* blob;    // copy: the host-built bytes
  uint64_t blob_bytes;
  const int64_t* segs;    // [nsegs][kPcCols]
  uint64_t nsegs;
};

struct PeCount {
  int64_t valid, bad, text_bytes, max_code, outside;
};

template <typename T>
PQ_HD inline T* pe_ptr(int64_t v) { return reinterpret_cast<T*>((uintptr_t)v); }

// The text value of row r of the column: false when it does not lie inside the data.
PQ_HD inline bool pe_text_window(const int64_t* pg, uint64_t r, int64_t* off, int64_t* len) {
  const int64_t* o = pe_ptr<const int64_t>(pg[kPeOffsets]);
  const int64_t a = o[r], b = o[r + 1];
  if (a < 0 || b < a || b > pg[kPeAux] || b - a > 0x7FFFFFFFll - 4) return false;
  *off = a;
  *len = b - a;
  return true;
}

// Row i of page pg: its flag and text size into the flat arrays, its counts into c.
PQ_HD inline void pe_measure_row(const PeArgs& a, const int64_t* pg, uint64_t i, PeCount& c) {
  const uint64_t r = (uint64_t)pg[kPeRow] + i, f = (uint64_t)pg[kPeFlat] + i;
  if (f >= a.flat_n) return;
  const uint8_t* status = pe_ptr<const uint8_t>(pg[kPeStatus]);
  const uint8_t st = status ? status[r] : 0;
  bool valid = st == 0;
  int32_t tb = 0;
  if (st > 1) ++c.bad;
  if (valid && pg[kPeKind] == kPeText) {
    int64_t off = 0, len = 0;
    if (pe_text_window(pg, r, &off, &len)) {
      tb = (int32_t)(4 + len);
      c.text_bytes += tb;
    } else {
      valid = false;
      ++c.bad;
    }
  } else if (valid && pg[kPeKind] == kPeIndex) {
    const int64_t code = pe_ptr<const int32_t>(pg[kPeValues])[r];
    if (code < 0 || code >= pg[kPeAux]) ++c.outside;
    else if (code > c.max_code) c.max_code = code;
  }
  if (valid) ++c.valid;
  a.flags[f] = valid ? 1 : 0;
  if (a.text_bytes) a.text_bytes[f] = tb;
}

// Whether [off, off + n) of the page's value area is inside the area and the area inside the buffer.
PQ_HD inline bool pe_area_ok(const PeArgs& a, const int64_t* pg, uint64_t off, uint64_t n) {
  const int64_t vo = pg[kPeValOff], vb = pg[kPeValBytes];
  if (vo < 0 || vb < 0 || (uint64_t)vo > a.out_bytes || (uint64_t)vb > a.out_bytes - (uint64_t)vo) return false;
  return off <= (uint64_t)vb && n <= (uint64_t)vb - off;
}

PQ_HD inline bool pe_is_value(const PeArgs& a, const int64_t* pg, uint64_t i) {
  if (!pg[kPeStatus]) return true;
  const uint64_t f = (uint64_t)pg[kPeFlat] + i;
  return f < a.flat_n && a.flags[f] != 0;
}

PQ_HD inline uint64_t pe_rank(const PeArgs& a, const int64_t* pg, uint64_t i) {
  if (!pg[kPeStatus]) return i;
  return (uint64_t)(a.rank[(uint64_t)pg[kPeFlat] + i] - a.rank[pg[kPeFlat]]);
}

// Byte b of the page's level bits, from the flags (the host form; a wave's ballot gives eight at once).
PQ_HD inline void pe_level_byte(const PeArgs& a, const int64_t* pg, uint64_t b) {
  const uint64_t rows = (uint64_t)pg[kPeRows];
  const int64_t lo = pg[kPeLevelOff];
  if (lo < 0 || (uint64_t)lo >= a.out_bytes || b >= a.out_bytes - (uint64_t)lo) return;
  uint32_t v = 0;
  for (uint32_t j = 0; j < 8; ++j) {
    const uint64_t i = 8 * b + j;
    if (i < rows && pe_is_value(a, pg, i)) v |= 1u << j;
  }
  a.out[(uint64_t)lo + b] = (uint8_t)v;
}

// A valid row i of a page that is not text: its value to its slot.
PQ_HD inline void pe_emit_value(const PeArgs& a, const int64_t* pg, uint64_t i) {
  const uint64_t r = (uint64_t)pg[kPeRow] + i, rank = pe_rank(a, pg, i);
  const int64_t kind = pg[kPeKind];
  if (kind == kPeFixed) {
    const uint64_t w = (uint64_t)pg[kPeWidth];
    if ((w != 4 && w != 8) || !pe_area_ok(a, pg, rank * w, w)) return;
    uint8_t* q = a.out + (uint64_t)pg[kPeValOff] + rank * w;      // any byte phase
    if (w == 8) {
      const uint64_t v = pe_ptr<const uint64_t>(pg[kPeValues])[r];
      __builtin_memcpy(q, &v, 8);
    } else {
      const uint32_t v = pe_ptr<const uint32_t>(pg[kPeValues])[r];
      __builtin_memcpy(q, &v, 4);
    }
  } else if (kind == kPeBool || kind == kPeIndex) {
    const uint64_t s = (uint64_t)pg[kPeFlat] + rank;
    if (rank >= (uint64_t)pg[kPeRows] || s >= a.flat_n) return;
    a.scratch[s] = kind == kPeBool ? (int32_t)(pe_ptr<const uint8_t>(pg[kPeValues])[r] != 0)
                                   : pe_ptr<const int32_t>(pg[kPeValues])[r];
  }
}

// Row i of a text page, by lane `lane` of `lanes`: the lanes share the value's bytes in pieces of 16,
// lane 0 writes the length.
PQ_HD inline void pe_emit_text(const PeArgs& a, const int64_t* pg, uint64_t i, uint32_t lane, uint32_t lanes) {
  if (!pe_is_value(a, pg, i)) return;
  const uint64_t r = (uint64_t)pg[kPeRow] + i;
  int64_t off = 0, len = 0;
  if (!pe_text_window(pg, r, &off, &len)) return;
  uint64_t at;
  if (pg[kPeStatus]) {
    at = (uint64_t)(a.text_at[(uint64_t)pg[kPeFlat] + i] - a.text_at[pg[kPeFlat]]);
  } else {                                            // a dictionary page: the entries are packed
    const int64_t* o = pe_ptr<const int64_t>(pg[kPeOffsets]);
    at = (uint64_t)(off - o[pg[kPeRow]]) + 4 * i;
  }
  if (!pe_area_ok(a, pg, at, 4 + (uint64_t)len)) return;
  uint8_t* q = a.out + (uint64_t)pg[kPeValOff] + at;
  if (lane == 0) {
    const uint32_t l = (uint32_t)len;
    __builtin_memcpy(q, &l, 4);
  }
  q += 4;
  const uint8_t* p = pe_ptr<const uint8_t>(pg[kPeValues]) + off;
  for (uint64_t pos = (uint64_t)lane * 16; pos < (uint64_t)len; pos += (uint64_t)lanes * 16) {
    const uint64_t rem = (uint64_t)len - pos;
    if (rem >= 16) {
      __builtin_memcpy(q + pos, p + pos, 16);
    } else {
      for (uint64_t j = 0; j < rem; ++j) q[pos + j] = p[pos + j];
    }
  }
}

// Byte b of the packed area of a boolean or index page: the values whose bits overlap it.
PQ_HD inline void pe_pack_byte(const PeArgs& a, const int64_t* pg, uint64_t b) {
  const uint64_t w = (uint64_t)pg[kPeWidth], n = (uint64_t)pg[kPeNumValid], flat = (uint64_t)pg[kPeFlat];
  if (w < 1 || w > 32 || !pe_area_ok(a, pg, b, 1)) return;
  const uint64_t bit0 = 8 * b;
  const uint64_t mask = w == 32 ? 0xFFFFFFFFull : ((1ull << w) - 1ull);
  uint64_t v = 0;
  for (uint64_t k = bit0 / w; k < n && k * w < bit0 + 8; ++k) {
    if (flat + k >= a.flat_n) break;
    const uint64_t x = (uint64_t)(uint32_t)a.scratch[flat + k] & mask;
    const uint64_t at = k * w;
    v |= at >= bit0 ? x << (at - bit0) : x >> (bit0 - at);
  }
  a.out[(uint64_t)pg[kPeValOff] + b] = (uint8_t)v;
}

// Segment s of the host-built bytes, by lane `lane` of `lanes`.
PQ_HD inline void pe_copy_seg(const PeArgs& a, uint64_t s, uint32_t lane, uint32_t lanes) {
  const int64_t* g = a.segs + s * kPcCols;
  const int64_t src = g[kPcSrc], dst = g[kPcDst], len = g[kPcLen];
  if (src < 0 || dst < 0 || len < 0 || (uint64_t)src > a.blob_bytes || (uint64_t)len > a.blob_bytes - (uint64_t)src ||
      (uint64_t)dst > a.out_bytes || (uint64_t)len > a.out_bytes - (uint64_t)dst)
    return;
  for (uint64_t j = lane; j < (uint64_t)len; j += lanes) a.out[(uint64_t)dst + j] = a.blob[(uint64_t)src + j];
}

// ---- the host loops ---------------------------------------------------------------------------------
inline void parquet_encode_measure_host(const PeArgs& a) {
  for (uint64_t p = a.first; p < a.last; ++p) {
    const int64_t* pg = a.pages + p * kPeCols;
    PeCount c{0, 0, 0, -1, 0};
    for (uint64_t i = 0; i < (uint64_t)pg[kPeRows]; ++i) pe_measure_row(a, pg, i, c);
    int64_t* m = a.measure + p * kPmCols;
    m[kPmValid] += c.valid;
    m[kPmBad] += c.bad;
    m[kPmTextBytes] += c.text_bytes;
    if (c.max_code > m[kPmMaxCode]) m[kPmMaxCode] = c.max_code;
    m[kPmOutside] += c.outside;
  }
}
inline void parquet_encode_rows_host(const PeArgs& a) {
  for (uint64_t p = a.first; p < a.last; ++p) {
    const int64_t* pg = a.pages + p * kPeCols;
    const uint64_t rows = (uint64_t)pg[kPeRows];
    if (pg[kPeLevelOff] >= 0)
      for (uint64_t b = 0; b < (rows + 7) / 8; ++b) pe_level_byte(a, pg, b);
    if (pg[kPeKind] == kPeText) continue;
    for (uint64_t i = 0; i < rows; ++i)
      if (pe_is_value(a, pg, i)) pe_emit_value(a, pg, i);
  }
}
inline void parquet_encode_text_host(const PeArgs& a) {
  for (uint64_t p = a.first; p < a.last; ++p) {
    const int64_t* pg = a.pages + p * kPeCols;
    if (pg[kPeKind] != kPeText) continue;
    for (uint64_t i = 0; i < (uint64_t)pg[kPeRows]; ++i) pe_emit_text(a, pg, i, 0, 1);
  }
}
inline void parquet_encode_pack_host(const PeArgs& a) {
  for (uint64_t p = a.first; p < a.last; ++p) {
    const int64_t* pg = a.pages + p * kPeCols;
    if (pg[kPeKind] != kPeBool && pg[kPeKind] != kPeIndex) continue;
    for (uint64_t b = 0; b < (uint64_t)pg[kPeValBytes]; ++b) pe_pack_byte(a, pg, b);
  }
}
inline void parquet_encode_copy_host(const PeArgs& a) {
  for (uint64_t s = 0; s < a.nsegs; ++s) pe_copy_seg(a, s, 0, 1);
}

}  // namespace amdx
