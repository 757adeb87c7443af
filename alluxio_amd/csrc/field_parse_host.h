// Typed columns from delimited text rows: the rule, as plain C++.  A row is data[off, off + len)
// without its terminator (and without the \r before a \n terminator); a separator splits it where
// an even number of quote bytes precedes it in the row; a field loses one pair of enclosing quotes,
// then blanks (0x20, 0x09) at both ends; what is left is parsed by the column's type.
//
// Everything here is written once and compiled twice: as the host loop (host batches, CPU-only
// use, the stand-alone check program) and, through FP_HD, as the device code that the kernels of
// field_parse.hip call for a located field.  No HIP include, so a stand-alone program can compile it.
//
// Floats: the device parses a float only where ONE correctly rounded fp64 operation is exact
// (Clinger's fast path): w = the digits without the point, e10 = exponent - fraction digits;
// w == 0 gives +-0.0, else with at most 19 significant digits, w <= 2^53 and |e10| <= 22 the value
// is double(w) * 10^e10 or double(w) / 10^-e10 with an exact power of ten.  Every other well-formed
// float gets status kFpDeferred and is resolved by the caller.  float32 is that float64 converted:
// two roundings by definition.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define FP_HD __attribute__((host)) __attribute__((device))
#else
#define FP_HD
#endif

namespace amdx {

enum : uint32_t { kFpSpan = 0, kFpInt64 = 1, kFpInt32 = 2, kFpFloat64 = 3, kFpFloat32 = 4 };
enum : uint8_t {
  kFpValid = 0,      // the parsed value
  kFpNone = 1,       // field absent or content empty: 0 for ints, NaN for floats, (0, 0) for spans
  kFpBad = 2,        // malformed, out of range, or a row outside the buffer
  kFpDeferred = 3,   // floats only: well-formed, outside the fast path; NaN until resolved
};

constexpr uint32_t kFieldParseMaxCols = 32;
constexpr uint32_t kFieldParseMaxField = 65535;

struct FieldParseCol {
  uint32_t field;    // field number in the row, from 0
  uint32_t type;     // kFp*
  void* values;      // [nrows] int64 / int32 / double / float; span: int64 start (offset into data)
  int32_t* length;   // [nrows] span only
  uint8_t* status;   // [nrows]
};

struct FieldParseArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* off;      // [nrows] bytes
  const void* len;         // [nrows] int32 or int64, bytes
  uint64_t nrows;
  uint32_t len_is_64;
  uint32_t sep;            // one byte
  int32_t quote;           // one byte, or -1: none
  uint32_t terminator;     // one byte
  uint32_t ncols;          // 1..kFieldParseMaxCols
  uint32_t max_field;      // the largest cols[i].field: the walk of a row ends after it
  FieldParseCol cols[kFieldParseMaxCols];
};

constexpr uint64_t kFpNaN64 = 0x7FF8000000000000ull;
constexpr uint32_t kFpNaN32 = 0x7FC00000u;

FP_HD inline bool fp_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }
FP_HD inline bool fp_blank(uint8_t c) { return c == 0x20 || c == 0x09; }

// The raw field p[b, e) -> its content: one pair of enclosing quotes off (never from a field of
// one byte), then blanks off both ends.
FP_HD inline void fp_content(const uint8_t* p, uint64_t* b, uint64_t* e, int32_t quote) {
  if (quote >= 0 && *e - *b >= 2 && p[*b] == (uint8_t)quote && p[*e - 1] == (uint8_t)quote) {
    ++*b;
    --*e;
  }
  while (*b < *e && fp_blank(p[*b])) ++*b;
  while (*e > *b && fp_blank(p[*e - 1])) --*e;
}

// [+-]?[0-9]+ inside the type's range.
FP_HD inline uint8_t fp_int(const uint8_t* p, uint64_t b, uint64_t e, bool is32, int64_t* out) {
  *out = 0;
  if (b == e) return kFpNone;
  bool neg = false;
  if (p[b] == '+' || p[b] == '-') {
    neg = p[b] == '-';
    ++b;
  }
  if (b == e) return kFpBad;
  while (b < e && p[b] == '0') ++b;                 // a digit was seen, or the loop below sees a byte
  uint64_t v = 0;
  uint32_t nd = 0;                                  // digits after the leading zeros, saturating
  for (; b < e; ++b) {
    if (!fp_digit(p[b])) return kFpBad;
    if (nd < 19) v = v * 10 + (uint64_t)(p[b] - '0');   // 19 digits stay below 10^19 < 2^64
    if (nd < 20) ++nd;
  }
  const uint64_t lim = (is32 ? 0x7FFFFFFFull : 0x7FFFFFFFFFFFFFFFull) + (neg ? 1u : 0u);
  if (nd > 19 || v > lim) return kFpBad;
  *out = (int64_t)(neg ? 0 - v : v);
  return kFpValid;
}

FP_HD inline double fp_pow10(int i) {               // exact: 10^22 = 2^22 * 5^22 and 5^22 < 2^53
  const double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[i];
}

FP_HD inline bool fp_word(const uint8_t* p, uint64_t n, const char* w, uint64_t wn) {
  if (n != wn) return false;
  for (uint64_t i = 0; i < n; ++i)
    if ((p[i] | 0x20) != (uint8_t)w[i]) return false;
  return true;
}

// [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? or [+-]?(nan|inf|infinity) in any case.
// *bits: the float64 bit pattern (the default quiet NaN unless the status is kFpValid).
FP_HD inline uint8_t fp_float(const uint8_t* p, uint64_t b, uint64_t e, uint64_t* bits) {
  *bits = kFpNaN64;
  if (b == e) return kFpNone;
  const uint64_t sign = p[b] == '-' ? 0x8000000000000000ull : 0ull;
  if (p[b] == '+' || p[b] == '-') ++b;
  if (b == e) return kFpBad;
  if ((p[b] | 0x20) == 'n' || (p[b] | 0x20) == 'i') {
    if (fp_word(p + b, e - b, "nan", 3)) return kFpValid;
    if (fp_word(p + b, e - b, "inf", 3) || fp_word(p + b, e - b, "infinity", 8)) {
      *bits = sign | 0x7FF0000000000000ull;
      return kFpValid;
    }
    return kFpBad;
  }
  uint64_t w = 0;
  uint32_t nd = 0;                                  // significant digits (leading zeros off), saturating
  int64_t fd = 0;                                   // fraction digits: at most the field's length
  bool any = false;
  for (; b < e && fp_digit(p[b]); ++b) {
    any = true;
    const uint32_t d = p[b] - '0';
    if (nd || d) {
      if (nd < 19) w = w * 10 + d;
      if (nd < 20) ++nd;
    }
  }
  if (b < e && p[b] == '.') {
    for (++b; b < e && fp_digit(p[b]); ++b) {
      any = true;
      ++fd;
      const uint32_t d = p[b] - '0';
      if (nd || d) {
        if (nd < 19) w = w * 10 + d;
        if (nd < 20) ++nd;
      }
    }
  }
  if (!any) return kFpBad;
  int64_t ex = 0;
  if (b < e && (p[b] | 0x20) == 'e') {
    ++b;
    bool eneg = false;
    if (b < e && (p[b] == '+' || p[b] == '-')) {
      eneg = p[b] == '-';
      ++b;
    }
    if (b == e || !fp_digit(p[b])) return kFpBad;
    for (; b < e && fp_digit(p[b]); ++b)
      if (ex < 100000) ex = ex * 10 + (p[b] - '0');  // clamped: any number of exponent digits is safe
    if (eneg) ex = -ex;
  }
  if (b != e) return kFpBad;
  if (nd == 0) {                                    // every digit is 0: +-0.0 whatever the exponent
    *bits = sign;
    return kFpValid;
  }
  const int64_t e10 = ex - fd;
  if (nd > 19 || w > (1ull << 53) || e10 > 22 || e10 < -22) return kFpDeferred;
  const double m = (double)w;                       // exact
  const double v = e10 >= 0 ? m * fp_pow10((int)e10) : m / fp_pow10((int)-e10);   // one rounding
  uint64_t vb;
  __builtin_memcpy(&vb, &v, 8);
  *bits = vb | sign;
  return kFpValid;
}

FP_HD inline void fp_store_float(const FieldParseCol& c, uint64_t r, uint64_t bits) {
  if (c.type == kFpFloat64) {
    static_cast<uint64_t*>(c.values)[r] = bits;
  } else {
    double d;
    __builtin_memcpy(&d, &bits, 8);
    const float f = (float)d;                       // the second rounding
    uint32_t fb;
    __builtin_memcpy(&fb, &f, 4);
    if (d != d) fb = kFpNaN32;
    static_cast<uint32_t*>(c.values)[r] = fb;
  }
}

// Row r of column c without a parsed value: status st.
FP_HD inline void fp_emit_none(const FieldParseCol& c, uint64_t r, uint8_t st) {
  switch (c.type) {
    case kFpSpan:
      static_cast<int64_t*>(c.values)[r] = 0;
      c.length[r] = 0;
      break;
    case kFpInt64: static_cast<int64_t*>(c.values)[r] = 0; break;
    case kFpInt32: static_cast<int32_t*>(c.values)[r] = 0; break;
    default: fp_store_float(c, r, kFpNaN64); break;
  }
  c.status[r] = st;
}

// Row r of column c from the raw field row[b, e); row_off: the row's offset in data.
FP_HD inline void fp_emit(const FieldParseCol& c, uint64_t r, const uint8_t* row, uint64_t row_off, uint64_t b,
                          uint64_t e, int32_t quote) {
  fp_content(row, &b, &e, quote);
  uint8_t st;
  switch (c.type) {
    case kFpSpan:
      static_cast<int64_t*>(c.values)[r] = (int64_t)(row_off + b);
      c.length[r] = (int32_t)(e - b);
      st = kFpValid;
      break;
    case kFpInt64:
    case kFpInt32: {
      int64_t v;
      st = fp_int(row, b, e, c.type == kFpInt32, &v);
      if (c.type == kFpInt32) static_cast<int32_t*>(c.values)[r] = (int32_t)v;
      else static_cast<int64_t*>(c.values)[r] = v;
      break;
    }
    default: {
      uint64_t bits;
      st = fp_float(row, b, e, &bits);
      fp_store_float(c, r, bits);
      break;
    }
  }
  c.status[r] = st;
}

// The row's bytes, or false when the row does not lie inside the buffer (it is not read then).
// *n: its length without the terminator.
FP_HD inline bool fp_row_bytes(const FieldParseArgs& a, uint64_t r, uint64_t* off, uint64_t* n) {
  const int64_t o = a.off[r];
  const int64_t l = a.len_is_64 ? static_cast<const int64_t*>(a.len)[r] : (int64_t)static_cast<const int32_t*>(a.len)[r];
  if (o < 0 || l < 0 || (uint64_t)o > a.data_bytes || (uint64_t)l > a.data_bytes - (uint64_t)o) return false;
  const uint8_t* row = a.data + o;
  uint64_t k = (uint64_t)l;
  if (k && row[k - 1] == (uint8_t)a.terminator) {
    --k;
    if (a.terminator == '\n' && k && row[k - 1] == '\r') --k;
  }
  *off = (uint64_t)o;
  *n = k;
  return true;
}

// One row, byte by byte with the quote parity in a register: the host loop, and one lane's work
// in kernel variant 0.
FP_HD inline void fp_row(const FieldParseArgs& a, uint64_t r) {
  uint64_t off, n;
  if (!fp_row_bytes(a, r, &off, &n)) {
    for (uint32_t j = 0; j < a.ncols; ++j) fp_emit_none(a.cols[j], r, kFpBad);
    return;
  }
  const uint8_t* row = a.data + off;
  uint32_t f = 0;                                   // number of the field that starts at fs
  uint64_t fs = 0;
  bool inside = false, open = true;                 // open: field f still runs to the end of the row
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t c = row[i];
    if (a.quote >= 0 && c == (uint8_t)a.quote) {
      inside = !inside;
    } else if (c == (uint8_t)a.sep && !inside) {
      for (uint32_t j = 0; j < a.ncols; ++j)
        if (a.cols[j].field == f) fp_emit(a.cols[j], r, row, off, fs, i, a.quote);
      ++f;
      fs = i + 1;
      if (f > a.max_field) {                        // nothing requested lies further right
        open = false;
        break;
      }
    }
  }
  if (open) {
    for (uint32_t j = 0; j < a.ncols; ++j)
      if (a.cols[j].field == f) fp_emit(a.cols[j], r, row, off, fs, n, a.quote);
    ++f;
  }
  for (uint32_t j = 0; j < a.ncols; ++j)
    if (a.cols[j].field >= f) fp_emit_none(a.cols[j], r, kFpNone);
}

// The scalars every path checks before it touches a row.
inline bool field_parse_scalars_ok(const FieldParseArgs& a) {
  if (a.sep > 255 || a.terminator > 255 || a.quote < -1 || a.quote > 255) return false;
  if (a.sep == a.terminator || a.quote == (int32_t)a.sep || a.quote == (int32_t)a.terminator) return false;
  if (a.ncols < 1 || a.ncols > kFieldParseMaxCols) return false;
  uint32_t mx = 0;
  for (uint32_t j = 0; j < a.ncols; ++j) {
    if (a.cols[j].field > kFieldParseMaxField || a.cols[j].type > kFpFloat32) return false;
    if (a.cols[j].field > mx) mx = a.cols[j].field;
  }
  return mx == a.max_field;
}

// The host loop.  The caller has checked the scalars.
inline void field_parse_host(const FieldParseArgs& a) {
  for (uint64_t r = 0; r < a.nrows; ++r) fp_row(a, r);
}

}  // namespace amdx
