// Typed columns from JSON Lines rows: the rule, as plain C++.  A row is data[off, off + len)
// without its terminator (and without the \r before a \n terminator), as in field_parse_host.h.
// The values of the requested top-level keys are located in one walk over the row and typed.
//
// This is the record structure of well-formed files, the same stance the quote-aware record index
// takes.  It is not a JSON validator.
//
// The walk keeps two things.  Inside a string: a " toggles it unless that " is the code byte of an
// escape; in a maximal run of backslashes those at even places (from 0) start an escape and the
// byte after an escape start is its code (whether or not the run lies in a string).  Depth:
// outside strings { and [ add one, } and ] subtract one; bracket kinds are not matched.
//
// A row is well-formed enough when its first non-whitespace byte is {, the depth first returns to
// 0 at a }, only whitespace (0x20 0x09 0x0A 0x0D) follows that } and the row does not end inside a
// string (which the second condition implies).  Any other row gives status 2 in every column; an
// empty or whitespace-only row gives status 1; a row outside the buffer is not read and gives 2.
//
// A member starts after the opening { or after a depth-1 comma outside strings.  Its key is the
// trimmed bytes before the first depth-1 colon outside strings in the member, its value the
// trimmed bytes from after that colon to the next depth-1 comma or the closing }.  A member
// matches a requested name when its key bytes are exactly " name ": a key written with an escape
// sequence in the file is never matched.  The last matching member wins; no match is status 1.
//
// Typing the value bytes v: empty is status 2; null is status 1 for every type; a span is v as it
// stands; an int is -?(0|[1-9][0-9]*) then fp_int; a float is
// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)? then fp_float (so NaN, Infinity, +1, 01, 1. and
// .5 are status 2, stricter than json.loads' defaults; status 3 is deferred as in the CSV path); a
// bool is true (1) or false (0), one byte each; a string is " ... " of at least two bytes and
// comes out as the span of its content without the quotes (json_text_host.h unescapes it).
//
// Written once and compiled twice, as field_parse_host.h is.  No HIP include.
#pragma once
#include <cstdint>

#include "field_parse_host.h"

namespace amdx {

// 0..4 are kFpSpan .. kFpFloat32.
enum : uint32_t { kJfBool = 5, kJfString = 6 };

constexpr uint32_t kJsonFieldsMaxCols = 32;
constexpr uint32_t kJsonFieldsMaxName = 255;
constexpr uint64_t kJfNoPos = ~0ull;

struct JsonFieldsCol {
  uint32_t name_off;   // the requested name is names[name_off, name_off + name_len)
  uint32_t name_len;   // 1..255
  uint32_t type;       // kFp* / kJf*
  uint32_t pad;
  void* values;        // [nrows] int64 / int32 / double / float / uint8 (bool); span, string: int64 start
  int32_t* length;     // [nrows] span and string only
  uint8_t* status;     // [nrows]
};

struct JsonFieldsArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* off;      // [nrows] bytes
  const void* len;         // [nrows] int32 or int64, bytes
  uint64_t nrows;
  const uint8_t* names;    // the requested names, end to end
  uint32_t names_bytes;
  uint32_t len_is_64;
  uint32_t terminator;     // one byte
  uint32_t ncols;          // 1..kJsonFieldsMaxCols
  JsonFieldsCol cols[kJsonFieldsMaxCols];
};

FP_HD inline bool jf_ws(uint8_t c) { return c == 0x20 || c == 0x09 || c == 0x0A || c == 0x0D; }

// fp_row_bytes' rule.
FP_HD inline bool jf_row_bytes(const JsonFieldsArgs& a, uint64_t r, uint64_t* off, uint64_t* n) {
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

FP_HD inline FieldParseCol jf_as_fp(const JsonFieldsCol& c) {
  FieldParseCol f;
  f.field = 0;
  f.type = c.type;
  f.values = c.values;
  f.length = c.length;
  f.status = c.status;
  return f;
}

// Row r of column c without a value: status st.
FP_HD inline void jf_emit_none(const JsonFieldsCol& c, uint64_t r, uint8_t st) {
  if (c.type == kJfBool) {
    static_cast<uint8_t*>(c.values)[r] = 0;
    c.status[r] = st;
  } else if (c.type == kJfString) {
    static_cast<int64_t*>(c.values)[r] = 0;
    c.length[r] = 0;
    c.status[r] = st;
  } else {
    fp_emit_none(jf_as_fp(c), r, st);
  }
}

// p[b, e) is 0 or [1-9][0-9]* up to *b (advanced past it); false when no such digits stand there.
FP_HD inline bool jf_int_part(const uint8_t* p, uint64_t* b, uint64_t e) {
  if (*b == e || !fp_digit(p[*b])) return false;
  if (p[*b] == '0') {
    ++*b;
    return true;
  }
  while (*b < e && fp_digit(p[*b])) ++*b;
  return true;
}

// -?(0|[1-9][0-9]*)
FP_HD inline bool jf_int_ok(const uint8_t* p, uint64_t b, uint64_t e) {
  if (b < e && p[b] == '-') ++b;
  return jf_int_part(p, &b, e) && b == e;
}

// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?
FP_HD inline bool jf_float_ok(const uint8_t* p, uint64_t b, uint64_t e) {
  if (b < e && p[b] == '-') ++b;
  if (!jf_int_part(p, &b, e)) return false;
  if (b < e && p[b] == '.') {
    ++b;
    if (b == e || !fp_digit(p[b])) return false;
    while (b < e && fp_digit(p[b])) ++b;
  }
  if (b < e && (p[b] | 0x20) == 'e') {
    ++b;
    if (b < e && (p[b] == '+' || p[b] == '-')) ++b;
    if (b == e || !fp_digit(p[b])) return false;
    while (b < e && fp_digit(p[b])) ++b;
  }
  return b == e;
}

FP_HD inline bool jf_is(const uint8_t* p, uint64_t b, uint64_t e, const char* w, uint64_t wn) {
  if (e - b != wn) return false;
  for (uint64_t i = 0; i < wn; ++i)
    if (p[b + i] != (uint8_t)w[i]) return false;
  return true;
}

// Row r of column c from the untrimmed value bytes row[b, e); row_off: the row's offset in data.
FP_HD inline void jf_emit(const JsonFieldsCol& c, uint64_t r, const uint8_t* row, uint64_t row_off, uint64_t b,
                          uint64_t e) {
  while (b < e && jf_ws(row[b])) ++b;
  while (e > b && jf_ws(row[e - 1])) --e;
  if (b == e) {
    jf_emit_none(c, r, kFpBad);
    return;
  }
  if (jf_is(row, b, e, "null", 4)) {
    jf_emit_none(c, r, kFpNone);
    return;
  }
  uint8_t st = kFpBad;
  switch (c.type) {
    case kFpSpan:
      static_cast<int64_t*>(c.values)[r] = (int64_t)(row_off + b);
      c.length[r] = (int32_t)(e - b);
      st = kFpValid;
      break;
    case kJfString:
      if (e - b >= 2 && row[b] == '"' && row[e - 1] == '"') {
        static_cast<int64_t*>(c.values)[r] = (int64_t)(row_off + b + 1);
        c.length[r] = (int32_t)(e - b - 2);
        st = kFpValid;
      }
      break;
    case kJfBool:
      if (jf_is(row, b, e, "true", 4) || jf_is(row, b, e, "false", 5)) {
        static_cast<uint8_t*>(c.values)[r] = row[b] == 't' ? 1 : 0;
        st = kFpValid;
      }
      break;
    case kFpInt64:
    case kFpInt32:
      if (jf_int_ok(row, b, e)) {
        int64_t v;
        st = fp_int(row, b, e, c.type == kFpInt32, &v);
        if (st == kFpValid) {
          if (c.type == kFpInt32) static_cast<int32_t*>(c.values)[r] = (int32_t)v;
          else static_cast<int64_t*>(c.values)[r] = v;
        }
      }
      break;
    default:
      if (jf_float_ok(row, b, e)) {
        uint64_t bits;
        st = fp_float(row, b, e, &bits);
        if (st == kFpValid || st == kFpDeferred) {
          fp_store_float(jf_as_fp(c), r, bits);
          c.status[r] = st;
          return;
        }
      }
      break;
  }
  if (st == kFpValid) c.status[r] = st;
  else jf_emit_none(c, r, st);
}

// The member whose key bytes are row[b, e) untrimmed: is its key " name "?
FP_HD inline bool jf_key_match(const uint8_t* row, uint64_t b, uint64_t e, const uint8_t* name, uint32_t nl) {
  while (b < e && jf_ws(row[b])) ++b;
  while (e > b && jf_ws(row[e - 1])) --e;
  if (e - b != (uint64_t)nl + 2 || row[b] != '"' || row[e - 1] != '"') return false;
  for (uint32_t i = 0; i < nl; ++i)
    if (row[b + 1 + i] != name[i]) return false;
  return true;
}

// What the walk leaves behind: 0 nothing but whitespace so far, 1 inside the object, 2 closed and
// only whitespace since, 3 bad.
enum : uint32_t { kJfBefore = 0, kJfOpen = 1, kJfClosed = 2, kJfBadRow = 3 };

// One row, byte by byte: the host loop, and one lane's work in kernel variant 0.
FP_HD inline void jf_row(const JsonFieldsArgs& a, uint64_t r) {
  uint64_t off, n;
  if (!jf_row_bytes(a, r, &off, &n)) {
    for (uint32_t j = 0; j < a.ncols; ++j) jf_emit_none(a.cols[j], r, kFpBad);
    return;
  }
  const uint8_t* row = a.data + off;
  uint64_t vs[kJsonFieldsMaxCols], ve[kJsonFieldsMaxCols];
  uint32_t found = 0, match = 0;                    // bit j: column j has a value / the member's key is column j's
  uint32_t state = kJfBefore, depth = 0;            // the depth wraps as the kernels' does
  bool inside = false, esc = false;
  uint64_t colon = kJfNoPos, mstart = 0;
  for (uint64_t i = 0; i < n && state != kJfBadRow; ++i) {
    const uint8_t c = row[i];
    if (state == kJfClosed) {
      if (!jf_ws(c)) state = kJfBadRow;
      continue;
    }
    if (state == kJfBefore) {
      if (jf_ws(c)) continue;
      if (c == '{') {
        state = kJfOpen;
        depth = 1;
        mstart = i + 1;
      } else {
        state = kJfBadRow;
      }
      continue;
    }
    const bool code = esc;
    esc = !code && c == '\\';
    if (c == '"') {
      if (!code) inside = !inside;
      continue;
    }
    if (inside) continue;
    if (c == '{' || c == '[') {
      ++depth;
    } else if (c == '}' || c == ']' || (c == ',' && depth == 1)) {
      if (c != ',' && depth != 1) {
        --depth;
        continue;
      }
      if (colon != kJfNoPos)                        // the member ends here
        for (uint32_t j = 0; j < a.ncols; ++j)
          if ((match >> j) & 1u) {
            vs[j] = colon + 1;
            ve[j] = i;
            found |= 1u << j;
          }
      colon = kJfNoPos;
      match = 0;
      mstart = i + 1;
      if (c != ',') state = c == '}' ? kJfClosed : kJfBadRow;
    } else if (c == ':' && depth == 1 && colon == kJfNoPos) {
      colon = i;
      for (uint32_t j = 0; j < a.ncols; ++j)
        if (jf_key_match(row, mstart, i, a.names + a.cols[j].name_off, a.cols[j].name_len)) match |= 1u << j;
    }
  }
  for (uint32_t j = 0; j < a.ncols; ++j) {
    if (state == kJfBefore) jf_emit_none(a.cols[j], r, kFpNone);
    else if (state != kJfClosed) jf_emit_none(a.cols[j], r, kFpBad);
    else if (!((found >> j) & 1u)) jf_emit_none(a.cols[j], r, kFpNone);
    else jf_emit(a.cols[j], r, row, off, vs[j], ve[j]);
  }
}

// Kernel variant 1 takes a row in vectors of 16 bytes.  bm: bit j set where byte j of the vector
// is a backslash; cin: the byte before the vector starts an escape.  Returns the bits of the code
// bytes (the byte after an escape start); *cout: the vector's last byte starts an escape.  A run
// that begins at an odd bit and reaches an even one carries into it in the addition.
FP_HD inline uint32_t jf_escaped16(uint32_t bm, uint32_t cin, uint32_t* cout) {
  bm &= 0xFFFFu & ~cin;                             // a code byte starts nothing
  const uint32_t follows = ((bm << 1) | cin) & 0xFFFFu;
  const uint32_t odd_starts = bm & 0xAAAAu & ~follows;
  const uint32_t sum = odd_starts + bm;
  *cout = (sum >> 16) & 1u;
  return (0x5555u ^ (sum << 1)) & follows;
}

// The scalars every path checks before it touches a row.
inline bool json_fields_scalars_ok(const JsonFieldsArgs& a) {
  if (a.terminator > 255) return false;
  if (a.ncols < 1 || a.ncols > kJsonFieldsMaxCols) return false;
  for (uint32_t j = 0; j < a.ncols; ++j) {
    const JsonFieldsCol& c = a.cols[j];
    if (c.type > kJfString) return false;
    if (c.name_len < 1 || c.name_len > kJsonFieldsMaxName) return false;
    if (c.name_off > a.names_bytes || c.name_len > a.names_bytes - c.name_off) return false;
  }
  return true;
}

// The host loop.  The caller has checked the scalars.
inline void json_fields_host(const JsonFieldsArgs& a) {
  for (uint64_t r = 0; r < a.nrows; ++r) jf_row(a, r);
}

}  // namespace amdx
