// JSON string values unescaped into packed bytes: the rule, as plain C++.  A value is
// data[start, start + length), the content of a JSON string without its quotes, as a string column
// of json_fields_host.h describes it.  Its output is the same bytes with every escape replaced:
//   \" \\ \/            that byte
//   \b \f \n \r \t      08 0C 0A 0D 09
//   \uXXXX              the UTF-8 of the code point, hex digits in either case
//   a high surrogate escape immediately followed by a low surrogate escape: the 4-byte UTF-8 of
//   the pair; any other surrogate escape: its 3-byte generalised encoding
// which is json.loads(b'"' + content + b'"') encoded with "surrogatepass".  Any other escape code,
// a \u with fewer than four hex digits, or a backslash as the value's last byte makes the value
// bad: status 2, length 0, and emit writes nothing for it.  Every byte that is not part of an
// escape is copied unchanged: there is no UTF-8 validation, and raw control bytes pass through.
// The output is never longer than the input.
//
// Liveness, the two passes and the window of emit are those of text_column_host.h (tc_live,
// tc_window; the quote of the TextColumnArgs is not used).  measure also writes out_status[r]: 0
// for a good live value, 2 for a bad one or one outside the buffer, the input status where that is
// not 0.
//
// Written once and compiled twice, as text_column_host.h is.  No HIP include.
#pragma once
#include <cstdint>

#include "text_column_host.h"

namespace amdx {

struct JsonTextArgs {
  TextColumnArgs t;
  uint8_t* out_status;       // measure: [n]
};

TC_HD inline int jt_hex(uint8_t c) {
  if ((uint8_t)(c - '0') < 10) return c - '0';
  const uint8_t l = c | 0x20;
  if ((uint8_t)(l - 'a') < 6) return l - 'a' + 10;
  return -1;
}

// The four hex digits p[i, i + 4) of a value of n bytes; false when they are not all there.
TC_HD inline bool jt_hex4(const uint8_t* p, uint64_t n, uint64_t i, uint32_t* cp) {
  if (n < 4 || i > n - 4) return false;
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const int h = jt_hex(p[i + k]);
    if (h < 0) return false;
    v = (v << 4) | (uint32_t)h;
  }
  *cp = v;
  return true;
}

// The byte a two-byte escape with this code stands for, or -1.
TC_HD inline int jt_simple(uint8_t code) {
  switch (code) {
    case '"':
    case '\\':
    case '/': return code;
    case 'b': return 0x08;
    case 'f': return 0x0C;
    case 'n': return 0x0A;
    case 'r': return 0x0D;
    case 't': return 0x09;
    default: return -1;
  }
}

// The escape that starts at the backslash p[*i]: its bytes in u[0, *cnt), *i moved past it.
// False: a bad escape.
TC_HD inline bool jt_escape(const uint8_t* p, uint64_t n, uint64_t* i, uint8_t* u, uint32_t* cnt) {
  if (n - *i < 2) return false;
  const uint8_t code = p[*i + 1];
  if (code != 'u') {
    const int s = jt_simple(code);
    if (s < 0) return false;
    u[0] = (uint8_t)s;
    *cnt = 1;
    *i += 2;
    return true;
  }
  uint32_t cp, lo;
  if (!jt_hex4(p, n, *i + 2, &cp)) return false;
  *i += 6;
  if (cp >= 0xD800u && cp < 0xDC00u && n - *i >= 6 && p[*i] == '\\' && p[*i + 1] == 'u' &&
      jt_hex4(p, n, *i + 2, &lo) && lo >= 0xDC00u && lo < 0xE000u) {
    cp = 0x10000u + ((cp - 0xD800u) << 10) + (lo - 0xDC00u);
    *i += 6;
    u[0] = (uint8_t)(0xF0u | (cp >> 18));
    u[1] = (uint8_t)(0x80u | ((cp >> 12) & 0x3Fu));
    u[2] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu));
    u[3] = (uint8_t)(0x80u | (cp & 0x3Fu));
    *cnt = 4;
  } else if (cp < 0x80u) {
    u[0] = (uint8_t)cp;
    *cnt = 1;
  } else if (cp < 0x800u) {
    u[0] = (uint8_t)(0xC0u | (cp >> 6));
    u[1] = (uint8_t)(0x80u | (cp & 0x3Fu));
    *cnt = 2;
  } else {
    u[0] = (uint8_t)(0xE0u | (cp >> 12));
    u[1] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu));
    u[2] = (uint8_t)(0x80u | (cp & 0x3Fu));
    *cnt = 3;
  }
  return true;
}

// The bytes p[*i, stop) of a value of n bytes, stop <= n; an escape that starts before stop is
// taken whole, so *i may end past stop.  *k counts the output bytes; with out != null, output byte
// j in [jlo, jhi) is written to out[lo + j].  False at a bad escape.
TC_HD inline bool jt_span(const uint8_t* p, uint64_t n, uint64_t* i, uint64_t stop, uint64_t* k, uint8_t* out,
                          int64_t lo, uint64_t jlo, uint64_t jhi) {
  while (*i < stop) {
    const uint8_t c = p[*i];
    if (c != '\\') {
      if (out && *k >= jlo && *k < jhi) out[lo + (int64_t)*k] = c;
      ++*k;
      ++*i;
      continue;
    }
    uint8_t u[4];
    uint32_t cnt;
    if (!jt_escape(p, n, i, u, &cnt)) return false;
    for (uint32_t j = 0; j < cnt; ++j) {
      if (out && *k >= jlo && *k < jhi) out[lo + (int64_t)*k] = u[j];
      ++*k;
    }
  }
  return true;
}

// The status of a value that is not live.
TC_HD inline uint8_t jt_dead_status(const TextColumnArgs& a, uint64_t r) {
  return a.status && a.status[r] != 0 ? a.status[r] : (uint8_t)2;
}

TC_HD inline void jt_measure_one(const JsonTextArgs& a, uint64_t r) {
  uint64_t s, n;
  if (!tc_live(a.t, r, &s, &n)) {
    a.t.out_len[r] = 0;
    a.out_status[r] = jt_dead_status(a.t, r);
    return;
  }
  uint64_t i = 0, k = 0;
  const bool good = jt_span(a.t.data + s, n, &i, n, &k, nullptr, 0, 0, 0);
  a.t.out_len[r] = good ? (int32_t)k : 0;
  a.out_status[r] = good ? 0 : 2;
}

// A first walk finds out whether the value is bad; only a good one is written.
TC_HD inline void jt_emit_one(const JsonTextArgs& a, uint64_t r) {
  uint64_t s, n, jlo, jhi;
  int64_t lo;
  if (!tc_live(a.t, r, &s, &n) || !tc_window(a.t, r, &lo, &jlo, &jhi)) return;
  uint64_t i = 0, k = 0;
  if (!jt_span(a.t.data + s, n, &i, n, &k, nullptr, 0, 0, 0)) return;
  i = k = 0;
  jt_span(a.t.data + s, n, &i, n, &k, a.t.out, lo, jlo, jhi);
}

// The host loops.  The caller has checked the pointers.
inline void json_text_measure_host(const JsonTextArgs& a) {
  for (uint64_t r = 0; r < a.t.n; ++r) jt_measure_one(a, r);
}
inline void json_text_emit_host(const JsonTextArgs& a) {
  for (uint64_t r = 0; r < a.t.n; ++r) jt_emit_one(a, r);
}

}  // namespace amdx
