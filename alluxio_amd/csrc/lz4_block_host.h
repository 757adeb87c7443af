// One standard LZ4 block per page body, of any size below 2^31: the rules, as plain C++.  A Parquet
// LZ4_RAW page is a single block, so a page is cut into segments that are parsed independently and
// stitched together again, as the 64 KiB chunk encoder of lz4_encode.hip does in small:
//
//   parse  one segment at a time (on the device: staged in LDS with the bytes before it, so the
//          dependent loads of probe and match extension do not go to memory).  The hash table holds
//          16-bit positions counted from
//          `begin - warm` (the bytes before the segment are hashed first, so that matches into them
//          are found; 0xFFFF is the empty slot, hence segment + warm <= 65535).  A match starts
//          inside the segment and ends by its end, and in every segment obeys the block's end rules:
//          it starts at least 12 bytes before the page's end and ends at least 5 before it.  The
//          sequences go to the segment's scratch area WITHOUT the first token and its literals, and
//          a record says where the first match starts, its length code, the scratch bytes and where
//          the last match ends.  Positions are 32-bit offsets in the page.
//   link   per page, over its segments in order: P, the end of the last match so far, is where the
//          next literal run starts; a segment with a match gets (P, offset of its first token in
//          the block); a segment without one gets no place, its bytes ride in the next run.  The
//          page gets its final literal run and the block's size.
//   merge  per segment with a match: the first token with the literal run joined across the segment
//          boundaries, the literals from the source, then the scratch bytes.  The page's last
//          segment also writes the closing literal-only sequence.  An empty body is the block `00`.
//
// All tables are rows of int64 that the caller lays out.  Every row is checked against the buffers
// before it is used, in every pass: a row that does not fit marks its page as refused (kLbStatus)
// and nothing of that page is written.
//
// Written once and compiled twice, as parquet_encode_host.h is: the host loops (CPU columns, the
// stand-alone check program) and, through PQ_HD, the rules, link and merge plan of the kernels in
// lz4_encode.hip, whose chunk encoders also use the hash, the length bytes and the format constants
// below.  The host parser is scalar and need not find the matches that the wave parse finds: its
// blocks are compared with the device's by what they decode to and by their sizes, never byte for byte.
#pragma once
#include <cstdint>
#include <cstring>

#include "parquet_host.h"

namespace amdx {

// Page row: the body's place in the source buffer and its segments.
enum { kLbPageOff = 0, kLbPageLen = 1, kLbPageSeg = 2, kLbPageSegs = 3, kLbPageCols = 4 };
// Segment row.
enum {
  kLbSegPage = 0,     // the page
  kLbSegSrc = 1,      // the page body's offset in the source buffer (the page row's, again)
  kLbSegBegin = 2,    // the segment is bytes [begin, end) of the body
  kLbSegEnd = 3,
  kLbSegLast = 4,     // 1: the page's last segment
  kLbSegScratch = 5,  // where its sequences go in the scratch buffer
  kLbSegCols = 8
};
// Result row, per page.
enum {
  kLbSize = 0,        // bytes of the block
  kLbFinP = 1,        // the closing literal run starts here in the body
  kLbFinOff = 2,      // and its token goes here in the block
  kLbStatus = 3,      // 0: fine; 1: a table row does not fit; 2: a segment's scratch overflowed;
                      // 3: the block does not fit the output buffer (merge)
  kLbResCols = 4
};
// Record of a parsed segment (uint32 each).
enum { kLbRecFirst = 0, kLbRecCode = 1, kLbRecBytes = 2, kLbRecTail = 3, kLbRecCols = 4 };
enum { kLbLinkP = 0, kLbLinkOff = 1, kLbLinkCols = 2 };

constexpr uint32_t kLbNone = 0xFFFFFFFFu;
constexpr uint32_t kLbSegment = 32 * 1024;      // the segment size the writer uses
constexpr uint32_t kLbWarm = 4096;
constexpr uint32_t kLbHashLog = 12;
constexpr uint32_t kLbMfLimit = 12, kLbLastLiterals = 5, kLbMinMatch = 4;
// the largest body whose bound stays below 2^31
constexpr uint64_t kLbMaxLen = 2139095000ull;

struct LbArgs {
  const uint8_t* src;       // the buffer the page bodies lie in
  uint64_t src_bytes;
  const int64_t* pages;     // [npages][kLbPageCols]
  uint64_t npages;
  const int64_t* segs;      // [nsegs][kLbSegCols]
  uint64_t nsegs;
  uint8_t* scratch;         // records, links, then the segments' sequences (lb_scratch_head)
  uint64_t scratch_bytes;
  int64_t* result;          // [npages][kLbResCols]
  const int64_t* dst;       // merge: [npages] where each block goes in out
  uint8_t* out;
  uint64_t out_bytes;
  uint32_t warm;            // bytes before a segment that are hashed first
  uint32_t segment;         // the most bytes of a segment: segment + warm <= 65535
};

PQ_HD inline uint64_t lb_bound(uint64_t n) { return n + n / 255 + 16; }
// The scratch buffer starts with nsegs records and nsegs links; the sequences lie behind them.
PQ_HD inline uint64_t lb_scratch_head(uint64_t nsegs) { return nsegs * 4 * (kLbRecCols + kLbLinkCols); }
PQ_HD inline uint32_t* lb_recs(const LbArgs& a) { return reinterpret_cast<uint32_t*>(a.scratch); }
PQ_HD inline uint32_t* lb_links(const LbArgs& a) { return lb_recs(a) + a.nsegs * kLbRecCols; }

PQ_HD inline uint32_t lb_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kLbHashLog); }
PQ_HD inline uint32_t lb_read32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
PQ_HD inline uint32_t lb_len_bytes(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }   // after a 4-bit field
PQ_HD inline uint8_t lb_token(uint32_t lit, uint32_t code) {
  return (uint8_t)(((lit >= 15 ? 15 : lit) << 4) | (code >= 15 ? 15 : code));
}
// Q: the caller's position type.  The wave parse counts in 32 bits: with 64-bit positions here its
// kernels take up to four more registers each.
template <typename Q>
PQ_HD inline Q lb_put_len(uint8_t* dst, Q q, uint32_t v) {
  if (v >= 15) {
    uint32_t r = v - 15;
    while (r >= 255) {
      dst[q++] = 255;
      r -= 255;
    }
    dst[q++] = (uint8_t)r;
  }
  return q;
}

// Segments of a body of `len` bytes cut at `segment`: an empty body has one (empty) segment.
PQ_HD inline uint64_t lb_segments(uint64_t len, uint64_t segment) { return len ? (len + segment - 1) / segment : 1; }

// A segment row fits its page, the source and the scratch buffer.
PQ_HD inline bool lb_seg_ok(const LbArgs& a, const int64_t* sg) {
  const int64_t p = sg[kLbSegPage], b = sg[kLbSegBegin], e = sg[kLbSegEnd], sc = sg[kLbSegScratch];
  if (p < 0 || (uint64_t)p >= a.npages || b < 0 || e < b) return false;
  const int64_t* pg = a.pages + (uint64_t)p * kLbPageCols;
  const int64_t off = pg[kLbPageOff], len = pg[kLbPageLen];
  if (off < 0 || len < 0 || (uint64_t)len > kLbMaxLen || (uint64_t)off > a.src_bytes ||
      (uint64_t)len > a.src_bytes - (uint64_t)off)
    return false;
  if (sg[kLbSegSrc] != off || e > len || (uint64_t)(e - b) > a.segment || (uint64_t)a.segment + a.warm > 65535)
    return false;
  if (sc < 0 || (uint64_t)sc < lb_scratch_head(a.nsegs) || (uint64_t)sc > a.scratch_bytes ||
      lb_bound((uint64_t)(e - b)) > a.scratch_bytes - (uint64_t)sc)
    return false;
  return true;
}

// Where a segment's matches may start (before *match_limit) and must end (by *end_match).
PQ_HD inline void lb_limits(uint32_t len, uint32_t se, uint32_t* match_limit, uint32_t* end_match) {
  const uint32_t ml = len > kLbMfLimit ? len - kLbMfLimit : 0, em = len > kLbLastLiterals ? len - kLbLastLiterals : 0;
  const uint32_t sl = se > 3 ? se - 3 : 0;
  *match_limit = sl < ml ? sl : ml;
  *end_match = se < em ? se : em;
}

// link: page p.
PQ_HD inline void lb_link_page(const LbArgs& a, uint64_t p) {
  const int64_t* pg = a.pages + p * kLbPageCols;
  int64_t* res = a.result + p * kLbResCols;
  const uint32_t* recs = lb_recs(a);
  uint32_t* links = lb_links(a);
  const int64_t first = pg[kLbPageSeg], n = pg[kLbPageSegs], len = pg[kLbPageLen];
  int64_t status = 0;
  if (first < 0 || n < 1 || (uint64_t)first > a.nsegs || (uint64_t)n > a.nsegs - (uint64_t)first) status = 1;
  uint64_t out = 0;
  uint32_t P = 0;
  int64_t expect = 0;
  for (int64_t k = 0; k < n && !status; ++k) {
    const uint64_t s = (uint64_t)(first + k);
    const int64_t* sg = a.segs + s * kLbSegCols;
    const uint32_t* rec = recs + s * kLbRecCols;
    if (!lb_seg_ok(a, sg) || (uint64_t)sg[kLbSegPage] != p || sg[kLbSegBegin] != expect ||
        (sg[kLbSegLast] != 0) != (k + 1 == n)) {
      status = 1;
      break;
    }
    expect = sg[kLbSegEnd];
    links[s * kLbLinkCols + kLbLinkP] = P;
    links[s * kLbLinkCols + kLbLinkOff] = kLbNone;
    if (rec[kLbRecBytes] == kLbNone) {
      status = 2;
      break;
    }
    const uint32_t m = rec[kLbRecFirst];
    if (m == kLbNone) continue;
    if (m < P || m < (uint64_t)sg[kLbSegBegin] || rec[kLbRecTail] < m + kLbMinMatch || rec[kLbRecTail] > (uint64_t)expect ||
        rec[kLbRecBytes] > lb_bound((uint64_t)(expect - sg[kLbSegBegin]))) {
      status = 1;
      break;
    }
    const uint32_t lit = m - P;
    links[s * kLbLinkCols + kLbLinkOff] = (uint32_t)out;
    out += 1 + lb_len_bytes(lit) + lit + rec[kLbRecBytes];
    P = rec[kLbRecTail];
  }
  if (!status && expect != len) status = 1;
  if (status) {
    res[kLbSize] = -1;
    res[kLbFinP] = res[kLbFinOff] = 0;
    res[kLbStatus] = status;
    return;
  }
  const uint32_t lit = (uint32_t)len - P;
  res[kLbFinP] = P;
  res[kLbFinOff] = (int64_t)out;
  res[kLbSize] = (int64_t)(out + 1 + lb_len_bytes(lit) + lit);
  res[kLbStatus] = 0;
}

// merge: what segment s writes.  head: the joined first token at o, `lit` literals from body
// position P and `bytes` scratch bytes; fin: the closing run of fin_lit literals from fin_p at fin_o.
struct LbMerge {
  bool head, fin;
  const uint8_t* src;       // the page body
  const uint8_t* seq;       // the segment's scratch bytes
  uint8_t* dst;             // the block
  uint32_t P, lit, code, bytes;
  uint64_t o;
  uint32_t fin_p, fin_lit;
  uint64_t fin_o;
};

PQ_HD inline void lb_merge_plan(const LbArgs& a, uint64_t s, LbMerge* m) {
  m->head = m->fin = false;
  const int64_t* sg = a.segs + s * kLbSegCols;
  if (!lb_seg_ok(a, sg)) return;
  const uint64_t p = (uint64_t)sg[kLbSegPage];
  int64_t* res = a.result + p * kLbResCols;
  const int64_t size = res[kLbSize], at = a.dst[p];
  if (res[kLbStatus] == 1 || res[kLbStatus] == 2 || size < 1) return;
  if (at < 0 || (uint64_t)at > a.out_bytes || (uint64_t)size > a.out_bytes - (uint64_t)at) {
    if (sg[kLbSegLast]) res[kLbStatus] = 3;
    return;
  }
  const int64_t len = a.pages[p * kLbPageCols + kLbPageLen];
  m->src = a.src + sg[kLbSegSrc];
  m->seq = a.scratch + sg[kLbSegScratch];
  m->dst = a.out + at;
  const uint32_t* rec = lb_recs(a) + s * kLbRecCols;
  const uint32_t* link = lb_links(a) + s * kLbLinkCols;
  if (rec[kLbRecFirst] != kLbNone && link[kLbLinkOff] != kLbNone) {
    m->P = link[kLbLinkP];
    m->o = link[kLbLinkOff];
    m->code = rec[kLbRecCode];
    m->bytes = rec[kLbRecBytes];
    if (rec[kLbRecFirst] >= m->P && rec[kLbRecFirst] < (uint64_t)sg[kLbSegEnd] &&
        m->bytes <= lb_bound((uint64_t)(sg[kLbSegEnd] - sg[kLbSegBegin]))) {
      m->lit = rec[kLbRecFirst] - m->P;
      m->head = m->o + 1 + lb_len_bytes(m->lit) + m->lit + m->bytes <= (uint64_t)size;
    }
  }
  if (sg[kLbSegLast]) {
    const int64_t fp = res[kLbFinP], fo = res[kLbFinOff];
    if (fp >= 0 && fp <= len && fo >= 0) {
      m->fin_p = (uint32_t)fp;
      m->fin_lit = (uint32_t)(len - fp);
      m->fin_o = (uint64_t)fo;
      m->fin = m->fin_o + 1 + lb_len_bytes(m->fin_lit) + m->fin_lit == (uint64_t)size;
    }
  }
}

PQ_HD inline void lb_put_head(const LbMerge& m) {
  m.dst[m.o] = lb_token(m.lit, m.code);
  lb_put_len(m.dst, m.o + 1, m.lit);
}
PQ_HD inline void lb_put_fin(const LbMerge& m) {
  m.dst[m.fin_o] = (uint8_t)((m.fin_lit >= 15 ? 15 : m.fin_lit) << 4);
  lb_put_len(m.dst, m.fin_o + 1, m.fin_lit);
}

// ---- the host loops --------------------------------------------------------------------------------

// parse: segment s, one position at a time.
inline void lb_parse_segment_host(const LbArgs& a, uint64_t s) {
  const int64_t* sg = a.segs + s * kLbSegCols;
  uint32_t* rec = lb_recs(a) + s * kLbRecCols;
  rec[kLbRecFirst] = kLbNone;
  rec[kLbRecCode] = rec[kLbRecTail] = 0;
  rec[kLbRecBytes] = kLbNone;
  if (!lb_seg_ok(a, sg)) return;
  const uint8_t* src = a.src + sg[kLbSegSrc];
  const uint32_t len = (uint32_t)a.pages[(uint64_t)sg[kLbSegPage] * kLbPageCols + kLbPageLen];
  const uint32_t sb = (uint32_t)sg[kLbSegBegin], se = (uint32_t)sg[kLbSegEnd];
  const uint32_t base = sb > a.warm ? sb - a.warm : 0;
  uint8_t* dst = a.scratch + sg[kLbSegScratch];
  const uint64_t cap = lb_bound(se - sb);
  uint16_t table[1u << kLbHashLog];
  std::memset(table, 0xFF, sizeof(table));
  for (uint32_t p = base; p < sb; ++p)
    if (p + 4 <= len) table[lb_hash(lb_read32(src + p))] = (uint16_t)(p - base);
  uint32_t match_limit, end_match;
  lb_limits(len, se, &match_limit, &end_match);
  uint32_t anchor = sb, ip = sb;
  uint64_t op = 0;
  bool first = true, overflow = false;
  while (ip < match_limit) {
    const uint32_t v = lb_read32(src + ip), h = lb_hash(v);
    const uint32_t c = table[h];
    table[h] = (uint16_t)(ip - base);
    if (c == 0xFFFF || base + c >= ip || lb_read32(src + base + c) != v) {
      ++ip;
      continue;
    }
    const uint32_t cand = base + c;
    uint32_t ml = kLbMinMatch;
    while (ip + ml < end_match && src[cand + ml] == src[ip + ml]) ++ml;
    const uint32_t lit = ip - anchor, code = ml - kLbMinMatch, off = ip - cand;
    const uint64_t need = (first ? 0 : 1 + lb_len_bytes(lit) + lit) + 2 + lb_len_bytes(code);
    if (op + need > cap) {
      overflow = true;
      break;
    }
    if (first) {
      rec[kLbRecFirst] = ip;
      rec[kLbRecCode] = code;
      first = false;
    } else {
      dst[op] = lb_token(lit, code);
      op = lb_put_len(dst, op + 1, lit);
      std::memcpy(dst + op, src + anchor, lit);
      op += lit;
    }
    dst[op] = (uint8_t)(off & 255);
    dst[op + 1] = (uint8_t)(off >> 8);
    op = lb_put_len(dst, op + 2, code);
    ip += ml;
    anchor = ip;
  }
  rec[kLbRecBytes] = overflow ? kLbNone : (uint32_t)op;
  rec[kLbRecTail] = anchor;
}

inline void lb_merge_segment_host(const LbArgs& a, uint64_t s) {
  LbMerge m;
  lb_merge_plan(a, s, &m);
  if (m.head) {
    lb_put_head(m);
    const uint64_t q = m.o + 1 + lb_len_bytes(m.lit);
    std::memcpy(m.dst + q, m.src + m.P, m.lit);
    std::memcpy(m.dst + q + m.lit, m.seq, m.bytes);
  }
  if (m.fin) {
    lb_put_fin(m);
    std::memcpy(m.dst + m.fin_o + 1 + lb_len_bytes(m.fin_lit), m.src + m.fin_p, m.fin_lit);
  }
}

inline void lz4_block_parse_host(const LbArgs& a) {
  for (uint64_t s = 0; s < a.nsegs; ++s) lb_parse_segment_host(a, s);
}
inline void lz4_block_link_host(const LbArgs& a) {
  for (uint64_t p = 0; p < a.npages; ++p) lb_link_page(a, p);
}
inline void lz4_block_merge_host(const LbArgs& a) {
  for (uint64_t s = 0; s < a.nsegs; ++s) lb_merge_segment_host(a, s);
}

}  // namespace amdx
