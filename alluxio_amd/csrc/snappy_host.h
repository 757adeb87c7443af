// The Snappy raw format (one stream per Parquet page body): the rules, as plain C++.  A stream is a
// varint preamble, the uncompressed length (at most 5 bytes, at most 2^31-1 here), followed by
// elements.  The low two bits of an element's tag byte give its kind:
//
//   0  literal: length-1 in the upper six bits; 60..63 there mean that length-1 follows in 1..4
//      little-endian bytes; the literal's bytes follow the header
//   1  copy of 4..11 bytes, 11-bit offset: three bits in the tag, eight in the next byte
//   2  copy of 1..64 bytes, 16-bit little-endian offset
//   3  copy of 1..64 bytes, 32-bit little-endian offset
//
// A copy may overlap its own output: byte i of it is out[op - offset + i % offset].  The size of a
// header is a function of the tag alone, an element is a literal or a copy and never both, and every
// element consumes at least one input byte and produces at least one output byte.
//
// Written once and compiled twice, as lz4_block_host.h is: the host loop (DRAM tiers, the tests'
// oracle of the kernels, tools/snappy_host_check.cpp) and, through PQ_HD, the header rules of the
// kernels in snappy_decode.hip.
#pragma once
#include <cstdint>

#include "parquet_host.h"

namespace amdx {

// What a malformed stream gives instead of a size.
enum {
  kSnPreamble = -1,   // the preamble is cut short, longer than 5 bytes or above 2^31-1
  kSnLength = -2,     // the preamble is not the capacity: the page header's size is authoritative
  kSnInput = -3,      // a header or a literal runs past the end of the stream
  kSnOffset = -4,     // offset 0, or an offset beyond the bytes produced so far
  kSnOutput = -5,     // an element would write past the capacity
  kSnShort = -6,      // the stream ends having produced fewer bytes than the preamble says
  kSnInternal = -7    // (device) a state the rules exclude; ends the page instead of looping
};

constexpr uint32_t kSnMaxLength = 0x7FFFFFFFu;
constexpr uint32_t kSnMaxHeader = 5;                  // bytes of the longest header, and of the preamble
constexpr uint32_t kSnMaxCopy = 64;                   // bytes of the longest copy

struct SnappyHeader {
  uint32_t kind;      // 0 literal, 1..3 copy
  uint32_t len;       // bytes produced (a literal of 2^32 bytes saturates at 2^32-1: above every capacity)
  uint32_t off;       // copies: the offset; literals: 0
  uint32_t hdr;       // bytes of the header; 0: needs more input than `avail`
};

PQ_HD inline uint32_t snappy_header_bytes(uint32_t tag) {
  const uint32_t kind = tag & 3u, v = tag >> 2;
  return kind == 0 ? (v >= 60 ? v - 58 : 1) : (kind == 1 ? 2 : (kind == 2 ? 3 : 5));
}

// The header of the element whose bytes `byte(0), byte(1), ...` are, of which `avail` exist.
// `byte` is called for indices below min(avail, header size) only.
template <typename F>
PQ_HD inline SnappyHeader snappy_header_at(F byte, uint32_t avail) {
  SnappyHeader h{0, 0, 0, 0};
  if (avail == 0) return h;
  const uint32_t tag = byte(0);
  const uint32_t need = snappy_header_bytes(tag);
  h.kind = tag & 3u;
  if (need > avail) return h;
  uint32_t x = 0;                                     // the little-endian bytes behind the tag
  for (uint32_t i = 1; i < need; ++i) x |= (uint32_t)byte(i) << (8u * (i - 1));
  if (h.kind == 0) {
    const uint32_t m = need == 1 ? tag >> 2 : x;
    h.len = m + (m != 0xFFFFFFFFu ? 1u : 0u);
  } else if (h.kind == 1) {
    h.len = 4 + ((tag >> 2) & 7u);
    h.off = ((tag >> 5) << 8) | x;
  } else {
    h.len = (tag >> 2) + 1;
    h.off = x;
  }
  h.hdr = need;
  return h;
}

PQ_HD inline SnappyHeader snappy_header(const uint8_t* p, uint32_t avail) {
  return snappy_header_at([p](uint32_t i) -> uint32_t { return p[i]; }, avail);
}

// The preamble of a stream of n bytes: its size (1..5) and *value, or a negative code.
template <typename F>
PQ_HD inline int32_t snappy_preamble_at(F byte, uint32_t n, uint32_t* value) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < kSnMaxHeader; ++i) {
    if (i >= n) return kSnPreamble;
    const uint32_t b = byte(i);
    v |= (uint64_t)(b & 127u) << (7u * i);
    if (!(b & 128u)) {
      if (v > kSnMaxLength) return kSnPreamble;
      *value = (uint32_t)v;
      return (int32_t)(i + 1);
    }
  }
  return kSnPreamble;
}

// The stream src[0, n) into dst[0, cap): the bytes produced (cap), or a negative code.  Reads
// nothing outside [src, src + n) and writes nothing outside [dst, dst + cap).
inline int64_t snappy_decompress_block(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap) {
  if (n > kSnMaxLength || cap > kSnMaxLength) return kSnPreamble;
  uint32_t want = 0;
  const int32_t pre = snappy_preamble_at([src](uint32_t i) -> uint32_t { return src[i]; }, (uint32_t)n, &want);
  if (pre < 0) return pre;
  if (want != cap) return kSnLength;
  uint32_t ip = (uint32_t)pre, op = 0;
  const uint32_t slen = (uint32_t)n, room = (uint32_t)cap;
  while (ip < slen) {
    const SnappyHeader h = snappy_header(src + ip, slen - ip);
    if (!h.hdr) return kSnInput;
    ip += h.hdr;
    if (h.kind == 0) {
      if (h.len > slen - ip) return kSnInput;
      if (h.len > room - op) return kSnOutput;
      for (uint32_t i = 0; i < h.len; ++i) dst[op + i] = src[ip + i];
      ip += h.len;
    } else {
      if (h.off == 0 || h.off > op) return kSnOffset;
      if (h.len > room - op) return kSnOutput;
      for (uint32_t i = 0; i < h.len; ++i) dst[op + i] = dst[op - h.off + i];   // i % off, unrolled in time
    }
    op += h.len;
  }
  return op == room ? (int64_t)op : (int64_t)kSnShort;
}

}  // namespace amdx
