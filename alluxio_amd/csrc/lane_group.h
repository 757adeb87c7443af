// The building blocks of the cooperative ("variant 1") text kernels, in one place.  A group of 16
// lanes owns a row or a value and walks it in steps of 256 bytes, lane l of the group taking the 16
// bytes at step * 256 + 16 * l.  A vector becomes 16-bit masks by a SWAR compare, state travels
// from vector to vector through ballots, and the bytes a lane keeps are placed by a 16-lane prefix
// sum.  field_parse.hip, text_column.hip, text_dict.hip and json_fields.hip are built from these
// pieces; delim_index.hip, whose unit is the wave, takes the bit functions only.
//
// Two parts, by the convention of the *_host.h files.  The pure part is plain C++ without a HIP
// include: bit functions with no loads and no cross-lane traffic, written once and compiled for
// the host (tools/lane_group_host_check.cpp and the replays in the other check programs) and,
// through LG_HD, for the device.  The device part (under __HIP__) adds the loads, the stores and
// everything that talks to other lanes.  Each of its functions that holds a ballot or a shuffle
// says so: every lane of the wave has to call it, so it never stands under a divergent branch.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define LG_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline))
#else
#define LG_HD __attribute__((always_inline))
#endif

namespace amdx {

// ---- pure part ----------------------------------------------------------------------------------

// 0x80 in every byte of w that equals the byte replicated in dw.  Exact: the add never carries
// from one byte into the next.
LG_HD inline uint32_t lg_match(uint32_t w, uint32_t dw) {
  const uint32_t x = w ^ dw;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// Bits 7, 15, 23, 31 of z -> bits 0..3.
LG_HD inline uint32_t lg_pack(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }

// Bit j: byte j of the 16 bytes in the words x, y, z, w (lowest address first) equals the byte
// replicated in dw.
LG_HD inline uint32_t lg_mask16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t dw) {
  return lg_pack(lg_match(x, dw)) | (lg_pack(lg_match(y, dw)) << 4) | (lg_pack(lg_match(z, dw)) << 8) |
         (lg_pack(lg_match(w, dw)) << 12);
}

// Bit j: an odd number of the bits below j is set in the 16-bit mask qm.  With qm the quotes of a
// vector that starts outside quotes, byte j lies inside.
LG_HD inline uint32_t lg_inside16(uint32_t qm) {
  uint32_t m = qm;
  m ^= m << 1;
  m ^= m << 2;
  m ^= m << 4;
  m ^= m << 8;
  return (m << 1) & 0xFFFFu;
}

// The bytes of (vlo, vhi) whose bit is set in keep, in order and without gaps, from byte 0 of *clo.
LG_HD inline void lg_compact(uint64_t vlo, uint64_t vhi, uint32_t keep, uint64_t* clo, uint64_t* chi) {
  uint64_t lo = 0, hi = 0;
  uint32_t k = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    if (!((keep >> j) & 1u)) continue;
    const uint64_t b = ((j < 8 ? vlo : vhi) >> (8 * (j & 7))) & 0xFFu;
    if (k < 8) lo |= b << (8 * k);
    else hi |= b << (8 * (k - 8));
    ++k;
  }
  *clo = lo;
  *chi = hi;
}

// The hand-off of one bit of state along the 16 vectors of a step.  A vector that is not "all set"
// (all quotes, all backslashes) knows what it hands on without knowing what it got, and one that is
// all set hands on what it got.  ga: bit l set when the vector of lane l is not all set; gb: bit l
// set when that vector hands on 1 (read only where ga is set); carry: the state before the step.
//
// The state before the vector of lane gl: that of the nearest lower lane in ga, or the carry.
LG_HD inline uint32_t lg_carry_in(uint32_t ga, uint32_t gb, uint32_t gl, uint32_t carry) {
  const uint32_t below = ga & ((1u << gl) - 1u);
  return below ? (gb >> (31 - __builtin_clz(below))) & 1u : carry;
}

// The state after the step: what the highest lane in ga hands on, or the carry unchanged.
LG_HD inline uint32_t lg_carry_next(uint32_t ga, uint32_t gb, uint32_t carry) {
  return ga ? (gb >> (31 - __builtin_clz(ga))) & 1u : carry;
}

// ---- device part --------------------------------------------------------------------------------
#if defined(__HIP__)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLgThreads = 256;                     // a workgroup of the cooperative kernels
constexpr int kLgGroup = 16;                        // lanes per row or value
constexpr int kLgVec = 16;                          // bytes per lane and step
constexpr int kLgPerBlock = kLgThreads / kLgGroup;  // rows or values per workgroup
constexpr uint64_t kLgStep = kLgGroup * kLgVec;     // bytes per group and step

__device__ __forceinline__ uint32_t lg_mask16(u32x4 v, uint32_t dw) { return lg_mask16(v.x, v.y, v.z, v.w, dw); }

// The two halves of a vector as words, lowest address in the lowest byte.
__device__ __forceinline__ uint64_t lg_lo64(u32x4 v) { return ((uint64_t)v.y << 32) | v.x; }
__device__ __forceinline__ uint64_t lg_hi64(u32x4 v) { return ((uint64_t)v.w << 32) | v.z; }

// The 16 bytes at p, or the first rem < 16 of them from byte loads (nothing past the end is read),
// zero padded.
__device__ __forceinline__ u32x4 lg_load16(const uint8_t* p, uint64_t rem) {
  u32x4 v;
  if (rem >= 16) {
    __builtin_memcpy(&v, p, 16);                    // any byte phase
  } else {
    uint64_t lo = 0, hi = 0;
    for (uint32_t j = 0; j < (uint32_t)rem; ++j) {
      const uint64_t b = p[j];
      if (j < 8) lo |= b << (8 * j);
      else hi |= b << (8 * (j - 8));
    }
    v.x = (uint32_t)lo;
    v.y = (uint32_t)(lo >> 32);
    v.z = (uint32_t)hi;
    v.w = (uint32_t)(hi >> 32);
  }
  return v;
}

// 64-bit shuffles from two 32-bit ones.  Every lane of the wave calls them.
// src is a lane index of the wave:
__device__ __forceinline__ uint64_t lg_shfl64_wave(uint64_t v, int src) {
  const uint32_t lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
// src is a lane index of the caller's group (width 16):
__device__ __forceinline__ uint64_t lg_shfl64_group(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, kLgGroup), hi = __shfl((uint32_t)(v >> 32), src, kLgGroup);
  return ((uint64_t)hi << 32) | lo;
}
// from lane gl ^ d of the caller's group:
__device__ __forceinline__ uint64_t lg_shfl64_xor_group(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, kLgGroup), hi = __shfl_xor((uint32_t)(v >> 32), d, kLgGroup);
  return ((uint64_t)hi << 32) | lo;
}

// Inclusive prefix sum of c over the lanes of a group (gl: the lane's index in it); *total: the
// group's sum.  Sums wrap, so a caller may scan signed differences.  Holds shuffles: every lane of
// the wave calls it.
__device__ __forceinline__ uint32_t lg_scan16(uint32_t c, uint32_t gl, uint32_t* total) {
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < kLgGroup; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, kLgGroup);
    if ((int)gl >= d) inc += o;
  }
  *total = __shfl(inc, kLgGroup - 1, kLgGroup);
  return inc;
}

// The 16 bits of group g (0..3) in a ballot of the wave, bit l for lane l of the group.
__device__ __forceinline__ uint32_t lg_group16(uint64_t ballot, uint32_t g) {
  return (uint32_t)(ballot >> (g * kLgGroup)) & 0xFFFFu;
}

// The hand-off of lg_carry_in / lg_carry_next among the lanes of group g.  all: this lane's vector
// is all set; out: what it hands on when it is not (the caller's 16-bit rule with incoming state
// 0).  Returns the state before this lane's vector, to which the caller applies its rule again;
// *carry, uniform in the group, moves from the state before the step to the state after it.
// Holds two ballots: every lane of the wave calls it.
__device__ __forceinline__ uint32_t lg_carry(bool all, bool out, uint32_t gl, uint32_t g, uint32_t* carry) {
  const uint32_t ga = ~lg_group16(__ballot(all), g) & 0xFFFFu;
  const uint32_t gb = lg_group16(__ballot(out), g);
  const uint32_t in = lg_carry_in(ga, gb, gl, *carry);
  *carry = lg_carry_next(ga, gb, *carry);
  return in;
}

// c <= 16 bytes, compact in (lo, hi), to q: at most one store of each size.
__device__ __forceinline__ void lg_store_pieces(uint8_t* q, uint64_t lo, uint64_t hi, uint32_t c) {
  if (c & 16) {
    const u32x4 v = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    __builtin_memcpy(q, &v, 16);
    return;
  }
  if (c & 8) {
    __builtin_memcpy(q, &lo, 8);
    q += 8;
    lo = hi;
  }
  if (c & 4) {
    const uint32_t w = (uint32_t)lo;
    __builtin_memcpy(q, &w, 4);
    q += 4;
    lo >>= 32;
  }
  if (c & 2) {
    const uint16_t w = (uint16_t)lo;
    __builtin_memcpy(q, &w, 2);
    q += 2;
    lo >>= 16;
  }
  if (c & 1) *q = (uint8_t)lo;
}

// The kept bytes of the vector (vlo, vhi) go to output index j0 and up: output byte j belongs at
// out[lo + j] and is stored only for j in [jlo, jhi).  keep: the bytes to place, c of them;
// compact: whether they have to be moved together first (false: they are the low c bytes as they
// stand).  Bytes that lie inside the window altogether go out as at most one store of each size
// (stores here are bound by their number, not their bytes); at the edge of the window the bytes
// inside it go out one by one.
__device__ __forceinline__ void lg_place(uint8_t* out, int64_t lo, uint64_t jlo, uint64_t jhi, uint64_t j0,
                                         uint64_t vlo, uint64_t vhi, uint32_t keep, uint32_t c, bool compact) {
  if (c == 0 || j0 >= jhi || j0 + c <= jlo) return;
  if (compact) lg_compact(vlo, vhi, keep, &vlo, &vhi);
  if (j0 >= jlo && j0 + c <= jhi) {
    lg_store_pieces(out + (lo + (int64_t)j0), vlo, vhi, c);
  } else {
    for (uint32_t k = 0; k < c; ++k) {
      const uint64_t j = j0 + k;
      if (j >= jlo && j < jhi) out[lo + (int64_t)j] = (uint8_t)((k < 8 ? vlo : vhi) >> (8 * (k & 7)));
    }
  }
}

#endif  // __HIP__

}  // namespace amdx
