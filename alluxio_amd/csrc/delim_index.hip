// Delimiter index for gfx950 (wave64): the positions of one byte value in a virtual byte range
// [vstart, vstart + bytes) that is read through a virtual page table.  See DelimIndexArgs in
// kernels.h.
//
// The range is cut into tiles of 2^tile_shift bytes, counted from the aligned 16-byte vector that
// holds its first byte, so every tile is a whole number of aligned vectors and an aligned vector
// never straddles a page.  One wave owns a tile; a lane reads one vector per step and kDiUnroll
// steps are in flight (4 KiB per wave and iteration).
//
// count: a SWAR compare (lg_match of lane_group.h) marks the matching bytes of each 32-bit word
//        and a popcount adds them up; a wave reduction gives tile_count[t].  Only the first vector of the range and the last
//        vector of the last tile can hold bytes outside the range: those two take the masked
//        16-bit form below.  Lanes past the end of the range load nothing.
// scan:  one workgroup, exclusive prefix sum of the tile counts in rounds of 4096 tiles with a
//        carry; tile_base[ntiles] is the total.
// emit:  the wave re-reads its tile.  Each vector becomes a 16-bit match mask (lg_mask16); a step
//        without a delimiter ends there (one ballot).  Otherwise the counts of the kDiUnroll vectors of a
//        lane travel through ONE 64-bit wave scan as four 16-bit fields (a field holds at most
//        64 * 16 = 1024), so a delimiter's slot is tile_base[t] + the delimiters before it in
//        address order.  No atomics: the output is the same on every run.
//
// Quoted form (the *_quoted kernels): a quote byte toggles "inside quotes" and only a delimiter
// outside is a cut.  The state is a prefix parity, so it rides the same three launches: count
// stores a tile's quote parity and its delimiters at even and odd parity relative to the tile's
// start, scan turns the parities into each tile's incoming state and sums the matching counts,
// emit starts from that state.  Inside a step the state before a lane's vector is the running
// parity plus popcount(ballot(vector parity) & lanes below); inside a vector it is a prefix xor
// of the quote flags (of the 16-bit mask in emit, of the 0x80 byte flags in count).
#include "kernels.h"
#include "lane_group.h"

#include <algorithm>

namespace amdx {

namespace {

constexpr int kDiThreads = 256;          // 4 waves, each with its own tile
constexpr int kDiWaves = kDiThreads / 64;
constexpr int kDiUnroll = 4;             // 16-byte vectors in flight per lane
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;
constexpr uint32_t kDiMinTileShift = 10;   // one step of a wave: 64 lanes x 16 bytes
constexpr uint32_t kDiMaxTileShift = 24;   // 16 MiB; a tile's count fits uint32 with room to spare
constexpr uint32_t kDiMaxTiles = 1u << 30;

template <int NT>
__device__ __forceinline__ u32x4 di_load(const DelimIndexArgs& a, uint64_t va) {
  const uint64_t pmask = (1ull << a.page_shift) - 1;
  const u32x4* p = reinterpret_cast<const u32x4*>(a.arena + ((uint64_t)a.vtab[va >> a.page_shift] << a.page_shift) +
                                                  (va & pmask));
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

// The bits j of a 16-bit mask with lo <= j < hi: the bytes of a vector that lie in the range.
__device__ __forceinline__ uint32_t di_range16(uint32_t lo, uint32_t hi) {
  return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// Delimiters among the bytes of vector d (at virtual address va) that lie in [vstart, t1).  Only
// the first vector of the range and the last vector of the last tile can hold bytes outside: those
// two take the masked 16-bit form.  A vector at or past t1 was not loaded and holds no match.
__device__ __forceinline__ uint32_t di_count(u32x4 d, uint32_t dw, uint64_t va, uint64_t vstart, uint64_t t1) {
  if (va < vstart || (va < t1 && t1 - va < 16)) {
    const uint32_t lo = va < vstart ? (uint32_t)(vstart - va) : 0u;
    const uint32_t hi = t1 - va < 16 ? (uint32_t)(t1 - va) : 16u;
    return __popc(lg_mask16(d, dw) & di_range16(lo, hi));
  }
  return __popc(lg_match(d.x, dw)) + __popc(lg_match(d.y, dw)) + __popc(lg_match(d.z, dw)) + __popc(lg_match(d.w, dw));
}

struct DiTile {
  uint64_t t0, t1;   // virtual addresses: first vector of the tile, end of its bytes (exclusive)
};
__device__ __forceinline__ DiTile di_tile(const DelimIndexArgs& a, uint32_t t) {
  DiTile r;
  const uint64_t vend = a.vstart + a.bytes;
  r.t0 = (a.vstart & ~15ull) + ((uint64_t)t << a.tile_shift);
  r.t1 = r.t0 + (1ull << a.tile_shift);
  if (r.t1 > vend) r.t1 = vend;
  return r;
}

template <int NT>
__global__ __launch_bounds__(kDiThreads) void delim_count_kernel(DelimIndexArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kDiWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kDiWaves;
  const uint32_t dw = (a.delim & 0xFFu) * 0x01010101u;
  const u32x4 none = {~dw, ~dw, ~dw, ~dw};          // no byte of it matches
  for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
    const DiTile tl = di_tile(a, t);
    uint32_t cnt = 0;
    for (uint64_t vb = tl.t0; vb < tl.t1; vb += 64 * 16 * kDiUnroll) {
      u32x4 d[kDiUnroll];
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        d[u] = none;
        if (va < tl.t1) d[u] = di_load<NT>(a, va);
      }
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u)
        cnt += di_count(d[u], dw, vb + ((uint64_t)u * 64 + lane) * 16, a.vstart, tl.t1);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) a.tile_count[t] = cnt;
  }
}

// Exclusive scan of v over the workgroup (kScanThreads); *total = the sum.  sh: 17 entries.
__device__ __forceinline__ uint64_t di_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up((unsigned long long)inc, d);
    if ((int)lane >= d) inc += o;
  }
  if (lane == 63) sh[wid] = inc;
  __syncthreads();
  if (wid == 0) {
    const uint64_t w = lane < kScanThreads / 64 ? sh[lane] : 0;
    uint64_t wi = w;
#pragma unroll
    for (int d = 1; d < kScanThreads / 64; d <<= 1) {
      const uint64_t o = __shfl_up((unsigned long long)wi, d);
      if ((int)lane >= d) wi += o;
    }
    if (lane < kScanThreads / 64) sh[lane] = wi - w;
    if (lane == kScanThreads / 64 - 1) sh[kScanThreads / 64] = wi;
  }
  __syncthreads();
  const uint64_t r = sh[wid] + inc - v;
  *total = sh[kScanThreads / 64];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kScanThreads) void delim_scan_kernel(DelimIndexArgs a) {
  __shared__ uint64_t sh[kScanThreads / 64 + 1];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < a.ntiles; base += kScanThreads * kScanItems) {
    const uint32_t r0 = base + threadIdx.x * kScanItems;
    uint32_t c[kScanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      c[i] = r0 + i < a.ntiles ? a.tile_count[r0 + i] : 0u;
      sum += c[i];
    }
    uint64_t total;
    uint64_t off = carry + di_scan(sum, sh, &total);
    carry += total;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      if (r0 + i < a.ntiles) a.tile_base[r0 + i] = off;
      off += c[i];
    }
  }
  if (threadIdx.x == 0) a.tile_base[a.ntiles] = carry;
}

template <int NT>
__global__ __launch_bounds__(kDiThreads) void delim_emit_kernel(DelimIndexArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kDiWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kDiWaves;
  const uint32_t dw = (a.delim & 0xFFu) * 0x01010101u;
  const u32x4 none = {~dw, ~dw, ~dw, ~dw};
  for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
    const DiTile tl = di_tile(a, t);
    uint64_t run = a.tile_base[t];                  // slot of the tile's next delimiter (wave-uniform)
    for (uint64_t vb = tl.t0; vb < tl.t1; vb += 64 * 16 * kDiUnroll) {
      u32x4 d[kDiUnroll];
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        d[u] = none;
        if (va < tl.t1) d[u] = di_load<NT>(a, va);
      }
      // Every vector becomes its 16-bit mask here, with or without a delimiter: building it only
      // for the vectors that hold one (behind a per-lane branch) measured 20..27 % slower.
      uint32_t m[kDiUnroll];
      uint64_t p = 0;
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        const uint32_t lo = va < a.vstart ? (uint32_t)(a.vstart - va) : 0u;
        const uint32_t hi = va >= tl.t1 ? 0u : (tl.t1 - va < 16 ? (uint32_t)(tl.t1 - va) : 16u);
        m[u] = lg_mask16(d[u], dw) & di_range16(lo, hi);
        p |= (uint64_t)__popc(m[u]) << (16 * u);
      }
      if (__ballot(p != 0) == 0ull) continue;       // wave-uniform
      uint64_t inc = p;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)inc, s);
        if ((int)lane >= s) inc += o;
      }
      const uint64_t tot = __shfl((unsigned long long)inc, 63);
      const uint64_t exc = inc - p;
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        uint64_t pos = run + ((exc >> (16 * u)) & 0xFFFFu);
        uint32_t mm = m[u];
        while (mm) {
          const uint32_t j = (uint32_t)__builtin_ctz(mm);
          if (pos < a.out_cap) a.out[pos] = a.add + (va + j - a.vstart) + 1;
          ++pos;
          mm &= mm - 1;
        }
        run += (tot >> (16 * u)) & 0xFFFFu;
      }
    }
  }
}

// ---- quoted form --------------------------------------------------------------------------------
// A byte that is neither the delimiter nor the quote: the content of a vector that was not loaded.
__device__ __forceinline__ uint32_t di_neither(uint32_t d, uint32_t q) {
  return (d != 0 && q != 0) ? 0u : ((d != 1 && q != 1) ? 1u : 2u);
}

// The masks of one vector: dm = delimiters, qm = quotes, both limited to the bytes of the range.
struct DiMasks {
  uint32_t dm, qm;
};
__device__ __forceinline__ DiMasks di_masks(u32x4 v, uint32_t dw, uint32_t qw, uint64_t va, uint64_t vstart,
                                            uint64_t t1) {
  const uint32_t lo = va < vstart ? (uint32_t)(vstart - va) : 0u;
  const uint32_t hi = va >= t1 ? 0u : (t1 - va < 16 ? (uint32_t)(t1 - va) : 16u);
  DiMasks r;
  r.dm = lg_mask16(v, dw) & di_range16(lo, hi);
  r.qm = lg_mask16(v, qw) & di_range16(lo, hi);
  return r;
}

// The delimiters of one vector that lie inside quotes.  par: the wave-uniform state before group
// u of this step; it moves on to the state after the group.  Within a step the address order is
// group u, then lane, so the state before this lane's vector is par plus the parity of the quote
// bytes of the lanes below: one ballot, no shuffle scan.
__device__ __forceinline__ uint32_t di_quoted_part(const DiMasks& k, uint32_t lane, uint32_t* par) {
  const uint64_t b = __ballot(__popc(k.qm) & 1);
  const uint32_t before = (*par ^ (uint32_t)__popcll(b & ((1ull << lane) - 1ull))) & 1u;
  *par = (*par ^ (uint32_t)__popcll(b)) & 1u;
  const uint32_t inq = lg_inside16(k.qm) ^ (before ? 0xFFFFu : 0u);
  return k.dm & inq;
}

// What the count kernel needs of one vector, relative to a vector that starts outside quotes:
// all = its delimiters, odd = those of them inside quotes, par = the parity of its quote bytes.
// The bytes stay where they are: lg_match leaves 0x80 per matching byte, and as the lowest address
// is the lowest byte of a word, p ^= p << 8; p ^= p << 16 turns the quote flags into the parity of
// the quotes up to and including each byte, p << 8 into that of the quotes before it, and bit 31
// of p carries on into the next word (m: all ones when the word starts inside).  No 16-bit mask
// and none of its multiplies; only the two vectors that can hold bytes outside the range build one.
struct DiRel {
  uint32_t all, odd, par;
};
__device__ __forceinline__ DiRel di_rel(u32x4 v, uint32_t dw, uint32_t qw, uint64_t va, uint64_t vstart, uint64_t t1) {
  DiRel r;
  if (va < vstart || (va < t1 && t1 - va < 16)) {
    const DiMasks k = di_masks(v, dw, qw, va, vstart, t1);
    r.all = __popc(k.dm);
    r.odd = __popc(k.dm & lg_inside16(k.qm));
    r.par = __popc(k.qm) & 1u;
    return r;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
  r.all = 0;
  r.odd = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t dz = lg_match(w[i], dw);
    uint32_t p = lg_match(w[i], qw);
    p ^= p << 8;
    p ^= p << 16;
    r.all += __popc(dz);
    r.odd += __popc(dz & ((p << 8) ^ m));
    m ^= (uint32_t)((int32_t)p >> 31);
  }
  r.par = m & 1u;
  return r;
}

// FAST: a step whose vectors hold no quote byte at all (one ballot; bytes outside the range make
// it take the exact path, never a wrong one) adds the SWAR popcount to the counter of the running
// parity.
template <int NT, int FAST>
__global__ __launch_bounds__(kDiThreads) void delim_count_quoted_kernel(DelimIndexArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kDiWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kDiWaves;
  const uint32_t dw = (a.delim & 0xFFu) * 0x01010101u;
  const uint32_t qw = (a.quote & 0xFFu) * 0x01010101u;
  const uint32_t nw = di_neither(a.delim & 0xFFu, a.quote & 0xFFu) * 0x01010101u;
  const u32x4 none = {nw, nw, nw, nw};
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
    const DiTile tl = di_tile(a, t);
    uint32_t all = 0, odd = 0;
    uint32_t par = 0;                               // relative to the tile's start (wave-uniform)
    for (uint64_t vb = tl.t0; vb < tl.t1; vb += 64 * 16 * kDiUnroll) {
      u32x4 d[kDiUnroll];
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        d[u] = none;
        if (va < tl.t1) d[u] = di_load<NT>(a, va);
      }
      if constexpr (FAST) {
        uint32_t any = 0;
#pragma unroll
        for (int u = 0; u < kDiUnroll; ++u)
          any |= lg_match(d[u].x, qw) | lg_match(d[u].y, qw) | lg_match(d[u].z, qw) | lg_match(d[u].w, qw);
        if (__ballot(any != 0) == 0ull) {           // wave-uniform
          uint32_t c = 0;
#pragma unroll
          for (int u = 0; u < kDiUnroll; ++u)
            c += di_count(d[u], dw, vb + ((uint64_t)u * 64 + lane) * 16, a.vstart, tl.t1);
          all += c;
          if (par) odd += c;
          continue;
        }
      }
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const DiRel r = di_rel(d[u], dw, qw, vb + ((uint64_t)u * 64 + lane) * 16, a.vstart, tl.t1);
        // address order is group u, then lane: the state before this vector is the running parity
        // plus the parity of the quote bytes of the lanes below (one ballot, no shuffle scan)
        const uint64_t b = __ballot(r.par);
        const uint32_t before = (par ^ (uint32_t)__popcll(b & below)) & 1u;
        par = (par ^ (uint32_t)__popcll(b)) & 1u;
        all += r.all;
        odd += before ? r.all - r.odd : r.odd;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      all += __shfl_xor(all, s);
      odd += __shfl_xor(odd, s);
    }
    if (lane == 0) {
      a.tile_count[t] = all - odd;
      a.tile_count_odd[t] = odd;
      a.tile_parity[t] = par;
    }
  }
}

__global__ __launch_bounds__(kScanThreads) void delim_scan_quoted_kernel(DelimIndexArgs a) {
  __shared__ uint64_t sh[kScanThreads / 64 + 1];
  uint64_t carry = 0;
  uint32_t state = a.in_quote & 1u;                 // before the round's first tile
  for (uint32_t base = 0; base < a.ntiles; base += kScanThreads * kScanItems) {
    const uint32_t r0 = base + threadIdx.x * kScanItems;
    uint32_t ce[kScanItems], co[kScanItems], pq[kScanItems];
    uint64_t psum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      const bool in = r0 + i < a.ntiles;
      ce[i] = in ? a.tile_count[r0 + i] : 0u;
      co[i] = in ? a.tile_count_odd[r0 + i] : 0u;
      pq[i] = in ? a.tile_parity[r0 + i] & 1u : 0u;
      psum += pq[i];
    }
    uint64_t ptotal;
    uint32_t s = (state + (uint32_t)di_scan(psum, sh, &ptotal)) & 1u;   // before this thread's first tile
    state = (state + (uint32_t)ptotal) & 1u;
    uint32_t c[kScanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      c[i] = s ? co[i] : ce[i];
      sum += c[i];
      if (r0 + i < a.ntiles) a.tile_parity[r0 + i] = s;
      s ^= pq[i];
    }
    uint64_t total;
    uint64_t off = carry + di_scan(sum, sh, &total);
    carry += total;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      if (r0 + i < a.ntiles) a.tile_base[r0 + i] = off;
      off += c[i];
    }
  }
  if (threadIdx.x == 0) {
    a.tile_base[a.ntiles] = carry;
    a.tile_parity[a.ntiles] = state;
  }
}

template <int NT>
__global__ __launch_bounds__(kDiThreads) void delim_emit_quoted_kernel(DelimIndexArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kDiWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kDiWaves;
  const uint32_t dw = (a.delim & 0xFFu) * 0x01010101u;
  const uint32_t qw = (a.quote & 0xFFu) * 0x01010101u;
  const uint32_t nw = di_neither(a.delim & 0xFFu, a.quote & 0xFFu) * 0x01010101u;
  const u32x4 none = {nw, nw, nw, nw};
  for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
    const DiTile tl = di_tile(a, t);
    uint64_t run = a.tile_base[t];                  // slot of the tile's next cut (wave-uniform)
    uint32_t par = __builtin_amdgcn_readfirstlane(a.tile_parity[t]) & 1u;   // the tile's incoming state
    for (uint64_t vb = tl.t0; vb < tl.t1; vb += 64 * 16 * kDiUnroll) {
      u32x4 d[kDiUnroll];
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        d[u] = none;
        if (va < tl.t1) d[u] = di_load<NT>(a, va);
      }
      uint32_t m[kDiUnroll];
      uint64_t p = 0;
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const DiMasks k = di_masks(d[u], dw, qw, vb + ((uint64_t)u * 64 + lane) * 16, a.vstart, tl.t1);
        m[u] = k.dm ^ di_quoted_part(k, lane, &par);      // dm & ~inside
        p |= (uint64_t)__popc(m[u]) << (16 * u);
      }
      if (__ballot(p != 0) == 0ull) continue;       // wave-uniform; par has moved past the step
      uint64_t inc = p;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)inc, s);
        if ((int)lane >= s) inc += o;
      }
      const uint64_t tot = __shfl((unsigned long long)inc, 63);
      const uint64_t exc = inc - p;
#pragma unroll
      for (int u = 0; u < kDiUnroll; ++u) {
        const uint64_t va = vb + ((uint64_t)u * 64 + lane) * 16;
        uint64_t pos = run + ((exc >> (16 * u)) & 0xFFFFu);
        uint32_t mm = m[u];
        while (mm) {
          const uint32_t j = (uint32_t)__builtin_ctz(mm);
          if (pos < a.out_cap) a.out[pos] = a.add + (va + j - a.vstart) + 1;
          ++pos;
          mm &= mm - 1;
        }
        run += (tot >> (16 * u)) & 0xFFFFu;
      }
    }
  }
}

// Defaults from tools/delim_index_bench.py on MI355X (profiles/delim_index.md, delim_index_quoted.md).
// Count variant 1 is 6..19 % faster in count on a file without any quote and up to 8 % slower at
// a CSV-like quote density; the three launches together differ by 1..6 % either way, about their
// spread, so the simpler one is the default.
int g_di_quote_variant = 0;
int g_di_variant = 1;           // nontemporal loads: every byte is read once per launch
uint32_t g_di_tile_shift = 15;   // 32 KiB per wave
unsigned g_di_grid_cap = 2048;   // 256 CUs x 8 workgroups of 4 waves

hipError_t di_check(const DelimIndexArgs& a) {
  if (a.page_shift < 4 || a.page_shift > 40 || a.tile_shift < kDiMinTileShift || a.tile_shift > kDiMaxTileShift ||
      a.delim > 255 || (reinterpret_cast<uint64_t>(a.arena) & 15) || a.bytes == 0 || a.vstart + a.bytes < a.vstart)
    return hipErrorInvalidValue;
  const uint64_t nt = delim_index_tiles(a.vstart, a.bytes, a.tile_shift);
  if (nt == 0 || nt > kDiMaxTiles || nt != a.ntiles) return hipErrorInvalidValue;
  return hipSuccess;
}

hipError_t di_check_quoted(const DelimIndexArgs& a) {
  if (a.quote > 255 || a.quote == a.delim || a.in_quote > 1) return hipErrorInvalidValue;
  return di_check(a);
}

unsigned di_grid(const DelimIndexArgs& a) {
  return std::min<unsigned>((a.ntiles + kDiWaves - 1) / kDiWaves, g_di_grid_cap);
}

}  // namespace

void set_delim_index_variant(int variant, unsigned tile_shift) {
  g_di_variant = variant ? 1 : 0;
  if (tile_shift >= kDiMinTileShift && tile_shift <= kDiMaxTileShift) g_di_tile_shift = tile_shift;
}

uint32_t delim_index_tile_shift() { return g_di_tile_shift; }

int delim_index_variant() { return g_di_variant; }

uint64_t delim_index_tiles(uint64_t vstart, uint64_t bytes, uint32_t tile_shift) {
  if (bytes == 0) return 0;
  const uint64_t span = (vstart & 15) + bytes;      // from the first aligned vector to the end of the range
  return (span + (1ull << tile_shift) - 1) >> tile_shift;
}

hipError_t launch_delim_count(const DelimIndexArgs& a, hipStream_t stream) {
  const hipError_t c = di_check(a);
  if (c != hipSuccess) return c;
  if (g_di_variant == 1) hipLaunchKernelGGL(delim_count_kernel<1>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  else hipLaunchKernelGGL(delim_count_kernel<0>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_delim_scan(const DelimIndexArgs& a, hipStream_t stream) {
  const hipError_t c = di_check(a);
  if (c != hipSuccess) return c;
  hipLaunchKernelGGL(delim_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_delim_emit(const DelimIndexArgs& a, uint64_t total, hipStream_t stream) {
  const hipError_t c = di_check(a);
  if (c != hipSuccess) return c;
  if (total > a.out_cap) return hipErrorInvalidValue;
  if (total == 0) return hipSuccess;
  if (g_di_variant == 1) hipLaunchKernelGGL(delim_emit_kernel<1>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  else hipLaunchKernelGGL(delim_emit_kernel<0>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  return hipGetLastError();
}

void set_delim_quote_variant(int variant) { g_di_quote_variant = variant ? 1 : 0; }

int delim_quote_variant() { return g_di_quote_variant; }

hipError_t launch_delim_count_quoted(const DelimIndexArgs& a, hipStream_t stream) {
  const hipError_t c = di_check_quoted(a);
  if (c != hipSuccess) return c;
  const dim3 grid(di_grid(a)), block(kDiThreads);
  if (g_di_variant == 1) {
    if (g_di_quote_variant == 1) hipLaunchKernelGGL((delim_count_quoted_kernel<1, 1>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((delim_count_quoted_kernel<1, 0>), grid, block, 0, stream, a);
  } else {
    if (g_di_quote_variant == 1) hipLaunchKernelGGL((delim_count_quoted_kernel<0, 1>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((delim_count_quoted_kernel<0, 0>), grid, block, 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_delim_scan_quoted(const DelimIndexArgs& a, hipStream_t stream) {
  const hipError_t c = di_check_quoted(a);
  if (c != hipSuccess) return c;
  hipLaunchKernelGGL(delim_scan_quoted_kernel, dim3(1), dim3(kScanThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_delim_emit_quoted(const DelimIndexArgs& a, uint64_t total, hipStream_t stream) {
  const hipError_t c = di_check_quoted(a);
  if (c != hipSuccess) return c;
  if (total > a.out_cap) return hipErrorInvalidValue;
  if (total == 0) return hipSuccess;
  if (g_di_variant == 1)
    hipLaunchKernelGGL(delim_emit_quoted_kernel<1>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  else hipLaunchKernelGGL(delim_emit_quoted_kernel<0>, dim3(di_grid(a)), dim3(kDiThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
