// Delimiter index for gfx950 (wave64): the positions of one byte value in a virtual byte range
// [vstart, vstart + bytes) that is read through a virtual page table.  See DelimIndexArgs in
// kernels.h.
//
// The range is cut into tiles of 2^tile_shift bytes, counted from the aligned 16-byte vector that
// holds its first byte, so every tile is a whole number of aligned vectors and an aligned vector
// never straddles a page.  One wave owns a tile; a lane reads one vector per step and kDiUnroll
// steps are in flight (4 KiB per wave and iteration).
//
// count: a SWAR compare marks the matching bytes of each 32-bit word and a popcount adds them up;
//        a wave reduction gives tile_count[t].  Only the first vector of the range and the last
//        vector of the last tile can hold bytes outside the range: those two take the masked
//        16-bit form below.  Lanes past the end of the range load nothing.
// scan:  one workgroup, exclusive prefix sum of the tile counts in rounds of 4096 tiles with a
//        carry; tile_base[ntiles] is the total.
// emit:  the wave re-reads its tile.  Each vector becomes a 16-bit match mask; a step without a
//        delimiter ends there (one ballot).  Otherwise the counts of the kDiUnroll vectors of a
//        lane travel through ONE 64-bit wave scan as four 16-bit fields (a field holds at most
//        64 * 16 = 1024), so a delimiter's slot is tile_base[t] + the delimiters before it in
//        address order.  No atomics: the output is the same on every run.
#include "kernels.h"

#include <algorithm>

namespace amdx {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

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

// 0x80 in every byte of w that equals the delimiter (dw: the delimiter in all four bytes).  Exact:
// the add never carries from one byte into the next.
__device__ __forceinline__ uint32_t di_match(uint32_t w, uint32_t dw) {
  const uint32_t x = w ^ dw;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// Bits 7, 15, 23, 31 of z -> bits 0..3.
__device__ __forceinline__ uint32_t di_pack(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }

// Bit j is set when byte j of the vector equals the delimiter and lo <= j < hi.
__device__ __forceinline__ uint32_t di_mask16(u32x4 v, uint32_t dw, uint32_t lo, uint32_t hi) {
  const uint32_t m = di_pack(di_match(v.x, dw)) | (di_pack(di_match(v.y, dw)) << 4) |
                     (di_pack(di_match(v.z, dw)) << 8) | (di_pack(di_match(v.w, dw)) << 12);
  return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// Delimiters among the bytes of vector d (at virtual address va) that lie in [vstart, t1).  Only
// the first vector of the range and the last vector of the last tile can hold bytes outside: those
// two take the masked 16-bit form.  A vector at or past t1 was not loaded and holds no match.
__device__ __forceinline__ uint32_t di_count(u32x4 d, uint32_t dw, uint64_t va, uint64_t vstart, uint64_t t1) {
  if (va < vstart || (va < t1 && t1 - va < 16)) {
    const uint32_t lo = va < vstart ? (uint32_t)(vstart - va) : 0u;
    const uint32_t hi = t1 - va < 16 ? (uint32_t)(t1 - va) : 16u;
    return __popc(di_mask16(d, dw, lo, hi));
  }
  return __popc(di_match(d.x, dw)) + __popc(di_match(d.y, dw)) + __popc(di_match(d.z, dw)) + __popc(di_match(d.w, dw));
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
        m[u] = di_mask16(d[u], dw, lo, hi);
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

// Defaults from tools/delim_index_bench.py on MI355X (profiles/delim_index.md).
int g_di_variant = 1;            // nontemporal loads: every byte is read once per launch
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

}  // namespace amdx
