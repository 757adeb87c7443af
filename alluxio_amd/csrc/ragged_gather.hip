// Ragged gather for gfx950 (wave64): variable-length records, read through a virtual page
// table, land in a packed (offsets) or padded (row stride) batch.  See RaggedGatherArgs in
// kernels.h for the layouts.
//
// Plan (one workgroup): each thread takes 4 consecutive rows per round, looks their lengths up
// and two workgroup scans give the row offsets and the work-item prefix; totals carry from one
// round of 4096 rows to the next, so any batch up to kRaggedGatherMaxBatch runs in one launch.
//
// Copy: a work item is 2^chunk_shift consecutive 16-byte vectors of the DESTINATION of one row,
// counted from the aligned vector that holds the row's first byte; one wave owns a work item
// (a uniform binary search in the work-item prefix finds its row).  Every lane writes whole
// aligned 16-byte vectors; only the first and last vector of a row, when the row does not start
// or end on a 16-byte boundary, are written byte by byte (inside the row, never outside).  The
// source sits at a fixed byte phase s = (src - dst) mod 16 for the whole row:
//   variant 0: an unaligned 16-byte load when the vector lies inside the record and inside one
//              page; the funnel otherwise;
//   variant 1: every lane loads the aligned 16-byte block that holds its first source byte,
//              takes the following block from the next lane (the last lane loads it) and
//              funnels the two registers by s bytes.
// Aligned blocks never straddle a page, so a vector whose two blocks sit in arena pages that are
// not neighbours needs nothing special.  Bytes past the record inside the row (the alignment gap
// of the packed layout, the padding of the padded one) are produced in registers and stored with
// the same vectors.
#include "kernels.h"

#include <algorithm>

namespace amdx {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

constexpr int kRgThreads = 256;          // 4 waves, each with its own work item
constexpr int kRgWaves = kRgThreads / 64;
constexpr int kRgUnroll = 4;             // 16-byte vectors in flight per lane
constexpr int kPlanThreads = 1024;
constexpr int kPlanItems = 4;

__device__ __forceinline__ const uint8_t* rg_xlate(const RaggedGatherArgs& a, uint64_t va) {
  const uint64_t pmask = (1ull << a.page_shift) - 1;
  return a.arena + ((uint64_t)a.vtab[va >> a.page_shift] << a.page_shift) + (va & pmask);
}

// The aligned 16-byte block at virtual address vb when it holds a byte of the record
// [src, end): such a block lies in a page of the record.  Zeros otherwise, without a load.
__device__ __forceinline__ u32x4 rg_block(const RaggedGatherArgs& a, int64_t vb, int64_t src, int64_t end) {
  u32x4 z = {0u, 0u, 0u, 0u};
  if (vb + 16 > src && vb < end) z = *reinterpret_cast<const u32x4*>(rg_xlate(a, (uint64_t)vb));
  return z;
}

// Bytes [s, s + 16) of the 32 bytes b0:b1 (s is the same in every lane of the wave).
__device__ __forceinline__ u32x4 rg_funnel(u32x4 b0, u32x4 b1, uint32_t s) {
  uint32_t w0 = b0.x, w1 = b0.y, w2 = b0.z, w3 = b0.w, w4 = b1.x, w5 = b1.y, w6 = b1.z, w7 = b1.w;
  if (s & 8) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; w5 = w7; }
  if (s & 4) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
  const uint32_t sb = s & 3;
  u32x4 o;
  o.x = __builtin_amdgcn_alignbyte(w1, w0, sb);
  o.y = __builtin_amdgcn_alignbyte(w2, w1, sb);
  o.z = __builtin_amdgcn_alignbyte(w3, w2, sb);
  o.w = __builtin_amdgcn_alignbyte(w4, w3, sb);
  return o;
}

// Keep the first k bytes of d (k may be <= 0), the rest becomes the fill byte.
__device__ __forceinline__ uint32_t rg_blend_word(uint32_t d, int64_t k, uint32_t fillw) {
  const uint32_t mask = k >= 4 ? 0xFFFFFFFFu : (k <= 0 ? 0u : ((1u << (8 * (uint32_t)k)) - 1u));
  return (d & mask) | (fillw & ~mask);
}
__device__ __forceinline__ u32x4 rg_blend(u32x4 d, int64_t k, uint32_t fillw) {
  d.x = rg_blend_word(d.x, k, fillw);
  d.y = rg_blend_word(d.y, k - 4, fillw);
  d.z = rg_blend_word(d.z, k - 8, fillw);
  d.w = rg_blend_word(d.w, k - 12, fillw);
  return d;
}

// Store the bytes [ws, we) of vector `dat` at the 16-byte aligned address d.
__device__ __forceinline__ void rg_store(uint8_t* d, u32x4 dat, int ws, int we) {
  if (ws == 0 && we == 16) {
    *reinterpret_cast<u32x4*>(d) = dat;
    return;
  }
  const uint32_t w[4] = {dat.x, dat.y, dat.z, dat.w};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (j >= ws && j < we) d[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

template <int VAR>
__global__ __launch_bounds__(kRgThreads) void ragged_copy_kernel(RaggedGatherArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kRgWaves + (threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kRgWaves;
  const uint64_t psize = 1ull << a.page_shift;
  const uint32_t fillw = a.padded ? (a.pad_value & 0xFFu) * 0x01010101u : 0u;
  const u32x4 fillv = {fillw, fillw, fillw, fillw};
  for (uint32_t c = wave; c < a.total_chunks; c += nwaves) {
    uint32_t lo = 0, hi = a.batch - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (a.chunk_pre[mid] <= c) lo = mid; else hi = mid - 1;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    const RaggedRow row = a.rows[lo];
    const uint64_t D = (uint64_t)a.dst + row.dst_off;
    const uint64_t vlast = (D + row.span + 15) >> 4;
    const uint64_t vfirst = (D >> 4) + ((uint64_t)(c - row.chunk0) << a.chunk_shift);
    uint64_t vend = vfirst + (1ull << a.chunk_shift);
    if (vend > vlast) vend = vlast;
    const int64_t src = (int64_t)row.src, len = (int64_t)row.len, end = src + len;
    const int64_t span = (int64_t)row.span;
    const uint32_t s = __builtin_amdgcn_readfirstlane((uint32_t)(row.src - D) & 15u);
    for (uint64_t vb = vfirst; vb < vend; vb += 64 * kRgUnroll) {
      u32x4 dat[kRgUnroll];
      if constexpr (VAR == 0) {
#pragma unroll
        for (int u = 0; u < kRgUnroll; ++u) {
          const uint64_t v = vb + (uint64_t)u * 64 + lane;
          dat[u] = fillv;
          if (v >= vend) continue;
          const int64_t p = (int64_t)((v << 4) - D);   // row-relative position of the vector
          if (p >= len) continue;
          const int64_t q = src + p;
          if (p >= 0 && p + 16 <= len && ((uint64_t)q & (psize - 1)) + 16 <= psize) {
            dat[u] = *reinterpret_cast<const u32x4_u*>(rg_xlate(a, (uint64_t)q));
          } else {
            const int64_t b = q & ~(int64_t)15;
            const u32x4 b0 = rg_block(a, b, src, end);
            u32x4 b1 = {0u, 0u, 0u, 0u};
            if (s) b1 = rg_block(a, b + 16, src, end);
            dat[u] = rg_funnel(b0, b1, s);
          }
        }
      } else {
        u32x4 b0[kRgUnroll], bx[kRgUnroll];
#pragma unroll
        for (int u = 0; u < kRgUnroll; ++u) {
          const uint64_t v = vb + (uint64_t)u * 64 + lane;
          const int64_t b = (src + (int64_t)((v << 4) - D)) & ~(int64_t)15;
          b0[u] = (u32x4){0u, 0u, 0u, 0u};
          bx[u] = (u32x4){0u, 0u, 0u, 0u};
          if (v < vend) {
            b0[u] = rg_block(a, b, src, end);
            // the next lane holds the following block unless this is the wave's or the item's last vector
            if (s && (lane == 63 || v + 1 >= vend)) bx[u] = rg_block(a, b + 16, src, end);
          }
        }
#pragma unroll
        for (int u = 0; u < kRgUnroll; ++u) {
          const uint64_t v = vb + (uint64_t)u * 64 + lane;
          u32x4 b1;
          b1.x = __shfl_down(b0[u].x, 1);
          b1.y = __shfl_down(b0[u].y, 1);
          b1.z = __shfl_down(b0[u].z, 1);
          b1.w = __shfl_down(b0[u].w, 1);
          if (lane == 63 || v + 1 >= vend) b1 = bx[u];
          dat[u] = rg_funnel(b0[u], b1, s);
        }
      }
#pragma unroll
      for (int u = 0; u < kRgUnroll; ++u) {
        const uint64_t v = vb + (uint64_t)u * 64 + lane;
        if (v >= vend) continue;
        const int64_t p = (int64_t)((v << 4) - D);
        u32x4 o = dat[u];
        if (len - p < 16) o = rg_blend(o, len - p, fillw);
        const int ws = p < 0 ? (int)-p : 0;
        const int we = span - p < 16 ? (int)(span - p) : 16;
        rg_store(reinterpret_cast<uint8_t*>(v << 4), o, ws, we);
      }
    }
  }
}

// Exclusive scan of v over the workgroup (kPlanThreads); *total = the sum.  sh: 17 entries.
__device__ __forceinline__ uint64_t rg_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
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
    const uint64_t w = lane < kPlanThreads / 64 ? sh[lane] : 0;
    uint64_t wi = w;
#pragma unroll
    for (int d = 1; d < kPlanThreads / 64; d <<= 1) {
      const uint64_t o = __shfl_up((unsigned long long)wi, d);
      if ((int)lane >= d) wi += o;
    }
    if (lane < kPlanThreads / 64) sh[lane] = wi - w;
    if (lane == kPlanThreads / 64 - 1) sh[kPlanThreads / 64] = wi;
  }
  __syncthreads();
  const uint64_t r = sh[wid] + inc - v;
  *total = sh[kPlanThreads / 64];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kPlanThreads) void ragged_plan_kernel(RaggedGatherArgs a) {
  __shared__ uint64_t sh[kPlanThreads / 64 + 1];
  uint64_t carry_off = 0, carry_ch = 0;
  const uint64_t vpc_mask = (1ull << a.chunk_shift) - 1;
  for (uint32_t base = 0; base < a.batch; base += kPlanThreads * kPlanItems) {
    const uint32_t r0 = base + threadIdx.x * kPlanItems;
    uint64_t src[kPlanItems], adv[kPlanItems], nch[kPlanItems];
    uint32_t len[kPlanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kPlanItems; ++i) {
      src[i] = 0;
      adv[i] = 0;
      len[i] = 0;
      if (r0 + i < a.batch) {
        const uint64_t id = (uint64_t)a.idx[r0 + i];
        if (id < a.n_rec) {          // the host rejected anything else; never index past the table
          const uint4 rec = *reinterpret_cast<const uint4*>(a.recs + id);
          src[i] = ((uint64_t)rec.y << 32) | rec.x;
          len[i] = rec.z;
        }
        if (a.padded) {
          if (len[i] > a.max_len) len[i] = a.max_len;
          adv[i] = a.row_stride;
        } else {
          adv[i] = ((uint64_t)len[i] + a.align - 1) & ~(uint64_t)(a.align - 1);
        }
      }
      sum += adv[i];
    }
    uint64_t total;
    uint64_t off = carry_off + rg_scan(sum, sh, &total);
    carry_off += total;
    uint64_t csum = 0;
    uint64_t o = off;
#pragma unroll
    for (int i = 0; i < kPlanItems; ++i) {
      nch[i] = 0;
      if (r0 + i < a.batch) {
        const uint64_t span = a.padded ? a.max_len : adv[i];
        const uint64_t D = (uint64_t)a.dst + o;
        const uint64_t nvec = span ? ((D + span + 15) >> 4) - (D >> 4) : 0;
        nch[i] = (nvec + vpc_mask) >> a.chunk_shift;
      }
      csum += nch[i];
      o += adv[i];
    }
    uint64_t ch = carry_ch + rg_scan(csum, sh, &total);
    carry_ch += total;
#pragma unroll
    for (int i = 0; i < kPlanItems; ++i) {
      if (r0 + i < a.batch) {
        RaggedRow row;
        row.src = src[i];
        row.dst_off = off;
        row.span = a.padded ? a.max_len : adv[i];
        row.len = len[i];
        row.chunk0 = (uint32_t)ch;
        a.rows[r0 + i] = row;
        a.chunk_pre[r0 + i] = (uint32_t)ch;
        a.out_off[r0 + i] = off;
        a.out_len[r0 + i] = len[i];
      }
      off += adv[i];
      ch += nch[i];
    }
  }
  if (threadIdx.x == 0) {
    a.out_off[a.batch] = carry_off;
    a.chunk_pre[a.batch] = (uint32_t)carry_ch;
  }
}

// Default from tools/ragged_gather_bench.py on MI355X (profiles/ragged_gather.md).
int g_rg_variant = 0;
uint32_t g_rg_chunk_shift = 8;   // 256 vectors = 4 KiB per wave
unsigned g_rg_grid_cap = 2048;   // 256 CUs x 8 workgroups of 4 waves

}  // namespace

void set_ragged_gather_variant(int variant, unsigned chunk_shift) {
  g_rg_variant = variant ? 1 : 0;
  if (chunk_shift >= 6 && chunk_shift <= 16) g_rg_chunk_shift = chunk_shift;
}

uint32_t ragged_gather_chunk_shift() { return g_rg_chunk_shift; }

hipError_t launch_ragged_gather(const RaggedGatherArgs& a, hipStream_t stream) {
  if (a.batch == 0) return hipSuccess;
  if (a.batch > kRaggedGatherMaxBatch || a.chunk_shift < 6 || a.chunk_shift > 16 || a.page_shift < 4 ||
      a.page_shift > 40)
    return hipErrorInvalidValue;
  if (a.padded ? a.row_stride < a.max_len : (a.align == 0 || a.align > 256 || (a.align & (a.align - 1))))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ragged_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.total_chunks == 0) return e;
  const unsigned grid = std::min<unsigned>((a.total_chunks + kRgWaves - 1) / kRgWaves, g_rg_grid_cap);
  if (g_rg_variant == 1) hipLaunchKernelGGL(ragged_copy_kernel<1>, dim3(grid), dim3(kRgThreads), 0, stream, a);
  else hipLaunchKernelGGL(ragged_copy_kernel<0>, dim3(grid), dim3(kRgThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
