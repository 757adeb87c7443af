// Text columns from spans for gfx950 (wave64): the two passes of text_column_host.h, measure and
// emit, each in two variants.  The rule and the liveness and window checks are those of the header,
// compiled for the device.
//
// Variant 0, one lane per value: tc_measure_one / tc_emit_one as they stand, a serial byte walk.
//
// Variant 1, cooperative: a group of 16 lanes owns a value (four values per wave) and walks it in
// steps of 256 bytes, lane l of the group loading the 16 bytes at step * 256 + 16 * l.  A vector
// becomes a 16-bit quote mask (the SWAR compare of field_parse.hip) and tc_drop16 marks the 2nd,
// 4th, ... quote of each run.  The one thing a vector needs from the bytes before it is whether the
// run that reaches it has odd length so far.  A vector that is not all quotes knows what it hands
// on without knowing what it got, and one of 16 quotes hands on what it got, so a lane's incoming
// state is that of the nearest lower lane whose vector is not all quotes, or the group's carried
// state: two ballots, no chain through the lanes.  Measure adds up the popcounts of the keep-masks.
// Emit places each lane's kept bytes by a 16-lane prefix sum of them plus a running count; a full
// vector without a dropped byte goes out as one 16-byte store at whatever phase the destination
// has, anything else is compacted in registers and goes out as at most one 8-, 4-, 2- and 1-byte
// store (stores here are bound by their number, not their bytes).  A lane whose bytes touch the
// edge of the value's window stores the bytes inside it one by one.
//
// No path loads a byte outside the value it was given: a vector that reaches past the end is
// assembled from byte loads.  Values are independent, so there are no atomics and no waits between
// workgroups, and two runs write the same bytes.
#include "kernels.h"

namespace amdx {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kTcThreads = 256;
constexpr int kTcGroup = 16;                        // lanes per value in variant 1
constexpr int kTcValuesPerBlock = kTcThreads / kTcGroup;

__global__ __launch_bounds__(kTcThreads) void text_measure_lane_kernel(TextColumnArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kTcThreads + threadIdx.x;
  if (r < a.n) tc_measure_one(a, r);
}

__global__ __launch_bounds__(kTcThreads) void text_emit_lane_kernel(TextColumnArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kTcThreads + threadIdx.x;
  if (r < a.n) tc_emit_one(a, r);
}

// 0x80 in every byte of w that equals the byte replicated in dw (exact: no carry between bytes).
__device__ __forceinline__ uint32_t tc_match(uint32_t w, uint32_t dw) {
  const uint32_t x = w ^ dw;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t tc_pack(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }
__device__ __forceinline__ uint32_t tc_mask16(u32x4 v, uint32_t dw) {
  return tc_pack(tc_match(v.x, dw)) | (tc_pack(tc_match(v.y, dw)) << 4) | (tc_pack(tc_match(v.z, dw)) << 8) |
         (tc_pack(tc_match(v.w, dw)) << 12);
}

// The 16 bytes at p, or the first rem < 16 of them from byte loads (nothing past the end is read).
__device__ __forceinline__ u32x4 tc_load(const uint8_t* p, uint64_t rem) {
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

// The drop mask of this lane's vector.  qm: its quote mask (a vector cut by the end of the value is
// never all quotes); *carry: the group's state before the step, replaced by the state after it
// (uniform in the group).  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t tc_lane_drop(uint32_t qm, uint32_t gl, uint32_t g, uint32_t* carry) {
  const bool all = qm == 0xFFFFu;
  const uint32_t mine = tc_carry_out16(qm, tc_drop16(qm, 0));     // exact unless `all`
  const uint32_t ga = ~(uint32_t)(__ballot(all) >> (g * kTcGroup)) & 0xFFFFu;   // lanes that are not all quotes
  const uint32_t gb = (uint32_t)(__ballot(mine != 0) >> (g * kTcGroup)) & 0xFFFFu;
  const uint32_t below = ga & ((1u << gl) - 1u);
  const uint32_t in = below ? (gb >> (31 - __builtin_clz(below))) & 1u : *carry;
  if (ga) *carry = (gb >> (31 - __builtin_clz(ga))) & 1u;
  return tc_drop16(qm, in);
}

__global__ __launch_bounds__(kTcThreads) void text_measure_coop_kernel(TextColumnArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kTcGroup - 1), g = lane / kTcGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kTcValuesPerBlock + threadIdx.x / kTcGroup;
  uint64_t off = 0, n = 0;
  const bool ok = r < a.n && tc_live(a, r, &off, &n);
  if (!ok) n = 0;                                   // such a value is not read
  const uint64_t walk = a.quote >= 0 ? n : 0;       // without a quote byte the length is the answer
  const uint8_t* p = a.data + off;
  const uint32_t qw = ((uint32_t)a.quote & 0xFFu) * 0x01010101u;
  uint32_t carry = 0, dropped = 0;
  for (uint64_t base = 0; __ballot(base < walk) != 0ull; base += kTcGroup * 16) {
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint32_t qm = 0;
    if (pos < walk) {
      const uint64_t rem = walk - pos;
      qm = tc_mask16(tc_load(p + pos, rem), qw) & (rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u));
    }
    if (__ballot(qm != 0) == 0ull) {                // wave-uniform: no quote in this step
      carry = 0;
      continue;
    }
    dropped += (uint32_t)__popc(tc_lane_drop(qm, gl, g, &carry));
  }
#pragma unroll
  for (int d = kTcGroup / 2; d; d >>= 1) dropped += __shfl_xor(dropped, d, kTcGroup);
  if (r < a.n && gl == 0) a.out_len[r] = (int32_t)((uint32_t)n - dropped);
}

// c <= 16 bytes, compact in (lo, hi), to q: at most one store of each size.
__device__ __forceinline__ void tc_store_pieces(uint8_t* q, uint64_t lo, uint64_t hi, uint32_t c) {
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

__global__ __launch_bounds__(kTcThreads) void text_emit_coop_kernel(TextColumnArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kTcGroup - 1), g = lane / kTcGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kTcValuesPerBlock + threadIdx.x / kTcGroup;
  uint64_t off = 0, n = 0, jlo = 0, jhi = 0;
  int64_t lo = 0;
  const bool ok = r < a.n && tc_live(a, r, &off, &n) && tc_window(a, r, &lo, &jlo, &jhi);
  if (!ok) n = 0;                                   // such a value is neither read nor written
  const uint8_t* p = a.data + off;
  // byte j of the value's output belongs at a.out[lo + j]; only j in [jlo, jhi) is ever stored
  const bool quoted = a.quote >= 0;
  const uint32_t qw = ((uint32_t)a.quote & 0xFFu) * 0x01010101u;
  uint32_t carry = 0;
  uint64_t done = 0;                                // output bytes before the step (uniform in the group)
  for (uint64_t base = 0; __ballot(base < n && done < jhi) != 0ull; base += kTcGroup * 16) {
    const uint64_t pos = base + (uint64_t)gl * 16;
    u32x4 v = {0, 0, 0, 0};
    uint32_t valid = 0, qm = 0;
    if (pos < n) {
      const uint64_t rem = n - pos;
      v = tc_load(p + pos, rem);
      valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      if (quoted) qm = tc_mask16(v, qw) & valid;
    }
    uint32_t keep = valid;
    uint64_t j0;                                    // the output index of this lane's first kept byte
    if (__ballot(qm != 0) == 0ull) {                // wave-uniform: no quote in this step, nothing moves
      carry = 0;
      j0 = done + (uint64_t)gl * 16;
      done += base >= n ? 0 : (n - base < kTcGroup * 16 ? n - base : kTcGroup * 16);
    } else {
      keep &= ~tc_lane_drop(qm, gl, g, &carry);
      const uint32_t c = (uint32_t)__popc(keep);
      uint32_t inc = c;
#pragma unroll
      for (int d = 1; d < kTcGroup; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, kTcGroup);
        if ((int)gl >= d) inc += o;
      }
      j0 = done + (inc - c);
      done += __shfl(inc, kTcGroup - 1, kTcGroup);
    }
    const uint32_t c = (uint32_t)__popc(keep);
    if (c == 0 || j0 >= jhi || j0 + c <= jlo) continue;
    uint64_t vlo = ((uint64_t)v.y << 32) | v.x, vhi = ((uint64_t)v.w << 32) | v.z;
    if (keep != valid) {                            // compact the kept bytes (valid is a run of low bits)
      uint64_t clo = 0, chi = 0;
      uint32_t k = 0;
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) {
        if (!((keep >> j) & 1u)) continue;
        const uint64_t b = ((j < 8 ? vlo : vhi) >> (8 * (j & 7))) & 0xFFu;
        if (k < 8) clo |= b << (8 * k);
        else chi |= b << (8 * (k - 8));
        ++k;
      }
      vlo = clo;
      vhi = chi;
    }
    if (j0 >= jlo && j0 + c <= jhi) {
      tc_store_pieces(a.out + (lo + (int64_t)j0), vlo, vhi, c);
    } else {                                        // the edge of the window: byte by byte, inside it
      for (uint32_t k = 0; k < c; ++k) {
        const uint64_t j = j0 + k;
        if (j >= jlo && j < jhi) a.out[lo + (int64_t)j] = (uint8_t)((k < 8 ? vlo : vhi) >> (8 * (k & 7)));
      }
    }
  }
}

// By analogy with field parse; tools/text_column_bench.py measures both, profiles/text_column.md.
int g_tc_variant = 1;

bool tc_args_ok(const TextColumnArgs& a) { return text_column_scalars_ok(a) && a.n <= (1ull << 31); }

}  // namespace

void set_text_column_variant(int variant) { g_tc_variant = variant ? 1 : 0; }

int text_column_variant() { return g_tc_variant; }

hipError_t launch_text_measure(const TextColumnArgs& a, hipStream_t stream) {
  if (!tc_args_ok(a)) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (!a.start || !a.length || !a.out_len || (!a.data && a.data_bytes)) return hipErrorInvalidValue;
  if (g_tc_variant == 1) {
    const unsigned grid = (unsigned)((a.n + kTcValuesPerBlock - 1) / kTcValuesPerBlock);
    hipLaunchKernelGGL(text_measure_coop_kernel, dim3(grid), dim3(kTcThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.n + kTcThreads - 1) / kTcThreads);
    hipLaunchKernelGGL(text_measure_lane_kernel, dim3(grid), dim3(kTcThreads), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_text_emit(const TextColumnArgs& a, hipStream_t stream) {
  if (!tc_args_ok(a)) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (!a.start || !a.length || !a.offsets || (!a.data && a.data_bytes) || (!a.out && a.out_bytes))
    return hipErrorInvalidValue;
  if (g_tc_variant == 1) {
    const unsigned grid = (unsigned)((a.n + kTcValuesPerBlock - 1) / kTcValuesPerBlock);
    hipLaunchKernelGGL(text_emit_coop_kernel, dim3(grid), dim3(kTcThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.n + kTcThreads - 1) / kTcThreads);
    hipLaunchKernelGGL(text_emit_lane_kernel, dim3(grid), dim3(kTcThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace amdx
