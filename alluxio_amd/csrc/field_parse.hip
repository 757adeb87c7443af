// Typed columns from delimited text rows for gfx950 (wave64).  The rule and the parsers of a
// located field are those of field_parse_host.h, compiled for the device; this file adds the two
// ways of locating the requested fields of a row.  See FieldParseArgs.
//
// Variant 0, one lane per row: fp_row as it stands, a serial byte walk with the quote parity in a
// register.  Lanes of a wave read 64 different rows, one byte at a time.
//
// Variant 1, cooperative: a group of 16 lanes owns a row (four rows per wave) and walks it in
// steps of 256 bytes, lane l of the group loading the 16 bytes at step * 256 + 16 * l of the row.
// A vector becomes a 16-bit separator mask and a 16-bit quote mask (the SWAR compare of
// delim_index.hip).  The state "inside quotes" before a lane's vector is the group's running
// parity plus the parity of the quote bytes of the lanes below (one ballot); inside the vector it
// is a prefix xor of the quote mask.  A 16-lane prefix sum of the popcounts of the splitting
// separators numbers them, so the lane that holds split k - 1 knows where field k starts and the
// lane that holds split k where it ends; both positions travel by one shuffle each to the lane
// that owns the column (column c: lane c % 16 of the group).  Parity and split count are carried
// from step to step.  After the walk the owner lanes parse their fields.
//
// No path loads a byte outside the row it was given: a vector that reaches past the end of the row
// is assembled from byte loads.  Rows are independent, so there are no atomics and no waits
// between workgroups, and two runs write the same bytes.
#include "kernels.h"

namespace amdx {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kFpThreads = 256;
constexpr int kFpGroup = 16;                        // lanes per row in variant 1
constexpr int kFpRowsPerBlock = kFpThreads / kFpGroup;
constexpr uint64_t kFpNoPos = ~0ull;

__global__ __launch_bounds__(kFpThreads) void field_parse_lane_kernel(FieldParseArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kFpThreads + threadIdx.x;
  if (r < a.nrows) fp_row(a, r);
}

// 0x80 in every byte of w that equals the byte replicated in dw (exact: no carry between bytes).
__device__ __forceinline__ uint32_t fp_match(uint32_t w, uint32_t dw) {
  const uint32_t x = w ^ dw;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t fp_pack(uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; }
__device__ __forceinline__ uint32_t fp_mask16(u32x4 v, uint32_t dw) {
  return fp_pack(fp_match(v.x, dw)) | (fp_pack(fp_match(v.y, dw)) << 4) | (fp_pack(fp_match(v.z, dw)) << 8) |
         (fp_pack(fp_match(v.w, dw)) << 12);
}
// Bit j: an odd number of the bits below j is set in qm.
__device__ __forceinline__ uint32_t fp_inside16(uint32_t qm) {
  uint32_t m = qm;
  m ^= m << 1;
  m ^= m << 2;
  m ^= m << 4;
  m ^= m << 8;
  return (m << 1) & 0xFFFFu;
}
// Position of set bit number i (from 0) of m, which has more than i bits set.
__device__ __forceinline__ uint32_t fp_nth_bit(uint32_t m, uint32_t i) {
  for (; i; --i) m &= m - 1;
  return (uint32_t)__builtin_ctz(m);
}
__device__ __forceinline__ uint64_t fp_shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kFpThreads) void field_parse_coop_kernel(FieldParseArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kFpGroup - 1), g = lane / kFpGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kFpRowsPerBlock + threadIdx.x / kFpGroup;
  const bool live = r < a.nrows;
  uint64_t off = 0, n = 0;
  const bool ok = live && fp_row_bytes(a, r, &off, &n);
  if (!ok) n = 0;                                   // such a row is not read
  const uint8_t* row = a.data + off;
  const uint32_t sw = (a.sep & 0xFFu) * 0x01010101u;
  const uint32_t qw = ((uint32_t)a.quote & 0xFFu) * 0x01010101u;
  const bool quoted = a.quote >= 0;

  // the two columns this lane owns: gl and gl + 16; positions are relative to the row
  uint64_t fs0 = kFpNoPos, fe0 = kFpNoPos, fs1 = kFpNoPos, fe1 = kFpNoPos;
  if (gl < a.ncols && a.cols[gl].field == 0) fs0 = 0;
  if (gl + kFpGroup < a.ncols && a.cols[gl + kFpGroup].field == 0) fs1 = 0;

  uint32_t par = 0;                                 // state before the step (uniform in the group)
  uint64_t cnt = 0;                                 // splits before the step (uniform in the group)
  // a row is done at its end, or once split number max_field has been seen
  for (uint64_t base = 0; __ballot(base < n && cnt <= a.max_field) != 0ull; base += kFpGroup * 16) {
    const bool walking = base < n && cnt <= a.max_field;
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint32_t sm = 0, qm = 0;
    if (walking && pos < n) {
      const uint64_t rem = n - pos;
      u32x4 v;
      if (rem >= 16) {
        __builtin_memcpy(&v, row + pos, 16);        // any byte phase
      } else {                                      // the row's last vector: byte loads, nothing past the end
        uint64_t lo = 0, hi = 0;
        for (uint32_t j = 0; j < (uint32_t)rem; ++j) {
          const uint64_t b = row[pos + j];
          if (j < 8) lo |= b << (8 * j);
          else hi |= b << (8 * (j - 8));
        }
        v.x = (uint32_t)lo;
        v.y = (uint32_t)(lo >> 32);
        v.z = (uint32_t)hi;
        v.w = (uint32_t)(hi >> 32);
      }
      const uint32_t valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      sm = fp_mask16(v, sw) & valid;
      if (quoted) qm = fp_mask16(v, qw) & valid;
    }
    const uint32_t gq = (uint32_t)(__ballot(__popc(qm) & 1) >> (g * kFpGroup)) & 0xFFFFu;
    const uint32_t before = (par ^ (uint32_t)__popc(gq & ((1u << gl) - 1u))) & 1u;
    par = (par ^ (uint32_t)__popc(gq)) & 1u;
    const uint32_t split = sm & ~(fp_inside16(qm) ^ (before ? 0xFFFFu : 0u));
    const uint32_t c = (uint32_t)__popc(split);
    if (__ballot(c != 0) == 0ull) continue;         // wave-uniform: no split in this step
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < kFpGroup; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d, kFpGroup);
      if ((int)gl >= d) inc += o;
    }
    const uint64_t first = cnt + (inc - c);         // number of this vector's first split
    cnt += __shfl(inc, kFpGroup - 1, kFpGroup);
    for (uint32_t col = 0; col < a.ncols; ++col) {
      const uint64_t k = a.cols[col].field;
      const bool he = c != 0 && k >= first && k < first + c;               // split k ends field k
      const bool hs = c != 0 && k >= 1 && k - 1 >= first && k - 1 < first + c;   // split k - 1 precedes it
      const uint64_t be = __ballot(he), bs = __ballot(hs);
      if ((be | bs) == 0ull) continue;              // wave-uniform
      const uint64_t ve = he ? pos + fp_nth_bit(split, (uint32_t)(k - first)) : kFpNoPos;
      const uint64_t vs = hs ? pos + fp_nth_bit(split, (uint32_t)(k - 1 - first)) + 1 : kFpNoPos;
      const uint32_t ge = (uint32_t)(be >> (g * kFpGroup)) & 0xFFFFu;
      const uint32_t gs = (uint32_t)(bs >> (g * kFpGroup)) & 0xFFFFu;
      const uint64_t xe = fp_shfl64(ve, ge ? (int)(g * kFpGroup + __builtin_ctz(ge)) : (int)lane);
      const uint64_t xs = fp_shfl64(vs, gs ? (int)(g * kFpGroup + __builtin_ctz(gs)) : (int)lane);
      if (gl == (col & (kFpGroup - 1))) {
        if (col < kFpGroup) {
          if (ge) fe0 = xe;
          if (gs) fs0 = xs;
        } else {
          if (ge) fe1 = xe;
          if (gs) fs1 = xs;
        }
      }
    }
  }

  if (!live) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t col = gl + j * kFpGroup;
    if (col >= a.ncols) break;
    const uint64_t fs = j ? fs1 : fs0, fe = j ? fe1 : fe0;
    if (!ok) fp_emit_none(a.cols[col], r, kFpBad);
    else if (fs == kFpNoPos) fp_emit_none(a.cols[col], r, kFpNone);
    else fp_emit(a.cols[col], r, row, off, fs, fe == kFpNoPos ? n : fe, a.quote);
  }
}

// tools/field_parse_bench.py on MI355X, profiles/field_parse.md.
int g_fp_variant = 1;

}  // namespace

void set_field_parse_variant(int variant) { g_fp_variant = variant ? 1 : 0; }

int field_parse_variant() { return g_fp_variant; }

hipError_t launch_field_parse(const FieldParseArgs& a, hipStream_t stream) {
  if (!field_parse_scalars_ok(a) || a.nrows > (1ull << 31)) return hipErrorInvalidValue;
  if (a.nrows == 0) return hipSuccess;
  if (g_fp_variant == 1) {
    const unsigned grid = (unsigned)((a.nrows + kFpRowsPerBlock - 1) / kFpRowsPerBlock);
    hipLaunchKernelGGL(field_parse_coop_kernel, dim3(grid), dim3(kFpThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.nrows + kFpThreads - 1) / kFpThreads);
    hipLaunchKernelGGL(field_parse_lane_kernel, dim3(grid), dim3(kFpThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace amdx
