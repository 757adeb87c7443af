// Typed columns from delimited text rows for gfx950 (wave64).  The rule and the parsers of a
// located field are those of field_parse_host.h, compiled for the device; this file adds the two
// ways of locating the requested fields of a row.  See FieldParseArgs.
//
// Variant 0, one lane per row: fp_row as it stands, a serial byte walk with the quote parity in a
// register.  Lanes of a wave read 64 different rows, one byte at a time.
//
// Variant 1, cooperative: a group of 16 lanes owns a row (four rows per wave) and walks it in
// steps of 256 bytes, lane l of the group loading the 16 bytes at step * 256 + 16 * l of the row.
// A vector becomes a 16-bit separator mask and a 16-bit quote mask (lg_mask16; the group's
// building blocks, here and below, are those of lane_group.h).  The state "inside quotes" before a
// lane's vector is the group's running parity plus the parity of the quote bytes of the lanes
// below (one ballot); inside the vector it is a prefix xor of the quote mask (lg_inside16).  A
// 16-lane prefix sum (lg_scan16) of the popcounts of the splitting separators numbers them, so the lane that holds split k - 1 knows where field k starts and the
// lane that holds split k where it ends; both positions travel by one shuffle each to the lane
// that owns the column (column c: lane c % 16 of the group).  Parity and split count are carried
// from step to step.  After the walk the owner lanes parse their fields.
//
// No path loads a byte outside the row it was given: a vector that reaches past the end of the row
// is assembled from byte loads.  Rows are independent, so there are no atomics and no waits
// between workgroups, and two runs write the same bytes.
#include "kernels.h"
#include "lane_group.h"

namespace amdx {

namespace {

constexpr uint64_t kFpNoPos = ~0ull;

__global__ __launch_bounds__(kLgThreads) void field_parse_lane_kernel(FieldParseArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.nrows) fp_row(a, r);
}

// Position of set bit number i (from 0) of m, which has more than i bits set.
__device__ __forceinline__ uint32_t fp_nth_bit(uint32_t m, uint32_t i) {
  for (; i; --i) m &= m - 1;
  return (uint32_t)__builtin_ctz(m);
}

__global__ __launch_bounds__(kLgThreads) void field_parse_coop_kernel(FieldParseArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
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
  if (gl + kLgGroup < a.ncols && a.cols[gl + kLgGroup].field == 0) fs1 = 0;

  uint32_t par = 0;                                 // state before the step (uniform in the group)
  uint64_t cnt = 0;                                 // splits before the step (uniform in the group)
  // a row is done at its end, or once split number max_field has been seen
  for (uint64_t base = 0; __ballot(base < n && cnt <= a.max_field) != 0ull; base += kLgStep) {
    const bool walking = base < n && cnt <= a.max_field;
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint32_t sm = 0, qm = 0;
    if (walking && pos < n) {
      const uint64_t rem = n - pos;
      const u32x4 v = lg_load16(row + pos, rem);
      const uint32_t valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      sm = lg_mask16(v, sw) & valid;
      if (quoted) qm = lg_mask16(v, qw) & valid;
    }
    const uint32_t gq = lg_group16(__ballot(__popc(qm) & 1), g);
    const uint32_t before = (par ^ (uint32_t)__popc(gq & ((1u << gl) - 1u))) & 1u;
    par = (par ^ (uint32_t)__popc(gq)) & 1u;
    const uint32_t split = sm & ~(lg_inside16(qm) ^ (before ? 0xFFFFu : 0u));
    const uint32_t c = (uint32_t)__popc(split);
    if (__ballot(c != 0) == 0ull) continue;         // wave-uniform: no split in this step
    uint32_t total;
    const uint64_t first = cnt + (lg_scan16(c, gl, &total) - c);   // number of this vector's first split
    cnt += total;
    for (uint32_t col = 0; col < a.ncols; ++col) {
      const uint64_t k = a.cols[col].field;
      const bool he = c != 0 && k >= first && k < first + c;               // split k ends field k
      const bool hs = c != 0 && k >= 1 && k - 1 >= first && k - 1 < first + c;   // split k - 1 precedes it
      const uint64_t be = __ballot(he), bs = __ballot(hs);
      if ((be | bs) == 0ull) continue;              // wave-uniform
      const uint64_t ve = he ? pos + fp_nth_bit(split, (uint32_t)(k - first)) : kFpNoPos;
      const uint64_t vs = hs ? pos + fp_nth_bit(split, (uint32_t)(k - 1 - first)) + 1 : kFpNoPos;
      const uint32_t ge = lg_group16(be, g), gs = lg_group16(bs, g);
      const uint64_t xe = lg_shfl64_wave(ve, ge ? (int)(g * kLgGroup + __builtin_ctz(ge)) : (int)lane);
      const uint64_t xs = lg_shfl64_wave(vs, gs ? (int)(g * kLgGroup + __builtin_ctz(gs)) : (int)lane);
      if (gl == (col & (kLgGroup - 1))) {
        if (col < kLgGroup) {
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
    const uint32_t col = gl + j * kLgGroup;
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
    const unsigned grid = (unsigned)((a.nrows + kLgPerBlock - 1) / kLgPerBlock);
    hipLaunchKernelGGL(field_parse_coop_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.nrows + kLgThreads - 1) / kLgThreads);
    hipLaunchKernelGGL(field_parse_lane_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace amdx
