// Text columns from spans for gfx950 (wave64): the two passes of text_column_host.h, measure and
// emit, each in two variants.  The rule and the liveness and window checks are those of the header,
// compiled for the device.
//
// Variant 0, one lane per value: tc_measure_one / tc_emit_one as they stand, a serial byte walk.
//
// Variant 1, cooperative: a group of 16 lanes owns a value (four values per wave) and walks it in
// steps of 256 bytes, lane l of the group loading the 16 bytes at step * 256 + 16 * l.  A vector
// becomes a 16-bit quote mask (lg_mask16 of lane_group.h, as all lg_ names) and tc_drop16 marks
// the 2nd, 4th, ... quote of each run.  The one thing a vector needs from the bytes before it is whether the
// run that reaches it has odd length so far.  A vector that is not all quotes knows what it hands
// on without knowing what it got, and one of 16 quotes hands on what it got, so a lane's incoming
// state is that of the nearest lower lane whose vector is not all quotes, or the group's carried
// state: two ballots, no chain through the lanes (lg_carry).  Measure adds up the popcounts of the keep-masks.
// Emit places each lane's kept bytes (lg_place) by a 16-lane prefix sum of them plus a running
// count; a full vector without a dropped byte goes out as one 16-byte store at whatever phase the destination
// has, anything else is compacted in registers and goes out as at most one 8-, 4-, 2- and 1-byte
// store (stores here are bound by their number, not their bytes).  A lane whose bytes touch the
// edge of the value's window stores the bytes inside it one by one.
//
// No path loads a byte outside the value it was given: a vector that reaches past the end is
// assembled from byte loads.  Values are independent, so there are no atomics and no waits between
// workgroups, and two runs write the same bytes.
#include "kernels.h"
#include "lane_group.h"

namespace amdx {

namespace {

__global__ __launch_bounds__(kLgThreads) void text_measure_lane_kernel(TextColumnArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.n) tc_measure_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void text_emit_lane_kernel(TextColumnArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.n) tc_emit_one(a, r);
}

// The drop mask of this lane's vector.  qm: its quote mask (a vector cut by the end of the value is
// never all quotes); *carry: the group's state before the step, replaced by the state after it
// (uniform in the group).  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t tc_lane_drop(uint32_t qm, uint32_t gl, uint32_t g, uint32_t* carry) {
  const uint32_t mine = tc_carry_out16(qm, tc_drop16(qm, 0));     // exact unless all quotes
  return tc_drop16(qm, lg_carry(qm == 0xFFFFu, mine != 0, gl, g, carry));
}

__global__ __launch_bounds__(kLgThreads) void text_measure_coop_kernel(TextColumnArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
  uint64_t off = 0, n = 0;
  const bool ok = r < a.n && tc_live(a, r, &off, &n);
  if (!ok) n = 0;                                   // such a value is not read
  const uint64_t walk = a.quote >= 0 ? n : 0;       // without a quote byte the length is the answer
  const uint8_t* p = a.data + off;
  const uint32_t qw = ((uint32_t)a.quote & 0xFFu) * 0x01010101u;
  uint32_t carry = 0, dropped = 0;
  for (uint64_t base = 0; __ballot(base < walk) != 0ull; base += kLgStep) {
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint32_t qm = 0;
    if (pos < walk) {
      const uint64_t rem = walk - pos;
      qm = lg_mask16(lg_load16(p + pos, rem), qw) & (rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u));
    }
    if (__ballot(qm != 0) == 0ull) {                // wave-uniform: no quote in this step
      carry = 0;
      continue;
    }
    dropped += (uint32_t)__popc(tc_lane_drop(qm, gl, g, &carry));
  }
#pragma unroll
  for (int d = kLgGroup / 2; d; d >>= 1) dropped += __shfl_xor(dropped, d, kLgGroup);
  if (r < a.n && gl == 0) a.out_len[r] = (int32_t)((uint32_t)n - dropped);
}

__global__ __launch_bounds__(kLgThreads) void text_emit_coop_kernel(TextColumnArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
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
  for (uint64_t base = 0; __ballot(base < n && done < jhi) != 0ull; base += kLgStep) {
    const uint64_t pos = base + (uint64_t)gl * 16;
    u32x4 v = {0, 0, 0, 0};
    uint32_t valid = 0, qm = 0;
    if (pos < n) {
      const uint64_t rem = n - pos;
      v = lg_load16(p + pos, rem);
      valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      if (quoted) qm = lg_mask16(v, qw) & valid;
    }
    uint32_t keep = valid;
    uint64_t j0;                                    // the output index of this lane's first kept byte
    if (__ballot(qm != 0) == 0ull) {                // wave-uniform: no quote in this step, nothing moves
      carry = 0;
      j0 = done + (uint64_t)gl * 16;
      done += base >= n ? 0 : (n - base < kLgStep ? n - base : kLgStep);
    } else {
      keep &= ~tc_lane_drop(qm, gl, g, &carry);
      const uint32_t c = (uint32_t)__popc(keep);
      uint32_t total;
      j0 = done + (lg_scan16(c, gl, &total) - c);
      done += total;
    }
    // valid is a run of low bits: kept bytes that are all of them need no compaction
    lg_place(a.out, lo, jlo, jhi, j0, lg_lo64(v), lg_hi64(v), keep, (uint32_t)__popc(keep), keep != valid);
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
    const unsigned grid = (unsigned)((a.n + kLgPerBlock - 1) / kLgPerBlock);
    hipLaunchKernelGGL(text_measure_coop_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.n + kLgThreads - 1) / kLgThreads);
    hipLaunchKernelGGL(text_measure_lane_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_text_emit(const TextColumnArgs& a, hipStream_t stream) {
  if (!tc_args_ok(a)) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (!a.start || !a.length || !a.offsets || (!a.data && a.data_bytes) || (!a.out && a.out_bytes))
    return hipErrorInvalidValue;
  if (g_tc_variant == 1) {
    const unsigned grid = (unsigned)((a.n + kLgPerBlock - 1) / kLgPerBlock);
    hipLaunchKernelGGL(text_emit_coop_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  } else {
    const unsigned grid = (unsigned)((a.n + kLgThreads - 1) / kLgThreads);
    hipLaunchKernelGGL(text_emit_lane_kernel, dim3(grid), dim3(kLgThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace amdx
