// Parquet column statistics for gfx950 (wave64): the passes of parquet_stats_host.h.  The rules are
// those of the header, compiled for the device.
//
// A launch covers the segments [first, last) of the table with `tiles` workgroups per segment (the
// caller sizes it for the largest segment of the range), as the launches of parquet_encode.hip cover
// pages; a workgroup whose tile lies past its segment's end leaves at once.  So the launches of a
// row group do not depend on how many columns it has: one mark launch over the dictionary-index
// segments, one first launch over all segments, and kPsRounds - 1 round launches over the text
// segments (the columns' and the dictionaries').
//
// One row per lane, text included: a round needs 7 bytes of a value, which one lane loads with byte
// loads at any phase; a 16-lane group per value would leave 15 lanes without work.  Each result is
// reduced over the wave with shuffles and goes to the segment's result row with one 64-bit atomic
// per wave: integer sums, minima and maxima, so two runs give the same rows.  A text row's alive
// bits are read and written by the one lane that owns the row in every round, and the winners a
// round compares against were written by the launch before it.  mark stores single bytes; lanes
// that store to the same byte store the same value.  No LDS, no inline assembly.
#include "kernels.h"

namespace amdx {

namespace {

constexpr int kPsThreads = 256;
constexpr int kPsRowsPerThread = 4;
constexpr int kPsTileRows = kPsThreads * kPsRowsPerThread;

__device__ __forceinline__ int64_t ps_wave_sum(int64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ int64_t ps_wave_min(int64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const int64_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int64_t ps_wave_max(int64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const int64_t o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t ps_wave_umin(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t ps_wave_umax(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

// The round's winners of the wave into the result row.
__device__ __forceinline__ void ps_round_out(int64_t* res, uint32_t round, const PsAcc& c) {
  const uint64_t kmin = ps_wave_umin(c.kmin), kmax = ps_wave_umax(c.kmax);
  if ((threadIdx.x & 63) == 0) {
    if (kmin != ~0ull) atomicMin((unsigned long long*)(res + kPsRoundMin + round), (unsigned long long)kmin);
    if (kmax != 0) atomicMax((unsigned long long*)(res + kPsRoundMax + round), (unsigned long long)kmax);
  }
}

__global__ __launch_bounds__(kPsThreads) void ps_mark_kernel(PsArgs a) {
  const uint64_t s = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (s >= a.last) return;
  const int64_t* sg = a.segs + s * kPeCols;
  const uint64_t rows = (uint64_t)sg[kPeRows], base = tile * kPsTileRows;
#pragma unroll
  for (int k = 0; k < kPsRowsPerThread; ++k) {
    const uint64_t i = base + (uint64_t)k * kPsThreads + threadIdx.x;
    if (i < rows) ps_mark_row(sg, i);
  }
}

__global__ __launch_bounds__(kPsThreads) void ps_first_kernel(PsArgs a) {
  const uint64_t s = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (s >= a.last) return;
  const int64_t* sg = a.segs + s * kPeCols;
  const uint64_t rows = (uint64_t)sg[kPeRows], base = tile * kPsTileRows;
  if (base >= rows) return;                           // uniform in the workgroup
  PsAcc c = ps_acc();
#pragma unroll
  for (int k = 0; k < kPsRowsPerThread; ++k) {
    const uint64_t i = base + (uint64_t)k * kPsThreads + threadIdx.x;
    if (i < rows) ps_first_row(a, sg, i, c);
  }
  int64_t* res = a.results + s * kPsCols;
  const int64_t nulls = ps_wave_sum(c.nulls), values = ps_wave_sum(c.values);
  if (sg[kPeKind] == kPeText) {                       // uniform in the workgroup
    const int64_t maxlen = ps_wave_max(c.maxlen);
    if ((threadIdx.x & 63) == 0 && maxlen > 0) atomicMax((long long*)(res + kPsMaxLen), (long long)maxlen);
    ps_round_out(res, 0, c);
  } else {
    const int64_t mn = ps_wave_min(c.mn), mx = ps_wave_max(c.mx);
    if ((threadIdx.x & 63) == 0 && mn <= mx) {
      atomicMin((long long*)(res + kPsMin), (long long)mn);
      atomicMax((long long*)(res + kPsMax), (long long)mx);
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (nulls) atomicAdd((unsigned long long*)(res + kPsNulls), (unsigned long long)nulls);
    if (values) atomicAdd((unsigned long long*)(res + kPsValues), (unsigned long long)values);
  }
}

__global__ __launch_bounds__(kPsThreads) void ps_round_kernel(PsArgs a) {
  const uint64_t s = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (s >= a.last) return;
  const int64_t* sg = a.segs + s * kPeCols;
  if (sg[kPeKind] != kPeText) return;
  const uint64_t rows = (uint64_t)sg[kPeRows], base = tile * kPsTileRows;
  if (base >= rows) return;
  int64_t* res = a.results + s * kPsCols;
  PsAcc c = ps_acc();
#pragma unroll
  for (int k = 0; k < kPsRowsPerThread; ++k) {
    const uint64_t i = base + (uint64_t)k * kPsThreads + threadIdx.x;
    if (i < rows) ps_round_row(a, sg, res, i, c);
  }
  ps_round_out(res, a.round, c);
}

constexpr uint64_t kPsLimit = 1ull << 31;

}  // namespace

hipError_t launch_parquet_stats(const PsArgs& args, int pass, uint64_t largest, hipStream_t stream) {
  PsArgs a = args;
  if (a.first == a.last) return hipSuccess;
  if (a.first > a.last || a.last > a.nsegs || !a.segs || !a.results) return hipErrorInvalidValue;
  a.tiles = largest ? (largest + kPsTileRows - 1) / kPsTileRows : 1;
  const uint64_t segs = a.last - a.first;
  if (a.tiles > kPsLimit || segs > kPsLimit / a.tiles) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(segs * a.tiles)), block(kPsThreads);
  if (pass == kPsPassMark) {
    hipLaunchKernelGGL(ps_mark_kernel, grid, block, 0, stream, a);
  } else if (pass == kPsPassFirst) {
    hipLaunchKernelGGL(ps_first_kernel, grid, block, 0, stream, a);
  } else if (pass == kPsPassRound) {
    if (!a.alive || a.round < 1 || a.round >= kPsRounds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ps_round_kernel, grid, block, 0, stream, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace amdx
