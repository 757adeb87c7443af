// Parquet page encode for gfx950 (wave64): the passes of parquet_encode_host.h.  The rules and the
// bounds checks are those of the header, compiled for the device.
//
// A launch covers the pages [first, last) of the table with `tiles` workgroups per page (the caller
// sizes it for the largest page of the range); a workgroup whose tile lies past its page's end
// leaves at once.  Rows are numbered from the page's first row, so a wave's 64 rows start at a
// multiple of 64 of the page whatever the page's place in the column, and the ballot of "is a
// value" over them is 8 whole bytes of the page's level bits: lanes 0 to 7 store one byte each,
// only those that the page has (a page that ends inside the wave has zero bits after its last
// row, and no byte after its last byte is touched).
//
// measure reduces its five counts over the wave with shuffles and adds them to the page's row with
// one atomic each per wave: integer sums and a maximum, so two runs give the same table.  The emit
// passes use no atomics: a value's slot is its rank, a packed byte is built by the one lane that
// owns it from the values that overlap it, and no two lanes write the same byte.
//
// Fixed-width values and text go out with 4-, 8- and 16-byte stores at whatever byte phase the
// headers before them left (as text_column.hip stores); text is copied by 16 lanes per value.
// No LDS, no inline assembly.
#include "kernels.h"

namespace amdx {

namespace {

constexpr int kPeThreads = 256;
constexpr int kPeRowsPerThread = 4;
constexpr int kPeTileRows = kPeThreads * kPeRowsPerThread;      // measure, rows, pack (bytes)
constexpr int kPeTextLanes = 16;
constexpr int kPeTextSteps = 16;
constexpr int kPeTextTileRows = kPeThreads / kPeTextLanes * kPeTextSteps;
constexpr int kPeCopySegs = kPeThreads / 64;                    // a wave per segment

__device__ __forceinline__ int64_t pe_wave_sum(int64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kPeThreads) void pe_measure_kernel(PeArgs a) {
  const uint64_t p = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (p >= a.last) return;
  const int64_t* pg = a.pages + p * kPeCols;
  const uint64_t rows = (uint64_t)pg[kPeRows], base = tile * kPeTileRows;
  if (base >= rows) return;                           // uniform in the workgroup
  PeCount c{0, 0, 0, -1, 0};
#pragma unroll
  for (int k = 0; k < kPeRowsPerThread; ++k) {
    const uint64_t i = base + (uint64_t)k * kPeThreads + threadIdx.x;
    if (i < rows) pe_measure_row(a, pg, i, c);
  }
  const int64_t valid = pe_wave_sum(c.valid), bad = pe_wave_sum(c.bad), tb = pe_wave_sum(c.text_bytes),
                outside = pe_wave_sum(c.outside);
  int64_t mx = c.max_code;
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const int64_t o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    int64_t* m = a.measure + p * kPmCols;
    if (valid) atomicAdd((unsigned long long*)(m + kPmValid), (unsigned long long)valid);
    if (bad) atomicAdd((unsigned long long*)(m + kPmBad), (unsigned long long)bad);
    if (tb) atomicAdd((unsigned long long*)(m + kPmTextBytes), (unsigned long long)tb);
    if (outside) atomicAdd((unsigned long long*)(m + kPmOutside), (unsigned long long)outside);
    if (mx >= 0) atomicMax((long long*)(m + kPmMaxCode), (long long)mx);
  }
}

__global__ __launch_bounds__(kPeThreads) void pe_rows_kernel(PeArgs a) {
  const uint64_t p = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (p >= a.last) return;
  const int64_t* pg = a.pages + p * kPeCols;
  const uint64_t rows = (uint64_t)pg[kPeRows], base = tile * kPeTileRows;
  if (base >= rows) return;
  const int64_t level_off = pg[kPeLevelOff];
  const bool text = pg[kPeKind] == kPeText;
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kPeRowsPerThread; ++k) {
    const uint64_t i = base + (uint64_t)k * kPeThreads + threadIdx.x;
    const bool value = i < rows && pe_is_value(a, pg, i);
    const uint64_t bits = __ballot(value);            // rows [i - lane, i - lane + 64) of the page
    if (level_off >= 0 && lane < 8) {
      const uint64_t first = i - lane + 8 * (uint64_t)lane, b = first / 8;
      if (first < rows && (uint64_t)level_off < a.out_bytes && b < a.out_bytes - (uint64_t)level_off)
        a.out[(uint64_t)level_off + b] = (uint8_t)(bits >> (8 * lane));
    }
    if (value && !text) pe_emit_value(a, pg, i);
  }
}

__global__ __launch_bounds__(kPeThreads) void pe_text_kernel(PeArgs a) {
  const uint64_t p = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (p >= a.last) return;
  const int64_t* pg = a.pages + p * kPeCols;
  if (pg[kPeKind] != kPeText) return;
  const uint64_t rows = (uint64_t)pg[kPeRows], base = tile * kPeTextTileRows;
  if (base >= rows) return;
  const uint32_t gl = threadIdx.x % kPeTextLanes, g = threadIdx.x / kPeTextLanes;
  for (int k = 0; k < kPeTextSteps; ++k) {
    const uint64_t i = base + (uint64_t)k * (kPeThreads / kPeTextLanes) + g;
    if (i < rows) pe_emit_text(a, pg, i, gl, kPeTextLanes);
  }
}

__global__ __launch_bounds__(kPeThreads) void pe_pack_kernel(PeArgs a) {
  const uint64_t p = a.first + blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  if (p >= a.last) return;
  const int64_t* pg = a.pages + p * kPeCols;
  if (pg[kPeKind] != kPeBool && pg[kPeKind] != kPeIndex) return;
  const uint64_t bytes = (uint64_t)pg[kPeValBytes], base = tile * kPeTileRows;
#pragma unroll
  for (int k = 0; k < kPeRowsPerThread; ++k) {
    const uint64_t b = base + (uint64_t)k * kPeThreads + threadIdx.x;
    if (b < bytes) pe_pack_byte(a, pg, b);
  }
}

__global__ __launch_bounds__(kPeThreads) void pe_copy_kernel(PeArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kPeCopySegs + threadIdx.x / 64;
  if (s < a.nsegs) pe_copy_seg(a, s, threadIdx.x & 63, 64);
}

constexpr uint64_t kPeMax = 1ull << 31;

// The workgroups of a launch, or 0 when the arguments do not describe one.
uint64_t pe_grid(PeArgs& a, uint64_t largest, int tile) {
  if (a.first > a.last || a.last > a.npages || !a.pages) return 0;
  a.tiles = largest ? (largest + tile - 1) / tile : 1;
  const uint64_t pages = a.last - a.first;
  if (pages == 0 || a.tiles > kPeMax || pages > kPeMax / a.tiles) return 0;
  return pages * a.tiles;
}

}  // namespace

hipError_t launch_parquet_encode(const PeArgs& args, int pass, uint64_t largest, hipStream_t stream) {
  PeArgs a = args;
  if (pass == kPePassCopy) {
    if (a.nsegs == 0) return hipSuccess;
    if (a.nsegs > kPeMax || !a.segs || !a.blob || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe_copy_kernel, dim3((unsigned)((a.nsegs + kPeCopySegs - 1) / kPeCopySegs)), dim3(kPeThreads), 0,
                       stream, a);
    return hipGetLastError();
  }
  if (a.first == a.last) return hipSuccess;
  const uint64_t grid = pe_grid(a, largest, pass == kPePassText ? kPeTextTileRows : kPeTileRows);
  if (grid == 0 || !a.flags) return hipErrorInvalidValue;
  if (pass == kPePassMeasure) {
    if (!a.measure) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe_measure_kernel, dim3((unsigned)grid), dim3(kPeThreads), 0, stream, a);
  } else if (pass == kPePassRows) {
    if (!a.out || !a.rank) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe_rows_kernel, dim3((unsigned)grid), dim3(kPeThreads), 0, stream, a);
  } else if (pass == kPePassText) {
    if (!a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe_text_kernel, dim3((unsigned)grid), dim3(kPeThreads), 0, stream, a);
  } else if (pass == kPePassPack) {
    if (!a.out || !a.scratch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pe_pack_kernel, dim3((unsigned)grid), dim3(kPeThreads), 0, stream, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace amdx
