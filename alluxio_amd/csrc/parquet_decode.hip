// Parquet page decode for gfx950 (wave64): the passes of parquet_host.h.  The rules, the window
// checks and the output bounds are those of the header, compiled for the device.
//
// walk, lz4 plan and bytes are serial chains (a header gives the place of the next one, a length
// prefix the place of the next value), so one lane takes a chunk or a page; their inputs are a few
// kilobytes per lane and the lanes of a launch are independent.
//
// Hybrid streams come in two variants.  Variant 0: one lane per stream decodes it serially
// (pq_stream_serial).  Variant 1, cooperative: one lane per stream only reads the run headers and
// writes a run table (counted in one launch, filled in a second, the caller's scan and one small
// readback between them); then one thread per output value finds its stream and its run by binary
// search and, for a bit-packed run, extracts its bits with one unaligned 8-byte load.  The serial
// part of variant 1 touches one header per run instead of every value, and the per-value part is as
// wide as the output.
//
// place is one thread per row: a binary search for the row's page, then a copy of `width` bytes
// from whatever byte phase the source has (byte loads: a PLAIN page starts wherever its header
// ended).
//
// No atomics, no waits between workgroups, no LDS: two runs write the same bytes.
#include "kernels.h"

namespace amdx {

namespace {

constexpr int kPqThreads = 256;
constexpr int kPqSerialThreads = 64;                  // serial passes: one wave per workgroup spreads the lanes over CUs

static_assert(sizeof(PqLz4Chunk) == sizeof(Lz4Chunk), "PqLz4Chunk is Lz4Chunk");

__global__ __launch_bounds__(kPqSerialThreads) void pq_walk_kernel(PqWalkArgs a) {
  const uint64_t c = (uint64_t)blockIdx.x * kPqSerialThreads + threadIdx.x;
  if (c < a.nchunks) pq_walk_chunk(a, c);
}

__global__ __launch_bounds__(kPqSerialThreads) void pq_lz4_plan_kernel(PqLz4Args a) {
  const uint64_t p = (uint64_t)blockIdx.x * kPqSerialThreads + threadIdx.x;
  if (p < a.npages) pq_lz4_page(a, p);
}

__global__ __launch_bounds__(kPqSerialThreads) void pq_hybrid_serial_kernel(PqStreamArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kPqSerialThreads + threadIdx.x;
  if (s < a.nstreams) pq_stream_serial(a, s);
}

__global__ __launch_bounds__(kPqSerialThreads) void pq_hybrid_runs_kernel(PqStreamArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kPqSerialThreads + threadIdx.x;
  if (s < a.nstreams) pq_stream_runs(a, s);
}

__global__ __launch_bounds__(kPqThreads) void pq_hybrid_values_kernel(PqStreamArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x;
  if (t < a.out_n) pq_stream_value(a, t);
}

__global__ __launch_bounds__(kPqThreads) void pq_place_kernel(PqPlaceArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kPqThreads + threadIdx.x;
  if (r < a.rows) pq_place_row(a, r);
}

__global__ __launch_bounds__(kPqSerialThreads) void pq_bytes_kernel(PqBytesArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * kPqSerialThreads + threadIdx.x;
  if (p < a.npages) pq_bytes_page(a, p);
}

// Variant 1 decodes the streams of a 65,536-row row group 3 to 6 times faster (profiles/parquet_columns.md).
int g_pq_variant = 1;

unsigned pq_grid(uint64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

constexpr uint64_t kPqMax = 1ull << 31;

}  // namespace

void set_parquet_decode_variant(int variant) { g_pq_variant = variant ? 1 : 0; }

int parquet_decode_variant() { return g_pq_variant; }

hipError_t launch_parquet_walk(const PqWalkArgs& a, hipStream_t stream) {
  if (a.nchunks > kPqMax || a.table_rows > kPqMax) return hipErrorInvalidValue;
  if (a.nchunks == 0) return hipSuccess;
  if (!a.chunk_off || !a.chunk_len || (!a.data && a.data_bytes)) return hipErrorInvalidValue;
  if (a.table ? !a.page_base : (!a.counts || !a.errors)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_walk_kernel, dim3(pq_grid(a.nchunks, kPqSerialThreads)), dim3(kPqSerialThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_parquet_lz4_plan(const PqLz4Args& a, hipStream_t stream) {
  if (a.npages > kPqMax) return hipErrorInvalidValue;
  if (a.npages == 0) return hipSuccess;
  if (!a.table || !a.dst_off || !a.chunks || !a.expect || (!a.data && a.data_bytes) || (!a.out && a.out_bytes))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_lz4_plan_kernel, dim3(pq_grid(a.npages, kPqSerialThreads)), dim3(kPqSerialThreads), 0, stream,
                     a);
  return hipGetLastError();
}

hipError_t launch_parquet_hybrid(const PqStreamArgs& a, int mode, hipStream_t stream) {
  if (a.nstreams > kPqMax || a.out_n > kPqMax || a.runs_rows > kPqMax || mode < 0 || mode > 3)
    return hipErrorInvalidValue;
  if (a.nstreams == 0) return hipSuccess;
  if (!a.streams || (!a.data && a.data_bytes) || (!a.out && a.out_n)) return hipErrorInvalidValue;
  if (mode == 0) {
    hipLaunchKernelGGL(pq_hybrid_serial_kernel, dim3(pq_grid(a.nstreams, kPqSerialThreads)), dim3(kPqSerialThreads), 0,
                       stream, a);
  } else if (mode == 1 || mode == 2) {
    PqStreamArgs b = a;
    if (mode == 1) {
      if (!a.run_counts || !a.errors) return hipErrorInvalidValue;
      b.runs = nullptr;
    } else if (!a.run_base || (!a.runs && a.runs_rows)) {
      return hipErrorInvalidValue;
    } else if (!a.runs) {
      return hipSuccess;                              // no stream has a run
    }
    hipLaunchKernelGGL(pq_hybrid_runs_kernel, dim3(pq_grid(a.nstreams, kPqSerialThreads)), dim3(kPqSerialThreads), 0,
                       stream, b);
  } else {
    if (!a.run_base || (!a.runs && a.runs_rows)) return hipErrorInvalidValue;
    if (a.out_n == 0) return hipSuccess;
    hipLaunchKernelGGL(pq_hybrid_values_kernel, dim3(pq_grid(a.out_n, kPqThreads)), dim3(kPqThreads), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_parquet_place(const PqPlaceArgs& a, hipStream_t stream) {
  if (a.rows > kPqMax || a.npages > kPqMax || (a.width != 1 && a.width != 4 && a.width != 8))
    return hipErrorInvalidValue;
  if (a.rows == 0) return hipSuccess;
  if (!a.values || !a.status || (!a.pages && a.npages) || (!a.data && a.data_bytes) || (!a.idx && a.idx_n) ||
      (!a.dict && a.dict_size))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_place_kernel, dim3(pq_grid(a.rows, kPqThreads)), dim3(kPqThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_parquet_bytes(const PqBytesArgs& a, hipStream_t stream) {
  if (a.npages > kPqMax || a.nvalues > kPqMax || a.rows > kPqMax) return hipErrorInvalidValue;
  if (a.npages == 0 || a.nvalues == 0) return hipSuccess;
  if (!a.pages || !a.start || !a.length || !a.status || (!a.data && a.data_bytes)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pq_bytes_kernel, dim3(pq_grid(a.npages, kPqSerialThreads)), dim3(kPqSerialThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
