// Wave-level helpers of the one-wave-per-chunk decoders (the LZ4 decoders of kernels.hip, the
// Snappy decoders of snappy_decode.hip): the wave barrier that orders LDS traffic between lanes,
// shuffles and inclusive scans over the 64 lanes, and the global byte pointer type.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace amdx {

__device__ __forceinline__ void lz_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ uint32_t lz_shfl(uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)src, 64); }
__device__ __forceinline__ uint32_t lz_scan_add(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t lz_scan_max(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v = v > t ? v : t;
  }
  return v;
}

}  // namespace amdx
