// wave_reduce.hpp -- reductions and the inclusive scan over the 64 lanes of a wavefront (gfx950 device code).  The butterflies
// (__shfl_xor 32, 16, .. 1) add or compare the same pairs in every lane: the result is the same bits in all 64.
#pragma once
#include <hip/hip_runtime.h>

namespace lto {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const int u = __shfl_xor(v, off, 64); v = u < v ? u : v; }
  return v;
}
__device__ __forceinline__ int wave_scan_incl(int v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

}  // namespace lto
