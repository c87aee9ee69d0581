// scan64.hpp -- the running sum of the mesh equidistributions (kernels_remesh.hip, kernels_direct_resample.hip), one workgroup of
// kRemeshBlock threads per trajectory.
//
// The scan has ONE summation order whatever the size and wherever the partial sums live (integer counts do not care, real weights
// do): radix 64 in three levels.  A tile of 64 consecutive entries is scanned by a wavefront with six shift-and-add steps
// (__shfl_up by 1, 2, .. 32: the DPP row / wave shifts; an LDS round trip per step would cost a barrier each); the tile totals are
// scanned the same way, and theirs; then every entry adds the inclusive sum of the tiles before its own, top level first.
// tests/remesh_reference.scan64 restates exactly this order.  64^3 = 262 144 segments is the limit (the host refuses more).
#pragma once
#include <hip/hip_runtime.h>

namespace lto {

constexpr int kRemeshBlock = 256;

__device__ __forceinline__ double tile_scan(double v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// x[0 .. cnt) -> its tiles' inclusive scans in place, tot[T] = total of tile T.  Every wavefront takes whole tiles.
__device__ __forceinline__ void scan_tiles(double* x, const int cnt, double* tot, const int tid) {
  const int lane = tid & 63, tiles = (cnt + 63) >> 6;
  for (int T = tid >> 6; T < tiles; T += kRemeshBlock / 64) {
    const int i = T * 64 + lane;
    const double v = tile_scan(i < cnt ? x[i] : 0.0, lane);
    if (i < cnt) x[i] = v;
    if (lane == 63) tot[T] = v;
  }
  __syncthreads();
}

// x[i] += inclusive sum of the tiles before i's (inc: the scanned tile totals)
__device__ __forceinline__ void add_tile_offsets(double* x, const int cnt, const double* inc, const int tid) {
  for (int i = tid; i < cnt; i += kRemeshBlock) {
    const int T = i >> 6;
    if (T) x[i] = inc[T - 1] + x[i];
  }
  __syncthreads();
}

}  // namespace lto
