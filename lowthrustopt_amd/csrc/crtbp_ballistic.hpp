// crtbp_ballistic.hpp -- the ballistic CRTBP as a one-lane system for run_dop853 / run_dop853_stop / rk4_step (gfx950 device code):
// what the section flights (kernels_manifold.hip) and the station-keeping flights (kernels_stationkeep.hip, DESIGN
// 4.29) both fly.
#pragma once
#include "dop853_lane.hpp"

namespace lto {

// The ballistic CRTBP, y = (r, v) (the expressions of kernels_stack.hip's SysBallistic), times sgn = +-1: sgn = -1 is the
// time-reversed system, flown over a positive span.
struct SysCrtbpDir {
  static constexpr int DIM = 6;
  double MU, sgn;
  __device__ __forceinline__ void rhs(const double (&y)[6], double (&k)[6]) const {
    const double x = y[0], yy = y[1], z = y[2];
    const double a = x + MU, b = a - 1.0;
    const double yz2 = __builtin_fma(yy, yy, z * z);
    const double d1 = __builtin_fma(a, a, yz2), d2 = __builtin_fma(b, b, yz2);
    const double i1 = rsqrt_nr(d1), i2 = rsqrt_nr(d2);
    const double c1 = (1.0 - MU) * (i1 * i1 * i1), c2 = MU * (i2 * i2 * i2);
    const double cs = c1 + c2;
    k[0] = sgn * y[3]; k[1] = sgn * y[4]; k[2] = sgn * y[5];
    k[3] = sgn * __builtin_fma(-c1, a, __builtin_fma(-c2, b, __builtin_fma(2.0, y[4], x)));
    k[4] = sgn * __builtin_fma(-cs, yy, __builtin_fma(-2.0, y[3], yy));
    k[5] = sgn * (-cs * z);
  }
};

template <int N>
__device__ __forceinline__ bool finite_all(const double (&y)[N]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) s += y[i];
  return (s - s) == 0.0;
}

}  // namespace lto
