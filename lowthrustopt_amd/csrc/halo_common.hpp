// halo_common.hpp -- what the periodic-orbit kernels share (kernels_halo.hip, kernels_halo_target.hip): the
// ballistic CRTBP with one column of its variational equations, the Jacobi constant, the start of a flight in a lane's view and the
// bisection that locates the return to y = 0.  gfx950 device code.
#pragma once
#include "kernels.hpp"
#include "dop853_lane.hpp"

namespace lto {

namespace {

// The CRTBP without thrust and one column c of its variational equations: y = (r, v, c_r, c_v), c' = [0 I; G 2W] c.
struct SysHaloVar {
  static constexpr int DIM = 12;
  double MU;
  __device__ __forceinline__ void rhs(const double (&y)[12], double (&k)[12]) const {
    const double x = y[0], yy = y[1], z = y[2];
    const double a = x + MU, b = a - 1.0;
    const double yz2 = __builtin_fma(yy, yy, z * z);
    const double d1 = __builtin_fma(a, a, yz2), d2 = __builtin_fma(b, b, yz2);
    const double i1 = rsqrt_nr(d1), i2 = rsqrt_nr(d2);
    const double c1 = (1.0 - MU) * (i1 * i1 * i1), c2 = MU * (i2 * i2 * i2);
    const double cs = c1 + c2;
    k[0] = y[3]; k[1] = y[4]; k[2] = y[5];
    k[3] = __builtin_fma(-c1, a, __builtin_fma(-c2, b, __builtin_fma(2.0, y[4], x)));
    k[4] = __builtin_fma(-cs, yy, __builtin_fma(-2.0, y[3], yy));
    k[5] = -cs * z;
    // gravity gradient G = d(acceleration) / d(position), symmetric
    const double q1 = 3.0 * c1 * (i1 * i1), q2 = 3.0 * c2 * (i2 * i2), qs = q1 + q2;
    const double qa = __builtin_fma(q1, a, q2 * b);
    const double gxx = __builtin_fma(q1 * a, a, __builtin_fma(q2 * b, b, 1.0 - cs));
    const double gyy = __builtin_fma(qs * yy, yy, 1.0 - cs);
    const double gzz = __builtin_fma(qs * z, z, -cs);
    const double gxy = qa * yy, gxz = qa * z, gyz = qs * yy * z;
    k[6] = y[9]; k[7] = y[10]; k[8] = y[11];
    k[9] = __builtin_fma(gxx, y[6], __builtin_fma(gxy, y[7], __builtin_fma(gxz, y[8], 2.0 * y[10])));
    k[10] = __builtin_fma(gxy, y[6], __builtin_fma(gyy, y[7], __builtin_fma(gyz, y[8], -2.0 * y[9])));
    k[11] = __builtin_fma(gxz, y[6], __builtin_fma(gyz, y[7], gzz * y[8]));
  }
};

// Jacobi constant C = x^2 + y^2 + 2 (1 - MU) / r1 + 2 MU / r2 - v^2
__device__ __forceinline__ double jacobi_constant(const double MU, const double (&y)[12]) {
  const double a = y[0] + MU, b = a - 1.0;
  const double yz2 = __builtin_fma(y[1], y[1], y[2] * y[2]);
  const double r1 = sqrt(__builtin_fma(a, a, yz2)), r2 = sqrt(__builtin_fma(b, b, yz2));
  const double v2 = __builtin_fma(y[3], y[3], __builtin_fma(y[4], y[4], y[5] * y[5]));
  return __builtin_fma(y[0], y[0], y[1] * y[1]) + 2.0 * (1.0 - MU) / r1 + 2.0 * MU / r2 - v2;
}

__device__ __forceinline__ bool finite12(const double (&y)[12]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i) s += y[i];
  return (s - s) == 0.0;
}

// the start of a flight in lane `col`'s view: the base state and column `col` of the identity
__device__ __forceinline__ void halo_start(const double (&x)[6], const int col, double (&y)[12]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) { y[i] = x[i]; y[6 + i] = (i == col) ? 1.0 : 0.0; }
}

// The step from time t over h took y across the plane: bracket the crossing in theta (kernels_events.hip locate_crossing's
// bisection) and return its time, the state one trial step of that length from the step's start in yc.
// trial(th, yt): the state one step of length th from the step's start; side: the sign of y before the crossing.
template <class Trial>
__device__ __forceinline__ double halo_crossing(const double t, const double h, const double side, Trial&& trial, double (&yc)[12]) {
  double lo = 0.0, hi = 1.0;
  for (int k = 0; k < 60; ++k) {
    const double mid = 0.5 * (lo + hi);
    double yt[12];
    trial(mid * h, yt);
    if (side * yt[1] > 0.0) lo = mid;
    else hi = mid;
    const double t_lo = __builtin_fma(lo, h, t), t_hi = __builtin_fma(hi, h, t);
    if (!(t_hi > nextafter(t_lo, __builtin_huge_val()))) break;     // adjacent doubles (or the same one)
  }
  trial(hi * h, yc);
  return __builtin_fma(hi, h, t);
}

}  // namespace

}  // namespace lto
