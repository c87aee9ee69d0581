// halo_common.hpp -- what the periodic-orbit kernels share (kernels_halo.hip, kernels_halo_target.hip, kernels_halo_arclength.hip,
// kernels_halo_stm.hip): the ballistic CRTBP with one column of its variational equations, the Jacobi constant, a
// lane's place in its group, the flight to the first return to y = 0 with the bisection that locates it, the 3 x 3 Newton solve, the
// columns of the correctors' Jacobian and what a corrector stores per member.  gfx950 device code that also compiles for the host
// (tests/host_stub).
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

// A lane's place in its GROUP of 8 adjacent lanes (dop853_lane.hpp), 8 groups per wavefront.  Group g of the grid works on record
// min(g, n_rec - 1): a group beyond the last record shadows it.  Lane c < NCOL of a group carries column STRIDE c of Phi = dx/dx0 and
// counts in the error norm (colw = 1); the other lanes shadow lane 0 and add nothing.  lead and column are fixed functions of the
// lane's index that only guard stores.  Index: int, or long where the record count may pass 2^31 / 8.
template <class Index>
struct GroupLane {
  Index rec;                 // the record the group works on
  int c, gbase;              // the lane within its group, and the wavefront lane of the group's lane 0
  int col;
  double colw;
  bool lead, column;         // lane 0 / a column lane of a group that has a record of its own
};
template <int NCOL, int STRIDE, class Index>
__device__ __forceinline__ GroupLane<Index> group_lane(const Index n_rec) {
  const Index gid = (Index)blockIdx.x * 64 + threadIdx.x;
  const Index g = gid >> 3;
  GroupLane<Index> L;
  L.c = (int)(gid & 7);
  L.gbase = threadIdx.x & ~7;
  L.rec = (g < n_rec) ? g : n_rec - 1;
  L.col = (L.c < NCOL) ? STRIDE * L.c : 0;
  L.colw = (L.c < NCOL) ? 1.0 : 0.0;
  L.lead = (g < n_rec) && (L.c == 0);
  L.column = (g < n_rec) && (L.c < NCOL);
  return L;
}

// The flight of the correctors under RK4: from (x0, 0, z0, 0, vy0, 0), with column `col` of the identity, a.steps steps over a.t_max
// to the first return to y = 0 -- the first step at whose end y has left the side vy0 sent it to.  The crossing is bracketed by trial
// steps of the same formula from the step's start (halo_crossing); tc is its time and yc the state and the column there, from one
// more trial step.  Returns 1.0 with tc and yc set (the caller still asks finite12(yc)), else 0.0 (no return within t_max, a step
// whose y is NaN): tc is then left alone and yc is not to be read.  Flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler
// hazards").  a: the corrector's argument block (t_max, steps).
// The adaptive flight is the same rule under run_dop853_group, and stands in each of the three correctors: wrapped in a function,
// even one that holds nothing but the driver's call and its hook, the DOP853 kernels are allocated differently.
template <class Args>
__device__ __forceinline__ double halo_return_rk4(const SysHaloVar& sys, const double x0, const double z0, const double vy0,
                                                  const int col, const Args& a, double& tc, double (&yc)[12]) {
  const double xs[6] = {x0, 0.0, z0, 0.0, vy0, 0.0};
  double y[12];
  halo_start(xs, col, y);
  const double side = (vy0 > 0.0) ? 1.0 : -1.0;
  double found = 0.0;
  const double h = a.t_max / (double)a.steps;
  for (int k = 0; k < a.steps; ++k) {
    double ys[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) ys[i] = y[i];
    rk4_step(sys, h, y);
    if (!(side * y[1] > 0.0)) {
      if (y[1] == y[1]) {
        tc = halo_crossing(__builtin_fma((double)k, h, 0.0), h, side, [&](const double th, double (&yt)[12]) {
#pragma unroll
          for (int i = 0; i < 12; ++i) yt[i] = ys[i];
          rk4_step(sys, th, yt);
        }, yc);
        found = 1.0;
      }
      break;
    }
  }
  return found;
}

__device__ __forceinline__ void swap_if(const bool p, double& u, double& v) {
  const double t = p ? v : u;
  v = p ? u : v;
  u = t;
}

// d = J^-1 r by an LU with partial pivoting done by selects (no index depends on data).  The singular rule: returns 1.0, with d all
// NaN, when |det| <= sing_tol x the product of the row 2-norms or det is not finite; else 0.0.
__device__ __forceinline__ double newton_solve3(const double (&J)[3][3], const double (&r)[3], const double sing_tol, double (&d)[3]) {
  const double m0 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double m1 = J[1][0] * J[2][2] - J[1][2] * J[2][0];
  const double m2 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * m0 - J[0][1] * m1 + J[0][2] * m2;
  double prod = 1.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) prod *= sqrt(__builtin_fma(J[i][0], J[i][0], __builtin_fma(J[i][1], J[i][1], J[i][2] * J[i][2])));
  d[0] = d[1] = d[2] = __builtin_nan("");
  if (!(fabs(det) > sing_tol * prod) || !((det - det) == 0.0)) return 1.0;
  double A[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i) { A[i][0] = J[i][0]; A[i][1] = J[i][1]; A[i][2] = J[i][2]; A[i][3] = r[i]; }
  // column 0: the largest of |A[.][0]| to row 0
  bool p = fabs(A[1][0]) > fabs(A[0][0]);
#pragma unroll
  for (int j = 0; j < 4; ++j) swap_if(p, A[0][j], A[1][j]);
  p = fabs(A[2][0]) > fabs(A[0][0]);
#pragma unroll
  for (int j = 0; j < 4; ++j) swap_if(p, A[0][j], A[2][j]);
  const double l1 = A[1][0] / A[0][0], l2 = A[2][0] / A[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) { A[1][j] = __builtin_fma(-l1, A[0][j], A[1][j]); A[2][j] = __builtin_fma(-l2, A[0][j], A[2][j]); }
  // column 1
  p = fabs(A[2][1]) > fabs(A[1][1]);
#pragma unroll
  for (int j = 1; j < 4; ++j) swap_if(p, A[1][j], A[2][j]);
  const double l3 = A[2][1] / A[1][1];
#pragma unroll
  for (int j = 2; j < 4; ++j) A[2][j] = __builtin_fma(-l3, A[1][j], A[2][j]);
  d[2] = A[2][3] / A[2][2];
  d[1] = __builtin_fma(-A[1][2], d[2], A[1][3]) / A[1][1];
  d[0] = __builtin_fma(-A[0][1], d[1], __builtin_fma(-A[0][2], d[2], A[0][3])) / A[0][0];
  return 0.0;
}

// The column of DF = d(vx, vz at the crossing) / d(start) that group lane j carries: rows (3, 5) of its column of Phi, less
// f[(3, 5)] / f[1] = (w3, w5) times row 1 (the crossing time moves with the start).  Row r of the column is component 6 + r of yc
// in lane gbase + j; p1 is row 1 itself.
__device__ __forceinline__ void halo_df_column(const double (&yc)[12], const double w3, const double w5, const int gbase, const int j,
                                               double& J0, double& J1, double& p1) {
  p1 = __shfl(yc[7], gbase + j, 64);
  const double p3 = __shfl(yc[9], gbase + j, 64), p5 = __shfl(yc[11], gbase + j, 64);
  J0 = __builtin_fma(-w3, p1, p3);
  J1 = __builtin_fma(-w5, p1, p5);
}

// The planar form (z0 = 0) of the 3 x 3 step in (x0, z0, vy0): the z0 row and column are the identity's, so that the determinant,
// the row-norm product and the solution are those of the 2 x 2 system in (x0, vy0).  Here the two DF rows and r; the z0 entry of the
// third row is its owner's to clear.
__device__ __forceinline__ void halo_planar_patch(double (&J)[3][3], double (&r)[3]) {
  J[0][1] = 0.0;
  J[1][0] = 0.0; J[1][1] = 1.0; J[1][2] = 0.0;
  r[1] = 0.0;
}

// What a corrector leaves of member m (a: its argument block): the start (x0, 0, z0, 0, vy0, 0) or six NaN after a failure
// (status >= 2), the period 2 tc, the last residual, the counts, and NaN in the history behind the nrec residuals recorded.
template <class Args>
__device__ __forceinline__ void halo_member_store(const Args& a, const long m, double* hist, const double x0, const double z0,
                                                  const double vy0, const double tc, const double res, const int it, const int nrec,
                                                  const double status) {
  const bool fail = status >= 2.0;
  const double nan = __builtin_nan("");
  double* so = a.state + 6 * m;
  so[0] = fail ? nan : x0; so[1] = fail ? nan : 0.0; so[2] = fail ? nan : z0;
  so[3] = fail ? nan : 0.0; so[4] = fail ? nan : vy0; so[5] = fail ? nan : 0.0;
  a.period[m] = fail ? nan : 2.0 * tc;
  a.resid[m] = fail ? nan : res;
  a.iters[m] = it;
  a.status[m] = (int)status;
  for (int k = nrec; k <= a.max_iter; ++k) hist[k] = nan;
}

}  // namespace

}  // namespace lto
