// kernels_halo_target.hip -- periodic orbits of the CRTBP at a given Jacobi constant or a given period, B orbits side by side, each
// marched through T target values inside one launch, gfx950.
//
// One GROUP of 8 adjacent lanes per orbit (dop853_lane.hpp), as in kernels_halo.hip, but the group carries only the three columns of
// Phi = dx/dx0 the Newton step reads: lane 0 column 0 (x0), lane 1 column 2 (z0), lane 2 column 4 (vy0); lanes 3..7 shadow lane 0
// and add nothing to the error norm, which therefore runs over 6 + 3 x 6 = 24 components.  Everything a group decides it decides
// from values every lane of it holds alike: no lane ever leaves the others.  A group beyond the batch shadows the last orbit.
// No LDS, plain vector stores.
//
// Per member and iteration: the flight of k_halo_correct -- from (x0, 0, z0, 0, vy0, 0) to the first return to y = 0, the crossing
// bracketed to adjacent doubles in time by halo_crossing, the state and Phi there from one more trial step -- then
//   r = (vx, vz, q - q*),   q = C(start) (what = 0)   or   q = 2 t_c (what = 1)
//   J = [ Phi[(3,5), j] - f[(3,5)] Phi[1, j] / f[1] ;  dq/d(x0, z0, vy0) ],   j = 0, 2, 4
// with dC/d. analytic and d(2 t_c)/d. = -2 Phi[1, j] / f[1].  The planar form (z0 = 0) is the same 3 x 3 system with the z0 row and
// column replaced by the identity's: its determinant, its row-norm product and its solution are those of the 2 x 2 system in
// (x0, vy0).  The solve is an LU with partial pivoting done by selects (no index depends on data) in every lane of the group alike.
//
// The march: member 0 starts from the seed, member 1 from member 0, member k >= 2 from the secant through the last two members in
// the target value; sum, difference and product of the predictor are rounded one by one (no fused multiply-add), so that the host
// can form the same point from the call's outputs.
#include "halo_common.hpp"

namespace lto {

namespace {

__device__ __forceinline__ void swap_if(const bool p, double& u, double& v) {
  const double t = p ? v : u;
  v = p ? u : v;
  u = t;
}

// d = J^-1 r.  Returns 1.0 for a singular step -- |det| <= sing_tol x the product of the row 2-norms, or det not finite -- else 0.0.
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

// s1 + (s1 - s2) w, every operation rounded on its own
__device__ __forceinline__ double secant_point(const double s1, const double s2, const double w) {
#pragma clang fp contract(off)
  const double ds = s1 - s2;
  const double step = ds * w;
  return s1 + step;
}

}  // namespace

template <int METHOD>
__global__ __launch_bounds__(64) void k_halo_target(const HaloTargetArgs a) {
  const int gid = blockIdx.x * 64 + threadIdx.x;
  const int g = gid >> 3, c = gid & 7;
  const int gbase = threadIdx.x & ~7;
  const int b = (g < a.B) ? g : a.B - 1;         // a group beyond the batch shadows the last orbit
  const int col = (c < 3) ? 2 * c : 0;           // lanes 0, 1, 2: columns 0, 2, 4
  const double colw = (c < 3) ? 1.0 : 0.0;
  const bool planar = a.planar != 0;
  const bool store = (g < a.B) && (c == 0);
  const double nan = __builtin_nan("");
  SysHaloVar sys;
  sys.MU = a.MU;
  const double MU = a.MU;

  // the last two points of the march and their target values
  double s1[3] = {a.seed[6 * (long)b + 0], a.seed[6 * (long)b + 2], a.seed[6 * (long)b + 4]};
  double s2[3] = {s1[0], s1[1], s1[2]};
  double q1 = 0.0, q2 = 0.0;
  double dead = 0.0;                             // per-lane flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler hazards")

  for (int k = 0; k < a.T; ++k) {
    const long m = (long)a.T * b + k;
    const double qs = a.target[m];
    double* hist = a.hist + (long)(a.max_iter + 1) * m;
    double w = 0.0;
    if (k >= 2 && q1 != q2) w = (qs - q1) / (q1 - q2);
    double x0 = secant_point(s1[0], s2[0], w), z0 = secant_point(s1[1], s2[1], w), vy0 = secant_point(s1[2], s2[2], w);

    double status = -1.0;
    double tc = 0.0, res = nan, qv = nan;
    int it = 0, nrec = 0;
    {
      const double s = x0 + z0 + vy0 + qs;
      if (dead != 0.0 || !((s - s) == 0.0) || vy0 == 0.0 || (planar && z0 != 0.0) || (a.what == LTO_HALO_TARGET_PERIOD && !(qs > 0.0)))
        status = 2.0;
    }
    while (status < 0.0) {
      const double xs[6] = {x0, 0.0, z0, 0.0, vy0, 0.0};
      double y[12], yc[12];
      halo_start(xs, col, y);
      const double C0 = jacobi_constant(MU, y);
      const double side = (vy0 > 0.0) ? 1.0 : -1.0;
      double found = 0.0;
      if (METHOD == M_RK4) {
        const double h = a.t_max / (double)a.steps;
        for (int n = 0; n < a.steps; ++n) {
          double ys[12];
#pragma unroll
          for (int i = 0; i < 12; ++i) ys[i] = y[i];
          rk4_step(sys, h, y);
          if (!(side * y[1] > 0.0)) {
            if (y[1] == y[1]) {
              tc = halo_crossing(__builtin_fma((double)n, h, 0.0), h, side, [&](const double th, double (&yt)[12]) {
#pragma unroll
                for (int i = 0; i < 12; ++i) yt[i] = ys[i];
                rk4_step(sys, th, yt);
              }, yc);
              found = 1.0;
            }
            break;
          }
        }
      } else {
        int na = 0, nr = 0;
        (void)run_dop853_group<SysHaloVar, 6, 3>(sys, a.t_max, a.rtol, a.atol, a.max_steps, colw, y, na, nr,
            [&](const double t, const double h, const double (&ys)[12], double (&K)[13][12], const double (&yn)[12]) -> double {
          if (side * yn[1] > 0.0) return 0.0;
          if (yn[1] == yn[1]) {
            tc = halo_crossing(t, h, side, [&](const double th, double (&yt)[12]) {
              double E5, E3;
              (void)dop853_try<SysHaloVar, 6>(sys, th, a.rtol, a.atol, ys, K, yt, E5, E3);
            }, yc);
            found = 1.0;
          }
          return 1.0;
        });
      }
      if (found == 0.0 || !finite12(yc)) { status = 2.0; break; }
      // the residual at the crossing
      qv = (a.what == LTO_HALO_TARGET_PERIOD) ? 2.0 * tc : C0;
      const double rq = qv - qs;
      res = fmax(fabs(yc[3]), fabs(rq));
      if (!planar) res = fmax(res, fabs(yc[5]));
      if (store) hist[it] = res;
      nrec = it + 1;
      if (res < a.tol) { status = 0.0; break; }
      if (it >= a.max_iter) { status = 1.0; break; }
      // f at the crossing and the entries of Phi the step reads: row r of column 2 j is component 6 + r of lane gbase + j
      double f[12];
      sys.rhs(yc, f);
      const double w1 = 1.0 / f[1], w3 = f[3] / f[1], w5 = f[5] / f[1];
      double J[3][3], r[3] = {yc[3], yc[5], rq}, d[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double p1 = __shfl(yc[7], gbase + j, 64), p3 = __shfl(yc[9], gbase + j, 64), p5 = __shfl(yc[11], gbase + j, 64);
        J[0][j] = __builtin_fma(-w3, p1, p3);
        J[1][j] = __builtin_fma(-w5, p1, p5);
        J[2][j] = -2.0 * p1 * w1;
      }
      if (a.what == LTO_HALO_TARGET_JACOBI) {
        const double aa = x0 + MU, bb = aa - 1.0;
        const double d1 = __builtin_fma(aa, aa, z0 * z0), d2 = __builtin_fma(bb, bb, z0 * z0);
        const double c1 = (1.0 - MU) / (d1 * sqrt(d1)), c2 = MU / (d2 * sqrt(d2));
        J[2][0] = 2.0 * x0 - 2.0 * c1 * aa - 2.0 * c2 * bb;
        J[2][1] = -2.0 * z0 * (c1 + c2);
        J[2][2] = -2.0 * vy0;
      }
      if (planar) {
        J[0][1] = 0.0; J[2][1] = 0.0;
        J[1][0] = 0.0; J[1][1] = 1.0; J[1][2] = 0.0;
        r[1] = 0.0;
      }
      if (newton_solve3(J, r, a.sing_tol, d) != 0.0) { status = 3.0; break; }
      x0 -= d[0];
      z0 -= d[1];
      vy0 -= d[2];
      ++it;
    }
    const bool fail = status >= 2.0;
    if (store) {
      double* so = a.state + 6 * m;
      so[0] = fail ? nan : x0; so[1] = fail ? nan : 0.0; so[2] = fail ? nan : z0;
      so[3] = fail ? nan : 0.0; so[4] = fail ? nan : vy0; so[5] = fail ? nan : 0.0;
      const double xs[12] = {x0, 0.0, z0, 0.0, vy0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      a.period[m] = fail ? nan : 2.0 * tc;
      a.jacobi[m] = fail ? nan : jacobi_constant(MU, xs);
      a.resid[m] = fail ? nan : res;
      a.iters[m] = it;
      a.status[m] = (int)status;
      for (int n = nrec; n <= a.max_iter; ++n) hist[n] = nan;
    }
    if (fail) {
      dead = 1.0;                                // the rest of this orbit's members: NaN, status 2
    } else {
      s2[0] = s1[0]; s2[1] = s1[1]; s2[2] = s1[2];
      s1[0] = x0; s1[1] = z0; s1[2] = vy0;
      q2 = q1; q1 = qs;
    }
  }
}

hipError_t launch_halo_target(int method, const HaloTargetArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(((long)a.B * kGroupLanes + 63) / 64));
  if (method == M_RK4) hipLaunchKernelGGL(k_halo_target<M_RK4>, grid, dim3(64), 0, st, a);
  else if (method == M_DOP853_ADAPTIVE) hipLaunchKernelGGL(k_halo_target<M_DOP853_ADAPTIVE>, grid, dim3(64), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lto
