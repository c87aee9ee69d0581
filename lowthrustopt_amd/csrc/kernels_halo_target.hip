// kernels_halo_target.hip -- periodic orbits of the CRTBP at a given Jacobi constant or a given period, B orbits side by side, each
// marched through T target values inside one launch, gfx950.
//
// One GROUP of 8 adjacent lanes per orbit (halo_common.hpp group_lane), but the group carries only the three columns of
// Phi = dx/dx0 the Newton step reads: lane 0 column 0 (x0), lane 1 column 2 (z0), lane 2 column 4 (vy0); lanes 3..7 shadow lane 0
// and add nothing to the error norm, which therefore runs over 6 + 3 x 6 = 24 components.  Everything a group decides it decides
// from values every lane of it holds alike: no lane ever leaves the others.  No LDS, plain vector stores.
//
// Per member and iteration: the return flight (halo_return_rk4, or the same rule under the group driver), then
//   r = (vx, vz, q - q*),   q = C(start) (what = 0)   or   q = 2 t_c (what = 1)
//   J = [ DF ;  dq/d(x0, z0, vy0) ]                   DF: halo_df_column, planar: halo_planar_patch
// with dC/d. analytic and d(2 t_c)/d. = -2 Phi[1, j] / f[1], solved by newton_solve3 in every lane of the group alike.
//
// The march: member 0 starts from the seed, member 1 from member 0, member k >= 2 from the secant through the last two members in
// the target value; sum, difference and product of the predictor are rounded one by one (no fused multiply-add), so that the host
// can form the same point from the call's outputs.
#include "halo_common.hpp"

namespace lto {

namespace {

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
  const GroupLane<int> L = group_lane<3, 2>(a.B);      // lanes 0, 1, 2: columns 0, 2, 4
  const int b = L.rec;
  const bool planar = a.planar != 0;
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
      const double xs[12] = {x0, 0.0, z0, 0.0, vy0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const double C0 = jacobi_constant(MU, xs);
      double yc[12];
      double found = 0.0;
      if (METHOD == M_RK4) {
        found = halo_return_rk4(sys, x0, z0, vy0, L.col, a, tc, yc);
      } else {                                     // halo_return_rk4's rule under the group driver (halo_common.hpp: why in place)
        const double xs[6] = {x0, 0.0, z0, 0.0, vy0, 0.0};
        double y[12];
        halo_start(xs, L.col, y);
        const double side = (vy0 > 0.0) ? 1.0 : -1.0;
        int na = 0, nr = 0;
        (void)run_dop853_group<SysHaloVar, 6, 3>(sys, a.t_max, a.rtol, a.atol, a.max_steps, L.colw, y, na, nr,
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
      if (L.lead) hist[it] = res;
      nrec = it + 1;
      if (res < a.tol) { status = 0.0; break; }
      if (it >= a.max_iter) { status = 1.0; break; }
      // f at the crossing, DF from the group's three columns, and d(2 t_c) / d. below it
      double f[12];
      sys.rhs(yc, f);
      const double w1 = 1.0 / f[1], w3 = f[3] / f[1], w5 = f[5] / f[1];
      double J[3][3], r[3] = {yc[3], yc[5], rq}, d[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double p1;
        halo_df_column(yc, w3, w5, L.gbase, j, J[0][j], J[1][j], p1);
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
      if (planar) { halo_planar_patch(J, r); J[2][1] = 0.0; }
      if (newton_solve3(J, r, a.sing_tol, d) != 0.0) { status = 3.0; break; }
      x0 -= d[0];
      z0 -= d[1];
      vy0 -= d[2];
      ++it;
    }
    const bool fail = status >= 2.0;
    if (L.lead) {
      halo_member_store(a, m, hist, x0, z0, vy0, tc, res, it, nrec, status);
      const double xs[12] = {x0, 0.0, z0, 0.0, vy0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      a.jacobi[m] = fail ? nan : jacobi_constant(MU, xs);
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
  return launch_by_method(method, k_halo_target<M_RK4>, k_halo_target<M_DOP853_ADAPTIVE>, (long)a.B * kGroupLanes, a, st);
}

}  // namespace lto
