// kernels_halo_arclength.hip -- families of periodic orbits of the CRTBP by pseudo-arclength continuation, B families side by side,
// each marched through T members inside one launch with its own step control, gfx950.
//
// The mapping is k_halo_target's (halo_common.hpp group_lane): lanes 0, 1, 2 of a group carry columns 0, 2, 4 of Phi = dx/dx0.
// Everything a group decides it decides from values every lane of it holds in the same bits.  No LDS, plain vector stores, flags
// are per-lane doubles.
//
// With u = (x0, z0, vy0), per flight (halo_return_rk4, or the same rule under the group driver): F = (vx, vz) at the first return
// to y = 0, DF from halo_df_column (planar: halo_planar_patch) and
//   c = DF_0 x DF_1,   n = |c|_2,   sigma = sign(c . t_row),   t = sigma c / n,   det = sigma n
// A member is the step from u_prev along the row vector t_row: u_pred = u_prev + ds t_row (product and sum rounded one by one), then
//   u <- u - [DF; t_row]^-1 (F; t_row . (u - u_pred))
// by newton_solve3.  An attempt that does not converge, or whose tangent turns beyond cos_min, is tried again from the same u_prev
// with half the step; after a fast member the step grows.
#include "halo_common.hpp"

namespace lto {

namespace {

// u + ds t, product and sum rounded on their own
__device__ __forceinline__ double predictor_point(const double u, const double ds, const double t) {
#pragma clang fp contract(off)
  const double step = ds * t;
  return u + step;
}

// a . b, fused in the fixed order a0 b0 + (a1 b1 + a2 b2)
__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) {
  return __builtin_fma(a[0], b[0], __builtin_fma(a[1], b[1], a[2] * b[2]));
}

__device__ __forceinline__ bool finite1(const double v) { return (v - v) == 0.0; }

}  // namespace

template <int METHOD>
__global__ __launch_bounds__(64) void k_halo_arclength(const HaloArclengthArgs a) {
  const GroupLane<int> L = group_lane<3, 2>(a.B);      // lanes 0, 1, 2: columns 0, 2, 4
  const int b = L.rec;
  const bool planar = a.planar != 0;
  const double nan = __builtin_nan("");
  SysHaloVar sys;
  sys.MU = a.MU;
  const double MU = a.MU;

  // the last accepted point, the row vector the next member steps along (only the seed's own correction replaces it within a
  // member, and that member has one attempt), and its step
  double up[3] = {a.seed[6 * (long)b + 0], a.seed[6 * (long)b + 2], a.seed[6 * (long)b + 4]};
  double tw[3] = {a.dir0[3 * (long)b + 0], a.dir0[3 * (long)b + 1], a.dir0[3 * (long)b + 2]};
  double ds = a.ds0[b];
  double dead = 0.0;                             // per-lane flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler hazards")
  {
    const double s = up[0] + up[1] + up[2] + tw[0] + tw[1] + tw[2];
    if (!finite1(s) || up[2] == 0.0 || (planar && up[1] != 0.0) || (tw[0] == 0.0 && tw[1] == 0.0 && tw[2] == 0.0)) dead = 1.0;
  }

  for (int k = 0; k < a.T; ++k) {
    const long m = (long)a.T * b + k;
    double* hist = a.hist + (long)(a.max_iter + 1) * m;
    const double orient = (k == 0 && a.dir_is_tangent == 0) ? 1.0 : 0.0;   // member 0 of a seed that is yet to be put on the family
    double status = -1.0;
    double u[3] = {up[0], up[1], up[2]}, tn[3] = {nan, nan, nan};
    double tc = 0.0, res = nan, det = nan, dsa = (orient != 0.0) ? 0.0 : ds;
    int it = 0, nrec = 0, halv = 0;
    if (dead != 0.0) { status = 2.0; dsa = nan; }

    while (status < 0.0) {                       // attempts at the member, each with half the step of the one before
      u[0] = predictor_point(up[0], dsa, tw[0]); u[1] = predictor_point(up[1], dsa, tw[1]); u[2] = predictor_point(up[2], dsa, tw[2]);
      it = 0; nrec = 0; res = nan;
      double oriented = 1.0 - orient;            // 0 until the seed's own tangent has been formed
      {
        const double s = u[0] + u[1] + u[2];
        if (!finite1(s) || u[2] == 0.0 || (planar && u[1] != 0.0)) status = 2.0;
      }
      while (status < 0.0) {                     // flights of the attempt
        double yc[12];
        double found = 0.0;
        if (METHOD == M_RK4) {
          found = halo_return_rk4(sys, u[0], u[1], u[2], L.col, a, tc, yc);
        } else {                                     // halo_return_rk4's rule under the group driver (halo_common.hpp: why in place)
          const double xs[6] = {u[0], 0.0, u[1], 0.0, u[2], 0.0};
          double y[12];
          halo_start(xs, L.col, y);
          const double side = (u[2] > 0.0) ? 1.0 : -1.0;
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
        // DF at the crossing from the group's three columns; the third row is set below, before the solve
        double f[12];
        sys.rhs(yc, f);
        const double w3 = f[3] / f[1], w5 = f[5] / f[1];
        double J[3][3], r[3] = {yc[3], yc[5], 0.0}, d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          double p1;
          halo_df_column(yc, w3, w5, L.gbase, j, J[0][j], J[1][j], p1);
        }
        if (planar) halo_planar_patch(J, r);
        // the tangent of this flight's DF, not yet oriented
        const double cr[3] = {__builtin_fma(J[0][1], J[1][2], -(J[0][2] * J[1][1])), __builtin_fma(J[0][2], J[1][0], -(J[0][0] * J[1][2])),
                              __builtin_fma(J[0][0], J[1][1], -(J[0][1] * J[1][0]))};
        const double nrm = sqrt(dot3(cr, cr));
        const bool no_tangent = !(nrm > 0.0) || !finite1(nrm);
        if (oriented == 0.0) {                   // the seed's tangent, pointing dir0's way, is the member's row vector
          const double dt = dot3(cr, tw);
          if (!finite1(dt) || dt == 0.0) { status = 2.0; break; }
          if (no_tangent) { status = 3.0; break; }
          const double sg = (dt > 0.0) ? 1.0 : -1.0;
          tw[0] = sg * cr[0] / nrm; tw[1] = sg * cr[1] / nrm; tw[2] = sg * cr[2] / nrm;
          oriented = 1.0;
        }
        const double dcr = dot3(cr, tw);
        // the predicted point again, not kept across the flight (the seed's own correction: ds = 0, the seed itself)
        const double du[3] = {u[0] - predictor_point(up[0], dsa, tw[0]), u[1] - predictor_point(up[1], dsa, tw[1]),
                              u[2] - predictor_point(up[2], dsa, tw[2])};
        r[2] = dot3(tw, du);
        res = fmax(fabs(r[0]), fabs(r[2]));
        if (!planar) res = fmax(res, fabs(r[1]));
        if (L.lead) hist[it] = res;
        nrec = it + 1;
        const bool conv = res < a.tol;
        if (conv || it >= a.max_iter) {
          if (no_tangent || !finite1(dcr) || dcr == 0.0) { status = 3.0; break; }
          const double sg = (dcr > 0.0) ? 1.0 : -1.0;
          tn[0] = sg * cr[0] / nrm; tn[1] = sg * cr[1] / nrm; tn[2] = sg * cr[2] / nrm;
          det = sg * nrm;
          status = conv ? 0.0 : 1.0;
          if (conv && dot3(tn, tw) < a.cos_min) status = 4.0;
          break;
        }
        J[2][0] = tw[0]; J[2][1] = tw[1]; J[2][2] = tw[2];
        if (newton_solve3(J, r, a.sing_tol, d) != 0.0) { status = 3.0; break; }
        u[0] -= d[0];
        u[1] -= d[1];
        u[2] -= d[2];
        ++it;
      }
      if (status == 0.0 || orient != 0.0) break;
      const double half = 0.5 * dsa;
      if (half < a.ds_min) break;
      dsa = half;
      ++halv;
      status = -1.0;
    }

    const bool fail = status >= 2.0;
    if (L.lead) {
      halo_member_store(a, m, hist, u[0], u[1], u[2], tc, res, it, nrec, status);
      double* to = a.tangent + 3 * m;
      to[0] = fail ? nan : tn[0]; to[1] = fail ? nan : tn[1]; to[2] = fail ? nan : tn[2];
      const double xs[12] = {u[0], 0.0, u[1], 0.0, u[2], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      a.det[m] = fail ? nan : det;
      a.ds[m] = dsa;
      a.jacobi[m] = fail ? nan : jacobi_constant(MU, xs);
      a.halvings[m] = halv;
    }
    if (status != 0.0) {
      dead = 1.0;                                // the rest of this orbit's members: NaN, status 2
    } else {
      up[0] = u[0]; up[1] = u[1]; up[2] = u[2];
      tw[0] = tn[0]; tw[1] = tn[1]; tw[2] = tn[2];
      if (orient == 0.0) {
        ds = dsa;
        if (it <= a.fast_iter) ds = fmin(ds * a.grow, a.ds_max);
      }
    }
  }
}

hipError_t launch_halo_arclength(int method, const HaloArclengthArgs& a, hipStream_t st) {
  return launch_by_method(method, k_halo_arclength<M_RK4>, k_halo_arclength<M_DOP853_ADAPTIVE>, (long)a.B * kGroupLanes, a, st);
}

}  // namespace lto
