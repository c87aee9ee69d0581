// kernels_halo_arclength.hip -- families of periodic orbits of the CRTBP by pseudo-arclength continuation, B families side by side,
// each marched through T members inside one launch with its own step control, gfx950.
//
// The mapping and the flight are k_halo_target's (kernels_halo_target.hip): one GROUP of 8 adjacent lanes per orbit, lanes 0, 1, 2
// carry columns 0, 2, 4 of Phi = dx/dx0, lanes 3..7 shadow lane 0 and add nothing to the error norm.  Everything a group decides it
// decides from values every lane of it holds in the same bits.  A group beyond the batch shadows the last orbit.  No LDS, plain
// vector stores, flags are per-lane doubles.
//
// With u = (x0, z0, vy0), per flight: F = (vx, vz) at the first return to y = 0 and
//   DF = Phi[(3,5), j] - f[(3,5)] Phi[1, j] / f[1],   j = 0, 2, 4            (planar: the z0 row and column are the identity's)
//   c = DF_0 x DF_1,   n = |c|_2,   sigma = sign(c . t_row),   t = sigma c / n,   det = sigma n
// A member is the step from u_prev along the row vector t_row: u_pred = u_prev + ds t_row (product and sum rounded one by one), then
//   u <- u - [DF; t_row]^-1 (F; t_row . (u - u_pred))
// by the LU with partial pivoting by selects of k_halo_target.  An attempt that does not converge, or whose tangent turns beyond
// cos_min, is tried again from the same u_prev with half the step; after a fast member the step grows.
#include "halo_common.hpp"

namespace lto {

namespace {

__device__ __forceinline__ void swap_if(const bool p, double& u, double& v) {
  const double t = p ? v : u;
  v = p ? u : v;
  u = t;
}

// d = J^-1 r (kernels_halo_target.hip's, kept in step with it).  Returns 1.0 for a singular step -- |det| <= sing_tol x the product
// of the row 2-norms, or det not finite -- else 0.0.
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
        const double xs[6] = {u[0], 0.0, u[1], 0.0, u[2], 0.0};
        double y[12], yc[12];
        halo_start(xs, col, y);
        const double side = (u[2] > 0.0) ? 1.0 : -1.0;
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
        // DF at the crossing: row r of column 2 j of Phi is component 6 + r of lane gbase + j
        double f[12];
        sys.rhs(yc, f);
        const double w3 = f[3] / f[1], w5 = f[5] / f[1];
        double J[3][3], r[3] = {yc[3], yc[5], 0.0}, d[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double p1 = __shfl(yc[7], gbase + j, 64), p3 = __shfl(yc[9], gbase + j, 64), p5 = __shfl(yc[11], gbase + j, 64);
          J[0][j] = __builtin_fma(-w3, p1, p3);
          J[1][j] = __builtin_fma(-w5, p1, p5);
        }
        if (planar) {
          J[0][1] = 0.0;
          J[1][0] = 0.0; J[1][1] = 1.0; J[1][2] = 0.0;
          r[1] = 0.0;
        }
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
        if (store) hist[it] = res;
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
    if (store) {
      double* so = a.state + 6 * m;
      so[0] = fail ? nan : u[0]; so[1] = fail ? nan : 0.0; so[2] = fail ? nan : u[1];
      so[3] = fail ? nan : 0.0; so[4] = fail ? nan : u[2]; so[5] = fail ? nan : 0.0;
      double* to = a.tangent + 3 * m;
      to[0] = fail ? nan : tn[0]; to[1] = fail ? nan : tn[1]; to[2] = fail ? nan : tn[2];
      const double xs[12] = {u[0], 0.0, u[1], 0.0, u[2], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      a.det[m] = fail ? nan : det;
      a.ds[m] = dsa;
      a.period[m] = fail ? nan : 2.0 * tc;
      a.jacobi[m] = fail ? nan : jacobi_constant(MU, xs);
      a.resid[m] = fail ? nan : res;
      a.halvings[m] = halv;
      a.iters[m] = it;
      a.status[m] = (int)status;
      for (int n = nrec; n <= a.max_iter; ++n) hist[n] = nan;
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
  const dim3 grid((unsigned)(((long)a.B * kGroupLanes + 63) / 64));
  if (method == M_RK4) hipLaunchKernelGGL(k_halo_arclength<M_RK4>, grid, dim3(64), 0, st, a);
  else if (method == M_DOP853_ADAPTIVE) hipLaunchKernelGGL(k_halo_arclength<M_DOP853_ADAPTIVE>, grid, dim3(64), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lto
