// kernels_halo.hip -- periodic orbits of the CRTBP with the xz-plane symmetry (halo, planar Lyapunov), B orbits side by side
// (DESIGN 4.25), gfx950.
//
// One GROUP of 8 adjacent lanes per orbit, 8 orbits per wavefront (halo_common.hpp group_lane, dop853_lane.hpp).  Lane c < 6 of a
// group integrates the ballistic base state with column c of Phi = dx/dx0 -- 12 components, the gravity gradient formed once per
// stage -- and lanes 6 and 7 shadow lane 0 and store nothing.  The lanes of a group take identical steps (the error norm runs over
// the base and all 36 variational components), and everything a group decides it decides from the base, which every lane carries:
// no lane of a group ever leaves the others.  No LDS, plain vector stores.
//
// k_halo_correct: the differential corrector, the whole Newton loop in the kernel.  Per iteration: the return flight
// (halo_return_rk4, or the same rule under the group driver), then the residual (vx, vz) and the 2 x 2 Jacobian from the columns
// (the position unknown, vy0) of DF (halo_df_column), solved in every lane of the group alike.
//
// k_halo_table: one revolution from (state0, P) with Phi carried through, stopped at t_i = i P / (n - 1), every sample interval a
// span of its own; the samples, M = Phi(P), the closure, the Jacobi constant and its drift, the stability indices.
#include "halo_common.hpp"

namespace lto {

template <int METHOD>
__global__ __launch_bounds__(64) void k_halo_correct(const HaloCorrectArgs a) {
  const GroupLane<int> L = group_lane<6, 1>(a.B);
  const int b = L.rec;
  SysHaloVar sys;
  sys.MU = a.MU;
  double x0 = a.seed[6 * (long)b + 0], z0 = a.seed[6 * (long)b + 2], vy0 = a.seed[6 * (long)b + 4];
  const int iu = (a.mode == LTO_HALO_HOLD_X0) ? 2 : 0;  // the position unknown: x0 (hold z0), z0 (hold x0); planar: none
  const bool planar = a.mode == LTO_HALO_PLANAR;
  double* hist = a.hist + (long)(a.max_iter + 1) * b;

  // per-lane flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler hazards")
  double status = -1.0;
  double tc = 0.0, res = __builtin_nan("");
  int it = 0, nrec = 0;
  {
    const double s = x0 + z0 + vy0;
    if (!((s - s) == 0.0) || vy0 == 0.0 || (planar && z0 != 0.0)) status = 2.0;
  }
  while (status < 0.0) {
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
      (void)run_dop853_group<SysHaloVar, 6, 6>(sys, a.t_max, a.rtol, a.atol, a.max_steps, L.colw, y, na, nr,
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
    res = planar ? fabs(yc[3]) : fmax(fabs(yc[3]), fabs(yc[5]));
    if (L.lead) hist[it] = res;
    nrec = it + 1;
    if (res < a.tol) { status = 0.0; break; }
    if (it >= a.max_iter) { status = 1.0; break; }
    // f at the crossing and the 2 x 2 Jacobian: the columns of DF in the position unknown and in vy0
    double f[12];
    sys.rhs(yc, f);
    const double w3 = f[3] / f[1], w5 = f[5] / f[1];
    double j00, j10, j01, j11, p1;
    halo_df_column(yc, w3, w5, L.gbase, iu, j00, j10, p1);
    halo_df_column(yc, w3, w5, L.gbase, 4, j01, j11, p1);
    if (planar) {
      if (!(fabs(j01) > 0.0) || !((j01 - j01) == 0.0)) { status = 3.0; break; }
      vy0 -= yc[3] / j01;
    } else {
      const double det = j00 * j11 - j01 * j10;
      const double n0 = sqrt(__builtin_fma(j00, j00, j01 * j01)), n1 = sqrt(__builtin_fma(j10, j10, j11 * j11));
      if (!(fabs(det) > a.sing_tol * (n0 * n1)) || !((det - det) == 0.0)) { status = 3.0; break; }
      const double du = (j11 * yc[3] - j01 * yc[5]) / det, dv = (j00 * yc[5] - j10 * yc[3]) / det;
      if (iu == 0) x0 -= du;
      else z0 -= du;
      vy0 -= dv;
    }
    ++it;
  }
  if (L.lead) halo_member_store(a, b, hist, x0, z0, vy0, tc, res, it, nrec, status);
}

hipError_t launch_halo_correct(int method, const HaloCorrectArgs& a, hipStream_t st) {
  return launch_by_method(method, k_halo_correct<M_RK4>, k_halo_correct<M_DOP853_ADAPTIVE>, (long)a.B * kGroupLanes, a, st);
}

template <int METHOD>
__global__ __launch_bounds__(64) void k_halo_table(const HaloTableArgs a) {
  const GroupLane<int> L = group_lane<6, 1>(a.B);
  const int b = L.rec, gbase = L.gbase;
  SysHaloVar sys;
  sys.MU = a.MU;
  double xs[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) xs[q] = a.state0[6 * (long)b + q];
  const double P = a.period[b];
  const int n = a.n;
  double y[12];
  halo_start(xs, L.col, y);
  const double C0 = jacobi_constant(a.MU, y);
  double drift = 0.0;
  double* Xb = a.X + 6 * (long)n * b;
  if (L.lead) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Xb[q] = y[q];
  }
  const double dt = P / (double)(n - 1);
  double tprev = 0.0;
  for (int i = 1; i < n; ++i) {
    const double ti = (i == n - 1) ? P : (double)i * dt;
    const double span = ti - tprev;
    tprev = ti;
    if (METHOD == M_RK4) {
      if (span > 0.0) {
        const double h = span / (double)a.steps;
        for (int k = 0; k < a.steps; ++k) rk4_step(sys, h, y);
      } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) y[q] = __builtin_nan("");
      }
    } else {
      int na = 0, nr = 0;
      const double done = run_dop853_group<SysHaloVar, 6, 6>(sys, span, a.rtol, a.atol, a.max_steps, L.colw, y, na, nr,
          [](const double, const double, const double (&)[12], double (&)[13][12], const double (&)[12]) -> double { return 0.0; });
      if (done == 0.0 || span == 0.0) {           // a period that is not positive has no table
#pragma unroll
        for (int q = 0; q < 12; ++q) y[q] = __builtin_nan("");
      }
    }
    const double dC = fabs(jacobi_constant(a.MU, y) - C0);
    drift = (dC > drift || dC != dC) ? dC : drift;     // a NaN stays
    if (L.lead) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Xb[6 * (long)i + q] = y[q];
    }
  }
  // M = Phi(P): lane j holds column j in y[6..11].  tr M and tr M^2 in a fixed order, in every lane alike.
  double tr = 0.0, tr2 = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    tr += __shfl(y[6 + r], gbase + r, 64);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double mrj = __shfl(y[6 + r], gbase + j, 64), mjr = __shfl(y[6 + j], gbase + r, 64);
      tr2 = __builtin_fma(mrj, mjr, tr2);
    }
  }
  const bool ok = finite12(y) && ((tr2 - tr2) == 0.0);
  if (L.column) {
    double* Mb = a.M + 36 * (long)b + 6 * L.c;
#pragma unroll
    for (int r = 0; r < 6; ++r) Mb[r] = y[6 + r];
  }
  if (L.lead) {
    double cl = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) cl = fmax(cl, fabs(y[q] - xs[q]));
    const double nan = __builtin_nan("");
    a.closure[b] = ok ? cl : nan;
    a.jacobi[2 * (long)b] = C0;
    a.jacobi[2 * (long)b + 1] = drift;
    // alpha = 2 - tr M, beta = (alpha^2 + 2 - tr M^2) / 2, nu = -(alpha +- sqrt(alpha^2 - 4 beta + 8)) / 4
    const double alpha = 2.0 - tr, beta = 0.5 * (alpha * alpha + 2.0 - tr2);
    const double disc = alpha * alpha - 4.0 * beta + 8.0;
    const double root = sqrt(disc);                      // NaN for a negative discriminant
    a.nu[2 * (long)b] = ok ? -0.25 * (alpha + root) : nan;
    a.nu[2 * (long)b + 1] = ok ? -0.25 * (alpha - root) : nan;
    a.status[b] = ok ? 0 : 2;
  }
}

hipError_t launch_halo_table(int method, const HaloTableArgs& a, hipStream_t st) {
  return launch_by_method(method, k_halo_table<M_RK4>, k_halo_table<M_DOP853_ADAPTIVE>, (long)a.B * kGroupLanes, a, st);
}

}  // namespace lto
