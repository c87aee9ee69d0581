// kernels_halo_stm.hip -- phase-to-phase state-transition matrices of periodic orbits of the CRTBP, gfx950: what the
// target-point station-keeping law is built from.
//
// k_halo_stm: one GROUP of 8 adjacent lanes per (phase, orbit) record, 8 records per wavefront, exactly k_halo_table's mapping
// (kernels_halo.hip, dop853_lane.hpp): lane c < 6 carries the base state with column c of Phi, lanes 6 and 7 shadow lane 0 with
// colw = 0 and store nothing, a group beyond the last record shadows it.  Per record:
//   1. the coast from state0 over tau_j P to the phase: the six-state system (SysCrtbpDir, crtbp_ballistic.hpp) under the one-lane
//      run_dop853, run redundantly in every lane of the group -- the same instructions on the same data, so all eight lanes hold the
//      same bits afterwards.  A span of 0 calls nothing.
//   2. X_out from lane 0; the columns set to the identity (halo_start).
//   3. the K spans (h_k - h_{k-1}) P under run_dop853_group<SysHaloVar, 6, 6>; after each, every lane stores its column of Phi_k and
//      lane 0 the target point.
// Whatever a group decides it decides from values that are the same bits in all of its lanes (the base state, the group's error
// sums, a group sum of the lanes' finite tests), so a group leaves the span loop as one: the shuffles inside the driver never meet
// a lane that has gone.  The span counter is the same in every lane of a wave that is still in the loop (k_stationkeep_flight's
// rule).  A record without a finite result leaves NaN in all of its outputs.  No LDS, no atomics, plain vector stores; the flags a
// lane sets while it flies (fail, done, bad) are doubles (DESIGN "Compiler hazards"); lead and column are fixed functions of the
// lane's index that only guard stores, as k_halo_table's `store`.
#include "halo_common.hpp"      // SysHaloVar, finite12, halo_start
#include "crtbp_ballistic.hpp"  // SysCrtbpDir, finite_all

namespace lto {

template <int METHOD>
__global__ __launch_bounds__(64) void k_halo_stm(const HaloStmArgs a) {
  const GroupLane<long> L = group_lane<6, 1>((long)a.P * a.B);
  const long rec = L.rec;
  const int b = (int)(rec / a.P), j = (int)(rec - (long)b * a.P);
  const int K = a.K;
  double* Xo = a.X + 6 * rec;
  double* Pc = a.Phi + 36 * (long)K * rec + 6 * L.col;   // this lane's column of block 0
  double* Xt = a.Xt ? a.Xt + 6 * (long)K * rec : nullptr;
  double xs[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) xs[q] = a.state0[6 * (long)b + q];
  const double P = a.period[b];
  double fail = 0.0;
  {
    double s = P;
#pragma unroll
    for (int q = 0; q < 6; ++q) s += xs[q];
    if (!((s - s) == 0.0) || !(P > 0.0)) fail = 1.0;
  }
  int nacc = 0, nrej = 0;
  if (fail == 0.0) {
    SysCrtbpDir dir;
    dir.MU = a.MU;
    dir.sgn = 1.0;
    const double coast = a.tau[j] * P;
    if (METHOD == M_RK4) {
      if (coast > 0.0) {
        const double h = coast / (double)a.steps;
        for (int k = 0; k < a.steps; ++k) rk4_step(dir, h, xs);
        nacc += a.steps;
      }
    } else {
      int na = 0, nr = 0;
      const double done = run_dop853<SysCrtbpDir, 6>(dir, coast, a.rtol, a.atol, a.max_steps, xs, na, nr);
      nacc += na; nrej += nr;
      if (done == 0.0) fail = 1.0;
    }
    if (!finite_all(xs)) fail = 1.0;
  }
  if (fail == 0.0) {
    if (L.lead) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Xo[q] = xs[q];
    }
    SysHaloVar sys;
    sys.MU = a.MU;
    double y[12];
    halo_start(xs, L.col, y);
    double hprev = 0.0;
    for (int k = 0; k < K; ++k) {
      const double hk = a.horizon[k];
      const double span = (hk - hprev) * P;
      hprev = hk;
      double done = 1.0;
      if (METHOD == M_RK4) {
        const double h = span / (double)a.steps;
        for (int s = 0; s < a.steps; ++s) rk4_step(sys, h, y);
        nacc += a.steps;
      } else {
        int na = 0, nr = 0;
        done = run_dop853_group<SysHaloVar, 6, 6>(sys, span, a.rtol, a.atol, a.max_steps, L.colw, y, na, nr,
            [](const double, const double, const double (&)[12], double (&)[13][12], const double (&)[12]) -> double { return 0.0; });
        nacc += na; nrej += nr;
      }
      // one decision for the group: a column that is not finite in any lane fails the record in all of them
      const double bad = group8_sum(finite12(y) ? 0.0 : 1.0);
      if (done == 0.0 || bad != 0.0) { fail = 1.0; break; }
      if (L.column) {
#pragma unroll
        for (int r = 0; r < 6; ++r) Pc[36 * (long)k + r] = y[6 + r];
      }
      if (L.lead && Xt) {
#pragma unroll
        for (int q = 0; q < 6; ++q) Xt[6 * (long)k + q] = y[q];
      }
    }
  }
  if (fail != 0.0) {
    const double nan = __builtin_nan("");
    for (int k = 0; k < K; ++k) {
      if (L.column) {
#pragma unroll
        for (int r = 0; r < 6; ++r) Pc[36 * (long)k + r] = nan;
      }
      if (L.lead && Xt) {
#pragma unroll
        for (int q = 0; q < 6; ++q) Xt[6 * (long)k + q] = nan;
      }
    }
    if (L.lead) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Xo[q] = nan;
    }
  }
  if (L.lead) {
    if (a.accepted) a.accepted[rec] = nacc;
    if (a.rejected) a.rejected[rec] = nrej;
    a.status[rec] = (fail != 0.0) ? 2 : 0;
  }
}

hipError_t launch_halo_stm(int method, const HaloStmArgs& a, hipStream_t st) {
  return launch_by_method(method, k_halo_stm<M_RK4>, k_halo_stm<M_DOP853_ADAPTIVE>, (long)a.P * a.B * kGroupLanes, a, st);
}

}  // namespace lto
