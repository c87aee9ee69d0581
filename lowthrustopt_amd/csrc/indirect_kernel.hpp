// indirect_kernel.hpp -- batched propagation of the 12-dim state+costate system and its STM.
//
// Replaces the serial `for i = 1:n_nodes-1` loops of defectCalc / jacobianCalc in
// src/multiShoot_CRTBP_indirect.jl:63-90 / :93-146.  One shooting segment (x one group of STM
// columns) per lane; state, RK stages and STM columns live in VGPRs for the whole integration; HBM is
// touched once on entry (node i, node i+1, t_i, t_{i+1}) and once on exit (defect, Phi), all
// struct-of-arrays so a wavefront moves 512 contiguous bytes per component.
//
// Why columns per lane instead of the whole 12x12 STM: 12 + 144 doubles x 3-4 RK work vectors
// exceeds the 512-VGPR file.  STM columns are independent given the base trajectory
// (Phi_dot = F(y(t)) Phi), so lane (segment s, column group g) re-integrates the cheap base state
// together with COLS columns.  The column group is blockIdx.y, i.e. wave-uniform.
#pragma once
#include <type_traits>
#include "kernels.hpp"
#include "dop853_lane.hpp"

namespace lto {

// ND = 12: the reference's state+costate system.  ND = 14: + mass and mass costate (extension, dynamics.hpp).
template <int ND, int PM, int COLS>
struct SysIndirect {
  static constexpr int DIM = ND + ND * COLS;
  double w2;
  TrajParams tp;
  __device__ __forceinline__ void rhs(const double (&y)[DIM], double (&k)[DIM]) const {
    if constexpr (ND == 12 && COLS == 1) {
      rhs12_fused1<PM>(y, tp, w2, k);
      return;
    }
    if constexpr (ND == 14 && COLS == 1) {
      rhs14_fused1<PM>(y, tp, w2, k);
      return;
    }
    if constexpr (COLS == 0) {     // defect-only sweeps: the lean base RHS of the pipeline kernels (no selects, short exp)
      if constexpr (ND == 12) rhs12_base<PM>(y, tp, k);
      else rhs14_base<PM, true>(y, tp, k);
      return;
    }
    double yb[ND], kb[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) yb[i] = y[i];
    typename std::conditional<ND == 12, VarCoef12, VarCoef14>::type vc;
    if constexpr (ND == 12) rhs12<PM, (COLS > 0)>(yb, tp, kb, vc);
    else rhs14<PM, (COLS > 0)>(yb, tp, kb, vc);
#pragma unroll
    for (int i = 0; i < ND; ++i) k[i] = kb[i];
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
      double c[ND], dc[ND];
#pragma unroll
      for (int i = 0; i < ND; ++i) c[i] = y[ND + ND * j + i];
      if constexpr (ND == 12) var_col12(vc, w2, c, dc);
      else var_col14(vc, w2, c, dc);
#pragma unroll
      for (int i = 0; i < ND; ++i) k[ND + ND * j + i] = dc[i];
    }
  }
};

// The augmented system (y[12], q) of the thrust events (kernels_events.hip) and the guided flight (kernels_guidance.hip): the lean base
// RHS of the defect-only sweeps and of k_indirect_dense, and q' = umag as that RHS forms it.
template <int PM>
struct SysEvents {
  static constexpr int DIM = 13;
  TrajParams tp;
  __device__ __forceinline__ void rhs(const double (&y)[13], double (&k)[13]) const {
    double yb[12], kb[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) yb[i] = y[i];
    rhs12_base<PM>(yb, tp, kb);
#pragma unroll
    for (int i = 0; i < 12; ++i) k[i] = kb[i];
    const double n2 = __builtin_fma(y[9], y[9], __builtin_fma(y[10], y[10], y[11] * y[11]));
    const double inv_n = inv_norm_guarded(n2);
    double m, ua;
    control_base12<PM>(tp, n2 * inv_n, inv_n, m, ua);
    k[12] = m;
  }
};

// The same for the 14-row variable-mass system, (y[14], q) (kernels_events.hip says why the mass is carried as
// m_i + y[6], y[6] = 0 at the span's start).
template <int PM>
struct SysEventsMass {
  static constexpr int DIM = 15;
  TrajParams tp;
  double m_i;
  __device__ __forceinline__ void rhs(const double (&y)[15], double (&k)[15]) const {
    double yb[14], kb[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) yb[i] = y[i];
    yb[6] = m_i + y[6];
    double umag;
    rhs14_base<PM, true>(yb, tp, kb, umag);
#pragma unroll
    for (int i = 0; i < 14; ++i) k[i] = kb[i];
    k[14] = umag;
  }
};

// The augmented system of an ND-row solution: what the thrust events and the guided flight integrate.
template <int ND, int PM>
struct AugmentedSys { using type = SysEvents<PM>; };
template <int PM>
struct AugmentedSys<14, PM> { using type = SysEventsMass<PM>; };

// ode78 (GeneralCode/ode.jl:479-534): h0 = span/50, hmax = span/2.5, hmin = span/1e7; accept when
// delta <= tau = tol max(|x|_inf, 1); h <- min(hmax, 0.8 h (tau/delta)^(1/8)).  Error and |x|_inf run
// over the first NERR components (the base state), so every column lane of a segment takes the same
// step sequence.
template <class Sys, int NERR>
__device__ __forceinline__ void run_rkf78_adaptive(const Sys& sys, const double span, const double tol, const int max_steps,
                                                   double (&y)[Sys::DIM], int& nacc, int& nrej) {
  constexpr int D = Sys::DIM;
  const double hmax = span / 2.5, hmin = span / 1e7;
  double h = span / 50.0, t = 0.0;
  nacc = 0; nrej = 0;
  while (t < span && h >= hmin && nacc + nrej < max_steps) {
    if (t + h > span) h = span - t;
    double yn[D];
    double delta;
    delta = rkf78_step<Sys, NERR, true>(sys, h, y, yn);
    double nx = 0.0;
#pragma unroll
    for (int i = 0; i < NERR; ++i) nx = fmax(nx, fabs(y[i]));
    const double tau = tol * fmax(nx, 1.0);
    if (delta <= tau) {
      t += h;
#pragma unroll
      for (int i = 0; i < D; ++i) y[i] = yn[i];
      ++nacc;
    } else {
      ++nrej;
      if (delta != delta) {                   // NaN step: poison the result instead of returning a partial one
#pragma unroll
        for (int i = 0; i < D; ++i) y[i] = delta;
        t = span;                             // (fmin below would drop the NaN and keep stepping)
      }
    }
    if (delta == 0.0) delta = 1e-16;
    h = fmin(hmax, 0.8 * h * sqrt(sqrt(sqrt(tau / delta))));
  }
  // not at t1 (max_steps used up, ode78's step-size floor ode.jl:479,524, or a decreasing grid: forward integration
  // only): no result -- NaN, never a state at some t < t1 that looks propagated
  if (t < span || !(span >= 0.0)) {           // a NaN span counts as a negative one
#pragma unroll
    for (int i = 0; i < D; ++i) y[i] = __builtin_nan("");
  }
}

// Propagate y over `span` with the plan's integrator (shared by the sweep and the dense-output kernels).
template <class Sys, int ND, int METHOD>
__device__ __forceinline__ void advance(const Sys& sys, const double span, const IndirectArgs& a, double (&y)[Sys::DIM],
                                        int& nacc, int& nrej, double& maxErr) {
  constexpr int D = Sys::DIM;
  if (METHOD == M_RK4) {
    const double h = span / (double)a.steps;
    for (int k = 0; k < a.steps; ++k) rk4_step(sys, h, y);
    nacc += a.steps;
  } else if (METHOD == M_RKF78_FIXED) {
    const double h = span / (double)a.steps;
    for (int k = 0; k < a.steps; ++k) {
      double yn[D];
      double delta;
      delta = rkf78_step<Sys, ND>(sys, h, y, yn);
      maxErr = fmax(maxErr, delta);
#pragma unroll
      for (int c = 0; c < D; ++c) y[c] = yn[c];
    }
    nacc += a.steps;
  } else if (METHOD == M_RKF78_ADAPTIVE) {
    int na = 0, nr = 0;
    run_rkf78_adaptive<Sys, ND>(sys, span, a.rtol, a.max_steps, y, na, nr);
    nacc += na; nrej += nr;
  } else {
    int na = 0, nr = 0;
    run_dop853<Sys, D>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr);
    nacc += na; nrej += nr;
  }
}

// Dense output (replaces the per-segment re-propagation of densify, src/HelperFunctions.jl:51-101):
// lane = segment; the segment's sample times are td[first[s] .. first[s+1]) (sorted, inside [t_i, t_{i+1})); the
// lane integrates from sample to sample and stores the state at each one.  The reference evaluates Vern8's
// interpolant at those times; stepping exactly onto them is at least as accurate.  If `final_state` is set the
// last segment of each trajectory also stores x(t_n) (the `sol_forward[:,end]` column densify appends, :94-97).
template <int ND, int PM, int METHOD>
__global__ __launch_bounds__(64) void k_indirect_dense(const IndirectArgs a, const DenseArgs d) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.S) return;
  const int traj = s / a.seg_per_traj;
  const int i = s - traj * a.seg_per_traj;
  const long node = (long)traj * a.n_nodes + i;
  const long tg = (long)traj * a.t_stride + i;
  using Sys = SysIndirect<ND, PM, 0>;
  Sys sys;
  sys.tp = a.tp[(long)traj * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;
  sys.w2 = 2.0 * sys.tp.omega;
  double y[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c) y[c] = a.X[c * a.ldx + node];
  double tcur = a.t[tg];
  int nacc = 0, nrej = 0;
  double maxErr = 0.0;
  const int j0 = d.first[s], j1 = d.first[s + 1];
  for (int j = j0; j < j1; ++j) {
    const double ts = d.td[j];
    if (ts > tcur) { advance<Sys, ND, METHOD>(sys, ts - tcur, a, y, nacc, nrej, maxErr); tcur = ts; }
#pragma unroll
    for (int c = 0; c < ND; ++c) d.Y[c * d.ldy + j] = y[c];
  }
  if (d.final_state && i == a.seg_per_traj - 1) {
    const double te = a.t[tg + 1];
    if (te > tcur) advance<Sys, ND, METHOD>(sys, te - tcur, a, y, nacc, nrej, maxErr);
#pragma unroll
    for (int c = 0; c < ND; ++c) d.final_state[c * (a.S / a.seg_per_traj) + traj] = y[c];
  }
}

// COLS = 0: defect only (K1).  COLS >= 1: lane integrates base + COLS STM columns (K2); the
// column group is blockIdx.y and the g = 0 lanes also emit the defect.
template <int ND, int PM, int METHOD, int COLS>
__global__ __launch_bounds__(64) void k_indirect(const IndirectArgs a) {
  const int sl = xcd_unit(a, blockIdx.x, gridDim.x) * 64 + threadIdx.x;   // an XCD's wavefronts own a contiguous range of segments (kernels.hpp)
  if (sl >= a.S) return;
  const int s = a.order ? a.order[sl] : sl;    // balanced order: neighbouring lanes take similar numbers of steps
  const int g = blockIdx.y;
  const int traj = s / a.seg_per_traj;
  const int i = s - traj * a.seg_per_traj;
  const long node = (long)traj * a.n_nodes + i;
  const long tg = (long)traj * a.t_stride + i;
  const double span = a.t[tg + 1] - a.t[tg];

  using Sys = SysIndirect<ND, PM, COLS>;
  constexpr int D = Sys::DIM;
  Sys sys;
  sys.tp = a.tp[(long)traj * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;   // mixed-class batch: another launch owns this trajectory
  sys.w2 = 2.0 * sys.tp.omega;

  double y[D];
#pragma unroll
  for (int c = 0; c < ND; ++c) y[c] = a.X[c * a.ldx + node];
#pragma unroll
  for (int j = 0; j < COLS; ++j)
#pragma unroll
    for (int r = 0; r < ND; ++r) y[ND + ND * j + r] = (r == g * COLS + j) ? 1.0 : 0.0;

  double maxErr = 0.0;
  int nacc = 0, nrej = 0;
  advance<Sys, ND, METHOD>(sys, span, a, y, nacc, nrej, maxErr);

  if (COLS > 0) {
#pragma unroll
    for (int j = 0; j < COLS; ++j)
#pragma unroll
      for (int r = 0; r < ND; ++r) a.Phi[(long)((g * COLS + j) * ND + r) * a.ldp + s] = y[ND + ND * j + r];
  }
  if (g == 0) {
    if (a.defect) {
#pragma unroll
      for (int c = 0; c < ND; ++c) a.defect[c * a.ldd + s] = y[c] - a.X[c * a.ldx + node + 1];
    }
    if (a.errors) a.errors[s] = maxErr;
    if (a.nacc) a.nacc[s] = nacc;
    if (a.nrej) a.nrej[s] = nrej;
  }
}

template <int ND, int PM, int METHOD, int COLS>
static hipError_t launch_one(const IndirectArgs& a, hipStream_t st) {
  dim3 grid((a.S + 63) / 64, COLS > 0 ? ND / COLS : 1);
  hipLaunchKernelGGL((k_indirect<ND, PM, METHOD, COLS>), grid, dim3(64), 0, st, a);
  return hipGetLastError();
}

// One launch per control-law class present in `pm` (kernels.hpp for_classes).

template <int ND, int METHOD>
static hipError_t launch_dense_pm(int pm, const IndirectArgs& a0, const DenseArgs& d, hipStream_t st) {
  dim3 grid((a0.S + 63) / 64);
  // every class is launched and the error state read once, behind the last launch
  (void)for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) {
    hipLaunchKernelGGL((k_indirect_dense<ND, decltype(cls)::value, METHOD>), grid, dim3(64), 0, st, a, d);
    return hipSuccess;
  });
  return hipGetLastError();
}

template <int ND, int METHOD, int COLS>
static hipError_t launch_pm(int pm, const IndirectArgs& a0, hipStream_t st) {
  return for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) { return launch_one<ND, decltype(cls)::value, METHOD, COLS>(a, st); });
}

// The per-lane family of one dimension: <12> is defined in kernels_indirect.hip, <14> in kernels_indirect14.hip (two translation
// units for compile time); launch_indirect_defect / launch_indirect_stm (kernels_indirect.hip) switch on ndim.
template <int ND> hipError_t launch_defect_nd(int pm, int method, const IndirectArgs& a, hipStream_t st);
template <int ND> hipError_t launch_stm_nd(int pm, int method, int cols, const IndirectArgs& a, hipStream_t st);
template <> hipError_t launch_defect_nd<12>(int pm, int method, const IndirectArgs& a, hipStream_t st);
template <> hipError_t launch_defect_nd<14>(int pm, int method, const IndirectArgs& a, hipStream_t st);
template <> hipError_t launch_stm_nd<12>(int pm, int method, int cols, const IndirectArgs& a, hipStream_t st);
template <> hipError_t launch_stm_nd<14>(int pm, int method, int cols, const IndirectArgs& a, hipStream_t st);
// dense output of the 14-row system (kernels_indirect14.hip)
hipError_t launch_dense14(int pm, int method, const IndirectArgs& a, const DenseArgs& d, hipStream_t st);

}  // namespace lto
