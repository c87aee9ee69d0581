// dop853_lane.hpp -- the adaptive DOP853 driver of every kernel that flies a trajectory in a lane (DESIGN.md 'Integrators'): one
// body, dop853_drive, and its three bindings run_dop853, run_dop853_stop and run_dop853_group.  Device code that also compiles for
// the host (tests/host_stub): it includes rk.hpp and nothing else of the project.
//
// Initial step by Hairer's d0/d1/d2 rule, trial step dop853_try, decision dp8_decide (accept if err < 1, factor
// min(10, 0.9 err^(-1/8)), at most 1 straight after a rejection; rejection factor max(0.2, 0.9 err^(-1/8))), FSAL hand-over.
//
// The error norm.  NCOL = 0: the first NB components of the lane.  NCOL > 0, the GROUP form: kGroupLanes = 8 adjacent lanes of a
// wavefront integrate one trajectory together, every lane carries the NB base components and its own column of the variational
// matrix (Sys::DIM - NB more components), and all lanes of the group must take identical steps.  The error sums therefore run over
// the base -- once -- and over the columns of the group's lanes, closed by a butterfly inside the group before dp8_decide.  A lane
// whose column weight `colw` is 0 shadows another lane of its group (its column is counted by that lane) and adds nothing; NCOL is
// the number of lanes with colw = 1.  The butterfly adds the same pairs in every lane, so the sums -- and with them the step
// sequence -- are the same bits in all eight.
//
// The hook.  After every ACCEPTED step, before it is taken over,
//   stop = hook(t, h, y, K, yn)        y = the state at t (relative to the span's start), K[0] = f(y), yn = the state at t + h
// may run further trial steps from y through K (dop853_try leaves y and K[0] alone and overwrites K[1..12]; the new state's slope
// is kept aside for it) and ends the flight with a non-zero return value, the state left at the step's start.  With NoHook nothing
// is kept aside and nothing is called.
//
// Returns 1.0 at t = span, 2.0 when the hook stopped the flight, 0.0 without a result: max_steps trial steps used up, a NaN step
// (counted as a rejection; it never recovers, so the loop ends there), a negative or NaN span -- the state is then NaN in every
// component, never a state at some t < span that looks propagated.  A span of 0 returns 1.0 and calls nothing.
#pragma once
#include "rk.hpp"

namespace lto {

constexpr int kGroupLanes = 8;

struct NoHook {};

// x^(1/9) without pow()
__device__ __forceinline__ double pow_9th(double x) { return cbrt(cbrt(x)); }

// the sum of v over the 8 lanes of the caller's group, the same bits in every one of them
__device__ __forceinline__ double group8_sum(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

// The two error sums of a trial step over the components [NB, DIM), as dop853_try forms them over [0, NERR).
template <class Sys, int NB>
__device__ __forceinline__ void dp8_tail_err(const double rtol, const double atol, const double (&y)[Sys::DIM],
                                             const double (&K)[13][Sys::DIM], const double (&ynew)[Sys::DIM], double& E5, double& E3) {
  double e5 = 0.0, e3 = 0.0;
#pragma unroll
  for (int i = NB; i < Sys::DIM; ++i) {
    double a5 = 0.0, a3 = 0.0;
#pragma unroll
    for (int k = 0; k <= DP8_NSTAGES; ++k) {
      if (DP8_E5[k] != 0.0) a5 = __builtin_fma(DP8_E5[k], K[k][i], a5);
      if (DP8_E3[k] != 0.0) a3 = __builtin_fma(DP8_E3[k], K[k][i], a3);
    }
    const double inv_sc = rcp_nr(__builtin_fma(rtol, fmax(fabs(y[i]), fabs(ynew[i])), atol));
    a5 *= inv_sc; a3 *= inv_sc;
    e5 = __builtin_fma(a5, a5, e5);
    e3 = __builtin_fma(a3, a3, e3);
  }
  E5 = e5; E3 = e3;
}

template <class Sys, int NB, int NCOL, class Hook>
__device__ __forceinline__ double dop853_drive(const Sys& sys, const double span, const double rtol, const double atol,
                                               const int max_steps, const double colw, double (&y)[Sys::DIM], int& nacc, int& nrej,
                                               Hook&& hook) {
  constexpr int D = Sys::DIM;
  constexpr bool GROUP = NCOL > 0;
  constexpr bool HOOKED = !std::is_same<typename std::decay<Hook>::type, NoHook>::value;
  constexpr int NSUM = GROUP ? D : NB;                    // the components this lane forms error terms of
  constexpr double NCOMP = (double)(NB + NCOL * (D - NB));
  static_assert(NB <= D, "the error norm runs over the system's own components");
  double K[13][D];
  nacc = 0; nrej = 0;
  if (!(span > 0.0)) {
    if (span != 0.0) {     // decreasing grid (forward integration only) or NaN span: no result
#pragma unroll
      for (int i = 0; i < D; ++i) y[i] = __builtin_nan("");
      return 0.0;
    }
    return 1.0;
  }
  sys.rhs(y, K[0]);
  double h_abs;
  {
    double b0 = 0.0, b1 = 0.0, c0 = 0.0, c1 = 0.0;
#pragma unroll
    for (int i = 0; i < NSUM; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      if (i < NB) { b0 = __builtin_fma(y[i] * isc, y[i] * isc, b0); b1 = __builtin_fma(K[0][i] * isc, K[0][i] * isc, b1); }
      else { c0 = __builtin_fma(y[i] * isc, y[i] * isc, c0); c1 = __builtin_fma(K[0][i] * isc, K[0][i] * isc, c1); }
    }
    double d0 = b0, d1 = b1;
    if constexpr (GROUP) { d0 += group8_sum(colw != 0.0 ? c0 : 0.0); d1 += group8_sum(colw != 0.0 ? c1 : 0.0); }
    d0 = sqrt(d0 / NCOMP); d1 = sqrt(d1 / NCOMP);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double yt[D];
#pragma unroll
    for (int i = 0; i < D; ++i) yt[i] = __builtin_fma(h0, K[0][i], y[i]);
    sys.rhs(yt, K[1]);
    double b2 = 0.0, c2 = 0.0;
#pragma unroll
    for (int i = 0; i < NSUM; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      const double df = (K[1][i] - K[0][i]) * isc;
      if (i < NB) b2 = __builtin_fma(df, df, b2);
      else c2 = __builtin_fma(df, df, c2);
    }
    double d2 = b2;
    if constexpr (GROUP) d2 += group8_sum(colw != 0.0 ? c2 : 0.0);
    d2 = sqrt(d2 / NCOMP) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow_9th(0.01 / fmax(d1, d2));
    h_abs = fmin(fmin(100.0 * h0, h1), span);
  }
  double t = 0.0;
  // Flags are kept as per-lane doubles, not bools: hipcc 7.2 turns per-lane booleans that stay live across these
  // spill-heavy bodies into SGPR lane masks that are spilled/reloaded, and a 14-dim kernel returned garbage that
  // way (DESIGN.md "Compiler hazards").
  double rejected = 0.0, stopped = 0.0, failed = 0.0;
  while (t < span && nacc + nrej < max_steps) {
    double h = h_abs;
    double last = 0.0;
    if (t + h >= span) { h = span - t; last = 1.0; }
    double yn[D];
    double E5, E3;
    (void)dop853_try<Sys, NB>(sys, h, rtol, atol, y, K, yn, E5, E3);
    if constexpr (GROUP) {
      double C5, C3;
      dp8_tail_err<Sys, NB>(rtol, atol, y, K, yn, C5, C3);
      E5 += group8_sum(colw != 0.0 ? C5 : 0.0); E3 += group8_sum(colw != 0.0 ? C3 : 0.0);
    }
    // the step decision every DOP853 kernel of this library takes (rk.hpp dp8_decide): the one- / two- / four-lane defect sweeps
    // AUTO switches between share one controller
    double h_next, accept, bad;
    dp8_decide(E5, E3, h, rejected, NCOMP, h_next, accept, bad);
    h_abs = h_next;
    if (accept != 0.0) {
      double fn[D];                               // with a hook: the new state's slope, kept aside from its trial steps
      if constexpr (HOOKED) {
#pragma unroll
        for (int i = 0; i < D; ++i) fn[i] = K[12][i];
        stopped = hook(t, h, y, K, yn);
        if (stopped != 0.0) break;
      }
      t = (last != 0.0) ? span : t + h;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        y[i] = yn[i];
        if constexpr (HOOKED) K[0][i] = fn[i];
        else K[0][i] = K[12][i];
      }
      ++nacc;
      rejected = 0.0;
    } else {
      rejected = 1.0;
      ++nrej;
      // A NaN never recovers: no result, instead of max_steps retries.  With a hook the loop is left here and the ending below
      // writes the NaN (t < span); without one the NaN is written here and the loop ends through its condition.  One result, two
      // ways there: each is what its callers' kernels were compiled from before the drivers became one body, and either way
      // alone moves the other's instruction streams (profiles/dop853_driver_kernel_resources.txt).
      if (bad != 0.0) {
        if constexpr (HOOKED) break;
#pragma unroll
        for (int i = 0; i < D; ++i) y[i] = bad;
        t = span;
        failed = 1.0;
      }
    }
  }
  if (stopped != 0.0) return 2.0;
  if (t < span) {                                 // max_steps trial steps used up before the span's end, or a NaN step
#pragma unroll
    for (int i = 0; i < D; ++i) y[i] = __builtin_nan("");
    return 0.0;
  }
  return (failed != 0.0) ? 0.0 : 1.0;
}

// One lane per trajectory, the first NERR components in the error norm.
template <class Sys, int NERR>
__device__ __forceinline__ double run_dop853(const Sys& sys, const double span, const double rtol, const double atol,
                                             const int max_steps, double (&y)[Sys::DIM], int& nacc, int& nrej) {
  return dop853_drive<Sys, NERR, 0>(sys, span, rtol, atol, max_steps, 0.0, y, nacc, nrej, NoHook{});
}

template <class Sys, int NERR, class Hook>
__device__ __forceinline__ double run_dop853_stop(const Sys& sys, const double span, const double rtol, const double atol,
                                                  const int max_steps, double (&y)[Sys::DIM], int& nacc, int& nrej, Hook&& hook) {
  return dop853_drive<Sys, NERR, 0>(sys, span, rtol, atol, max_steps, 0.0, y, nacc, nrej, hook);
}

// Eight lanes per trajectory: NB base components, NCOL columns of Sys::DIM - NB components between the group's lanes.
template <class Sys, int NB, int NCOL, class Hook>
__device__ __forceinline__ double run_dop853_group(const Sys& sys, const double span, const double rtol, const double atol,
                                                   const int max_steps, const double colw, double (&y)[Sys::DIM], int& nacc, int& nrej,
                                                   Hook&& hook) {
  static_assert(NCOL > 0, "the group form carries columns");
  return dop853_drive<Sys, NB, NCOL>(sys, span, rtol, atol, max_steps, colw, y, nacc, nrej, hook);
}

}  // namespace lto
