// dop853_group.hpp -- the group form of the adaptive DOP853 driver (gfx950 device code).
//
// A GROUP is 8 adjacent lanes of a wavefront that integrate one trajectory together: every lane carries the NB base components and
// its own column of the variational matrix (Sys::DIM - NB more components), and all lanes of the group must take identical steps.
// The error sums of a trial step therefore run over the base -- once -- and over the columns of all the group's lanes, closed by
// a butterfly inside the group (__shfl_xor 1, 2, 4) before dp8_decide.  A lane whose column weight `colw` is 0 shadows another
// lane of its group (its column is counted by that lane) and adds nothing.  The butterfly adds the same pairs in every lane, so
// the sums -- and with them the step sequence -- are the same bits in all eight.
//
// The start (Hairer's d0/d1/d2 rule), the trial step (dop853_try) and the decision (dp8_decide) are those of run_dop853 and
// run_dop853_stepping (indirect_kernel.hpp), which keep their code; only the error norm is wider.  After every accepted step
//   stop = hook(t, h, y, K, yn)        y = the state at t, K[0] = f(y), yn = the state at t + h
// may run further trial steps from y through K (dop853_try leaves y and K[0] alone) and ends the integration with a non-zero
// return value, the state left at the step's start.  Returns 1.0 at t = span, 2.0 when the hook stopped it, 0.0 without a result
// (max_steps used up, a NaN, a span that is not positive: the state is NaN).  Flags are doubles (run_dop853's comment).
#pragma once
#include "indirect_kernel.hpp"

namespace lto {

constexpr int kGroupLanes = 8;

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

// NCOL: the columns a group carries between its lanes (the lanes with colw = 1)
template <class Sys, int NB, int NCOL, class Hook>
__device__ __forceinline__ double run_dop853_group(const Sys& sys, const double span, const double rtol, const double atol,
                                                   const int max_steps, const double colw, double (&y)[Sys::DIM], int& nacc, int& nrej,
                                                   Hook&& hook) {
  constexpr int D = Sys::DIM;
  constexpr double NCOMP = (double)(NB + NCOL * (D - NB));
  double K[13][D];
  nacc = 0; nrej = 0;
  if (!(span > 0.0)) {
    if (span != 0.0) {
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
    for (int i = 0; i < D; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      if (i < NB) { b0 = __builtin_fma(y[i] * isc, y[i] * isc, b0); b1 = __builtin_fma(K[0][i] * isc, K[0][i] * isc, b1); }
      else { c0 = __builtin_fma(y[i] * isc, y[i] * isc, c0); c1 = __builtin_fma(K[0][i] * isc, K[0][i] * isc, c1); }
    }
    double d0 = b0 + group8_sum(colw != 0.0 ? c0 : 0.0), d1 = b1 + group8_sum(colw != 0.0 ? c1 : 0.0);
    d0 = sqrt(d0 / NCOMP); d1 = sqrt(d1 / NCOMP);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double yt[D];
#pragma unroll
    for (int i = 0; i < D; ++i) yt[i] = __builtin_fma(h0, K[0][i], y[i]);
    sys.rhs(yt, K[1]);
    double b2 = 0.0, c2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      const double df = (K[1][i] - K[0][i]) * isc;
      if (i < NB) b2 = __builtin_fma(df, df, b2);
      else c2 = __builtin_fma(df, df, c2);
    }
    double d2 = b2 + group8_sum(colw != 0.0 ? c2 : 0.0);
    d2 = sqrt(d2 / NCOMP) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow_9th(0.01 / fmax(d1, d2));
    h_abs = fmin(fmin(100.0 * h0, h1), span);
  }
  double t = 0.0;
  double rejected = 0.0, stopped = 0.0;
  while (t < span && nacc + nrej < max_steps) {
    double h = h_abs;
    double last = 0.0;
    if (t + h >= span) { h = span - t; last = 1.0; }
    double yn[D];
    double B5, B3, C5, C3;
    (void)dop853_try<Sys, NB>(sys, h, rtol, atol, y, K, yn, B5, B3);
    dp8_tail_err<Sys, NB>(rtol, atol, y, K, yn, C5, C3);
    const double E5 = B5 + group8_sum(colw != 0.0 ? C5 : 0.0), E3 = B3 + group8_sum(colw != 0.0 ? C3 : 0.0);
    double h_next, accept, bad;
    dp8_decide(E5, E3, h, rejected, NCOMP, h_next, accept, bad);
    h_abs = h_next;
    if (accept != 0.0) {
      double fn[D];
#pragma unroll
      for (int i = 0; i < D; ++i) fn[i] = K[12][i];
      stopped = hook(t, h, y, K, yn);
      if (stopped != 0.0) break;
      t = (last != 0.0) ? span : t + h;
#pragma unroll
      for (int i = 0; i < D; ++i) { y[i] = yn[i]; K[0][i] = fn[i]; }
      ++nacc;
      rejected = 0.0;
    } else {
      rejected = 1.0;
      ++nrej;
      if (bad != 0.0) break;                    // a NaN never recovers
    }
  }
  if (stopped != 0.0) return 2.0;
  if (t < span) {
#pragma unroll
    for (int i = 0; i < D; ++i) y[i] = __builtin_nan("");
    return 0.0;
  }
  return 1.0;
}

}  // namespace lto
