// dop853_stop.hpp -- the stepping form of the adaptive DOP853 driver with a hook that can end the flight (gfx950 device code;
// DESIGN 4.26), one lane per trajectory.
//
// The start (Hairer's d0/d1/d2 rule), the trial step (dop853_try) and the decision (dp8_decide) are those of run_dop853 and
// run_dop853_stepping (indirect_kernel.hpp), which keep their code; the hook has the shape of run_dop853_group's
// (dop853_group.hpp).  After every ACCEPTED step
//   stop = hook(t, h, y, K, yn)        y = the state at t (relative to the span's start), K[0] = f(y), yn = the state at t + h
// may run further trial steps from y through K (dop853_try leaves y and K[0] alone and overwrites K[1..12]; the new state's slope
// is kept aside) and ends the integration with a non-zero return value, the state left at the step's start.
// Returns 1.0 at t = span, 2.0 when the hook stopped it, 0.0 without a result (max_steps trial steps used up, a NaN, a span that is
// not positive: the state is NaN); a span of 0 returns 1.0 and calls nothing.  Flags are doubles (run_dop853's comment).
#pragma once
#include "indirect_kernel.hpp"

namespace lto {

template <class Sys, int NERR, class Hook>
__device__ __forceinline__ double run_dop853_stop(const Sys& sys, const double span, const double rtol, const double atol,
                                                  const int max_steps, double (&y)[Sys::DIM], int& nacc, int& nrej, Hook&& hook) {
  constexpr int D = Sys::DIM;
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
    double d0 = 0.0, d1 = 0.0;
#pragma unroll
    for (int i = 0; i < NERR; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      d0 = __builtin_fma(y[i] * isc, y[i] * isc, d0);
      d1 = __builtin_fma(K[0][i] * isc, K[0][i] * isc, d1);
    }
    d0 = sqrt(d0 / NERR); d1 = sqrt(d1 / NERR);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double yt[D];
#pragma unroll
    for (int i = 0; i < D; ++i) yt[i] = __builtin_fma(h0, K[0][i], y[i]);
    sys.rhs(yt, K[1]);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < NERR; ++i) {
      const double isc = rcp_nr(__builtin_fma(rtol, fabs(y[i]), atol));
      const double df = (K[1][i] - K[0][i]) * isc;
      d2 = __builtin_fma(df, df, d2);
    }
    d2 = sqrt(d2 / NERR) / h0;
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
    double E5, E3;
    (void)dop853_try<Sys, NERR>(sys, h, rtol, atol, y, K, yn, E5, E3);
    double h_next, accept, bad;
    dp8_decide(E5, E3, h, rejected, (double)NERR, h_next, accept, bad);
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
