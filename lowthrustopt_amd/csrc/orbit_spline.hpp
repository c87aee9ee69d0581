// orbit_spline.hpp -- the natural cubic spline of an orbit table on the device (EndOrbitsDev, kernels.hpp): interpEndStates
// (direct.jl:434-461) for the free-end step (kernels_direct_qp.hip) and find_tau (HelperFunctions.jl:38-48) for the time-of-flight
// change (kernels_addtime.hip).  One definition, so both read the same bits off a table.
#pragma once
#include "kernels.hpp"

namespace lto {

// table e (0 departure, 1 arrival), component j, at normalised time x wrapped into [0, 1] as the reference does
__device__ inline double end_spline(const EndOrbitsDev& o, const int e, const int j, double x) {
  int guard = 0;                                   // the reference's wrap (:438-449); a non-finite or absurd tau gives NaN
  if (!(fabs(x) < 1e6)) return __builtin_nan("");
  while (x > 1.0 && guard++ < 2000000) x -= 1.0;
  while (x < 0.0 && guard++ < 2000000) x += 1.0;
  const int n = o.n[e];
  const double* t = o.t[e];
  const double* Y = o.Y[e];
  const double* M = o.M[e];
  int lo = 0, hi = n - 1;                          // the last i with t[i] <= x, clipped to [0, n-2]
  if (x < t[0]) hi = 0;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (t[mid] <= x) lo = mid; else hi = mid;
  }
  const int i = lo < n - 2 ? lo : n - 2;
  const double h = t[i + 1] - t[i], a = t[i + 1] - x, b = x - t[i];
  const double Mi = M[j + 6 * i], Mj = M[j + 6 * (i + 1)];
  return (Mi * a * a * a + Mj * b * b * b) / (6.0 * h) + (Y[j + 6 * i] - Mi * h * h / 6.0) * a / h +
         (Y[j + 6 * (i + 1)] - Mj * h * h / 6.0) * b / h;
}
}  // namespace lto
