// The adaptive DOP853 lane driver (lowthrustopt_amd/csrc/dop853_lane.hpp) compiled for the host: one flight of the ballistic CRTBP
// per call, for tests/test_host_dop853.py.
#include "dop853_lane.hpp"
using namespace lto;

// The expressions of SysCrtbpDir (crtbp_ballistic.hpp) with sgn = 1, and a count of the calls.
struct SysCheck {
  static constexpr int DIM = 6;
  double MU;
  mutable long calls = 0;
  void rhs(const double (&y)[6], double (&k)[6]) const {
    ++calls;
    const double x = y[0], yy = y[1], z = y[2];
    const double a = x + MU, b = a - 1.0;
    const double yz2 = __builtin_fma(yy, yy, z * z);
    const double d1 = __builtin_fma(a, a, yz2), d2 = __builtin_fma(b, b, yz2);
    const double i1 = rsqrt_nr(d1), i2 = rsqrt_nr(d2);
    const double c1 = (1.0 - MU) * (i1 * i1 * i1), c2 = MU * (i2 * i2 * i2);
    const double cs = c1 + c2;
    k[0] = y[3]; k[1] = y[4]; k[2] = y[5];
    k[3] = __builtin_fma(-c1, a, __builtin_fma(-c2, b, __builtin_fma(2.0, y[4], x)));
    k[4] = __builtin_fma(-cs, yy, __builtin_fma(-2.0, y[3], yy));
    k[5] = -cs * z;
  }
};

// counts: nacc, nrej, calls of rhs
extern "C" double chk_dop853_plain(const double* y0, double mu, double span, double tol, int max_steps, double* y_out, long* counts) {
  SysCheck sys;
  sys.MU = mu;
  double y[6];
  for (int i = 0; i < 6; ++i) y[i] = y0[i];
  int na = -1, nr = -1;
  const double ret = run_dop853<SysCheck, 6>(sys, span, tol, tol, max_steps, y, na, nr);
  for (int i = 0; i < 6; ++i) y_out[i] = y[i];
  counts[0] = na; counts[1] = nr; counts[2] = sys.calls;
  return ret;
}

// The same flight under run_dop853_stop.  The hook records (t, h, y[6], yn[6]) of call k in rec[14 k ..], up to max_rec calls, and
// returns non-zero at its stop_at-th call (1-based; 0: never).  counts[3]: calls of the hook.
extern "C" double chk_dop853_hooked(const double* y0, double mu, double span, double tol, int max_steps, int stop_at, double* y_out,
                                    long* counts, double* rec, int max_rec) {
  SysCheck sys;
  sys.MU = mu;
  double y[6];
  for (int i = 0; i < 6; ++i) y[i] = y0[i];
  int na = -1, nr = -1;
  long hooks = 0;
  const double ret = run_dop853_stop<SysCheck, 6>(sys, span, tol, tol, max_steps, y, na, nr,
                                                  [&](const double t, const double h, const double (&ys)[6], double (&K)[13][6], const double (&yn)[6]) {
    if (hooks < max_rec) {
      double* r = rec + 14 * hooks;
      r[0] = t; r[1] = h;
      for (int i = 0; i < 6; ++i) { r[2 + i] = ys[i]; r[8 + i] = yn[i]; }
    }
    ++hooks;
    (void)K;
    return (hooks == stop_at) ? 1.0 : 0.0;
  });
  for (int i = 0; i < 6; ++i) y_out[i] = y[i];
  counts[0] = na; counts[1] = nr; counts[2] = sys.calls; counts[3] = hooks;
  return ret;
}
