// What the periodic-orbit correctors share (lowthrustopt_amd/csrc/halo_common.hpp) compiled for the host, one lane: the 3 x 3 Newton
// solve with its planar patch and the RK4 return flight, for tests/test_host_halo_common.py.  The adaptive flight needs the group's
// shuffles and stays with the GPU suite.
#include "halo_common.hpp"
using namespace lto;

// J row-major [3][3]; planar != 0: the patch first, J and r as patched come back.  Returns newton_solve3's flag.
extern "C" double chk_newton_solve3(double* J9, double* r3, int planar, double sing_tol, double* d3) {
  double J[3][3], r[3], d[3];
  for (int i = 0; i < 3; ++i) { r[i] = r3[i]; for (int j = 0; j < 3; ++j) J[i][j] = J9[3 * i + j]; }
  if (planar) { halo_planar_patch(J, r); J[2][1] = 0.0; }   // as k_halo_target: the third row is the caller's
  const double flag = newton_solve3(J, r, sing_tol, d);
  for (int i = 0; i < 3; ++i) { r3[i] = r[i]; d3[i] = d[i]; for (int j = 0; j < 3; ++j) J9[3 * i + j] = J[i][j]; }
  return flag;
}

// halo_return_rk4 from (x0, 0, z0, 0, vy0, 0) with column col.  tc_yc: tc, then yc[12] (all NaN when nothing was found).
// before[12]: the state one RK4 step of length th_before from the start of the step that crossed -- the whole steps before tc flown
// again here -- for th_before = shrink x (tc - the step's start).
extern "C" double chk_halo_return_rk4(double mu, double x0, double z0, double vy0, int col, double t_max, int steps, double shrink,
                                      double* tc_yc, double* before) {
  SysHaloVar sys;
  sys.MU = mu;
  double tc = __builtin_nan(""), yc[12];
  struct { double t_max; int steps; } a = {t_max, steps};
  const double found = halo_return_rk4(sys, x0, z0, vy0, col, a, tc, yc);
  tc_yc[0] = tc;
  for (int i = 0; i < 12; ++i) { tc_yc[1 + i] = (found != 0.0) ? yc[i] : __builtin_nan(""); before[i] = __builtin_nan(""); }
  if (found != 0.0) {
    const double h = t_max / (double)steps;
    const double xs[6] = {x0, 0.0, z0, 0.0, vy0, 0.0};
    double y[12];
    halo_start(xs, col, y);
    int k = 0;
    while ((double)(k + 1) * h < tc) { rk4_step(sys, h, y); ++k; }
    rk4_step(sys, shrink * (tc - (double)k * h), y);
    for (int i = 0; i < 12; ++i) before[i] = y[i];
  }
  return found;
}
