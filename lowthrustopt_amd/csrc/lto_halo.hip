// lto_halo.hip -- periodic orbits with the xz-plane symmetry for a batch of seeds: the differential corrector and the orbit table
// with its monodromy matrix and stability indices.
#include <cmath>
#include <cstring>

#include "lto_host.hpp"

// what the flying calls of this unit and of lto_manifold.hip ask of the integrator: 0, or the error code with the context's message set
int halo_integrator_check(lto_ctx* c, const lto_integrator* integ, const char* unsupported, const char* steps) {
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE) return set_err(c, LTO_EUNSUPPORTED, unsupported);
  if (integ->method == LTO_RK4 && integ->steps < 1) return set_err(c, LTO_EINVAL, steps);
  return LTO_OK;
}

extern "C" {

/* The differential corrector for n_batch seeds side by side: one upload, one launch (k_halo_correct runs every orbit's Newton loop
 * to its end), the results come down behind it. */
int lto_halo_correct_batch(lto_ctx* c, int n_batch, double MU, int mode, const double* seeds, double tol, int max_iter, double t_max,
                           double sing_tol, const lto_integrator* integ, double* state_out, double* period_out, double* resid_out,
                           int* iterations, double* history, int* status) {
  if (!c) return LTO_ENULL;
  if (n_batch < 1 || max_iter < 0 || !(tol > 0.0))
    return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: need n_batch >= 1, max_iter >= 0 and tol > 0");
  if (!seeds || !integ || !state_out || !period_out || !status)
    return set_err(c, LTO_ENULL, "lto_halo_correct_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_correct_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_halo_correct_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (mode < LTO_HALO_HOLD_Z0 || mode > LTO_HALO_PLANAR) return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: mode must be LTO_HALO_HOLD_Z0, _HOLD_X0 or _PLANAR");
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: MU must lie in (0, 1)");
  if (!(t_max > 0.0) || !std::isfinite(t_max)) return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: t_max must be finite and > 0");
  if (!(sing_tol >= 0.0 && sing_tol < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: sing_tol must lie in [0, 1)");
  if (((long)max_iter + 1) * n_batch > 0x7fffffffL || (long)n_batch * 8 > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_correct_batch: batch too large");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t B = (size_t)n_batch, nh = (size_t)max_iter + 1;
  double *d_seed, *d_state, *d_sc, *d_hist;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(6 * B, d_seed, d_state);
  scratch.add(2 * B, d_sc);
  scratch.add(nh * B, d_hist);
  scratch.add(2 * B, d_int);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  HaloCorrectArgs a;
  a.seed = d_seed; a.B = n_batch; a.mode = mode; a.max_iter = max_iter;
  a.MU = MU; a.tol = tol; a.t_max = t_max; a.sing_tol = sing_tol;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.state = d_state; a.period = d_sc; a.resid = d_sc + B; a.hist = d_hist; a.iters = d_int; a.status = d_int + B;
  hipError_t e = hipMemcpyAsync(d_seed, seeds, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_halo_correct(integ->method, a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(state_out, d_state, sizeof(double) * 6 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(period_out, d_sc, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && resid_out) e = hipMemcpyAsync(resid_out, d_sc + B, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && history) e = hipMemcpyAsync(history, d_hist, sizeof(double) * nh * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && iterations) e = hipMemcpyAsync(iterations, d_int, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + B, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_correct_batch", e);
  return LTO_OK;
}

/* One revolution per orbit from (state0, period): one upload, one launch, the table and the per-orbit facts come down behind it;
 * the normalised times are made here. */
int lto_halo_table_batch(lto_ctx* c, int n_samples, int n_batch, double MU, const double* state0, const double* period,
                         const lto_integrator* integ, double* X_out, double* tau_out, double* M_out, double* closure, double* jacobi,
                         double* nu, int* status) {
  if (!c) return LTO_ENULL;
  if (n_samples < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_halo_table_batch: need n_samples >= 2 and n_batch >= 1");
  if (!state0 || !period || !integ || !X_out || !status) return set_err(c, LTO_ENULL, "lto_halo_table_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_table_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_halo_table_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_table_batch: MU must lie in (0, 1)");
  if ((long)6 * n_samples * n_batch > 0x7fffffffL || (long)n_batch * 36 > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_table_batch: batch too large");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t B = (size_t)n_batch, n = (size_t)n_samples;
  double *d_in, *d_X, *d_M, *d_sc;
  int* d_status;
  ArenaLayout scratch;
  scratch.add(7 * B, d_in);                    // state0 [6][B] | period [B]
  scratch.add(6 * n * B, d_X);
  scratch.add(36 * B, d_M);
  scratch.add(5 * B, d_sc);                    // closure [B] | jacobi [2][B] | nu [2][B]
  scratch.add(B, d_status);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  HaloTableArgs a;
  a.state0 = d_in; a.period = d_in + 6 * B; a.n = n_samples; a.B = n_batch; a.MU = MU;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.X = d_X; a.M = d_M; a.closure = d_sc; a.jacobi = d_sc + B; a.nu = d_sc + 3 * B; a.status = d_status;
  hipError_t e = hipMemcpyAsync(d_in, state0, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + 6 * B, period, sizeof(double) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_halo_table(integ->method, a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(X_out, d_X, sizeof(double) * 6 * n * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && M_out) e = hipMemcpyAsync(M_out, d_M, sizeof(double) * 36 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && closure) e = hipMemcpyAsync(closure, d_sc, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && jacobi) e = hipMemcpyAsync(jacobi, d_sc + B, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nu) e = hipMemcpyAsync(nu, d_sc + 3 * B, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_table_batch", e);
  if (tau_out) {
    for (size_t i = 0; i < n; ++i) tau_out[i] = (i == n - 1) ? 1.0 : (double)i / (double)(n - 1);
  }
  return LTO_OK;
}

}  // extern "C"
