// lto_halo_target.hip -- periodic orbits at a given Jacobi constant or period for a batch of seeds, each marched through its own
// list of target values.
#include <cmath>
#include <cstring>

#include "lto_host.hpp"

extern "C" {

/* The targeted corrector for n_batch seeds side by side, n_targets members each: one upload, one launch (k_halo_target runs every
 * orbit's march and every member's Newton loop to its end), the results come down behind it. */
int lto_halo_target_batch(lto_ctx* c, int n_targets, int n_batch, double MU, int planar, int what, const double* seeds,
                          const double* targets, double tol, int max_iter, double t_max, double sing_tol, const lto_integrator* integ,
                          double* state_out, double* period_out, double* jacobi_out, double* resid_out, int* iterations,
                          double* history, int* status) {
  if (!c) return LTO_ENULL;
  if (n_targets < 1 || n_batch < 1 || max_iter < 0 || !(tol > 0.0))
    return set_err(c, LTO_EINVAL, "lto_halo_target_batch: need n_targets >= 1, n_batch >= 1, max_iter >= 0 and tol > 0");
  if (!seeds || !targets || !integ || !state_out || !period_out || !status)
    return set_err(c, LTO_ENULL, "lto_halo_target_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_target_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_halo_target_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (what != LTO_HALO_TARGET_JACOBI && what != LTO_HALO_TARGET_PERIOD)
    return set_err(c, LTO_EINVAL, "lto_halo_target_batch: what must be LTO_HALO_TARGET_JACOBI or LTO_HALO_TARGET_PERIOD");
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_target_batch: MU must lie in (0, 1)");
  if (!(t_max > 0.0) || !std::isfinite(t_max)) return set_err(c, LTO_EINVAL, "lto_halo_target_batch: t_max must be finite and > 0");
  if (!(sing_tol >= 0.0 && sing_tol < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_target_batch: sing_tol must lie in [0, 1)");
  const long members = (long)n_targets * n_batch;
  if (members > 0x7fffffffL / 6 || ((long)max_iter + 1) * members > 0x7fffffffL || (long)n_batch * 8 > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_target_batch: batch too large");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t B = (size_t)n_batch, N = (size_t)members, nh = (size_t)max_iter + 1;
  double *d_seed, *d_target, *d_state, *d_sc, *d_hist;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(6 * B, d_seed);
  scratch.add(N, d_target);
  scratch.add(6 * N, d_state);
  scratch.add(3 * N, d_sc);                    // period [N] | jacobi [N] | resid [N]
  scratch.add(nh * N, d_hist);
  scratch.add(2 * N, d_int);                   // iterations [N] | status [N]
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  HaloTargetArgs a;
  a.seed = d_seed; a.target = d_target; a.T = n_targets; a.B = n_batch; a.planar = planar != 0; a.what = what; a.max_iter = max_iter;
  a.MU = MU; a.tol = tol; a.t_max = t_max; a.sing_tol = sing_tol;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.state = d_state; a.period = d_sc; a.jacobi = d_sc + N; a.resid = d_sc + 2 * N; a.hist = d_hist;
  a.iters = d_int; a.status = d_int + N;
  hipError_t e = hipMemcpyAsync(d_seed, seeds, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_target, targets, sizeof(double) * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_halo_target(integ->method, a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(state_out, d_state, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(period_out, d_sc, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && jacobi_out) e = hipMemcpyAsync(jacobi_out, d_sc + N, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && resid_out) e = hipMemcpyAsync(resid_out, d_sc + 2 * N, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && history) e = hipMemcpyAsync(history, d_hist, sizeof(double) * nh * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && iterations) e = hipMemcpyAsync(iterations, d_int, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + N, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_target_batch", e);
  return LTO_OK;
}

}  // extern "C"
