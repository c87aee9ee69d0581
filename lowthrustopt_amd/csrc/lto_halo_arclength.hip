// lto_halo_arclength.hip -- families of periodic orbits by pseudo-arclength continuation for a batch of seeds, each marched through
// its members with its own step control.
#include <cmath>
#include <cstring>

#include "lto_host.hpp"

extern "C" {

/* The continuation for n_batch seeds side by side, n_members members each: one upload, one launch (k_halo_arclength runs every
 * orbit's march, every member's attempts and every attempt's Newton loop to its end), the results come down behind it. */
int lto_halo_arclength_batch(lto_ctx* c, int n_members, int n_batch, double MU, int planar, int dir_is_tangent, const double* seeds,
                             const double* dir0, const double* ds0, double ds_min, double ds_max, double grow, int fast_iter,
                             double cos_min, double tol, int max_iter, double t_max, double sing_tol, const lto_integrator* integ,
                             double* state_out, double* tangent_out, double* det_out, double* ds_out, int* halvings,
                             double* period_out, double* jacobi_out, double* resid_out, int* iterations, double* history,
                             int* status) {
  if (!c) return LTO_ENULL;
  if (n_members < 1 || n_batch < 1 || max_iter < 0 || !(tol > 0.0))
    return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: need n_members >= 1, n_batch >= 1, max_iter >= 0 and tol > 0");
  if (!seeds || !dir0 || !ds0 || !integ || !state_out || !status)
    return set_err(c, LTO_ENULL, "lto_halo_arclength_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_arclength_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_halo_arclength_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: MU must lie in (0, 1)");
  if (!(t_max > 0.0) || !std::isfinite(t_max)) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: t_max must be finite and > 0");
  if (!(sing_tol >= 0.0 && sing_tol < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: sing_tol must lie in [0, 1)");
  if (!(ds_min > 0.0) || !(ds_min <= ds_max) || !std::isfinite(ds_max))
    return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: need 0 < ds_min <= ds_max, both finite");
  if (!(grow >= 1.0) || !std::isfinite(grow)) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: grow must be finite and >= 1");
  if (fast_iter < 0) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: fast_iter must be >= 0");
  if (!(cos_min >= 0.0 && cos_min < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: cos_min must lie in [0, 1)");
  const long members = (long)n_members * n_batch;
  if (members > 0x7fffffffL / 6 || ((long)max_iter + 1) * members > 0x7fffffffL || (long)n_batch * 8 > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: batch too large");
  for (int b = 0; b < n_batch; ++b)
    if (!(ds0[b] > 0.0) || !std::isfinite(ds0[b])) return set_err(c, LTO_EINVAL, "lto_halo_arclength_batch: every ds0 must be finite and > 0");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t B = (size_t)n_batch, N = (size_t)members, nh = (size_t)max_iter + 1;
  double *d_seed, *d_dir, *d_ds0, *d_state, *d_tan, *d_sc, *d_hist;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(6 * B, d_seed);
  scratch.add(3 * B, d_dir);
  scratch.add(B, d_ds0);
  scratch.add(6 * N, d_state);
  scratch.add(3 * N, d_tan);
  scratch.add(5 * N, d_sc);                    // det [N] | ds [N] | period [N] | jacobi [N] | resid [N]
  scratch.add(nh * N, d_hist);
  scratch.add(3 * N, d_int);                   // halvings [N] | iterations [N] | status [N]
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  HaloArclengthArgs a;
  a.seed = d_seed; a.dir0 = d_dir; a.ds0 = d_ds0;
  a.T = n_members; a.B = n_batch; a.planar = planar != 0; a.dir_is_tangent = dir_is_tangent != 0; a.max_iter = max_iter;
  a.fast_iter = fast_iter;
  a.MU = MU; a.ds_min = ds_min; a.ds_max = ds_max; a.grow = grow; a.cos_min = cos_min; a.tol = tol; a.t_max = t_max;
  a.sing_tol = sing_tol;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.state = d_state; a.tangent = d_tan;
  a.det = d_sc; a.ds = d_sc + N; a.period = d_sc + 2 * N; a.jacobi = d_sc + 3 * N; a.resid = d_sc + 4 * N; a.hist = d_hist;
  a.halvings = d_int; a.iters = d_int + N; a.status = d_int + 2 * N;
  hipError_t e = hipMemcpyAsync(d_seed, seeds, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_dir, dir0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_ds0, ds0, sizeof(double) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_halo_arclength(integ->method, a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(state_out, d_state, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && tangent_out) e = hipMemcpyAsync(tangent_out, d_tan, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, st);
  double* const sc_out[5] = {det_out, ds_out, period_out, jacobi_out, resid_out};
  for (int i = 0; i < 5; ++i)
    if (e == hipSuccess && sc_out[i]) e = hipMemcpyAsync(sc_out[i], d_sc + i * N, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && history) e = hipMemcpyAsync(history, d_hist, sizeof(double) * nh * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && halvings) e = hipMemcpyAsync(halvings, d_int, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && iterations) e = hipMemcpyAsync(iterations, d_int + N, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + 2 * N, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_arclength_batch", e);
  return LTO_OK;
}

}  // extern "C"
