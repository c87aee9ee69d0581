// lto_stationkeep.hip -- station-keeping on periodic orbits: the Floquet-mode feedback gains from the manifold seeds'
// directions, and batched flights with impulsive linear feedback; the state-transition matrices between phases of an orbit and
// the target-point gains built from them.
#include <cmath>

#include "lto_host.hpp"

extern "C" {

/* One upload (the directions), one launch, one lane per (phase, orbit), the results come down behind it. */
int lto_stationkeep_gains_batch(lto_ctx* c, int n_phase, int n_batch, const double* V, double sing_tol, double* W, double* G,
                                double* alpha, int* status) {
  if (!c) return LTO_ENULL;
  if (n_phase < 1 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_stationkeep_gains_batch: need n_phase >= 1 and n_batch >= 1");
  if (!V || !G || !status) return set_err(c, LTO_ENULL, "lto_stationkeep_gains_batch: a required argument is NULL");
  if (!(sing_tol >= 0.0 && sing_tol < 1.0)) return set_err(c, LTO_EINVAL, "lto_stationkeep_gains_batch: sing_tol must lie in [0, 1)");
  if ((long)n_phase * n_batch > 0x7fffffffL / 18) return set_err(c, LTO_EINVAL, "lto_stationkeep_gains_batch: batch too large");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t n = (size_t)n_phase * (size_t)n_batch;
  double *d_V, *d_W, *d_G, *d_alpha;
  int* d_status;
  ArenaLayout scratch;
  scratch.add(12 * n, d_V);
  scratch.add(6 * n, d_W);
  scratch.add(18 * n, d_G);
  scratch.add(n, d_alpha);
  scratch.add(n, d_status);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  StationGainsArgs a;
  a.V = d_V; a.n = (long)n; a.sing_tol = sing_tol; a.W = d_W; a.G = d_G; a.alpha = d_alpha; a.status = d_status;
  hipError_t e = hipMemcpyAsync(d_V, V, sizeof(double) * 12 * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_stationkeep_gains(a, st);
  if (e == hipSuccess && W) e = hipMemcpyAsync(W, d_W, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G, d_G, sizeof(double) * 18 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && alpha) e = hipMemcpyAsync(alpha, d_alpha, sizeof(double) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_stationkeep_gains_batch", e);
  return LTO_OK;
}

/* One upload (the orbit records, the starts, the error draws), one launch, one lane per run, the results come down behind it. */
int lto_stationkeep_flight_batch(lto_ctx* c, int n_man, int n_rev, int n_batch, double MU, const double* X_ref, const double* dt,
                                 const double* G, int n_orb, const double* x0, const double* nav, const double* exe, double dv_min,
                                 double dv_max, double r_lost, const lto_integrator* integ, double* x_final, double* dv_total,
                                 int* n_burn, double* dev, double* dv_hist, double* dev_final, int* accepted, int* rejected,
                                 int* status, int* lost_at) {
  if (!c) return LTO_ENULL;
  if (n_man < 1 || n_rev < 1 || n_batch < 1)
    return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: need n_man >= 1, n_rev >= 1 and n_batch >= 1");
  if (!X_ref || !dt || !G || !x0 || !integ || !x_final || !dv_total || !status)
    return set_err(c, LTO_ENULL, "lto_stationkeep_flight_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_stationkeep_flight_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_stationkeep_flight_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (n_orb != 1 && n_orb != n_batch) return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: n_orb must be 1 or n_batch");
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: MU must lie in (0, 1)");
  if (!(dv_min >= 0.0) || !std::isfinite(dv_min) || !(dv_max >= 0.0) || !std::isfinite(dv_max) || !(r_lost >= 0.0) ||
      !std::isfinite(r_lost))
    return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: dv_min, dv_max and r_lost must be finite and >= 0");
  if ((long)n_man * n_rev > 0x7fffffffL / 6 || (long)6 * n_man * n_rev * n_batch > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: batch too large");
  const size_t B = (size_t)n_batch, nm = (size_t)n_man, no = (size_t)n_orb, nu = (size_t)n_man * (size_t)n_rev;
  for (size_t k = 0; k < nm * no; ++k)
    if (!std::isfinite(dt[k]) || !(dt[k] > 0.0))
      return set_err(c, LTO_EINVAL, "lto_stationkeep_flight_batch: every dt must be finite and > 0");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  double *d_orb, *d_x0, *d_nav, *d_exe, *d_xf, *d_sc, *d_dev, *d_hist;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(25 * nm * no, d_orb);            // X_ref [6][n_man][n_orb] | G [3][6][n_man][n_orb] | dt [n_man][n_orb]
  scratch.add(6 * B, d_x0);
  scratch.add(nav ? 6 * nu * B : 0, d_nav);
  scratch.add(exe ? 4 * nu * B : 0, d_exe);
  scratch.add(6 * B, d_xf);
  scratch.add(3 * B, d_sc);                    // dv_total [B] | dev_final [2][B]
  scratch.add(dev ? 2 * nu * B : 0, d_dev);
  scratch.add(dv_hist ? nu * B : 0, d_hist);
  scratch.add(5 * B, d_int);                   // n_burn | accepted | rejected | status | lost_at
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  StationFlightArgs a;
  a.X_ref = d_orb; a.G = d_orb + 6 * nm * no; a.dt = d_orb + 24 * nm * no;
  a.x0 = d_x0; a.nav = nav ? d_nav : nullptr; a.exe = exe ? d_exe : nullptr;
  a.n_man = n_man; a.n_rev = n_rev; a.B = n_batch; a.n_orb = n_orb;
  a.MU = MU; a.dv_min = dv_min; a.dv_max = dv_max; a.r_lost = r_lost;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.x_final = d_xf; a.dv_total = d_sc; a.dev_final = d_sc + B;
  a.dev = dev ? d_dev : nullptr; a.dv_hist = dv_hist ? d_hist : nullptr;
  a.n_burn = d_int; a.accepted = d_int + B; a.rejected = d_int + 2 * B; a.status = d_int + 3 * B; a.lost_at = d_int + 4 * B;
  hipError_t e = hipMemcpyAsync(d_orb, X_ref, sizeof(double) * 6 * nm * no, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_orb + 6 * nm * no, G, sizeof(double) * 18 * nm * no, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_orb + 24 * nm * no, dt, sizeof(double) * nm * no, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_x0, x0, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && nav) e = hipMemcpyAsync(d_nav, nav, sizeof(double) * 6 * nu * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && exe) e = hipMemcpyAsync(d_exe, exe, sizeof(double) * 4 * nu * B, hipMemcpyHostToDevice, st);
  timing_begin(c, st);
  if (e == hipSuccess) e = launch_stationkeep_flight(integ->method, a, st);
  timing_end(c, st);                             // the flight kernel alone
  if (e == hipSuccess) e = hipMemcpyAsync(x_final, d_xf, sizeof(double) * 6 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dv_total, d_sc, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dev_final) e = hipMemcpyAsync(dev_final, d_sc + B, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dev) e = hipMemcpyAsync(dev, d_dev, sizeof(double) * 2 * nu * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dv_hist) e = hipMemcpyAsync(dv_hist, d_hist, sizeof(double) * nu * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_burn) e = hipMemcpyAsync(n_burn, d_int, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && accepted) e = hipMemcpyAsync(accepted, d_int + B, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rejected) e = hipMemcpyAsync(rejected, d_int + 2 * B, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + 3 * B, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && lost_at) e = hipMemcpyAsync(lost_at, d_int + 4 * B, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_stationkeep_flight_batch", e);
  return LTO_OK;
}

/* One upload (state0, period, the wrapped phases, the horizons), one launch, one group of eight lanes per (phase, orbit), the results
 * come down behind it. */
int lto_halo_stm_batch(lto_ctx* c, int n_phase, int n_tgt, int n_batch, double MU, const double* state0, const double* period,
                       const double* tau, const double* horizon, const lto_integrator* integ, double* X_out, double* Phi_out,
                       double* X_tgt, int* accepted, int* rejected, int* status) {
  if (!c) return LTO_ENULL;
  if (n_phase < 1 || n_tgt < 1 || n_batch < 1)
    return set_err(c, LTO_EINVAL, "lto_halo_stm_batch: need n_phase >= 1, n_tgt >= 1 and n_batch >= 1");
  if (!state0 || !period || !tau || !horizon || !integ || !X_out || !Phi_out || !status)
    return set_err(c, LTO_ENULL, "lto_halo_stm_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_stm_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                 "lto_halo_stm_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_stm_batch: MU must lie in (0, 1)");
  if ((long)n_tgt * n_phase > 0x7fffffffL / 36 || (long)36 * n_tgt * n_phase * n_batch > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_stm_batch: batch too large");
  for (int k = 0; k < n_tgt; ++k)
    if (!std::isfinite(horizon[k]) || !(horizon[k] > (k ? horizon[k - 1] : 0.0)))
      return set_err(c, LTO_EINVAL, "lto_halo_stm_batch: the horizons must be finite, > 0 and strictly increasing");
  for (int j = 0; j < n_phase; ++j)
    if (!std::isfinite(tau[j])) return set_err(c, LTO_EINVAL, "lto_halo_stm_batch: every tau must be finite");
  const size_t B = (size_t)n_batch, P = (size_t)n_phase, K = (size_t)n_tgt, n = P * B;
  lto::HostBuf<double> h_tau(P);
  if (!h_tau.ok()) return set_err(c, LTO_ENOMEM, "lto_halo_stm_batch: out of host memory");
  for (size_t j = 0; j < P; ++j) {
    double w = tau[j] - std::floor(tau[j]);         // [0, 1]; a tiny negative tau rounds to 1
    h_tau[j] = (w >= 1.0) ? 0.0 : w;
  }
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  double *d_in, *d_ph, *d_X, *d_Phi, *d_Xt;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(7 * B, d_in);                    // state0 [6][B] | period [B]
  scratch.add(P + K, d_ph);                    // tau [P] | horizon [K]
  scratch.add(6 * n, d_X);
  scratch.add(36 * K * n, d_Phi);
  scratch.add(X_tgt ? 6 * K * n : 0, d_Xt);
  scratch.add(3 * n, d_int);                   // accepted | rejected | status
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  HaloStmArgs a;
  a.state0 = d_in; a.period = d_in + 6 * B; a.tau = d_ph; a.horizon = d_ph + P;
  a.P = n_phase; a.K = n_tgt; a.B = n_batch; a.MU = MU;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.X = d_X; a.Phi = d_Phi; a.Xt = X_tgt ? d_Xt : nullptr;
  a.accepted = d_int; a.rejected = d_int + n; a.status = d_int + 2 * n;
  hipError_t e = hipMemcpyAsync(d_in, state0, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + 6 * B, period, sizeof(double) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_ph, h_tau.data(), sizeof(double) * P, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_ph + P, horizon, sizeof(double) * K, hipMemcpyHostToDevice, st);
  timing_begin(c, st);
  if (e == hipSuccess) e = launch_halo_stm(integ->method, a, st);
  timing_end(c, st);                             // the STM kernel alone
  if (e == hipSuccess) e = hipMemcpyAsync(X_out, d_X, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(Phi_out, d_Phi, sizeof(double) * 36 * K * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && X_tgt) e = hipMemcpyAsync(X_tgt, d_Xt, sizeof(double) * 6 * K * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && accepted) e = hipMemcpyAsync(accepted, d_int, sizeof(int) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rejected) e = hipMemcpyAsync(rejected, d_int + n, sizeof(int) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + 2 * n, sizeof(int) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_stm_batch", e);
  return LTO_OK;
}

/* One upload (the STMs and the weights), one launch, one lane per record, the results come down behind it. */
int lto_stationkeep_target_gains_batch(lto_ctx* c, int n_tgt, int n_rec, const double* Phi, double q, const double* r,
                                       double sing_tol, double* G, double* pivot, int* status) {
  if (!c) return LTO_ENULL;
  if (n_tgt < 1 || n_rec < 1) return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: need n_tgt >= 1 and n_rec >= 1");
  if (!Phi || !r || !G || !status) return set_err(c, LTO_ENULL, "lto_stationkeep_target_gains_batch: a required argument is NULL");
  if (n_tgt > 0x7fffffffL / 36 / n_rec) return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: batch too large");
  if (!(q >= 0.0) || !std::isfinite(q)) return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: q must be finite and >= 0");
  bool any = false;
  for (int k = 0; k < n_tgt; ++k) {
    if (!(r[k] >= 0.0) || !std::isfinite(r[k]))
      return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: every r must be finite and >= 0");
    any = any || r[k] > 0.0;
  }
  if (!any) return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: at least one r must be > 0");
  if (!(sing_tol >= 0.0 && sing_tol < 1.0))
    return set_err(c, LTO_EINVAL, "lto_stationkeep_target_gains_batch: sing_tol must lie in [0, 1)");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t n = (size_t)n_rec, K = (size_t)n_tgt;
  double *d_Phi, *d_r, *d_G, *d_pivot;
  int* d_status;
  ArenaLayout scratch;
  scratch.add(36 * K * n, d_Phi);
  scratch.add(K, d_r);
  scratch.add(18 * n, d_G);
  scratch.add(pivot ? n : 0, d_pivot);
  scratch.add(n, d_status);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  StationTargetGainsArgs a;
  a.Phi = d_Phi; a.r = d_r; a.K = n_tgt; a.n = (long)n; a.q = q; a.sing_tol = sing_tol;
  a.G = d_G; a.pivot = pivot ? d_pivot : nullptr; a.status = d_status;
  hipError_t e = hipMemcpyAsync(d_Phi, Phi, sizeof(double) * 36 * K * n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_r, r, sizeof(double) * K, hipMemcpyHostToDevice, st);
  timing_begin(c, st);
  if (e == hipSuccess) e = launch_stationkeep_target_gains(a, st);
  timing_end(c, st);
  if (e == hipSuccess) e = hipMemcpyAsync(G, d_G, sizeof(double) * 18 * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && pivot) e = hipMemcpyAsync(pivot, d_pivot, sizeof(double) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * n, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_stationkeep_target_gains_batch", e);
  return LTO_OK;
}

}  // extern "C"
