// lto_manifold.hip -- invariant manifolds of periodic orbits: the eigen-directions and perturbed starts along an
// orbit, ballistic arcs flown to a Poincare section, and the nearest partner between two sets of states.
#include <cmath>
#include <cstring>

#include "lto_host.hpp"

extern "C" {

/* One upload (state0, period, M, the wrapped phases), three launches behind one another (eigen step, transport, starts), the results
 * come down behind them. */
int lto_halo_manifold_seeds_batch(lto_ctx* c, int n_phase, int n_batch, double MU, const double* state0, const double* period,
                                  const double* M, const double* tau, double eps, const lto_integrator* integ, double* lambda_out,
                                  double* X_out, double* V_out, double* starts_out, int* status) {
  if (!c) return LTO_ENULL;
  if (n_phase < 1 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_halo_manifold_seeds_batch: need n_phase >= 1 and n_batch >= 1");
  if (!state0 || !period || !M || !tau || !integ || !starts_out || !status)
    return set_err(c, LTO_ENULL, "lto_halo_manifold_seeds_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_halo_manifold_seeds_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                     "lto_halo_manifold_seeds_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_halo_manifold_seeds_batch: MU must lie in (0, 1)");
  if (!(eps > 0.0) || !std::isfinite(eps)) return set_err(c, LTO_EINVAL, "lto_halo_manifold_seeds_batch: eps must be finite and > 0");
  for (int j = 0; j < n_phase; ++j)
    if (!std::isfinite(tau[j])) return set_err(c, LTO_EINVAL, "lto_halo_manifold_seeds_batch: every tau must be finite");
  if ((long)24 * n_phase * n_batch > 0x7fffffffL || (long)n_batch * 36 > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_halo_manifold_seeds_batch: batch too large");
  const size_t B = (size_t)n_batch, P = (size_t)n_phase;
  lto::HostBuf<double> h_tau(P);
  if (!h_tau.ok()) return set_err(c, LTO_ENOMEM, "lto_halo_manifold_seeds_batch: out of host memory");
  for (size_t j = 0; j < P; ++j) {
    double w = tau[j] - std::floor(tau[j]);         // [0, 1]; a tiny negative tau rounds to 1
    h_tau[j] = (w >= 1.0) ? 0.0 : w;
  }
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  double *d_in, *d_M, *d_tau, *d_lambda, *d_vec0, *d_eig, *d_fly, *d_X, *d_V, *d_starts;
  int* d_status;
  ArenaLayout scratch;
  scratch.add(7 * B, d_in);                    // state0 [6][B] | period [B]
  scratch.add(36 * B, d_M);
  scratch.add(P, d_tau);
  scratch.add(2 * B, d_lambda);
  scratch.add(12 * B, d_vec0);
  scratch.add(B, d_eig);
  scratch.add(2 * P * B, d_fly);
  scratch.add(12 * P * B, d_X, d_V);
  scratch.add(24 * P * B, d_starts);
  scratch.add(B, d_status);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  ManifoldSeedArgs a;
  a.state0 = d_in; a.period = d_in + 6 * B; a.M = d_M; a.tau = d_tau; a.P = n_phase; a.B = n_batch; a.MU = MU; a.eps = eps;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.lambda = d_lambda; a.vec0 = d_vec0; a.eig_flag = d_eig; a.fly_flag = d_fly; a.X = d_X; a.V = d_V; a.starts = d_starts;
  a.status = d_status;
  hipError_t e = hipMemcpyAsync(d_in, state0, sizeof(double) * 6 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + 6 * B, period, sizeof(double) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_M, M, sizeof(double) * 36 * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tau, h_tau.data(), sizeof(double) * P, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_manifold_seeds(integ->method, a, st);
  if (e == hipSuccess && lambda_out) e = hipMemcpyAsync(lambda_out, d_lambda, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && X_out) e = hipMemcpyAsync(X_out, d_X, sizeof(double) * 12 * P * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && V_out) e = hipMemcpyAsync(V_out, d_V, sizeof(double) * 12 * P * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(starts_out, d_starts, sizeof(double) * 24 * P * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_halo_manifold_seeds_batch", e);
  return LTO_OK;
}

/* One upload (the starts and their signed flight times), one launch, one lane per arc, the results come down behind it. */
int lto_section_flight_batch(lto_ctx* c, int n_arcs, double MU, const double* y0, const double* t_max, int sec_axis, double sec_value,
                             int sec_dir, int n_cross, const double* r_min, int n_samples, const lto_integrator* integ, double* x_end,
                             double* t_end, int* count, double* dC, double* X_out, int* status) {
  if (!c) return LTO_ENULL;
  if (n_arcs < 1 || n_samples == 1 || n_samples < 0 || n_cross < 0)
    return set_err(c, LTO_EINVAL, "lto_section_flight_batch: need n_arcs >= 1, n_cross >= 0 and n_samples = 0 or >= 2");
  if (!y0 || !t_max || !r_min || !integ || !x_end || !t_end || !count || !status || (n_samples >= 2 && !X_out))
    return set_err(c, LTO_ENULL, "lto_section_flight_batch: a required argument is NULL");
  int rc = halo_integrator_check(c, integ, "lto_section_flight_batch: the flight is built for LTO_RK4 and LTO_DOP853_ADAPTIVE",
                                     "lto_section_flight_batch: LTO_RK4 needs steps >= 1");
  if (rc) return rc;
  if (sec_axis < 0 || sec_axis > 5) return set_err(c, LTO_EINVAL, "lto_section_flight_batch: sec_axis must lie in 0..5");
  if (sec_dir < -1 || sec_dir > 1) return set_err(c, LTO_EINVAL, "lto_section_flight_batch: sec_dir must be -1, 0 or +1");
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_section_flight_batch: MU must lie in (0, 1)");
  if (!std::isfinite(sec_value)) return set_err(c, LTO_EINVAL, "lto_section_flight_batch: sec_value must be finite");
  for (int k = 0; k < 2; ++k)
    if (!(r_min[k] >= 0.0) || !std::isfinite(r_min[k]))
      return set_err(c, LTO_EINVAL, "lto_section_flight_batch: r_min must be finite and >= 0");
  for (int b = 0; b < n_arcs; ++b)
    if (!std::isfinite(t_max[b]) || t_max[b] == 0.0)
      return set_err(c, LTO_EINVAL, "lto_section_flight_batch: every t_max must be finite and non-zero");
  if ((long)6 * n_samples * n_arcs > 0x7fffffffL || (long)6 * n_arcs > 0x7fffffffL)
    return set_err(c, LTO_EINVAL, "lto_section_flight_batch: batch too large");
  rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t N = (size_t)n_arcs, n = (size_t)n_samples;
  double *d_in, *d_xe, *d_sc, *d_X;
  int* d_int;
  ArenaLayout scratch;
  scratch.add(7 * N, d_in);                    // y0 [6][N] | t_max [N]
  scratch.add(6 * N, d_xe);
  scratch.add(2 * N, d_sc);                    // t_end [N] | dC [N]
  scratch.add(6 * n * N, d_X);
  scratch.add(2 * N, d_int);                   // count [N] | status [N]
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  SectionFlightArgs a;
  a.y0 = d_in; a.t_max = d_in + 6 * N; a.N = n_arcs; a.axis = sec_axis; a.dir = sec_dir; a.n_cross = n_cross; a.n_samples = n_samples;
  a.MU = MU; a.value = sec_value; a.rmin1 = r_min[0]; a.rmin2 = r_min[1];
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  a.x_end = d_xe; a.t_end = d_sc; a.dC = d_sc + N; a.X = d_X; a.count = d_int; a.status = d_int + N;
  hipError_t e = hipMemcpyAsync(d_in, y0, sizeof(double) * 6 * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in + 6 * N, t_max, sizeof(double) * N, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_section_flight(integ->method, a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(x_end, d_xe, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_end, d_sc, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dC) e = hipMemcpyAsync(dC, d_sc + N, sizeof(double) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_samples >= 2) e = hipMemcpyAsync(X_out, d_X, sizeof(double) * 6 * n * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(count, d_int, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_int + N, sizeof(int) * N, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_section_flight_batch", e);
  return LTO_OK;
}

/* One upload (both sets), one launch, one workgroup per state of A, the results come down behind it. */
int lto_state_match_batch(lto_ctx* c, int nA, int nB, const double* A, const double* Bs, double w, int* index, double* dist, double* dr,
                          double* dv) {
  if (!c) return LTO_ENULL;
  if (nA < 1 || nB < 1) return set_err(c, LTO_EINVAL, "lto_state_match_batch: need nA >= 1 and nB >= 1");
  if (!A || !Bs || !index || !dist) return set_err(c, LTO_ENULL, "lto_state_match_batch: a required argument is NULL");
  if (!(w >= 0.0) || !std::isfinite(w)) return set_err(c, LTO_EINVAL, "lto_state_match_batch: w must be finite and >= 0");
  if ((long)6 * nA > 0x7fffffffL || (long)6 * nB > 0x7fffffffL) return set_err(c, LTO_EINVAL, "lto_state_match_batch: set too large");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  const size_t na = (size_t)nA, nb = (size_t)nB;
  double *d_A, *d_B, *d_out;
  int* d_idx;
  ArenaLayout scratch;
  scratch.add(6 * na, d_A);
  scratch.add(6 * nb, d_B);
  scratch.add(3 * na, d_out);                  // dist [nA] | dr [nA] | dv [nA]
  scratch.add(na, d_idx);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve(c);
  if (rc) return rc;
  StateMatchArgs a;
  a.A = d_A; a.Bs = d_B; a.nA = nA; a.nB = nB; a.w = w; a.index = d_idx; a.dist = d_out; a.dr = d_out + na; a.dv = d_out + 2 * na;
  hipError_t e = hipMemcpyAsync(d_A, A, sizeof(double) * 6 * na, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_B, Bs, sizeof(double) * 6 * nb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_state_match(a, st);
  if (e == hipSuccess) e = hipMemcpyAsync(index, d_idx, sizeof(int) * na, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dist, d_out, sizeof(double) * na, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dr) e = hipMemcpyAsync(dr, d_out + na, sizeof(double) * na, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dv) e = hipMemcpyAsync(dv, d_out + 2 * na, sizeof(double) * na, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_state_match_batch", e);
  return LTO_OK;
}

}  // extern "C"
