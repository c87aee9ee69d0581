// lto_replay.hip -- control replay: the host-pointer calls.  They stage the starts and the control histories in, form
// the spline's moments on the device, fly every start through the knot intervals and bring the end states, the samples, dv, the
// step counts and the status back.  The parameters travel on a short-lived plan of the call (12-row for 6 states, 14-row for 7: the
// plan's TrajParams are those of the matching state+costate system), the scratch is laid out by ArenaLayout.
#include <cmath>

#include "lto_host.hpp"

extern "C" {

int lto_control_replay_batch(lto_ctx* c, int nstate, int n_knots, int n_batch, double t0, double t1, const double* lamv, int n_hist,
                             const double* x0, const lto_params* prm, int n_prm, const lto_integrator* integ, int sample_every,
                             double* x_final, double* X_samples, double* dv, int* accepted, int* rejected, int* status) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!lamv || !x0 || !prm || !integ || !x_final || !dv || !status)
    return set_err(c, LTO_ENULL, "lto_control_replay_batch: lamv, x0, prm, integ, x_final, dv or status is NULL");
  if (sample_every > 0 && !X_samples) return set_err(c, LTO_ENULL, "lto_control_replay_batch: sample_every > 0 needs X_samples");
  if (nstate != 6 && nstate != 7) return set_err(c, LTO_EUNSUPPORTED, "control replay is built for nstate = 6 or 7");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE)
    return set_err(c, LTO_EUNSUPPORTED, "control replay is built for LTO_RK4 or LTO_DOP853_ADAPTIVE");
  if (n_knots < 4 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_control_replay_batch: need n_knots >= 4 and n_batch >= 1");
  if (!std::isfinite(t0) || !std::isfinite(t1) || !(t1 > t0) || !std::isfinite(t1 - t0))
    return set_err(c, LTO_EINVAL, "lto_control_replay_batch: t0 and t1 must be finite with t1 > t0");
  if (n_hist != 1 && n_hist != n_batch) return set_err(c, LTO_EINVAL, "lto_control_replay_batch: n_hist must be 1 or n_batch");
  if (n_prm != 1 && n_prm != n_batch) return set_err(c, LTO_EINVAL, "lto_control_replay_batch: n_prm must be 1 or n_batch");
  if (sample_every < 0) return set_err(c, LTO_EINVAL, "lto_control_replay_batch: sample_every must be >= 0");
  const int B = n_batch, m = n_knots, last = n_knots - 1;
  const int ns = sample_every > 0 ? last / sample_every + 1 + (last % sample_every ? 1 : 0) : 0;
  const double h = (t1 - t0) / (double)last;
  if (!(h > 0.0)) return set_err(c, LTO_EINVAL, "lto_control_replay_batch: the knot spacing underflows");
  lto::HostBuf<double> h_cp((size_t)m, 0.0);     // the Thomas factors; ahead of the call's scope: the stream copies from it
  if (!h_cp.ok()) return set_err(c, LTO_ENOMEM, "lto_control_replay_batch: out of host memory");
  for (int i = 1; i < m - 1; ++i) h_cp[i] = 1.0 / (4.0 - h_cp[i - 1]);
  HostCall call(c);
  // two nodes per trajectory: the plan is asked for the parameters, the classes and the integrator's defaults only
  int rc = plan_build(c, nstate == 6 ? 12 : 14, 2, B, prm, n_prm, integ, &call.plan[0]);
  if (rc) return rc;
  lto_indirect_plan* p = call.plan[0];
  const size_t nl = (size_t)3 * m * n_hist, nx = (size_t)nstate * B, nsmp = (size_t)nstate * ns * B;
  double *d_x0a, *d_x0, *d_lamv, *d_cp, *d_mom, *d_vm, *d_xfa, *d_xf, *d_sa, *d_s, *d_dv;
  int *d_acc, *d_rej, *d_status;
  ArenaLayout scratch;
  scratch.add(nx, d_x0a, d_x0, d_xfa, d_xf);
  scratch.add(nl, d_lamv, d_mom);
  scratch.add((size_t)m, d_cp);
  scratch.add(2 * nl, d_vm);
  scratch.add(nsmp, d_sa, d_s);
  scratch.add((size_t)B, d_dv);
  scratch.add((size_t)B, d_acc, d_rej, d_status);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, x0, nstate, (long)B, d_x0a, d_x0, (long)B, st);
  if (e == hipSuccess) e = vec_in(c, lamv, (long)nl, d_lamv, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cp, h_cp.data(), sizeof(double) * m, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_control_replay_batch: stage in", e);
  IndirectArgs a{};
  a.tp = p->d_tp; a.tp_stride = (n_prm == 1) ? 0 : 1;
  a.steps = p->integ.steps; a.rtol = p->integ.rtol; a.atol = p->integ.atol; a.max_steps = p->integ.max_steps;
  ReplayArgs r{};
  r.vm = d_vm; r.n_hist = n_hist; r.n_knots = m; r.n_batch = B; r.h = h;
  r.x0 = d_x0; r.x_final = d_xf; r.dv = d_dv; r.nacc = d_acc; r.nrej = d_rej; r.status = d_status;
  r.samples = ns ? d_s : nullptr; r.ld_s = (long)ns * B; r.n_samples = ns; r.sample_every = sample_every;
  timing_begin(c, st);
  e = launch_replay_moments(d_lamv, d_cp, d_mom, d_vm, m, n_hist, h, st);
  if (e == hipSuccess) e = launch_control_replay(nstate, p->pm, p->integ.method, a, r, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_control_replay", e);
  e = stage_out(c, d_xf, (long)B, nstate, (long)B, d_xfa, x_final, st);
  if (e == hipSuccess && ns) e = stage_out(c, d_s, (long)ns * B, nstate, (long)ns * B, d_sa, X_samples, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dv, d_dv, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && accepted) e = hipMemcpyAsync(accepted, d_acc, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rejected) e = hipMemcpyAsync(rejected, d_rej, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_control_replay_batch: stage out", e);
  return LTO_OK;
}

int lto_control_replay(lto_ctx* c, int nstate, int n_knots, double t0, double t1, const double* lamv, const double* x0,
                       const lto_params* prm, const lto_integrator* integ, int sample_every, double* x_final, double* X_samples,
                       double* dv, int* accepted, int* rejected, int* status) {
  return lto_control_replay_batch(c, nstate, n_knots, 1, t0, t1, lamv, 1, x0, prm, 1, integ, sample_every, x_final, X_samples, dv,
                                  accepted, rejected, status);
}

}  // extern "C"
