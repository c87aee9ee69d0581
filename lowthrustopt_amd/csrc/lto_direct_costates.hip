// lto_direct_costates.hip -- costates of the direct transcription from the multipliers of its frozen QP step: the
// device entry on a plan and the host-pointer calls that run one Jacobian sweep, one frozen step and the costates kernel.
#include <cstring>

#include "lto_host.hpp"

// the factor between the controls of the direct method (N) and the acceleration of the 6-state right-hand side (DU/TU^2):
// a = c u, c = TU^2 / DU / 1e3 / m with the literal m = 1000 kg of that right-hand side (prop_EP_deriv.jl:32)
static double costate_scale(const lto_direct_params& prm) { return (prm.TU * prm.TU) / prm.DU / 1e3 / 1000.0; }

int direct_costates_launch(lto_direct_plan* p, hipStream_t st, const double* Jac, long ldj, double* Lambda, long ldl, double* mult,
                           long ldm, double* kkt_res, const double* X, long ldx, double* XC, long ldxc) {
  lto_ctx* c = p->ctx;
  if (!p->qp_ws || p->qp_last_nr != 1)
    return set_err(c, LTO_EINVAL, "costates: valid after a frozen QP step (lto_direct_qp_step_dev) on this plan");
  if (!p->cs_acc) {
    const hipError_t e = hipMalloc(&p->cs_acc, direct_costates_acc_bytes(p->n_batch));
    if (e != hipSuccess) { p->cs_acc = nullptr; return set_err(c, LTO_EHIP, "costates scratch", e); }
  }
  DirectCostatesArgs o;
  std::memset(&o, 0, sizeof o);
  o.n_nodes = p->n_nodes; o.n_batch = p->n_batch;
  o.Jac = Jac; o.ldj = ldj; o.Lambda = Lambda; o.ldl = ldl; o.mult = mult; o.ldm = ldm; o.kkt_res = kkt_res;
  o.X = X; o.ldx = ldx; o.XC = XC; o.ldxc = ldxc;
  const double cu = costate_scale(p->prm);
  o.cc = cu * cu;
  timing_begin(c, st);
  const hipError_t e = launch_direct_costates(p->nstate, o, p->qp_ws, p->cs_acc, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_direct_costates", e);
  return LTO_OK;
}

extern "C" {

int lto_direct_costates_dev(lto_direct_plan* p, void* stream, const double* Jac, long ldj, double* Lambda, long ldl, double* mult,
                            long ldm, double* kkt_res) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!Jac || !Lambda || !kkt_res) return set_err(c, LTO_ENULL, "lto_direct_costates_dev: Jac, Lambda or kkt_res is NULL");
  if (ldj < p->S) return set_err(c, LTO_EINVAL, "lto_direct_costates_dev: ldj smaller than the segment count");
  if (ldl < (long)p->n_nodes * p->n_batch) return set_err(c, LTO_EINVAL, "lto_direct_costates_dev: ldl smaller than n_nodes*n_batch");
  if (mult && ldm < p->S) return set_err(c, LTO_EINVAL, "lto_direct_costates_dev: ldm smaller than the segment count");
  const int rc = bind_device(c);
  if (rc) return rc;
  return direct_costates_launch(p, (hipStream_t)stream, Jac, ldj, Lambda, ldl, mult, ldm, kkt_res);
}

int lto_direct_costates_batch(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                              int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                              int n_targets, int allow_impulsive, double* Lambda, double* mult, double* XC, double* kkt_res,
                              int* status) {
  if ((nstate != 6 && nstate != 7) || n_nodes < 2 || n_batch < 1)
    return c ? set_err(c, LTO_EINVAL, "need nstate 6 or 7, n_nodes >= 2, n_batch >= 1") : LTO_EINVAL;
  if (!c) return LTO_ENULL;
  if (!X || !U || !t || !prm || !targets || !Lambda || !kkt_res || !status)
    return set_err(c, LTO_ENULL, "lto_direct_costates_batch: a required array is NULL");
  if ((n_targets != 1 && n_targets != n_batch) || (n_tgrids != 1 && n_tgrids != n_batch))
    return set_err(c, LTO_EINVAL, "n_targets / n_tgrids must be 1 or n_batch");
  if (XC && nstate == 7)
    return set_err(c, LTO_EUNSUPPORTED, "lto_direct_costates_batch: XC is the 12-dim node vector; the 14-dim hand-over is not built");
  CallTimer call_timer(c);
  const int B = n_batch;
  lto::HostBuf<lto_direct_targets> tg((size_t)B);
  HostCall call(c);
  int rc = direct_plan_build(c, nstate, n_nodes, n_batch, nsteps, prm, &call.dplan[0]);
  if (rc) return rc;
  lto_direct_plan* p = call.dplan[0];
  if (!tg.ok()) return set_err(c, LTO_ENOMEM, "lto_direct_costates_batch: out of host memory");
  for (int b = 0; b < B; ++b) tg[(size_t)b] = targets[n_targets == 1 ? 0 : b];
  const long J = (long)n_nodes * B, S = p->S;
  const int nj = nstate * 2 * (nstate + 3);
  double *d_xa, *d_X, *d_dX, *d_L, *d_La, *d_ua, *d_U, *d_dU, *d_t, *d_jac, *d_def, *d_m, *d_ma, *d_xc, *d_xca, *d_dV, *d_cost, *d_res;
  lto_direct_targets* d_tg;
  ArenaLayout scratch;
  scratch.add((size_t)nstate * J, d_xa, d_X, d_dX, d_L, d_La);
  scratch.add((size_t)3 * J, d_ua, d_U, d_dU);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)nj * S, d_jac);
  scratch.add((size_t)nstate * S, d_def);
  scratch.add(mult ? (size_t)nstate * S : 0, d_m, d_ma);
  scratch.add(XC ? (size_t)12 * J : 0, d_xc, d_xca);
  scratch.add((size_t)B, d_tg);
  scratch.add((size_t)6 * B, d_dV);
  scratch.add((size_t)B, d_cost, d_res);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, X, nstate, J, d_xa, d_X, J, st);
  if (e == hipSuccess) e = stage_in(c, U, 3, J, d_ua, d_U, J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)n_nodes * n_tgrids, d_t, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tg, tg.data(), sizeof(lto_direct_targets) * B, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  rc = lto_direct_jacobian_dev(p, st, d_X, J, d_U, J, d_t, n_tgrids, d_jac, S, nullptr, d_def, S, nullptr);
  if (rc == LTO_OK)
    rc = direct_qp_launch(p, st, 1, d_jac, S, d_def, S, d_X, J, d_U, J, d_t, n_tgrids, d_tg, allow_impulsive, d_dX, d_dU, d_dV, d_cost);
  if (rc == LTO_OK)
    rc = direct_costates_launch(p, st, d_jac, S, d_L, J, mult ? d_m : nullptr, S, d_res, d_X, J, XC ? d_xc : nullptr, J);
  if (rc != LTO_OK) return rc;
  e = stage_out(c, d_L, J, nstate, J, d_La, Lambda, st);
  if (e == hipSuccess && mult) e = stage_out(c, d_m, S, nstate, S, d_ma, mult, st);
  if (e == hipSuccess && XC) e = stage_out(c, d_xc, J, 12, J, d_xca, XC, st);
  if (e == hipSuccess) e = hipMemcpyAsync(kkt_res, d_res, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, lto_direct_plan_qp_status(p), sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage out", e);
  return LTO_OK;
}

int lto_direct_costates(lto_ctx* c, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                        const lto_direct_params* prm, const lto_direct_targets* targets, int allow_impulsive, double* Lambda,
                        double* mult, double* XC, double* kkt_res, int* status) {
  return lto_direct_costates_batch(c, nstate, n_nodes, 1, X, U, t, 1, nsteps, prm, targets, 1, allow_impulsive, Lambda, mult, XC,
                                   kkt_res, status);
}

}  // extern "C"
