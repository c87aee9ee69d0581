// lto_direct_plan.hip -- direct plans: construction, the device-resident defect / mid-point / Jacobian sweeps and the QP step.
#include <cstring>
#include <new>

#include "lto_host.hpp"

/* ------------------------------------------------------------------------------ direct plans */
int direct_plan_build(lto_ctx* c, int nstate, int n_nodes, int n_batch, int nsteps, const lto_direct_params* prm,
                             lto_direct_plan** out) {
  if (!c || !out) return LTO_ENULL;
  *out = nullptr;
  if (!prm) return set_err(c, LTO_ENULL, "prm is NULL");
  if (nstate != 6 && nstate != 7) return set_err(c, LTO_EINVAL, "nstate must be 6 or 7");
  if (n_nodes < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "need n_nodes >= 2 and n_batch >= 1");
  if (nsteps < 2) return set_err(c, LTO_EINVAL, "nsteps (grid points per half segment) must be >= 2");
  if ((long)(n_nodes - 1) * n_batch > 0x3fffffffL) return set_err(c, LTO_EINVAL, "too many segments");
  lto_direct_plan* p = new (std::nothrow) lto_direct_plan();
  if (!p) return set_err(c, LTO_EHIP, "host allocation failed");
  p->ctx = c; p->nstate = nstate; p->n_nodes = n_nodes; p->n_batch = n_batch; p->S = (n_nodes - 1) * n_batch;
  p->nsteps = nsteps; p->prm = *prm; p->kernel = LTO_KERNEL_AUTO;
  *out = p;
  return LTO_OK;
}

void direct_plan_free(lto_direct_plan* p) {
  if (p->qp_ws) (void)hipFree(p->qp_ws);        // hipFree waits for the device
  if (p->cs_acc) (void)hipFree(p->cs_acc);
  delete p;
}

// the QP workspace for nr right-hand sides (1: frozen ends, 3: free ends, 4: free ends and free tf); a smaller workspace grows at
// the first step that needs more
int direct_qp_workspace(lto_direct_plan* p, int nr) {
  if (p->qp_ws && p->qp_ws_nr >= nr) return LTO_OK;
  if (p->qp_ws) { (void)hipFree(p->qp_ws); p->qp_ws = nullptr; }
  const size_t bytes = direct_qp_workspace_bytes(p->nstate, p->n_nodes, p->n_batch, nr);
  const hipError_t e = hipMalloc(&p->qp_ws, bytes);
  if (e != hipSuccess) { p->qp_ws = nullptr; return set_err(p->ctx, LTO_EHIP, "QP workspace", e); }
  p->qp_ws_nr = nr;
  return LTO_OK;
}

static int fill_direct_args(lto_direct_plan* p, const double* X, long ldx, const double* U, long ldu, const double* t,
                            int n_tgrids, DirectArgs* a) {
  lto_ctx* c = p->ctx;
  if (!X || !U || !t) return set_err(c, LTO_ENULL, "X, U or t is NULL");
  const long J = (long)p->n_nodes * p->n_batch;
  if (ldx < J || ldu < J) return set_err(c, LTO_EINVAL, "ldx/ldu smaller than n_nodes*n_batch");
  if (n_tgrids != 1 && n_tgrids != p->n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  std::memset(a, 0, sizeof *a);
  a->X = X; a->ldx = ldx; a->U = U; a->ldu = ldu; a->t = t; a->t_stride = (n_tgrids == 1) ? 0 : p->n_nodes;
  a->MU = p->prm.MU;
  a->kk = (p->prm.TU * p->prm.TU) / p->prm.DU / 1e3;  // N/kg -> DU/TU^2   (prop_EP_deriv.jl:32)
  a->isp_g0 = p->prm.Isp * 9.81;                       // prop_EP_deriv.jl:41-42
  a->TU = p->prm.TU;
  a->n_nodes = p->n_nodes; a->seg_per_traj = p->n_nodes - 1; a->S = p->S;
  a->half_steps = p->nsteps - 1;
  return LTO_OK;
}

int direct_defect_launch(lto_direct_plan* p, void* stream, const double* X, long ldx, const double* U, long ldu,
                                const double* t, int n_tgrids, double* defect, long ldd, double* errors, double* mid,
                                long ldm) {
  lto_ctx* c = p->ctx;
  DirectArgs a;
  int rc = fill_direct_args(p, X, ldx, U, ldu, t, n_tgrids, &a);
  if (rc) return rc;
  if (defect && ldd < p->S) return set_err(c, LTO_EINVAL, "ldd smaller than the segment count");
  a.defect = defect; a.ldd = ldd; a.errors = errors; a.mid = mid; a.ldm = ldm;
  rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  hipError_t e = launch_direct_defect(p->nstate, a, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_direct_defect", e);
  return LTO_OK;
}

/* ------------------------------------------------------------------------------ direct QP step and solve loop */
// the QP step on device operands (kernels_direct_qp.hip) with nr right-hand sides: 1 frozen ends; 3 free ends (flagEnd = true,
// DESIGN 4.8c) with the end models and beta of every trajectory and the phase updates p [n_batch][2]; 4 free ends and free tf
// (DESIGN 4.8e), also with the sweep's tf column dtf [nstate][ldd], tfb [n_batch][3], tf [n_batch], and p [n_batch][3].  The
// operands of a variant other than nr's are not passed on.
int direct_qp_launch(lto_direct_plan* p, hipStream_t st, int nr, const double* Jac, long ldj, const double* defect, long ldd,
                            const double* X, long ldx, const double* U, long ldu, const double* t, int n_tgrids,
                            const lto_direct_targets* targets, int allow_impulsive, double* dX, double* dU, double* dV, double* cost,
                            const lto_direct_end_model* model, const double* beta, double* pout,
                            const double* dtf, const double* tfb, const double* tf) {
  lto_ctx* c = p->ctx;
  const int rc = direct_qp_workspace(p, nr);
  if (rc) return rc;
  DirectQpArgs q;
  std::memset(&q, 0, sizeof q);
  q.n_nodes = p->n_nodes; q.n_batch = p->n_batch;
  q.Jac = Jac; q.ldj = ldj; q.defect = defect; q.ldd = ldd; q.X = X; q.ldx = ldx; q.U = U; q.ldu = ldu;
  q.t = t; q.t_stride = (n_tgrids == 1) ? 0 : p->n_nodes;
  q.targets = (const double*)targets; q.impulsive = allow_impulsive ? 1 : 0;
  const double vu = p->prm.DU / p->prm.TU;                 // costEnd = sum(((dV + dV_jump) * DU/TU).^2)  (:377)
  q.c2 = vu * vu;
  q.dX = dX; q.ldX = ldx; q.dU = dU; q.ldU = ldu; q.dV = dV; q.cost = cost;
  q.singular = p->qp_singular_out;
  if (nr > 1) { q.model = (const double*)model; q.beta = beta; q.p = pout; }
  if (nr == 4) { q.dtf = dtf; q.tfb = tfb; q.tf = tf; }
  timing_begin(c, st);
  const hipError_t e = launch_direct_qp(p->nstate, nr, q, p->qp_ws, st);
  timing_end(c, st);
  p->qp_last_nr = (e == hipSuccess) ? nr : 0;
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_direct_qp", e);
  return LTO_OK;
}

extern "C" {

// user-visible direct plans keep the context alive like indirect ones (lto_destroy)
int lto_direct_plan_create(lto_ctx* c, int nstate, int n_nodes, int n_batch, int nsteps, const lto_direct_params* prm,
                           lto_direct_plan** out) {
  const int rc = direct_plan_build(c, nstate, n_nodes, n_batch, nsteps, prm, out);
  if (rc == LTO_OK) ctx_plan_added(c);
  return rc;
}

void lto_direct_plan_destroy(lto_direct_plan* p) {
  if (!p) return;
  lto_ctx* c = p->ctx;
  direct_plan_free(p);
  if (ctx_release(c, OWNER_PLAN)) ctx_free(c);
}

int lto_direct_plan_set_kernel(lto_direct_plan* p, int kernel) {
  if (!p) return LTO_ENULL;
  if (kernel == LTO_KERNEL_COOP)
    return set_err(p->ctx, LTO_EINVAL, "the wave-specialised direct Jacobian kernel was removed in round 3 (never faster than _PER_LANE or _PIPE)");
  if (kernel != LTO_KERNEL_AUTO && kernel != LTO_KERNEL_PER_LANE && kernel != LTO_KERNEL_DIRECT_PIPE)
    return set_err(p->ctx, LTO_EINVAL, "kernel must be LTO_KERNEL_AUTO, _PER_LANE or _DIRECT_PIPE");
  p->kernel = kernel;
  return LTO_OK;
}

int lto_direct_defect_dev(lto_direct_plan* p, void* stream, const double* X, long ldx, const double* U, long ldu,
                          const double* t, int n_tgrids, double* defect, long ldd, double* errors) {
  if (!p) return LTO_ENULL;
  if (!defect) return set_err(p->ctx, LTO_ENULL, "defect is NULL");
  return direct_defect_launch(p, stream, X, ldx, U, ldu, t, n_tgrids, defect, ldd, errors, nullptr, 0);
}

int lto_direct_midpoints_dev(lto_direct_plan* p, void* stream, const double* X, long ldx, const double* U, long ldu,
                             const double* t, int n_tgrids, double* x_mid, long ldm, double* defect, long ldd,
                             double* errors) {
  if (!p) return LTO_ENULL;
  if (!x_mid) return set_err(p->ctx, LTO_ENULL, "x_mid is NULL");
  if (ldm < p->S) return set_err(p->ctx, LTO_EINVAL, "ldm smaller than the segment count");
  return direct_defect_launch(p, stream, X, ldx, U, ldu, t, n_tgrids, defect, ldd, errors, x_mid, ldm);
}

int lto_direct_jacobian_dev(lto_direct_plan* p, void* stream, const double* X, long ldx, const double* U, long ldu,
                            const double* t, int n_tgrids, double* Jac, long ldj, double* dtf, double* defect, long ldd,
                            double* errors) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  DirectArgs a;
  int rc = fill_direct_args(p, X, ldx, U, ldu, t, n_tgrids, &a);
  if (rc) return rc;
  if (!Jac) return set_err(c, LTO_ENULL, "Jac is NULL");
  if (ldj < p->S || ((defect || dtf) && ldd < p->S)) return set_err(c, LTO_EINVAL, "ldj/ldd smaller than the segment count");
  a.Jac = Jac; a.ldj = ldj; a.dtf = dtf; a.defect = defect; a.ldd = ldd; a.errors = errors;
  rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  // measured (MI355X, bench.py --workload c3, ms per sweep; per-lane / wave-specialised / software-pipelined):
  //   29 segments 0.032 / - / 0.047;  2 048: 0.036 / - / 0.049;  4 096: 0.069 / - / 0.051;  8 192: 0.108 / - / 0.055;
  //   16 384 (BASELINE configs[2]): 0.181 / 0.176 / 0.106;  65 536: 0.592 / - / 0.383
  // The pipelined kernel does ~half the arithmetic (the half-arc base state is integrated once per arc, not once per
  // sensitivity column) but needs 10 waves of one workgroup resident per 32 segments: it wins once the per-lane kernel no
  // longer fits the chip in one round.
  int kern = p->kernel;
  if (kern == LTO_KERNEL_AUTO) kern = (p->S >= 3072) ? LTO_KERNEL_DIRECT_PIPE : LTO_KERNEL_PER_LANE;
  hipError_t e = (kern == LTO_KERNEL_DIRECT_PIPE) ? launch_direct_jacobian_pipe(p->nstate, a, st) : launch_direct_jacobian(p->nstate, a, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_direct_jacobian", e);
  return LTO_OK;
}

int lto_direct_qp_step_dev(lto_direct_plan* p, void* stream, const double* Jac, long ldj, const double* defect, long ldd,
                           const double* X, long ldx, const double* U, long ldu, const double* t, int n_tgrids,
                           const lto_direct_targets* targets, int allow_impulsive, double* dX, double* dU, double* dV,
                           double* cost) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!Jac || !defect || !X || !U || !t || !targets || !dX || !dU || !dV || !cost)
    return set_err(c, LTO_ENULL, "lto_direct_qp_step_dev: a required array is NULL");
  const long J = (long)p->n_nodes * p->n_batch;
  if (ldj < p->S || ldd < p->S || ldx < J || ldu < J) return set_err(c, LTO_EINVAL, "ldj/ldd smaller than the segment count or ldx/ldu than the node count");
  if (n_tgrids != 1 && n_tgrids != p->n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  const int rc = bind_device(c);
  if (rc) return rc;
  return direct_qp_launch(p, (hipStream_t)stream, 1, Jac, ldj, defect, ldd, X, ldx, U, ldu, t, n_tgrids, targets, allow_impulsive, dX,
                          dU, dV, cost);
}

const int* lto_direct_plan_qp_status(const lto_direct_plan* p) {
  return (p && p->qp_ws) ? direct_qp_status(p->qp_ws, p->n_batch) : nullptr;
}

}  // extern "C"
