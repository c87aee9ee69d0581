// lto_direct_refine.hip -- errors-driven mesh refinement of the direct transcription in one host call: the
// trajectories go up once, the removal phase is one launch, every insertion pass is two launches and one read-back of the node
// counts, and the refined meshes come down once.
#include <cmath>

#include "lto_host.hpp"

extern "C" {

int lto_direct_refine_batch(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                            int n_tgrids, int nsteps, const lto_direct_params* prm, double tol_min, double tol_max, int max_nodes,
                            double* X_out, double* U_out, double* t_out, int* n_out, int* n_removed, int* passes, int* status,
                            double* errors_out) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!X || !U || !t || !prm || !X_out || !t_out || !n_out)
    return set_err(c, LTO_ENULL, "lto_direct_refine_batch: X, U, t, prm, X_out, t_out or n_out is NULL");
  if (nstate != 6 && nstate != 7) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: nstate must be 6 or 7");
  if (n_nodes < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: need n_nodes >= 2 and n_batch >= 1");
  if (nsteps < 2) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: nsteps (grid points per half segment) must be >= 2");
  if (max_nodes < n_nodes) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: max_nodes is the capacity of the outputs: it must be >= n_nodes");
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: n_tgrids must be 1 or n_batch");
  if (std::isnan(tol_min) || std::isnan(tol_max)) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: a tolerance is NaN");
  const int B = n_batch, M = max_nodes, NS = nstate;
  if ((long)M * B * NS > 0x7fffffffL || B > 65535) return set_err(c, LTO_EINVAL, "lto_direct_refine_batch: max_nodes * n_batch too large, or more than 65535 trajectories");
  int rc = bind_device(c);
  if (rc) return rc;

  const size_t Jin = (size_t)n_nodes * B, J = (size_t)M * B;
  DirectRefineArgs a{};
  double *d_Xin, *d_Uin, *d_tin;
  lto::HostBuf<int> h_ctl((size_t)RC_ROWS * B);
  if (!h_ctl.ok()) return set_err(c, LTO_ENOMEM, "lto_direct_refine_batch: out of host memory");
  HostCall call(c);
  ArenaLayout scratch;
  scratch.add(NS * Jin, d_Xin);
  scratch.add(3 * Jin, d_Uin);
  scratch.add((size_t)n_nodes * n_tgrids, d_tin);
  scratch.add(Jin, a.E0);
  scratch.add(NS * J, a.X[0], a.X[1], a.X_out);
  scratch.add(3 * J, a.U[0], a.U[1], a.U_out);
  scratch.add(J, a.t[0], a.t[1], a.t_out, a.E[0], a.E[1], a.E_out);
  scratch.add(J, a.list);
  scratch.add((size_t)RC_ROWS * B, a.ctl);
  const bool in_lds = n_nodes <= kRefineLdsNodes;
  scratch.add(in_lds ? 0 : Jin, a.rm_est);
  scratch.add(in_lds ? 0 : 2 * Jin, a.rm_link);
  // a small call works in the context's arena, which only grows: up to 2^14 nodes of capacity, about 5 MB at 37 doubles per
  // node, is the most this call leaves in the context; a larger one takes a block of its own, given back at return
  rc = (J <= ((size_t)1 << 14)) ? scratch.reserve(c) : scratch.reserve_block(c, call.block[0], "lto_direct_refine_batch");
  if (rc) return rc;
  if (in_lds) { a.rm_est = nullptr; a.rm_link = nullptr; }
  a.X_in = d_Xin; a.U_in = d_Uin; a.t_in = d_tin; a.t_in_stride = (n_tgrids == 1) ? 0 : n_nodes;
  a.n_in = n_nodes; a.M = M; a.B = B;
  a.MU = prm->MU;
  a.kk = (prm->TU * prm->TU) / prm->DU / 1e3;    // as fill_direct_args: N/kg -> DU/TU^2   (prop_EP_deriv.jl:32)
  a.isp_g0 = prm->Isp * 9.81;
  a.TU = prm->TU;
  a.half_steps = nsteps - 1;
  a.tol_min = tol_min; a.tol_max = tol_max;

  hipStream_t st = c->stream;
  hipError_t e = hipMemcpyAsync(d_Xin, X, sizeof(double) * NS * Jin, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_Uin, U, sizeof(double) * 3 * Jin, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tin, t, sizeof(double) * (size_t)n_nodes * n_tgrids, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_refine_batch: stage in", e);
  timing_begin(c, st);
  e = launch_direct_refine_begin(NS, a, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_refine_batch: removal", e);
  // Insertion passes.  The grid of a pass' evaluation is sized by what the host knows: a trajectory of n nodes splits at most
  // min(n - 1, max_nodes - n) segments; before the first read-back n <= n_nodes.
  int bound = n_nodes - 1;
  for (;;) {
    e = launch_direct_refine_pass(NS, a, bound, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_ctl.data(), a.ctl, sizeof(int) * RC_ROWS * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_refine_batch: insertion pass", e);
    bound = 0;
    for (int b = 0; b < B; ++b) {
      if (!h_ctl[RC_ACTIVE * B + b]) continue;
      const int n = h_ctl[RC_N * B + b];
      const int most = (n - 1 < M - n) ? n - 1 : M - n;
      if (most > bound) bound = most;
      if (bound < 1) bound = 1;                  // at its limit: one more visit of k_refine_split sets its status
    }
    if (bound == 0) break;                       // nobody is left in the loop
  }
  call.idle = false;
  e = launch_direct_refine_finish(NS, a, st);
  timing_end(c, st);
  if (e == hipSuccess) e = hipMemcpyAsync(X_out, a.X_out, sizeof(double) * NS * J, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && U_out) e = hipMemcpyAsync(U_out, a.U_out, sizeof(double) * 3 * J, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_out, a.t_out, sizeof(double) * J, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && errors_out) e = hipMemcpyAsync(errors_out, a.E_out, sizeof(double) * (size_t)(M - 1) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_refine_batch: stage out", e);
  for (int b = 0; b < B; ++b) {
    n_out[b] = h_ctl[RC_N * B + b];
    if (n_removed) n_removed[b] = h_ctl[RC_REMOVED * B + b];
    if (passes) passes[b] = h_ctl[RC_PASSES * B + b];
    if (status) status[b] = h_ctl[RC_STATUS * B + b];
  }
  return LTO_OK;
}

int lto_direct_refine(lto_ctx* c, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                      const lto_direct_params* prm, double tol_min, double tol_max, int max_nodes, double* X_out, double* U_out,
                      double* t_out, int* n_out, int* n_removed, int* passes, int* status, double* errors_out) {
  return lto_direct_refine_batch(c, nstate, n_nodes, 1, X, U, t, 1, nsteps, prm, tol_min, tol_max, max_nodes, X_out, U_out, t_out,
                                 n_out, n_removed, passes, status, errors_out);
}

}  // extern "C"
