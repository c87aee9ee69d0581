// lto_direct_resample.hip -- direct solutions resampled onto one common node count in one host call: the
// trajectories go up once, every pass is three launches (estimates, grid, nodes) with nothing read back between them, and the
// resampled meshes, their estimates and the statuses come down once.
#include <cmath>

#include "lto_host.hpp"

extern "C" {

int lto_direct_resample_batch(lto_ctx* c, int nstate, int n_cap, int n_batch, const double* X, const double* U, const double* t,
                              const int* n_in, int nsteps, const lto_direct_params* prm, int n_new, const double* weights,
                              double w_floor, int passes, double* X_out, double* U_out, double* t_out, double* errors_before,
                              double* errors_after, int* status) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!X || !U || !t || !prm || !X_out || !U_out || !t_out)
    return set_err(c, LTO_ENULL, "lto_direct_resample_batch: X, U, t, prm, X_out, U_out or t_out is NULL");
  if (nstate != 6 && nstate != 7) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: nstate must be 6 or 7");
  if (n_cap < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: need n_cap >= 2 and n_batch >= 1");
  if (n_new < 2) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: need n_new >= 2");
  if (passes < 1) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: need passes >= 1");
  if (nsteps < 2) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: nsteps (grid points per half segment) must be >= 2");
  if (!std::isfinite(w_floor) || w_floor < 0.0 || !(w_floor < 1.0))
    return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: w_floor must lie in [0, 1)");
  if (weights && passes > 1)
    return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: passes > 1 needs the estimates as the monitor (weights == NULL)");
  const int B = n_batch, NS = nstate, nmax = n_cap > n_new ? n_cap : n_new;
  if (nmax - 1 > kRemeshMaxSegs) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: more than 262144 segments per trajectory");
  if (B > 65535) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: more than 65535 trajectories");
  if ((long)nmax * B * NS > 0x7fffffffL) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: max(n_cap, n_new) * n_batch * nstate beyond 2^31 - 1");
  for (int b = 0; b < B; ++b) {
    const int n = n_in ? n_in[b] : n_cap;
    if (n < 2 || n > n_cap) return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: every n_in[b] must lie in [2, n_cap]");
    const double* tb = t + (size_t)b * n_cap;
    for (int i = 0; i + 1 < n; ++i)
      if (!(tb[i] < tb[i + 1]) || !std::isfinite(tb[i + 1] - tb[i]))
        return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: t must be finite and strictly increasing inside every valid part");
    if (weights) {
      const double* wb = weights + (size_t)b * (n_cap - 1);
      for (int i = 0; i + 1 < n; ++i)
        if (!(wb[i] > 0.0) || !std::isfinite(wb[i]))
          return set_err(c, LTO_EINVAL, "lto_direct_resample_batch: every weight of a valid segment must be finite and > 0");
    }
  }
  int rc = bind_device(c);
  if (rc) return rc;

  const size_t Jin = (size_t)n_cap * B, Jn = (size_t)n_new * B, Smax = (size_t)(nmax - 1) * B;
  const size_t c_stride = nmax - 1 > kRemeshLdsSegs ? remesh_scratch_doubles(nmax) : 0;
  const bool two = passes > 1;
  double *d_Xin, *d_Uin, *d_tin, *d_X[2], *d_U[2], *d_t[2], *d_E, *d_W, *d_C;
  int *d_n, *d_status;
  lto::HostBuf<int> h_status((size_t)B);
  if (!h_status.ok()) return set_err(c, LTO_ENOMEM, "lto_direct_resample_batch: out of host memory");
  HostCall call(c);
  ArenaLayout scratch;
  scratch.add(NS * Jin, d_Xin);
  scratch.add(3 * Jin, d_Uin);
  scratch.add(Jin, d_tin);
  scratch.add(NS * Jn, d_X[0]);
  scratch.add(3 * Jn, d_U[0]);
  scratch.add(Jn, d_t[0]);
  scratch.add(two ? NS * Jn : 0, d_X[1]);
  scratch.add(two ? 3 * Jn : 0, d_U[1]);
  scratch.add(two ? Jn : 0, d_t[1]);
  scratch.add(Smax, d_E, d_W);
  scratch.add(c_stride * B, d_C);
  scratch.add(n_in ? (size_t)B : 0, d_n);
  scratch.add((size_t)B, d_status);
  // a small call works in the context's arena, which only grows (as lto_direct_refine_batch): up to 2^14 nodes; a larger one
  // takes a block of its own, given back at return
  rc = (Jin + Jn <= ((size_t)1 << 14)) ? scratch.reserve(c) : scratch.reserve_block(c, call.block[0], "lto_direct_resample_batch");
  if (rc) return rc;

  hipStream_t st = c->stream;
  hipError_t e = hipMemcpyAsync(d_Xin, X, sizeof(double) * NS * Jin, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_Uin, U, sizeof(double) * 3 * Jin, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tin, t, sizeof(double) * Jin, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_in) e = hipMemcpyAsync(d_n, n_in, sizeof(int) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && weights) e = hipMemcpyAsync(d_W, weights, sizeof(double) * (size_t)(n_cap - 1) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, sizeof(int) * B, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_resample_batch: stage in", e);

  DirectResampleArgs a{};
  a.X = d_Xin; a.U = d_Uin; a.t = d_tin; a.n = n_in ? d_n : nullptr;
  a.cap = n_cap; a.B = B; a.n_new = n_new;
  a.MU = prm->MU;
  a.kk = (prm->TU * prm->TU) / prm->DU / 1e3;    // as fill_direct_args: N/kg -> DU/TU^2   (prop_EP_deriv.jl:32)
  a.isp_g0 = prm->Isp * 9.81;
  a.TU = prm->TU;
  a.half_steps = nsteps - 1;
  a.E = d_E; a.W = d_W; a.from_E = weights ? 0 : 1; a.w_floor = w_floor;
  a.C = c_stride ? d_C : nullptr; a.c_stride = (long)c_stride;
  a.status = d_status;
  timing_begin(c, st);
  for (int pass = 0; pass < passes; ++pass) {
    a.t_new = d_t[pass & 1]; a.X_new = d_X[pass & 1]; a.U_new = d_U[pass & 1];
    const bool before = pass == 0 && errors_before;
    if (a.from_E || before) e = launch_direct_resample_errors(NS, a, st);
    if (e == hipSuccess && before)
      e = hipMemcpyAsync(errors_before, d_E, sizeof(double) * (size_t)(n_cap - 1) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = launch_direct_resample_grid(a, st);
    if (e == hipSuccess) e = launch_direct_resample_nodes(NS, a, st);
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_resample_batch: pass", e);
    a.X = a.X_new; a.U = a.U_new; a.t = a.t_new; a.n = nullptr; a.cap = n_new;   // rectangular from here on
  }
  if (errors_after) e = launch_direct_resample_errors(NS, a, st);
  timing_end(c, st);
  if (e == hipSuccess && errors_after)
    e = hipMemcpyAsync(errors_after, d_E, sizeof(double) * (size_t)(n_new - 1) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(X_out, a.X, sizeof(double) * NS * Jn, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(U_out, a.U, sizeof(double) * 3 * Jn, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_out, a.t, sizeof(double) * Jn, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_resample_batch: stage out", e);
  if (status)
    for (int b = 0; b < B; ++b) status[b] = h_status[b];
  return LTO_OK;
}

int lto_direct_resample(lto_ctx* c, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                        const lto_direct_params* prm, int n_new, const double* weights, double w_floor, int passes, double* X_out,
                        double* U_out, double* t_out, double* errors_before, double* errors_after, int* status) {
  return lto_direct_resample_batch(c, nstate, n_nodes, 1, X, U, t, nullptr, nsteps, prm, n_new, weights, w_floor, passes, X_out,
                                   U_out, t_out, errors_before, errors_after, status);
}

}  // extern "C"
