// lto_stack.hip -- the trajectory-stacking initial guess for a batch of starts.
#include <cmath>
#include <cstring>

#include "lto_host.hpp"

extern "C" {

/* The stacking block of the reference demos (CRTBP_Multishoot_direct_demo.jl:116-157) for n_batch starts (tau1, tof1, tof2) side by
 * side, every phase on the device: the candidates of find_tau and the start states (k_stack_prepare), the coast on the departure
 * halo up to tof1 (k_stack_arc), the junction search (k_stack_find), the coast on the arrival halo (k_stack_arc) and the end
 * search, which also snaps the last node and lays the nodes out for the caller (k_stack_find).  One upload, five launches, the
 * nodes and the per-start scalars come down behind the last launch. */
int lto_stack_guess_batch(lto_ctx* c, int n_nodes, int n_batch, double MU, const lto_direct_orbits* orbits, const lto_integrator* integ,
                          const double* tau1, const double* tof1, const double* tof2, double* X_out, double* t_out, double* tau_out,
                          double* gap_out, int* status) {
  if (!c) return LTO_ENULL;
  if (n_nodes < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: need n_nodes >= 2 and n_batch >= 1");
  if (!orbits || !integ || !tau1 || !tof1 || !tof2 || !X_out || !t_out || !tau_out || !status)
    return set_err(c, LTO_ENULL, "lto_stack_guess_batch: a required argument is NULL");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE)
    return set_err(c, LTO_EUNSUPPORTED, "lto_stack_guess_batch: the coast is built for LTO_RK4 and LTO_DOP853_ADAPTIVE");
  if ((long)6 * n_nodes * n_batch > 0x7fffffffL) return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: batch too large");
  if (integ->method == LTO_RK4 && integ->steps < 1) return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: LTO_RK4 needs steps >= 1");
  if (!(MU > 0.0 && MU < 1.0)) return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: MU must lie in (0, 1)");
  const int n = n_nodes, B = n_batch;
  for (int b = 0; b < B; ++b) {
    if (!(tof1[b] > 0.0) || !std::isfinite(tof1[b]) || !(tof2[b] > 0.0) || !std::isfinite(tof2[b]))
      return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: every tof1 and tof2 must be finite and > 0");
    if (!(std::fabs(tau1[b]) < 1e6)) return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: every tau1 must be finite with |tau1| < 1e6");
  }
  if (orbits->n0 < 2 || orbits->nf < 2 || !orbits->t0 || !orbits->X0 || !orbits->tf || !orbits->Xf)
    return set_err(c, LTO_EINVAL, "lto_stack_guess_batch: orbit tables need >= 2 samples each and non-NULL arrays");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  // host side: the grids (t_out [n x B] for the caller, [n][B] for the device), the arcs' node ranges, the wrapped tau1.
  // One block goes up: tau1 [B] | tof1 [B] | t [n][B] | n1 [B] (ints), n1 = the nodes with t_k < tof1 (strict, :122)
  const size_t in_doubles = (size_t)(2 + n) * B, in_bytes = al256(sizeof(double) * in_doubles) + sizeof(int) * (size_t)B;
  lto::HostBuf<char> h_in(in_bytes);
  lto::HostBuf<double> h_sc((size_t)5 * B);      // what comes down: tau2_0 | tau2 | gap0 | gap1 | status (ints)
  if (!h_in.ok() || !h_sc.ok()) return set_err(c, LTO_ENOMEM, "lto_stack_guess_batch: out of host memory");
  double* h_tau1 = (double*)h_in.data();
  double* h_tof1 = h_tau1 + B;
  double* h_t = h_tof1 + B;
  int* h_n1 = (int*)(h_in.data() + al256(sizeof(double) * in_doubles));
  for (int b = 0; b < B; ++b) {
    h_tau1[b] = tau1[b];
    h_tof1[b] = tof1[b];
    double* tb = t_out + (size_t)b * n;
    linrange(0.0, tof1[b] + tof2[b], n, tb);
    int n1 = 0;
    for (int k = 0; k < n; ++k) {
      h_t[(size_t)k * B + b] = tb[k];
      if (tb[k] < tof1[b]) n1 = k + 1;           // the grid increases: the count of nodes before tof1
    }
    h_n1[b] = n1;
    double x = tau1[b];                          // the reference's wrap (interpEndStates), as end_spline applies it
    while (x > 1.0) x -= 1.0;
    while (x < 0.0) x += 1.0;
    tau_out[(size_t)3 * b] = x;
  }
  // device side
  char* d_in;
  double *d_cand, *d_y0, *d_x1e, *d_yf0, *d_xend, *d_X, *d_Xo, *d_sc;
  ArenaLayout scratch;
  scratch.add(in_bytes, d_in);
  scratch.add((size_t)6 * kStackCandLd, d_cand);
  scratch.add((size_t)6 * B, d_y0, d_x1e, d_yf0, d_xend);
  scratch.add((size_t)6 * n * B, d_X, d_Xo);
  scratch.add((size_t)5 * B, d_sc);
  DevOrbits dob;
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = orbits_upload(c, orbits, dob, st);
  if (rc) return rc;
  rc = scratch.reserve(c);
  if (rc) return rc;
  const double* d_tau1 = (const double*)d_in;
  const double* d_tof1 = d_tau1 + B;
  const double* d_t = d_tof1 + B;
  const int* d_n1 = (const int*)(d_in + al256(sizeof(double) * in_doubles));
  double *d_tau20 = d_sc, *d_tau2 = d_sc + B, *d_gap0 = d_sc + 2 * (size_t)B, *d_gap1 = d_sc + 3 * (size_t)B;
  int* d_status = (int*)(d_sc + 4 * (size_t)B);
  hipError_t e = hipMemcpyAsync(d_in, h_in.data(), in_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_stack_prepare(dob.o, d_tau1, B, d_cand, d_y0, st);
  StackArcArgs a;
  a.t = d_t; a.n = n; a.B = B; a.MU = MU; a.X = d_X;
  a.steps = integ->steps; a.rtol = integ->rtol; a.atol = integ->atol;
  a.max_steps = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  // arc 1: nodes [0, n1) from the departure state at time 0, then on to tof1 itself
  a.y0 = d_y0; a.k0 = nullptr; a.k1 = d_n1; a.t_start = nullptr; a.t_end = d_tof1; a.xe = d_x1e;
  if (e == hipSuccess) e = launch_stack_arc(integ->method, a, st);
  StackFindArgs f;
  f.o = dob.o; f.cand = d_cand; f.n = n; f.B = B;
  f.x = d_x1e; f.tau = d_tau20; f.gap = d_gap0; f.snap = d_yf0; f.X = nullptr; f.X_out = nullptr; f.status = nullptr;
  if (e == hipSuccess) e = launch_stack_find(f, st);
  // arc 2: nodes [n1, n) from the junction state at time tof1; its end state is node n - 1
  a.y0 = d_yf0; a.k0 = d_n1; a.k1 = nullptr; a.t_start = d_tof1; a.t_end = nullptr; a.xe = d_xend;
  if (e == hipSuccess) e = launch_stack_arc(integ->method, a, st);
  f.x = d_xend; f.tau = d_tau2; f.gap = d_gap1; f.snap = nullptr; f.X = d_X; f.X_out = d_Xo; f.status = d_status;
  if (e == hipSuccess) e = launch_stack_find(f, st);
  if (e == hipSuccess) e = hipMemcpyAsync(X_out, d_Xo, sizeof(double) * 6 * n * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_sc.data(), d_sc, sizeof(double) * 5 * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_stack_guess_batch", e);
  const int* h_status = (const int*)(h_sc.data() + 4 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    tau_out[(size_t)3 * b + 1] = h_sc[b];
    tau_out[(size_t)3 * b + 2] = h_sc[(size_t)B + b];
    if (gap_out) { gap_out[(size_t)2 * b] = h_sc[2 * (size_t)B + b]; gap_out[(size_t)2 * b + 1] = h_sc[3 * (size_t)B + b]; }
    status[b] = h_status[b];
  }
  return LTO_OK;
}

}  // extern "C"
