// lto_direct_solve.hip -- the direct multiple-shooting host paths: end states on the orbit tables, the QP step on host arrays and
// the batched solve loop with frozen ends, free ends and free tf.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "lto_host.hpp"

// the argument rules of a free tf, per trajectory b (bounds tfb[n_targets == 1 ? 0 : b], grid n_tgrids == 1 ? 0 : b): step >= 0,
// tf_min <= tf <= tf_max with tf the grid's last entry, and tf_min > t0 (the reference's tf >= 0 with t0 = 0 allows an empty grid)
static int tf_bounds_check(lto_ctx* c, const lto_direct_tf_bounds* tfb, int n_targets, const double* t, int n_tgrids, int n_nodes,
                           int n_batch) {
  for (int b = 0; b < n_batch; ++b) {
    const lto_direct_tf_bounds& q = tfb[n_targets == 1 ? 0 : b];
    const double* g = t + (size_t)(n_tgrids == 1 ? 0 : b) * n_nodes;
    const double t0 = g[0], tf = g[n_nodes - 1];
    const char* why = !(q.step >= 0.0) ? "tf bounds: step must be >= 0"
                      : !(tf >= q.tf_min && tf <= q.tf_max) ? "tf bounds: tf (the grid's last entry) outside [tf_min, tf_max]"
                      : !(q.tf_min > t0) ? "tf bounds: tf_min must lie past t0"
                                         : nullptr;
    if (why) return c ? set_err(c, LTO_EINVAL, why) : LTO_EINVAL;
  }
  return LTO_OK;
}

// the checks the direct QP-step and solve entries share, in their order: the shape, and for a free tf (free_tf) the counts and the tf
// bounds (given t and tfb), answer without a context, so without a device; then the context.  The entry checks its arrays next.
static int direct_entry_check(lto_ctx* c, int nstate, int n_nodes, int n_batch, int n_tgrids, int n_targets, bool free_tf,
                              const double* t, const lto_direct_tf_bounds* tfb) {
  if ((nstate != 6 && nstate != 7) || n_nodes < 2 || n_batch < 1) return c ? set_err(c, LTO_EINVAL, "need nstate 6 or 7, n_nodes >= 2, n_batch >= 1") : LTO_EINVAL;
  if (free_tf) {
    if ((n_targets != 1 && n_targets != n_batch) || (n_tgrids != 1 && n_tgrids != n_batch))
      return c ? set_err(c, LTO_EINVAL, "n_targets / n_tgrids must be 1 or n_batch") : LTO_EINVAL;
    if (t && tfb) {
      const int rc = tf_bounds_check(c, tfb, n_targets, t, n_tgrids, n_nodes, n_batch);
      if (rc) return rc;
    }
  }
  return c ? LTO_OK : LTO_ENULL;
}

static bool orbits_ok(const lto_direct_orbits* ob) {
  return ob && ob->n0 >= 2 && ob->nf >= 2 && ob->t0 && ob->X0 && ob->tf && ob->Xf;
}
int orbits_upload(lto_ctx* c, const lto_direct_orbits* ob, DevOrbits& d, hipStream_t st) {
  const int n[2] = {ob->n0, ob->nf};
  const double* T[2] = {ob->t0, ob->tf};
  const double* Y[2] = {ob->X0, ob->Xf};
  for (int e = 0; e < 2; ++e)
    for (int i = 0; i + 1 < n[e]; ++i)
      if (!(T[e][i + 1] > T[e][i])) return set_err(c, LTO_EINVAL, "orbit table times must increase strictly");
  const size_t tot = (size_t)13 * (n[0] + n[1]);
  lto::HostBuf<double> h(tot, 0.0), cp, dp;
  if (!h.ok() || !cp.alloc((size_t)std::max(n[0], n[1])) || !dp.alloc((size_t)6 * std::max(n[0], n[1])))
    return set_err(c, LTO_ENOMEM, "orbit tables: out of host memory");
  size_t off = 0;
  size_t offs[2][3];
  for (int e = 0; e < 2; ++e) {
    const int m = n[e];
    const double* t = T[e];
    double* ht = &h[off];
    double* hY = ht + m;
    double* hM = hY + 6 * (size_t)m;
    offs[e][0] = off; offs[e][1] = off + m; offs[e][2] = off + 7 * (size_t)m;
    off += 13 * (size_t)m;
    for (int i = 0; i < m; ++i) { ht[i] = t[i]; for (int j = 0; j < 6; ++j) hY[j + 6 * i] = Y[e][j + 6 * (size_t)i]; }
    // natural spline (M_0 = M_{m-1} = 0): h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 (slope_i - slope_{i-1}), Thomas
    for (int j = 0; j < 6; ++j) { hM[j] = 0.0; hM[j + 6 * (size_t)(m - 1)] = 0.0; }
    if (m > 2) {
      for (int i = 1; i < m - 1; ++i) {
        const double h0 = t[i] - t[i - 1], h1 = t[i + 1] - t[i];
        const double diag = 2.0 * (h0 + h1) - (i > 1 ? h0 * cp[i - 1] : 0.0);
        cp[i] = h1 / diag;
        for (int j = 0; j < 6; ++j) {
          const double r = 6.0 * ((hY[j + 6 * (i + 1)] - hY[j + 6 * i]) / h1 - (hY[j + 6 * i] - hY[j + 6 * (i - 1)]) / h0);
          dp[j + 6 * (size_t)i] = (r - (i > 1 ? h0 * dp[j + 6 * (size_t)(i - 1)] : 0.0)) / diag;
        }
      }
      for (int i = m - 2; i >= 1; --i)
        for (int j = 0; j < 6; ++j) hM[j + 6 * (size_t)i] = dp[j + 6 * (size_t)i] - cp[i] * hM[j + 6 * (size_t)(i + 1)];
    }
  }
  hipError_t e = hipMalloc(&d.buf, sizeof(double) * tot);
  if (e != hipSuccess) { d.buf = nullptr; return set_err(c, LTO_EHIP, "orbit tables", e); }
  e = hipMemcpyAsync(d.buf, h.data(), sizeof(double) * tot, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = stream_wait(st);                // h is released on return
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "orbit tables", e);
  for (int k = 0; k < 2; ++k) {
    d.o.n[k] = n[k];
    d.o.t[k] = d.buf + offs[k][0]; d.o.Y[k] = d.buf + offs[k][1]; d.o.M[k] = d.buf + offs[k][2];
  }
  return LTO_OK;
}

static bool direct_targets_expand(const lto_direct_targets* targets, int n_targets, int B, lto::HostBuf<lto_direct_targets>& out) {
  if (!out.alloc((size_t)B)) return false;
  for (int b = 0; b < B; ++b) out[(size_t)b] = targets[n_targets == 1 ? 0 : b];
  return true;
}

// one Jacobian sweep and one QP step on host arrays with nr right-hand sides (direct_qp_launch): model and beta for nr > 1, tfb for
// nr = 4, one or one per target; p_out [n_batch][nr - 1] for nr > 1.  tf is each grid's last entry.
static int direct_qp_step_host(lto_ctx* c, const char* who, int nr, int nstate, int n_nodes, int n_batch, const double* X,
                               const double* U, const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                               const lto_direct_targets* targets, const lto_direct_end_model* model, const double* beta,
                               const lto_direct_tf_bounds* tfb, int n_targets, int allow_impulsive, double* dX, double* dU, double* dV,
                               double* p_out, double* cost) {
  int rc = direct_entry_check(c, nstate, n_nodes, n_batch, n_tgrids, n_targets, nr == 4, t, tfb);
  if (rc) return rc;
  char msg[96];
  if (!X || !U || !t || !prm || !targets || !dX || !dU || !dV || !cost || (nr > 1 && (!model || !beta || !p_out)) || (nr == 4 && !tfb)) {
    std::snprintf(msg, sizeof msg, "%s: a required array is NULL", who);
    return set_err(c, LTO_ENULL, msg);
  }
  if ((n_targets != 1 && n_targets != n_batch) || (n_tgrids != 1 && n_tgrids != n_batch))
    return set_err(c, LTO_EINVAL, "n_targets / n_tgrids must be 1 or n_batch");
  CallTimer call_timer(c);
  const int B = n_batch;
  const size_t nh = nr == 4 ? 5 * (size_t)B : nr == 3 ? (size_t)B : 0;   // beta [B] (| tf bounds [B][3] | tf [B])
  lto::HostBuf<lto_direct_targets> tg;
  lto::HostBuf<lto_direct_end_model> em(nr > 1 ? (size_t)B : 0);
  lto::HostBuf<double> hb(nh);
  lto::HostBuf<int> h_stat(B, 0);
  HostCall call(c);
  rc = direct_plan_build(c, nstate, n_nodes, n_batch, nsteps, prm, &call.dplan[0]);
  if (rc) return rc;
  lto_direct_plan* p = call.dplan[0];
  if (!direct_targets_expand(targets, n_targets, B, tg) || !em.ok() || !hb.ok() || !h_stat.ok()) {
    std::snprintf(msg, sizeof msg, "%s: out of host memory", who);
    return set_err(c, LTO_ENOMEM, msg);
  }
  for (int b = 0; b < B && nr > 1; ++b) {
    const int k = n_targets == 1 ? 0 : b;
    em[b] = model[k]; hb[b] = beta[k];
    if (nr == 4) {
      hb[B + 3 * b] = tfb[k].step; hb[B + 3 * b + 1] = tfb[k].tf_min; hb[B + 3 * b + 2] = tfb[k].tf_max;
      hb[4 * (size_t)B + b] = t[(size_t)(n_tgrids == 1 ? 0 : b) * n_nodes + n_nodes - 1];
    }
  }
  const long J = (long)n_nodes * B, S = p->S;
  const int nj = nstate * 2 * (nstate + 3);
  double *d_xa, *d_X, *d_dX, *d_dXa, *d_ua, *d_U, *d_dU, *d_dUa, *d_t, *d_jac, *d_def, *d_dtf = nullptr, *d_dV, *d_cost, *d_p, *d_hb;
  lto_direct_targets* d_tg;
  lto_direct_end_model* d_em;
  ArenaLayout scratch;
  scratch.add((size_t)nstate * J, d_xa, d_X, d_dX, d_dXa);
  scratch.add((size_t)3 * J, d_ua, d_U, d_dU, d_dUa);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)nj * S, d_jac);
  scratch.add((size_t)nstate * S, d_def);
  if (nr == 4) scratch.add((size_t)nstate * S, d_dtf);
  scratch.add((size_t)B, d_tg);
  scratch.add(em.size(), d_em);
  scratch.add((size_t)7 * B, d_dV, d_cost, d_p);
  scratch.add(nh, d_hb);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, X, nstate, J, d_xa, d_X, J, st);
  if (e == hipSuccess) e = stage_in(c, U, 3, J, d_ua, d_U, J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)n_nodes * n_tgrids, d_t, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tg, tg.data(), sizeof(lto_direct_targets) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && nr > 1) e = hipMemcpyAsync(d_em, em.data(), sizeof(lto_direct_end_model) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && nr > 1) e = hipMemcpyAsync(d_hb, hb.data(), sizeof(double) * nh, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  rc = lto_direct_jacobian_dev(p, st, d_X, J, d_U, J, d_t, n_tgrids, d_jac, S, d_dtf, d_def, S, nullptr);
  if (rc == LTO_OK)
    rc = direct_qp_launch(p, st, nr, d_jac, S, d_def, S, d_X, J, d_U, J, d_t, n_tgrids, d_tg, allow_impulsive, d_dX, d_dU, d_dV, d_cost,
                          d_em, d_hb, d_p, d_dtf, d_hb + B, d_hb + 4 * (size_t)B);
  if (rc == LTO_OK) {
    e = stage_out(c, d_dX, J, nstate, J, d_dXa, dX, st);
    if (e == hipSuccess) e = stage_out(c, d_dU, J, 3, J, d_dUa, dU, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dV, d_dV, sizeof(double) * 6 * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && nr > 1) e = hipMemcpyAsync(p_out, d_p, sizeof(double) * (nr - 1) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cost, d_cost, sizeof(double) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_stat.data(), lto_direct_plan_qp_status(p), sizeof(int) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
    for (int b = 0; b < B && rc == LTO_OK; ++b)
      if (h_stat[b]) rc = set_err(c, LTO_ESINGULAR, "the KKT system of a trajectory's QP step is singular (too few nodes to reach the terminal state?)");
  }
  return rc;
}

// free ends of lto_direct_solve_free_batch (null for lto_direct_solve_batch); tfb non-null: lto_direct_solve_free_tf_batch
struct DirectFreeEnds {
  const lto_direct_orbits* orbits;
  const double* tau_in;       // [2 x n_batch]
  const double* beta;        // [n_targets]
  int flag_end;
  double* tau_out;            // [2 x n_batch] or null
  const lto_direct_tf_bounds* tfb;   // [n_targets] or null
};

static int direct_solve_impl(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                             const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                             const lto_direct_targets* targets, int n_targets, int allow_impulsive, int maxIter, double* X_out,
                             double* U_out, double* dV_out, double* t_out, double* defect_out, int* status_flag, int* iterations,
                             double* history, const DirectFreeEnds* fe) {
  int rc = direct_entry_check(c, nstate, n_nodes, n_batch, n_tgrids, n_targets, false, nullptr, nullptr);
  if (rc) return rc;
  if (!X_in || !U_in || !t || !prm || !targets || !X_out || !status_flag)
    return set_err(c, LTO_ENULL, "X_in, U_in, t, prm, targets, X_out or status is NULL");
  if (fe && (!fe->orbits || !fe->tau_in || !fe->beta)) return set_err(c, LTO_ENULL, "orbits, tau_in or beta is NULL");
  if (fe && !orbits_ok(fe->orbits)) return set_err(c, LTO_EINVAL, "orbit tables need >= 2 samples each and non-NULL arrays");
  const int hw = fe ? (fe->tfb ? 6 : 5) : 3;               // history row: max|defect|, cost, alpha (, tau1, tau2 (, tf))
  if (maxIter < 0) return set_err(c, LTO_EINVAL, "maxIter must be >= 0");
  if ((n_tgrids != 1 && n_tgrids != n_batch) || (n_targets != 1 && n_targets != n_batch)) return set_err(c, LTO_EINVAL, "n_tgrids / n_targets must be 1 or n_batch");
  constexpr int NA = 10;                                   // LinRange(0.1, 1, 10), :412
  const int B = n_batch;
  // free tf: with flag_end and a positive step for some trajectory.  Otherwise a free-tf call is the free-end loop
  // with history row 5 the constant tf.
  bool tfm = false;
  if (fe && fe->tfb && fe->flag_end)
    for (int b = 0; b < B; ++b) if (fe->tfb[n_targets == 1 ? 0 : b].step > 0.0) tfm = true;
  if ((long)B * NA * (n_nodes - 1) > 0x3fffffffL) return set_err(c, LTO_EINVAL, "too many line-search segments");
  const long n = n_nodes, J = n * B, S = (n - 1) * B;
  const int nj = nstate * 2 * (nstate + 3);
  // t recomputed through tau with tf unchanged (:478-480, :582): the grid of every iteration after the first update, and the
  // grid of the QP's weights (t_TU_fixed, :321); the ten trial trajectories of trajectory b carry its grid
  lto::HostBuf<double> t1((size_t)n * n_tgrids), tl((size_t)n * B * NA);
  lto::HostBuf<lto_direct_targets> tg;
  if (!t1.ok() || !tl.ok() || !direct_targets_expand(targets, n_targets, B, tg)) return set_err(c, LTO_ENOMEM, "lto_direct_solve_batch: out of host memory");
  for (int g = 0; g < n_tgrids; ++g) {
    const double* tg0 = t + (size_t)g * n;
    const double t0 = tg0[0], tf = tg0[n - 1];
    for (long k = 0; k < n; ++k) {
      const double tau = (tg0[k] - t0) / (tf - t0) * 2.0 - 1.0;
      t1[(size_t)g * n + k] = t0 + (tau + 1.0) / 2.0 * (tf - t0);
    }
  }
  for (int b = 0; b < B; ++b) for (int a = 0; a < NA; ++a)
    std::memcpy(&tl[((size_t)b * NA + a) * n], &t1[(size_t)(n_tgrids == 1 ? 0 : b) * n], sizeof(double) * n);
  DevOrbits dob;
  NewtonBatch nb(B, NA);                                   // er = 1.0 (:488)
  lto::HostBuf<double> h_back((size_t)(fe ? 7 : 4) * B);
  lto::HostBuf<char> moved(B, 0);
  HostCall call(c);
  rc = direct_plan_build(c, nstate, n_nodes, B, nsteps, prm, &call.dplan[0]);
  if (rc == LTO_OK) rc = direct_plan_build(c, nstate, n_nodes, B * NA, nsteps, prm, &call.dplan[1]);
  if (rc) return rc;
  lto_direct_plan* p = call.dplan[0];
  lto_direct_plan* pl = call.dplan[1];                     // the line search's trial trajectories
  const size_t n_small = 6 * (size_t)B + 2 * (size_t)NA * B + NA + 64;
  double *d_aos, *d_X, *d_dX, *d_uaos, *d_U, *d_dU, *d_Xt, *d_t, *d_t1, *d_tl, *d_jac, *d_def, *d_def_aos, *d_deft, *d_dV, *d_small;
  lto_direct_targets* d_tg;
  ArenaLayout scratch;
  scratch.add((size_t)nstate * J, d_aos, d_X, d_dX);
  scratch.add((size_t)3 * J, d_uaos, d_U, d_dU);
  scratch.add((size_t)(nstate + 3) * J * NA, d_Xt);
  scratch.add((size_t)n * n_tgrids, d_t, d_t1);
  scratch.add((size_t)n * B * NA, d_tl);
  scratch.add((size_t)nj * S, d_jac);
  scratch.add((size_t)nstate * S, d_def, d_def_aos);
  scratch.add((size_t)nstate * S * NA, d_deft);
  scratch.add((size_t)B, d_tg);
  scratch.add((size_t)6 * B, d_dV);
  scratch.add(n_small, d_small);
  rc = scratch.reserve(c);
  if (rc) return rc;
  double* d_Ut = d_Xt + (size_t)nstate * J * NA;
  double* d_step = d_small;                                // [B]    step length (0 = frozen)      } read back together
  double* d_mx = d_step + B;                               // [B]    max |defect|                 }
  double* d_cost = d_mx + B;                               // [B]    QP objective                 } read back together
  double* d_sing = d_cost + B;                             // [B]    1 = singular KKT system      }
  double* d_act = d_sing + B;                              // [B]    1 = trajectory still in its loop
  double* d_search = d_act + B;                            // [B]    1 = line search on (iteration > 10)
  double* d_ss = d_search + B;                             // [NA*B] per-trial sums of squares
  double* d_alphas = d_ss + (size_t)NA * B;                // [NA]
  p->qp_singular_out = d_sing;
  (void)report_reserve(c, (size_t)(fe ? 7 : 4) * B);
  hipStream_t st = c->stream;
  // free ends: tau [2B] | tf [B] (one buffer: the loop reads them back in one run), p [3B], end model [14B], beta [B], tf bounds [3B],
  // t0 [B] on the device, the orbit tables with their spline moments; free tf also: the grids [B][n] | tau_grid [B][n] (one buffer:
  // they arrive in one copy) and the tf column [nstate][S]
  double *d_tau = nullptr, *d_tf = nullptr, *d_p = nullptr, *d_em = nullptr, *d_beta = nullptr, *d_tfb = nullptr, *d_t0 = nullptr;
  double *d_tb = nullptr, *d_taug = nullptr, *d_dtf = nullptr;
  if (fe) {
    rc = orbits_upload(c, fe->orbits, dob, st);
    lto::HostBuf<double> hb((size_t)6 * B), hg(tfm ? (size_t)2 * n * B : 1);   // beta [B] | tf [B] | t0 [B] | tf bounds [3B]
    if (rc == LTO_OK && (!hb.ok() || !hg.ok())) rc = set_err(c, LTO_ENOMEM, "lto_direct_solve_free_batch: out of host memory");
    if (rc == LTO_OK) {
      for (int b = 0; b < B; ++b) hb[b] = fe->beta[n_targets == 1 ? 0 : b];
      ArenaLayout ends;
      ends.add((size_t)3 * B, d_tau);                      // tau [2B] | tf [B]
      ends.add((size_t)3 * B, d_p);
      ends.add((size_t)14 * B, d_em);
      ends.add((size_t)B, d_beta);
      ends.add((size_t)3 * B, d_tfb);
      ends.add((size_t)B, d_t0);
      rc = ends.reserve_block(c, call.block[0], "free-end buffers");
    }
    if (rc == LTO_OK) {
      d_tf = d_tau + 2 * (size_t)B;
      hipError_t e0 = hipMemcpyAsync(d_tau, fe->tau_in, sizeof(double) * 2 * B, hipMemcpyHostToDevice, st);
      if (e0 == hipSuccess) e0 = hipMemcpyAsync(d_beta, hb.data(), sizeof(double) * B, hipMemcpyHostToDevice, st);
      if (e0 == hipSuccess) e0 = hipMemsetAsync(d_p, 0, sizeof(double) * 3 * B, st);
      if (e0 == hipSuccess && tfm) {
        // tf, t0, the bounds and tau_grid of every trajectory from its entry grid (:478-480); the grids start as t1
        for (int b = 0; b < B; ++b) {
          const lto_direct_tf_bounds& q = fe->tfb[n_targets == 1 ? 0 : b];
          const double* g = t + (size_t)(n_tgrids == 1 ? 0 : b) * n;
          hb[B + b] = g[n - 1]; hb[2 * (size_t)B + b] = g[0];
          hb[3 * (size_t)B + 3 * b] = q.step; hb[3 * (size_t)B + 3 * b + 1] = q.tf_min; hb[3 * (size_t)B + 3 * b + 2] = q.tf_max;
          for (long k = 0; k < n; ++k) {
            hg[(size_t)b * n + k] = t1[(size_t)(n_tgrids == 1 ? 0 : b) * n + k];
            hg[(size_t)(B + b) * n + k] = (g[k] - g[0]) / (g[n - 1] - g[0]) * 2.0 - 1.0;
          }
        }
        ArenaLayout grids;
        grids.add((size_t)2 * n * B, d_tb);                // grids [B][n] | tau_grid [B][n]
        grids.add((size_t)nstate * S, d_dtf);
        rc = grids.reserve_block(c, call.block[1], "free-end buffers");
        if (rc == LTO_OK) {
          d_taug = d_tb + (size_t)n * B;
          e0 = hipMemcpyAsync(d_tf, &hb[B], sizeof(double) * B, hipMemcpyHostToDevice, st);
          if (e0 == hipSuccess) e0 = hipMemcpyAsync(d_t0, &hb[2 * (size_t)B], sizeof(double) * B, hipMemcpyHostToDevice, st);
          if (e0 == hipSuccess) e0 = hipMemcpyAsync(d_tfb, &hb[3 * (size_t)B], sizeof(double) * 3 * B, hipMemcpyHostToDevice, st);
          if (e0 == hipSuccess) e0 = hipMemcpyAsync(d_tb, hg.data(), sizeof(double) * 2 * n * B, hipMemcpyHostToDevice, st);
        }
      }
      if (rc == LTO_OK && e0 == hipSuccess) e0 = stream_wait(st);        // hb and hg are released at the end of this block
      if (rc == LTO_OK && e0 != hipSuccess) rc = set_err(c, LTO_EHIP, "free-end buffers", e0);
    }
    if (rc == LTO_OK && fe->flag_end) rc = direct_qp_workspace(p, tfm ? 4 : 3);
    if (rc) return rc;
  }
  if (!nb.ok() || !h_back.ok() || !moved.ok()) return set_err(c, LTO_ENOMEM, "lto_direct_solve_batch: out of host memory");
  hipError_t e = stage_in(c, X_in, nstate, J, d_aos, d_X, J, st);
  if (e == hipSuccess) e = stage_in(c, U_in, 3, J, d_uaos, d_U, J, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t, t, sizeof(double) * n * n_tgrids, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t1, t1.data(), sizeof(double) * n * n_tgrids, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tl, tl.data(), sizeof(double) * n * B * NA, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tg, tg.data(), sizeof(lto_direct_targets) * B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_alphas, nb.alphas.data(), sizeof(double) * NA, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_small, 0, sizeof(double) * 4 * B, st);
  // free ends: s0 and sf of the targets from tau (interpEndStates at the current tau, :339-349)
  if (e == hipSuccess && fe) e = launch_end_states(dob.o, d_tau, B, (double*)d_tg, 19, d_em, st);
  if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage in", e);
  const double* t_cur = d_t;                               // the caller's grid until the first update, then t through tau
  int ntg_cur = n_tgrids;
  const double* t_qp = tfm ? d_tb : d_t1;                  // the grid of the QP's weights: with free tf every trajectory has its own
  const int ntg_qp = tfm ? B : n_tgrids;

  if (rc == LTO_OK) rc = lto_direct_defect_dev(p, st, d_X, J, d_U, J, t_cur, ntg_cur, d_def, S, nullptr);    // :485 (er = 1.0: one step at least)
  // `while er > 1e-6` (:491) + the iteration limit (:492-496), trajectory by trajectory
  while (rc == LTO_OK && nb.next(1e-6, maxIter)) {
    e = nb.upload_flags(10, d_act, d_search, st);                                                       // line search from iteration 11 (:557)
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "flag upload", e); break; }
    bool search = false;
    for (int b = 0; b < B; ++b) search |= nb.h_search[b] != 0.0;
    // flagEnd: free ends on odd iterations, frozen on even ones (:521-526).  The active trajectories share the iteration count.
    bool free_it = false;
    if (fe && fe->flag_end)
      for (int b = 0; b < B; ++b) if (nb.active[b] && (nb.it[b] & 1)) free_it = true;
    if (tfm && free_it)                                    // :500 with the tf column (:503-516)
      rc = lto_direct_jacobian_dev(p, st, d_X, J, d_U, J, t_cur, ntg_cur, d_jac, S, d_dtf, nullptr, S, nullptr);
    else
      rc = lto_direct_jacobian_dev(p, st, d_X, J, d_U, J, t_cur, ntg_cur, d_jac, S, nullptr, nullptr, 0, nullptr);   // :500
    if (rc == LTO_OK)                                      // :525-529
      rc = direct_qp_launch(p, st, free_it ? (tfm ? 4 : 3) : 1, d_jac, S, d_def, S, d_X, J, d_U, J, t_qp, ntg_qp, d_tg, allow_impulsive,
                            d_dX, d_dU, d_dV, d_cost, (const lto_direct_end_model*)d_em, d_beta, d_p, d_dtf, d_tfb, d_tf);
    if (rc != LTO_OK) break;
    // lineSearch (:405-430): the ten trial points of every problem, one sweep.  With free tf they are evaluated on the current grid
    // (`lineSearch(..., t_TU, ...)`, :560), not at tf + alpha p3: d_tl holds each trajectory's current grid (k_tf_grid)
    if (search) {
      e = launch_trial_points(d_X, d_dX, J, nstate, n_nodes, B, NA, d_alphas, d_Xt, J * NA, st);
      if (e == hipSuccess) e = launch_trial_points(d_U, d_dU, J, 3, n_nodes, B, NA, d_alphas, d_Ut, J * NA, st);
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "trial points", e); break; }
      rc = lto_direct_defect_dev(pl, st, d_Xt, J * NA, d_Ut, J * NA, d_tl, B * NA, d_deft, S * NA, nullptr);
      if (rc != LTO_OK) break;
      e = launch_defect_norms(d_deft, S * NA, nstate, n_nodes - 1, B * NA, d_ss, nullptr, st);      // sum(defect[:].^2), :422
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "line search", e); break; }
    }
    // alpha (:428-429), 1 (:556), or 0 for a frozen trajectory
    e = launch_pick_alpha(d_ss, d_alphas, NA, d_act, d_search, d_step, B, nullptr, nullptr, st);
    if (e == hipSuccess) e = launch_axpy_traj(d_X, d_dX, d_step, d_X, J, nstate, n_nodes, B, st);     // :562
    if (e == hipSuccess) e = launch_axpy_traj(d_U, d_dU, d_step, d_U, J, 3, n_nodes, B, st);          // :563
    if (e == hipSuccess) e = launch_direct_qp_update_dv((double*)d_tg, d_dV, d_step, B, st);           // :568-569
    if (e == hipSuccess && free_it && !tfm) e = launch_tau_update(d_tau, d_p, d_step, B, st);           // :564-565
    if (e == hipSuccess && free_it && tfm) e = launch_tf_update(d_tau, d_tf, d_p, d_step, d_tfb, B, st);  // :564-567
    if (e == hipSuccess && free_it) e = launch_end_states(dob.o, d_tau, B, (double*)d_tg, 19, d_em, st);  // targets at the new tau
    if (e == hipSuccess && free_it && tfm) e = launch_tf_grid(d_taug, d_t0, d_tf, (int)n, B, d_tb, d_tl, NA, st);   // :582
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "update", e); break; }
    t_cur = tfm ? d_tb : d_t1;                                                                           // :582
    ntg_cur = tfm ? B : n_tgrids;
    rc = lto_direct_defect_dev(p, st, d_X, J, d_U, J, t_cur, ntg_cur, d_def, S, nullptr);               // :585
    if (rc != LTO_OK) break;
    e = launch_defect_norms(d_def, S, nstate, (int)(n - 1), B, nullptr, d_mx, st);                      // :588
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "norm", e); break; }
    rc = read_scalars(c, st, d_step, 4 * B, d_tau, fe ? (tfm ? 3 : 2) * B : 0, h_back.data());         // step | max|d| | cost | singular (| tau (| tf))
    if (rc != LTO_OK) break;
    for (int b = 0; b < B; ++b) {
      if (!nb.active[b]) continue;
      moved[b] = 1;
      nb.h_er[b] = h_back[B + b];
      if (history) {
        double* hrow = history + ((size_t)b * maxIter + (nb.it[b] - 1)) * hw;
        hrow[0] = nb.h_er[b]; hrow[1] = h_back[2 * B + b]; hrow[2] = h_back[b];
        if (fe) { hrow[3] = h_back[4 * B + 2 * b]; hrow[4] = h_back[4 * B + 2 * b + 1]; }
        if (fe && fe->tfb) hrow[5] = tfm ? h_back[6 * B + b] : t[(size_t)(n_tgrids == 1 ? 0 : b) * n + n - 1];
      }
      if (h_back[3 * B + b] != 0.0) { nb.status[b] = 3; nb.active[b] = 0; }
    }
  }
  if (rc == LTO_OK) {
    e = stage_out(c, d_X, J, nstate, J, d_aos, X_out, st);
    if (e == hipSuccess && U_out) e = stage_out(c, d_U, J, 3, J, d_uaos, U_out, st);
    if (e == hipSuccess && defect_out) e = stage_out(c, d_def, S, nstate, S, d_def_aos, defect_out, st);
    if (e == hipSuccess && dV_out) e = hipMemcpy2DAsync(dV_out, sizeof(double) * 6, (const double*)d_tg + 13, sizeof(lto_direct_targets),
                                                         sizeof(double) * 6, B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && fe && fe->tau_out) e = hipMemcpyAsync(fe->tau_out, d_tau, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, st);
    lto::HostBuf<double> h_tb(tfm && t_out ? (size_t)n * B : 1);
    if (e == hipSuccess && tfm && t_out) e = h_tb.ok() ? hipMemcpyAsync(h_tb.data(), d_tb, sizeof(double) * n * B, hipMemcpyDeviceToHost, st)
                                                       : hipErrorOutOfMemory;
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
    if (rc == LTO_OK)
      for (int b = 0; b < B; ++b)
        if (nb.status[b] != 3 && (X_out[(size_t)nstate * n * b] != X_out[(size_t)nstate * n * b] || nb.h_er[b] != nb.h_er[b])) nb.status[b] = 2;
    if (rc == LTO_OK && t_out)
      for (int b = 0; b < B; ++b) {
        const size_t g = (size_t)(n_tgrids == 1 ? 0 : b) * n;
        std::memcpy(t_out + (size_t)b * n, !moved[b] ? t + g : tfm ? &h_tb[(size_t)b * n] : &t1[g], sizeof(double) * n);
      }
  }
  for (int b = 0; b < B; ++b) nb.it[b] = std::min(nb.it[b], maxIter);   // a trajectory that reached the limit reports maxIter (:492-496)
  nb.copy_out(status_flag, iterations);
  return rc;
}

extern "C" {

int lto_direct_end_states(lto_ctx* c, const lto_direct_orbits* orbits, int n_batch, const double* tau, double* s_out,
                          lto_direct_end_model* model) {
  if (n_batch < 1) return c ? set_err(c, LTO_EINVAL, "n_batch must be >= 1") : LTO_EINVAL;
  if (!c) return LTO_ENULL;
  if (!orbits || !tau || !s_out || !model) return set_err(c, LTO_ENULL, "lto_direct_end_states: a required argument is NULL");
  if (!orbits_ok(orbits)) return set_err(c, LTO_EINVAL, "orbit tables need >= 2 samples each and non-NULL arrays");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  DevOrbits dob;
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = orbits_upload(c, orbits, dob, st);
  if (rc) return rc;
  double *d_tau, *d_s, *d_m;
  ArenaLayout scratch;
  scratch.add((size_t)2 * n_batch, d_tau);
  scratch.add((size_t)12 * n_batch, d_s);
  scratch.add((size_t)14 * n_batch, d_m);
  rc = scratch.reserve_block(c, call.block[0], "lto_direct_end_states");
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d_tau, tau, sizeof(double) * 2 * n_batch, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_end_states(dob.o, d_tau, n_batch, d_s, 12, d_m, st);
  if (e == hipSuccess) e = hipMemcpyAsync(s_out, d_s, sizeof(double) * 12 * n_batch, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(model, d_m, sizeof(double) * 14 * n_batch, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_direct_end_states", e);
  return LTO_OK;
}

int lto_direct_qp_step(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                       int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets, int n_targets,
                       int allow_impulsive, double* dX, double* dU, double* dV, double* cost) {
  return direct_qp_step_host(c, "lto_direct_qp_step", 1, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, targets, nullptr,
                             nullptr, nullptr, n_targets, allow_impulsive, dX, dU, dV, nullptr, cost);
}

int lto_direct_qp_step_free(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                            int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                            const lto_direct_end_model* model, const double* beta, int n_targets, int allow_impulsive, double* dX,
                            double* dU, double* dV, double* p_out, double* cost) {
  return direct_qp_step_host(c, "lto_direct_qp_step_free", 3, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, targets, model,
                             beta, nullptr, n_targets, allow_impulsive, dX, dU, dV, p_out, cost);
}

int lto_direct_qp_step_free_tf(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                               int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                               const lto_direct_end_model* model, const double* beta, const lto_direct_tf_bounds* tfb, int n_targets,
                               int allow_impulsive, double* dX, double* dU, double* dV, double* p_out, double* cost) {
  return direct_qp_step_host(c, "lto_direct_qp_step_free_tf", 4, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, targets,
                             model, beta, tfb, n_targets, allow_impulsive, dX, dU, dV, p_out, cost);
}

int lto_direct_solve_batch(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                           const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                           const lto_direct_targets* targets, int n_targets, int allow_impulsive, int maxIter, double* X_out,
                           double* U_out, double* dV_out, double* t_out, double* defect_out, int* status_flag, int* iterations,
                           double* history) {
  return direct_solve_impl(c, nstate, n_nodes, n_batch, X_in, U_in, t, n_tgrids, nsteps, prm, targets, n_targets, allow_impulsive,
                           maxIter, X_out, U_out, dV_out, t_out, defect_out, status_flag, iterations, history, nullptr);
}

int lto_direct_solve_free_batch(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                                const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                                const lto_direct_orbits* orbits, const lto_direct_targets* targets, int n_targets,
                                const double* tau_in, const double* beta, int flag_end, int allow_impulsive, int maxIter,
                                double* X_out, double* U_out, double* dV_out, double* t_out, double* defect_out, double* tau_out,
                                int* status_flag, int* iterations, double* history) {
  const DirectFreeEnds fe = {orbits, tau_in, beta, flag_end ? 1 : 0, tau_out, nullptr};
  return direct_solve_impl(c, nstate, n_nodes, n_batch, X_in, U_in, t, n_tgrids, nsteps, prm, targets, n_targets, allow_impulsive,
                           maxIter, X_out, U_out, dV_out, t_out, defect_out, status_flag, iterations, history, &fe);
}

int lto_direct_solve_free(lto_ctx* c, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t, int nsteps,
                          const lto_direct_params* prm, const lto_direct_orbits* orbits, const lto_direct_targets* targets,
                          const double* tau_in, double beta, int flag_end, int allow_impulsive, int maxIter, double* X_out,
                          double* U_out, double* dV_out, double* t_out, double* defect_out, double* tau_out, int* status,
                          int* iterations, double* history) {
  return lto_direct_solve_free_batch(c, nstate, n_nodes, 1, X_in, U_in, t, 1, nsteps, prm, orbits, targets, 1, tau_in, &beta, flag_end,
                                     allow_impulsive, maxIter, X_out, U_out, dV_out, t_out, defect_out, tau_out, status, iterations,
                                     history);
}

int lto_direct_solve_free_tf_batch(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                                   const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                                   const lto_direct_orbits* orbits, const lto_direct_targets* targets, int n_targets,
                                   const double* tau_in, const double* beta, const lto_direct_tf_bounds* tfb, int flag_end,
                                   int allow_impulsive, int maxIter, double* X_out, double* U_out, double* dV_out, double* t_out,
                                   double* defect_out, double* tau_out, int* status_flag, int* iterations, double* history) {
  const int rc = direct_entry_check(c, nstate, n_nodes, n_batch, n_tgrids, n_targets, true, t, tfb);
  if (rc) return rc;
  if (!tfb) return set_err(c, LTO_ENULL, "tfb is NULL");
  const DirectFreeEnds fe = {orbits, tau_in, beta, flag_end ? 1 : 0, tau_out, tfb};
  return direct_solve_impl(c, nstate, n_nodes, n_batch, X_in, U_in, t, n_tgrids, nsteps, prm, targets, n_targets, allow_impulsive,
                           maxIter, X_out, U_out, dV_out, t_out, defect_out, status_flag, iterations, history, &fe);
}

int lto_direct_solve_free_tf(lto_ctx* c, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t, int nsteps,
                             const lto_direct_params* prm, const lto_direct_orbits* orbits, const lto_direct_targets* targets,
                             const double* tau_in, double beta, const lto_direct_tf_bounds* tfb, int flag_end, int allow_impulsive,
                             int maxIter, double* X_out, double* U_out, double* dV_out, double* t_out, double* defect_out,
                             double* tau_out, int* status, int* iterations, double* history) {
  return lto_direct_solve_free_tf_batch(c, nstate, n_nodes, 1, X_in, U_in, t, 1, nsteps, prm, orbits, targets, 1, tau_in, &beta, tfb,
                                        flag_end, allow_impulsive, maxIter, X_out, U_out, dV_out, t_out, defect_out, tau_out, status,
                                        iterations, history);
}

int lto_direct_solve(lto_ctx* c, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t, int nsteps,
                     const lto_direct_params* prm, const lto_direct_targets* targets, int allow_impulsive, int maxIter,
                     double* X_out, double* U_out, double* dV_out, double* t_out, double* defect_out, int* status,
                     int* iterations, double* history) {
  return lto_direct_solve_batch(c, nstate, n_nodes, 1, X_in, U_in, t, 1, nsteps, prm, targets, 1, allow_impulsive, maxIter, X_out,
                                U_out, dV_out, t_out, defect_out, status, iterations, history);
}

}  // extern "C"
