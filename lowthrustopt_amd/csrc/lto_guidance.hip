// lto_guidance.hip -- neighbouring-extremal guidance: the host-pointer calls.  The gains call stages the trajectories
// in, runs the STM sweep of a short-lived plan of its own (the kernel AUTO picks), leaves Phi in HBM and runs the backward sweep over
// it.  The guided flight stages the nominal, the gains, the grid, the starts and the navigation errors into the [row][lanes]
// layouts of k_guided_flight and brings the end states, the nodes, dv, the step counts and the status back.  The scratch is laid
// out by ArenaLayout.  One host path for both row counts: the 12-row entries (ndim must be 12) and the _mass entries of the 14-row
// variable-mass system, half-dimension nx = 6 or 7.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "lto_host.hpp"

namespace {

// nd: the row count the entry is built for (12, or 14 for the _mass entries); ndim: what the caller passed
int guidance_supported(lto_ctx* c, int nd, int ndim, const lto_integrator* integ, const char* who) {
  if (ndim != nd)
    return set_err(c, LTO_EUNSUPPORTED, "guidance gains and guided flights take ndim = 12; 14-row solutions go to lto_guidance_gains_mass_batch and lto_guided_flight_mass_batch");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE) return set_err(c, LTO_EUNSUPPORTED, who);
  return LTO_OK;
}

// "<entry>: <what>" with the entry's own name
int fail(lto_ctx* c, int code, const char* who, const char* what, hipError_t e = hipSuccess) {
  char msg[256];
  std::snprintf(msg, sizeof msg, "%s: %s", who, what);
  return set_err(c, code, msg, e);
}

bool grids_increase(const double* t, int n_nodes, int n_grids) {
  for (int g = 0; g < n_grids; ++g) {
    const double* tb = t + (size_t)g * n_nodes;
    for (int i = 0; i + 1 < n_nodes; ++i)
      if (!(tb[i] < tb[i + 1]) || !std::isfinite(tb[i + 1] - tb[i])) return false;
  }
  return true;
}

// host [rows x count] column-major -> device [row][count]; one column is its own transpose
hipError_t lanes_in(const double* host, long rows, long count, double* d_tmp, double* d_out, hipStream_t st) {
  if (count == 1) return hipMemcpyAsync(d_out, host, sizeof(double) * (size_t)rows, hipMemcpyHostToDevice, st);
  const hipError_t e = hipMemcpyAsync(d_tmp, host, sizeof(double) * (size_t)rows * count, hipMemcpyHostToDevice, st);
  return e == hipSuccess ? launch_rows_to_lanes(d_tmp, rows, count, d_out, st) : e;
}
hipError_t lanes_out(const double* d_in, long rows, long count, double* d_tmp, double* host, hipStream_t st) {
  if (count == 1) return hipMemcpyAsync(host, d_in, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, st);
  const hipError_t e = launch_lanes_to_rows(d_in, rows, count, d_tmp, st);
  return e == hipSuccess ? hipMemcpyAsync(host, d_tmp, sizeof(double) * (size_t)rows * count, hipMemcpyDeviceToHost, st) : e;
}

// The covariance call's own arguments (lto_guidance_covariance_batch): the gains call with `cov` set runs the forward pass of
// k_guidance_covariance over the Phi and K it has in HBM, and K becomes optional.
struct CovCall {
  int n_cases;
  const double* P0; const double* R; const int* every;
  double* Phi; double* P_nodes; double* P_final; int* status;
};

int gains_batch(int nd, const char* who, lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, double* K, double* pivot,
                int* status, const CovCall* cov = nullptr) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!XC || !t || !prm || !integ || !status || (!cov && !K))
    return fail(c, LTO_ENULL, who, cov ? "XC, t, prm, integ or gain_status is NULL" : "XC, t, prm, integ, K or status is NULL");
  if (cov && (!cov->P0 || !cov->R || !cov->every || !cov->P_final || !cov->status))
    return fail(c, LTO_ENULL, who, "P0, R, update_every, P_final or cov_status is NULL");
  int rc = guidance_supported(c, nd, ndim, integ, "guidance gains are built for LTO_RK4 or LTO_DOP853_ADAPTIVE");
  if (rc) return rc;
  if (n_nodes < 2 || n_batch < 1) return fail(c, LTO_EINVAL, who, "need n_nodes >= 2 and n_batch >= 1");
  if (n_tgrids != 1 && n_tgrids != n_batch) return fail(c, LTO_EINVAL, who, "n_tgrids must be 1 or n_batch");
  if (n_prm != 1 && n_prm != n_batch) return fail(c, LTO_EINVAL, who, "n_prm must be 1 or n_batch");
  if (!(sing_tol > 0.0 && sing_tol < 1.0)) return fail(c, LTO_EINVAL, who, "sing_tol must lie in (0, 1)");
  if (!grids_increase(t, n_nodes, n_tgrids))
    return fail(c, LTO_EINVAL, who, "t must be finite and strictly increasing");
  if (cov) {
    if (cov->n_cases < 1 || cov->n_cases > 4 * 65535) return fail(c, LTO_EINVAL, who, "need 1 <= n_cases <= 262140");
    for (int i = 0; i < cov->n_cases; ++i)
      if (cov->every[i] < 0) return fail(c, LTO_EINVAL, who, "update_every must be >= 0");
  }
  const int B = n_batch, nx = nd / 2;
  const size_t ne = (size_t)nx * nx, nc = cov ? (size_t)cov->n_cases : 0;
  // 14 rows, DOP853: AUTO takes the two-lanes-per-state STM kernel for batches whose laws are all p = 0 or p = 1 and the one-piece
  // cooperative kernel otherwise, and the two differ in the last bits -- swept as one batch, a p <= 1 trajectory's gains would
  // depend on the classes of its neighbours.  A batch that mixes the two kinds is therefore run as two calls, one per kind, each
  // with the kernel AUTO picks for it and for each of its trajectories alone.
  if (nd == 14 && integ->method == LTO_DOP853_ADAPTIVE && n_prm == B) {
    HostBuf<int> idx((size_t)B);                  // the p <= 1 trajectories from the front, the others from the back
    if (!idx.ok()) return fail(c, LTO_ENOMEM, who, "host memory");
    int n_lim = 0, n_oth = 0;
    for (int b = 0; b < B; ++b) {
      if ((1 << lto::p_class(prm[b].p)) & kThrustLimitedClasses) idx[n_lim++] = b;
      else idx[B - 1 - n_oth++] = b;
    }
    if (n_lim > 0 && n_oth > 0) {
      const size_t xc = (size_t)nd * n_nodes, kk = (size_t)nx * nx * (n_nodes - 1), segs = (size_t)n_nodes - 1;
      for (int kind = 0; kind < 2; ++kind) {
        const int* ix = idx.data() + (kind == 0 ? 0 : n_lim);
        const size_t m = kind == 0 ? n_lim : n_oth;
        HostBuf<double> Xs(xc * m), ts(n_tgrids == 1 ? 0 : (size_t)n_nodes * m), Ks(kk * m), ps(segs * m);
        HostBuf<lto_params> prms(m);
        HostBuf<int> sts(m);
        if (!Xs.ok() || !ts.ok() || !Ks.ok() || !ps.ok() || !prms.ok() || !sts.ok()) return fail(c, LTO_ENOMEM, who, "host memory");
        // the covariance outputs of this kind's trajectories, scattered back like the gains
        const size_t ph = (size_t)nd * nd * segs, pn = ne * n_nodes * nc, pf = ne * nc;
        HostBuf<double> Phs(cov && cov->Phi ? ph * m : 0), Pns(cov && cov->P_nodes ? pn * m : 0), Pfs(cov ? pf * m : 0);
        HostBuf<int> css(cov ? nc * m : 0);
        if (!Phs.ok() || !Pns.ok() || !Pfs.ok() || !css.ok()) return fail(c, LTO_ENOMEM, who, "host memory");
        CovCall sub{};
        if (cov) {
          sub = *cov;
          sub.Phi = cov->Phi ? Phs.data() : nullptr; sub.P_nodes = cov->P_nodes ? Pns.data() : nullptr;
          sub.P_final = Pfs.data(); sub.status = css.data();
        }
        for (size_t j = 0; j < m; ++j) {
          std::memcpy(Xs.data() + xc * j, XC + xc * ix[j], sizeof(double) * xc);
          if (n_tgrids != 1) std::memcpy(ts.data() + (size_t)n_nodes * j, t + (size_t)n_nodes * ix[j], sizeof(double) * n_nodes);
          prms[j] = prm[ix[j]];
        }
        rc = gains_batch(nd, who, c, ndim, n_nodes, (int)m, Xs.data(), n_tgrids == 1 ? t : ts.data(), n_tgrids == 1 ? 1 : (int)m,
                         prms.data(), (int)m, integ, sing_tol, Ks.data(), ps.data(), sts.data(), cov ? &sub : nullptr);
        if (rc) return rc;
        for (size_t j = 0; j < m; ++j) {
          if (K) std::memcpy(K + kk * ix[j], Ks.data() + kk * j, sizeof(double) * kk);
          if (pivot) std::memcpy(pivot + segs * ix[j], ps.data() + segs * j, sizeof(double) * segs);
          status[ix[j]] = sts[j];
          if (!cov) continue;
          if (cov->Phi) std::memcpy(cov->Phi + ph * ix[j], Phs.data() + ph * j, sizeof(double) * ph);
          if (cov->P_nodes) std::memcpy(cov->P_nodes + pn * ix[j], Pns.data() + pn * j, sizeof(double) * pn);
          std::memcpy(cov->P_final + pf * ix[j], Pfs.data() + pf * j, sizeof(double) * pf);
          std::memcpy(cov->status + nc * ix[j], css.data() + nc * j, sizeof(int) * nc);
        }
      }
      return LTO_OK;
    }
  }
  const size_t J = (size_t)n_nodes * B, S = (size_t)(n_nodes - 1) * B, nt = (size_t)n_nodes * n_tgrids;
  HostCall call(c);
  rc = plan_build(c, nd, n_nodes, n_batch, prm, n_prm, integ, &call.plan[0]);
  if (rc) return rc;
  double *d_aos, *d_X, *d_t, *d_def, *d_phi, *d_K, *d_piv, *d_phi_aos, *d_P0, *d_R, *d_Pn, *d_Pf;
  int *d_status, *d_every, *d_cst;
  ArenaLayout scratch;
  scratch.add((size_t)nd * J, d_aos, d_X);
  scratch.add(nt, d_t);
  scratch.add((size_t)nd * S, d_def);
  scratch.add((size_t)nd * nd * S, d_phi);
  scratch.add((size_t)nx * nx * S, d_K);
  scratch.add(S, d_piv);
  scratch.add((size_t)B, d_status);
  scratch.add(cov && cov->Phi ? (size_t)nd * nd * S : 0, d_phi_aos);
  scratch.add(ne * nc, d_P0, d_R);
  scratch.add(cov && cov->P_nodes ? ne * nc * J : 0, d_Pn);
  scratch.add(ne * nc * B, d_Pf);
  scratch.add(nc, d_every);
  scratch.add(nc * B, d_cst);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, XC, nd, (long)J, d_aos, d_X, (long)J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)nt, d_t, st);
  if (e == hipSuccess && cov) e = hipMemcpyAsync(d_P0, cov->P0, sizeof(double) * ne * nc, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cov) e = hipMemcpyAsync(d_R, cov->R, sizeof(double) * ne * nc, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cov) e = hipMemcpyAsync(d_every, cov->every, sizeof(int) * nc, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail(c, LTO_EHIP, who, "stage in", e);
  rc = lto_indirect_jacobian_dev(call.plan[0], st, d_X, (long)J, d_t, n_tgrids, d_phi, (long)S, d_def, (long)S);
  if (rc) return rc;
  GainsArgs g{};
  g.Phi = d_phi; g.ldp = (long)S; g.n_nodes = n_nodes; g.n_batch = B; g.sing_tol = sing_tol;
  g.K = d_K; g.pivot = d_piv; g.status = d_status; g.nx = nx;
  e = launch_guidance_gains(g, st);
  if (e == hipSuccess && cov) {                  // Phi and K stay where they are: the forward pass reads them from HBM
    CovArgs v{};
    v.Phi = d_phi; v.ldp = (long)S; v.K = d_K; v.n_nodes = n_nodes; v.n_batch = B; v.n_cases = cov->n_cases;
    v.P0 = d_P0; v.R = d_R; v.every = d_every; v.P_nodes = cov->P_nodes ? d_Pn : nullptr; v.P_final = d_Pf; v.status = d_cst;
    v.nx = nx;
    e = launch_guidance_covariance(v, st);
  }
  timing_end(c, st);                             // the sweep's start to the gains' (and the covariance pass's) end
  if (e != hipSuccess) return set_err(c, LTO_EHIP, cov ? "launch_guidance_gains / launch_guidance_covariance" : "launch_guidance_gains", e);
  if (K) e = hipMemcpyAsync(K, d_K, sizeof(double) * nx * nx * S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && pivot) e = hipMemcpyAsync(pivot, d_piv, sizeof(double) * S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && cov) {
    if (cov->Phi) e = stage_out(c, d_phi, (long)S, nd * nd, (long)S, d_phi_aos, cov->Phi, st);
    if (e == hipSuccess && cov->P_nodes)
      e = hipMemcpyAsync(cov->P_nodes, d_Pn, sizeof(double) * ne * nc * J, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cov->P_final, d_Pf, sizeof(double) * ne * nc * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cov->status, d_cst, sizeof(int) * nc * B, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return fail(c, LTO_EHIP, who, "stage out", e);
  return LTO_OK;
}

int flight_batch(int nd, const char* who, lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC_nom, const double* t,
                 const double* K, int n_nom, const double* x0, int update_every, const double* nav, const lto_params* prm, int n_prm,
                 const lto_integrator* integ, double* x_final, double* lam_final, double* dv, double* X_nodes, int* accepted,
                 int* rejected, int* status) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!XC_nom || !t || !K || !x0 || !prm || !integ || !x_final || !dv || !status)
    return fail(c, LTO_ENULL, who, "XC_nom, t, K, x0, prm, integ, x_final, dv or status is NULL");
  int rc = guidance_supported(c, nd, ndim, integ, "guided flights are built for LTO_RK4 or LTO_DOP853_ADAPTIVE");
  if (rc) return rc;
  if (n_nodes < 2 || n_batch < 1) return fail(c, LTO_EINVAL, who, "need n_nodes >= 2 and n_batch >= 1");
  if (n_nom != 1 && n_nom != n_batch) return fail(c, LTO_EINVAL, who, "n_nom must be 1 or n_batch");
  if (n_prm != 1 && n_prm != n_batch) return fail(c, LTO_EINVAL, who, "n_prm must be 1 or n_batch");
  if (update_every < 0) return fail(c, LTO_EINVAL, who, "update_every must be >= 0");
  if (!grids_increase(t, n_nodes, n_nom))
    return fail(c, LTO_EINVAL, who, "t must be finite and strictly increasing");
  const int B = n_batch, n = n_nodes, nx = nd / 2;
  const int n_upd = update_every > 0 ? (n - 2) / update_every + 1 : 0;
  const bool with_nav = nav && n_upd > 0;
  HostCall call(c);
  // two nodes per trajectory: the plan is asked for the parameters, the classes and the integrator's defaults only
  rc = plan_build(c, nd, 2, B, prm, n_prm, integ, &call.plan[0]);
  if (rc) return rc;
  lto_indirect_plan* p = call.plan[0];
  const long r_nom = (long)nd * n, r_K = (long)nx * nx * (n - 1), r_nav = (long)nx * n_upd, r_nodes = (long)nx * n;
  const bool tr_nom = n_nom > 1, tr_B = B > 1;   // a single column needs no transpose and no second buffer
  double *d_nom, *d_noma, *d_K, *d_Ka, *d_t, *d_ta, *d_x0, *d_x0a, *d_nav, *d_nava;
  double *d_xf, *d_xfa, *d_lf, *d_lfa, *d_nd, *d_nda, *d_dv;
  int *d_acc, *d_rej, *d_status;
  ArenaLayout scratch;
  scratch.add((size_t)r_nom * n_nom, d_nom);
  scratch.add(tr_nom ? (size_t)r_nom * n_nom : 0, d_noma);
  scratch.add((size_t)r_K * n_nom, d_K);
  scratch.add(tr_nom ? (size_t)r_K * n_nom : 0, d_Ka);
  scratch.add((size_t)n * n_nom, d_t);
  scratch.add(tr_nom ? (size_t)n * n_nom : 0, d_ta);
  scratch.add((size_t)nx * B, d_x0, d_xf);
  scratch.add(tr_B ? (size_t)nx * B : 0, d_x0a, d_xfa);
  scratch.add(with_nav ? (size_t)r_nav * B : 0, d_nav);
  scratch.add(with_nav && tr_B ? (size_t)r_nav * B : 0, d_nava);
  scratch.add(lam_final ? (size_t)nx * B : 0, d_lf);
  scratch.add(lam_final && tr_B ? (size_t)nx * B : 0, d_lfa);
  scratch.add(X_nodes ? (size_t)r_nodes * B : 0, d_nd);
  scratch.add(X_nodes && tr_B ? (size_t)r_nodes * B : 0, d_nda);
  scratch.add((size_t)B, d_dv);
  scratch.add((size_t)B, d_acc, d_rej, d_status);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = lanes_in(XC_nom, r_nom, n_nom, d_noma, d_nom, st);
  if (e == hipSuccess) e = lanes_in(K, r_K, n_nom, d_Ka, d_K, st);
  if (e == hipSuccess) e = lanes_in(t, n, n_nom, d_ta, d_t, st);
  if (e == hipSuccess) e = lanes_in(x0, nx, B, d_x0a, d_x0, st);
  if (e == hipSuccess && with_nav) e = lanes_in(nav, r_nav, B, d_nava, d_nav, st);
  if (e != hipSuccess) return fail(c, LTO_EHIP, who, "stage in", e);
  IndirectArgs a{};
  a.tp = p->d_tp; a.tp_stride = (n_prm == 1) ? 0 : 1;
  a.steps = p->integ.steps; a.rtol = p->integ.rtol; a.atol = p->integ.atol; a.max_steps = p->integ.max_steps;
  GuidedArgs g{};
  g.nom = d_nom; g.K = d_K; g.t = d_t; g.n_nom = n_nom; g.n_nodes = n; g.n_batch = B; g.every = update_every;
  g.x0 = d_x0; g.nav = with_nav ? d_nav : nullptr;
  g.x_final = d_xf; g.lam_final = lam_final ? d_lf : nullptr; g.dv = d_dv; g.nodes = X_nodes ? d_nd : nullptr;
  g.nacc = d_acc; g.nrej = d_rej; g.status = d_status; g.nx = nx;
  timing_begin(c, st);
  e = launch_guided_flight(p->pm, p->integ.method, a, g, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_guided_flight", e);
  e = lanes_out(d_xf, nx, B, d_xfa, x_final, st);
  if (e == hipSuccess && lam_final) e = lanes_out(d_lf, nx, B, d_lfa, lam_final, st);
  if (e == hipSuccess && X_nodes) e = lanes_out(d_nd, r_nodes, B, d_nda, X_nodes, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dv, d_dv, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && accepted) e = hipMemcpyAsync(accepted, d_acc, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rejected) e = hipMemcpyAsync(rejected, d_rej, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return fail(c, LTO_EHIP, who, "stage out", e);
  return LTO_OK;
}

}  // namespace

extern "C" {

int lto_guidance_gains_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                             const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, double* K,
                             double* pivot, int* status) {
  return gains_batch(12, "lto_guidance_gains_batch", c, ndim, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, sing_tol, K, pivot,
                     status);
}

int lto_guidance_gains(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                       const lto_integrator* integ, double sing_tol, double* K, double* pivot, int* status) {
  return lto_guidance_gains_batch(c, ndim, n_nodes, 1, XC, t, 1, prm, 1, integ, sing_tol, K, pivot, status);
}

int lto_guidance_gains_mass_batch(lto_ctx* c, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                  const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, double* K,
                                  double* pivot, int* status) {
  return gains_batch(14, "lto_guidance_gains_mass_batch", c, 14, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, sing_tol, K,
                     pivot, status);
}

int lto_guidance_gains_mass(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                            const lto_integrator* integ, double sing_tol, double* K, double* pivot, int* status) {
  return lto_guidance_gains_mass_batch(c, n_nodes, 1, XC, t, 1, prm, 1, integ, sing_tol, K, pivot, status);
}

int lto_guidance_covariance_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                  const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, int n_cases,
                                  const double* P0, const double* R, const int* update_every, double* K, double* pivot,
                                  int* gain_status, double* Phi, double* P_nodes, double* P_final, int* cov_status) {
  const char* who = "lto_guidance_covariance_batch";
  if (!c) return LTO_ENULL;
  if (ndim != 12 && ndim != 14) return fail(c, LTO_EUNSUPPORTED, who, "ndim must be 12 or 14");
  const CovCall cov{n_cases, P0, R, update_every, Phi, P_nodes, P_final, cov_status};
  return gains_batch(ndim, who, c, ndim, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, sing_tol, K, pivot, gain_status, &cov);
}

int lto_guided_flight_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC_nom, const double* t, const double* K,
                            int n_nom, const double* x0, int update_every, const double* nav, const lto_params* prm, int n_prm,
                            const lto_integrator* integ, double* x_final, double* lam_final, double* dv, double* X_nodes,
                            int* accepted, int* rejected, int* status) {
  return flight_batch(12, "lto_guided_flight_batch", c, ndim, n_nodes, n_batch, XC_nom, t, K, n_nom, x0, update_every, nav, prm, n_prm,
                      integ, x_final, lam_final, dv, X_nodes, accepted, rejected, status);
}

int lto_guided_flight(lto_ctx* c, int ndim, int n_nodes, const double* XC_nom, const double* t, const double* K, const double* x0,
                      int update_every, const double* nav, const lto_params* prm, const lto_integrator* integ, double* x_final,
                      double* lam_final, double* dv, double* X_nodes, int* accepted, int* rejected, int* status) {
  return lto_guided_flight_batch(c, ndim, n_nodes, 1, XC_nom, t, K, 1, x0, update_every, nav, prm, 1, integ, x_final, lam_final, dv,
                                 X_nodes, accepted, rejected, status);
}

int lto_guided_flight_mass_batch(lto_ctx* c, int n_nodes, int n_batch, const double* XC_nom, const double* t, const double* K,
                                 int n_nom, const double* x0, int update_every, const double* nav, const lto_params* prm, int n_prm,
                                 const lto_integrator* integ, double* x_final, double* lam_final, double* dv, double* X_nodes,
                                 int* accepted, int* rejected, int* status) {
  return flight_batch(14, "lto_guided_flight_mass_batch", c, 14, n_nodes, n_batch, XC_nom, t, K, n_nom, x0, update_every, nav, prm,
                      n_prm, integ, x_final, lam_final, dv, X_nodes, accepted, rejected, status);
}

int lto_guided_flight_mass(lto_ctx* c, int n_nodes, const double* XC_nom, const double* t, const double* K, const double* x0,
                           int update_every, const double* nav, const lto_params* prm, const lto_integrator* integ, double* x_final,
                           double* lam_final, double* dv, double* X_nodes, int* accepted, int* rejected, int* status) {
  return lto_guided_flight_mass_batch(c, n_nodes, 1, XC_nom, t, K, 1, x0, update_every, nav, prm, 1, integ, x_final, lam_final, dv,
                                      X_nodes, accepted, rejected, status);
}

}  // extern "C"
