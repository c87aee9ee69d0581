// lto_indirect_solve.hip -- the batched indirect Newton loop and what starts it from a new grid: addTimeFinal and mesh
// equidistribution.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "lto_host.hpp"

/* Whole Newton loop of multiShoot_CRTBP_indirect (src/multiShoot_CRTBP_indirect.jl:254-345) with the trajectories
 * resident in HBM: per iteration one STM sweep, the structured least-squares step (+ second-order correction), the
 * 20-point line search as ONE batched sweep after iteration 3, end-state pinning and the defect check.  Only scalars
 * cross PCIe inside the loop (per trajectory: max|xc_update|, 20 sums of squares, max|defect|).
 * n_batch independent problems (homotopy levels, thrust levels, different guesses) run the loop side by side: every
 * device operation covers the whole batch; a trajectory that has left the reference loop (converged, NaN, iteration
 * limit) is frozen by a zero step length and its results are kept. */
// d_Xin: the starting trajectories already on the device ([ndim][n_nodes n_batch] struct-of-arrays, the loop's own layout) instead
// of XC_in; d_Xout: if set, the final trajectories are also copied there (same layout).  lto_indirect_add_time_batch starts the loop
// from its re-meshed guesses this way.
int indirect_solve_impl(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC_in, const double* d_Xin, const double* t,
                               int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, int flag_adjointsOnly,
                               int maxIter, double* XC_out, double* d_Xout, double* defect, int* status_flag, int* iterations,
                               double* history) {
  if (!c) return LTO_ENULL;
  if ((!XC_in && !d_Xin) || !t || !prm || !integ || !XC_out || !status_flag) return set_err(c, LTO_ENULL, "XC_in, t, prm, integ, XC_out or status_flag is NULL");
  if (ndim != 12 && ndim != 14) return set_err(c, LTO_EUNSUPPORTED, "the device Newton loop is built for ndim = 12 and 14");
  if (maxIter < 0) return set_err(c, LTO_EINVAL, "maxIter must be >= 0");
  if (n_batch < 1 || n_nodes < 2) return set_err(c, LTO_EINVAL, "need n_nodes >= 2 and n_batch >= 1");
  if ((n_tgrids != 1 && n_tgrids != n_batch) || (n_prm != 1 && n_prm != n_batch)) return set_err(c, LTO_EINVAL, "n_tgrids / n_prm must be 1 or n_batch");
  constexpr int NA = 20;                                   // LinRange(0.1, 1, 20), :227
  const int B = n_batch;
  if ((long)B * NA * (n_nodes - 1) > 0x7fffffffL) return set_err(c, LTO_EINVAL, "too many line-search segments");
  // parameters / time grids of the B*NA line-search trial trajectories: trajectory b's, NA times
  lto::HostBuf<lto_params> prm_l;
  lto::HostBuf<double> t_l;
  if (n_prm != 1) {
    if (!prm_l.alloc((size_t)B * NA)) return set_err(c, LTO_ENOMEM, "lto_indirect_solve_batch: out of host memory");
    for (int b = 0; b < B; ++b) for (int a = 0; a < NA; ++a) prm_l[(size_t)b * NA + a] = prm[b];
  }
  if (n_tgrids != 1) {
    if (!t_l.alloc((size_t)B * NA * n_nodes)) return set_err(c, LTO_ENOMEM, "lto_indirect_solve_batch: out of host memory");
    for (int b = 0; b < B; ++b) for (int a = 0; a < NA; ++a)
      std::memcpy(&t_l[((size_t)b * NA + a) * n_nodes], t + (size_t)b * n_nodes, sizeof(double) * n_nodes);
  }
  const int nd = ndim;                                     // 12: state + costate; 14: + mass and mass costate
  NewtonBatch nb(B, NA);                                   // er = 1.0: :279
  lto::HostBuf<double> h_mx(B), h_step(B), h_back((size_t)3 * B);
  HostCall call(c);
  int rc = plan_build(c, nd, n_nodes, B, prm, n_prm, integ, &call.plan[0]);
  if (rc == LTO_OK) rc = plan_build(c, nd, n_nodes, B * NA, n_prm == 1 ? prm : prm_l.data(), n_prm == 1 ? 1 : B * NA, integ, &call.plan[1]);
  if (rc) return rc;
  lto_indirect_plan* p = call.plan[0];
  lto_indirect_plan* pl = call.plan[1];                    // the line search's trial trajectories
  const long n = n_nodes, J = n * B, S = (n - 1) * B;
  const int ntl = (n_tgrids == 1) ? 1 : B * NA;
  const size_t n_small = (size_t)nd * B + NA + 6 * (size_t)B + 2 * (size_t)NA * B + 64;
  double *d_aos, *d_X, *d_X2, *d_del, *d_del2, *d_Xt, *d_t, *d_tl, *d_def, *d_def2, *d_defj, *d_def_aos, *d_deft, *d_phi, *d_small;
  ArenaLayout scratch;
  scratch.add((size_t)nd * J, d_aos, d_X, d_X2, d_del, d_del2);
  scratch.add((size_t)nd * J * NA, d_Xt);
  scratch.add((size_t)n * n_tgrids, d_t);
  if (n_tgrids != 1) scratch.add((size_t)n * ntl, d_tl);
  // d_defj: the STM sweep's own defect (right-hand side of the step); d_def stays defectCalc's
  scratch.add((size_t)nd * S, d_def, d_def2, d_defj, d_def_aos);
  scratch.add((size_t)nd * S * NA, d_deft);
  scratch.add((size_t)nd * nd * S, d_phi);
  scratch.add(n_small, d_small);
  rc = scratch.reserve(c);
  if (rc) return rc;
  if (n_tgrids == 1) d_tl = d_t;
  double* d_saved = d_small;                               // [B][nd] pinned end states (12: 6 + 6, 14: 7 + 7)
  double* d_alphas = d_saved + (size_t)nd * B;             // [NA]   trial step lengths
  double* d_step = d_alphas + NA;                          // [B]    step length / SOC mask per trajectory
  double* d_mx = d_step + B;                               // [B]    per-trajectory max norms
  double* d_ss = d_mx + B;                                 // [NA*B] per-trial sums of squares
  double* d_act = d_ss + (size_t)NA * B;                   // [B]    1 = trajectory still in its loop
  double* d_search = d_act + B;                            // [B]    1 = line search on (iteration > 3)
  double* d_mxdel = d_search + B;                          // [B]    max |xc_update| of the iteration
  double* d_mxt = d_mxdel + B;                             // [NA*B] per-trial max |defect|
  (void)report_reserve(c, (size_t)3 * B);
  hipStream_t st = c->stream;
  bool soc_speculative = false;
  unsigned trial_sweeps = 0;
  if (!nb.ok() || !h_mx.ok() || !h_step.ok() || !h_back.ok()) return set_err(c, LTO_ENOMEM, "lto_indirect_solve_batch: out of host memory");

  hipError_t e = d_Xin ? hipMemcpyAsync(d_X, d_Xin, sizeof(double) * nd * J, hipMemcpyDeviceToDevice, st)
                       : hipMemcpyAsync(d_aos, XC_in, sizeof(double) * nd * J, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t, t, sizeof(double) * n * n_tgrids, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_tgrids != 1) e = hipMemcpyAsync(d_tl, t_l.data(), sizeof(double) * n * ntl, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_alphas, nb.alphas.data(), sizeof(double) * NA, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !d_Xin) e = launch_pack_soa(d_aos, nd, J, d_X, J, st);
  // state_0, state_f  (:270-271); 14-dim: also m0, and lambda_m(tf) set to 0 (free final mass)
  if (e == hipSuccess) e = launch_end_pins(d_X, J, n_nodes, B, nd, d_saved, 0, st);
  if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage in", e);

  // per-trajectory max |v| of an SoA block [rows][ld], `per` columns per trajectory -> host (NaN-propagating)
  auto max_abs = [&](const double* v, long ld, long per, double* out) -> int {
    hipError_t q = launch_defect_norms(v, ld, nd, (int)per, B, nullptr, d_mx, st);
    if (q == hipSuccess) q = hipMemcpyAsync(out, d_mx, sizeof(double) * B, hipMemcpyDeviceToHost, st);
    if (q == hipSuccess) q = hipStreamSynchronize(st);
    return q == hipSuccess ? LTO_OK : set_err(c, LTO_EHIP, "norm", q);
  };

  if (rc == LTO_OK) rc = lto_indirect_defect_dev(p, st, d_X, J, d_t, n_tgrids, d_def, S, nullptr);      // :274
  // `while er > 1e-10` (:280) + the iteration limit (:281-286), trajectory by trajectory
  while (rc == LTO_OK && nb.next(1e-10, maxIter)) {
    // Round 4: the loop's decisions are taken on the device -- the second-order-correction mask from max |xc_update| (:190) and the
    // line search's first minimiser (:244-245) -- so the host reads back ONCE per iteration (max |defect|, the step lengths and
    // max |xc_update| together) instead of three times.  While the last known max |xc_update| of some active trajectory is
    // >= 0.1 the correction is still decided on the host (one more read-back, but a defect sweep and a re-solve whose result would
    // be discarded are not launched); once every active trajectory has been below, it is computed for all and applied by mask.
    e = nb.upload_flags(3, d_act, d_search, st);                                                      // line search from iteration 4
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "flag upload", e); break; }
    rc = lto_indirect_jacobian_dev(p, st, d_X, J, d_t, n_tgrids, d_phi, S, d_defj, S);             // :290
    // large adaptive problems: the next sweeps of this plan run with the lanes ordered by this sweep's step counts
    if (rc == LTO_OK && host_order_wanted(p, true)) rc = lto_indirect_plan_rebalance(p, st);
    if (rc == LTO_OK) rc = lto_indirect_newton_solve_dev(p, st, d_phi, S, d_defj, S, flag_adjointsOnly, d_del, J);  // :182
    if (rc != LTO_OK) break;
    e = launch_defect_norms(d_del, J, nd, (int)n, B, nullptr, d_mxdel, st);                          // max |xc_update| per trajectory
    if (e == hipSuccess) e = launch_soc_mask(d_mxdel, d_act, 1e-1, d_step, B, st);                   // second-order correction, :190-214
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "soc mask", e); break; }
    bool soc = true;
    if (!soc_speculative) {                                // early iterations: read max |xc_update| and skip the work if nobody needs it
      rc = read_scalars(c, st, d_mxdel, B, nullptr, 0, h_mx.data());
      if (rc != LTO_OK) break;
      soc = false;
      for (int b = 0; b < B; ++b) soc |= (nb.active[b] && h_mx[b] == h_mx[b] && h_mx[b] < 1e-1);
    }
    if (soc) {
      e = launch_axpy(d_X, d_del, 1.0, d_X2, nd * J, st);
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "axpy", e); break; }
      rc = lto_indirect_defect_dev(p, st, d_X2, J, d_t, n_tgrids, d_def2, S, nullptr);
      if (rc == LTO_OK) rc = lto_indirect_newton_solve_dev(p, st, nullptr, 0, d_def2, S, flag_adjointsOnly, d_del2, J);
      if (rc != LTO_OK) break;
      e = launch_axpy_traj(d_del, d_del2, d_step, d_del, J, nd, n_nodes, B, st);                      // masked: step = 0 keeps d_del
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "axpy", e); break; }
    }
    bool search = false, all_search = true;
    for (int b = 0; b < B; ++b) if (nb.active[b]) { search |= nb.it[b] > 3; all_search &= nb.it[b] > 3; }
    if (search) {                                          // :300-302: the 20 trial trajectories of every problem, one sweep
      e = launch_trial_points(d_X, d_del, J, nd, n_nodes, B, NA, d_alphas, d_Xt, J * NA, st);
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "trial points", e); break; }
      rc = lto_indirect_defect_dev(pl, st, d_Xt, J * NA, d_tl, ntl, d_deft, S * NA, nullptr);
      // the next trial sweeps run with the lanes ordered by this one's step counts; near convergence the counts hardly move, so the
      // order (always a valid permutation, whatever its age) is renewed every fourth sweep only
      if (rc == LTO_OK && host_order_wanted(pl, false) && (trial_sweeps++ & 3) == 0) rc = lto_indirect_plan_rebalance(pl, st);
      if (rc != LTO_OK) break;
      e = launch_defect_norms(d_deft, S * NA, nd, n_nodes - 1, B * NA, d_ss, d_mxt, st);           // sum(defect.^2), :240 (+ max |defect|)
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "line search", e); break; }
    }
    // alpha (:244-245), 1, or 0 (frozen).  When every active trajectory searched, the same launch takes the chosen trial's max
    // |defect| and defect block: CHECK UPDATE (:328-331) without a sweep -- the new XC_all is the chosen trial point bit for bit
    // (same fma, the update's end-state rows are zero), so defectCalc there is the lanes of the line search's sweep that integrated it.
    const bool reuse = search && all_search;
    e = reuse ? launch_take_trial(d_deft, S * NA, d_ss, d_act, d_search, NA, n_nodes - 1, nd, B, d_def, S, d_alphas, d_step, d_mxt, d_mx, st)
              : launch_pick_alpha(d_ss, d_alphas, NA, d_act, d_search, d_step, B, nullptr, nullptr, st);
    if (e == hipSuccess) e = launch_axpy_traj(d_X, d_del, d_step, d_X, J, nd, n_nodes, B, st);      // :304
    if (e == hipSuccess) e = launch_end_pins(d_X, J, n_nodes, B, nd, d_saved, 1, st);                // :324-325
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "update", e); break; }
    if (!reuse) {
      rc = lto_indirect_defect_dev(p, st, d_X, J, d_t, n_tgrids, d_def, S, nullptr);               // :328
      if (rc != LTO_OK) break;
      e = launch_defect_norms(d_def, S, nd, (int)(n - 1), B, nullptr, d_mx, st);                     // :331
      if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "norm", e); break; }
    }
    // one read-back: [step | max |defect|] are adjacent in the small block, max |xc_update| follows the flags
    rc = read_scalars(c, st, d_step, 2 * B, d_mxdel, B, h_back.data());
    if (rc != LTO_OK) break;
    soc_speculative = true;
    for (int b = 0; b < B; ++b) {
      h_step[b] = h_back[b]; h_mx[b] = h_back[B + b];
      const double md = h_back[2 * B + b];
      if (nb.active[b] && !(md < 1e-1)) soc_speculative = false;     // somebody is still taking big steps (or NaN): decide on the host next time
    }
    for (int b = 0; b < B; ++b) {
      if (!nb.active[b]) continue;
      nb.h_er[b] = h_mx[b];
      if (history && nb.it[b] <= maxIter) {
        history[((size_t)b * maxIter + (nb.it[b] - 1)) * 2] = nb.h_er[b];
        history[((size_t)b * maxIter + (nb.it[b] - 1)) * 2 + 1] = h_step[b];
      }
      if (nb.h_er[b] > 1e3) nb.it[b] += 100;               // "Not likely to converge. Aborting." (:333-336)
    }
  }
  if (rc == LTO_OK) {
    e = launch_unpack_soa(d_X, J, nd, J, d_aos, st);
    if (e == hipSuccess) e = hipMemcpyAsync(XC_out, d_aos, sizeof(double) * nd * J, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && d_Xout) e = hipMemcpyAsync(d_Xout, d_X, sizeof(double) * nd * J, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && defect) {
      e = launch_unpack_soa(d_def, S, nd, S, d_def_aos, st);
      if (e == hipSuccess) e = hipMemcpyAsync(defect, d_def_aos, sizeof(double) * nd * S, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = max_abs(d_def, S, n - 1, h_mx.data()) == LTO_OK ? hipSuccess : hipErrorUnknown;   // (ends in a stream synchronise)
    call.idle = e == hipSuccess;
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
    // :339-341 flags a NaN trajectory; a NaN defect leaves the loop the same way (NaN > 1e-10 is false), so both
    // report status 2 here, as drivers.multiShoot_CRTBP_indirect does
    if (rc == LTO_OK)
      for (int b = 0; b < B; ++b)
        if (XC_out[(size_t)nd * n * b] != XC_out[(size_t)nd * n * b] || h_mx[b] != h_mx[b]) nb.status[b] = 2;
  }
  nb.copy_out(status_flag, iterations);
  return rc;
}

extern "C" {

int lto_indirect_solve_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC_in, const double* t, int n_tgrids,
                             const lto_params* prm, int n_prm, const lto_integrator* integ, int flag_adjointsOnly, int maxIter,
                             double* XC_out, double* defect, int* status_flag, int* iterations, double* history) {
  if (c && !XC_in) return set_err(c, LTO_ENULL, "XC_in, t, prm, integ, XC_out or status_flag is NULL");
  return indirect_solve_impl(c, ndim, n_nodes, n_batch, XC_in, nullptr, t, n_tgrids, prm, n_prm, integ, flag_adjointsOnly, maxIter,
                             XC_out, nullptr, defect, status_flag, iterations, history);
}

int lto_indirect_solve(lto_ctx* c, int ndim, int n_nodes, const double* XC_in, const double* t, const lto_params* prm,
                       const lto_integrator* integ, int flag_adjointsOnly, int maxIter, double* XC_out, double* defect,
                       int* status_flag, int* iterations, double* history) {
  return lto_indirect_solve_batch(c, ndim, n_nodes, 1, XC_in, t, 1, prm, 1, integ, flag_adjointsOnly, maxIter, XC_out, defect,
                                  status_flag, iterations, history);
}

}  // extern "C"

/* addTimeFinal (src/HelperFunctions.jl:196-250, re-specified in DESIGN 4.12, 4.21) for K time-of-flight changes dt[K] of one converged
 * solution of nd = 12 or 14 rows (`who` names the entry in the error texts), every phase on the device: the K extended trajectories
 * (end costates zeroed, a tail node at t[n-1] + dt) through the dense-output sweep at LinRange(t[0], t_end, n_desired); the
 * natural-spline re-mesh onto LinRange(t[0], t_end, n) (k_remesh_spline); the snap of the last node onto the arrival orbit
 * (k_find_tau); then, if XC_out is set, the Newton loop of lto_indirect_solve_batch started from the guesses in HBM, and the cost of
 * its results (k_dense_cost / k_dense_cost_mass).  14 rows: the tail is the 14-row system's own flow with zero costates (the thrust
 * acceleration exactly zero, the mass by mdot = -kappa umag(0, m) m of the same right-hand side), the re-solve leaves the final mass
 * free, and propellant [K] = XC[6, 0] - XC_out[6, n-1, k]. */
static int add_time_rows(const int nd, const char* who, lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t,
                         const lto_params* prm, const lto_integrator* integ, const lto_direct_orbits* orbits, int n_dt, const double* dt,
                         int n_desired, int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out,
                         double* tau_out, double* defect, int* status_flag, int* iterations, double* history, double* cost,
                         double* propellant) {
  if (!c) return LTO_ENULL;
  const auto fail = [&](int code, const char* what, hipError_t q = hipSuccess) {
    char text[384];
    std::snprintf(text, sizeof text, "%s: %s", who, what);
    return set_err(c, code, text, q);
  };
  if (!XC || !t || !prm || !integ || !orbits || !dt || !t_out || !tau_out || (XC_out && !status_flag))
    return fail(LTO_ENULL, "a required argument is NULL");
  if (ndim != nd) return fail(LTO_EUNSUPPORTED, nd == 12 ? "ndim must be 12 (dense output)" : "ndim must be 14");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE)
    return fail(LTO_EUNSUPPORTED, "dense output is built for LTO_RK4 and LTO_DOP853_ADAPTIVE");
  if (n_dt < 1 || n_nodes < 2 || n_desired < 4 || maxIter < 0)
    return fail(LTO_EINVAL, "need n_dt >= 1, n_nodes >= 2, n_desired >= 4, maxIter >= 0");
  for (int b = 0; b < n_dt; ++b)
    if (!(dt[b] > 0.0) || !std::isfinite(dt[b])) return fail(LTO_EINVAL, "every dt must be finite and > 0");
  if (orbits->nf < 2 || !orbits->tf || !orbits->Xf) return fail(LTO_EINVAL, "the arrival table needs >= 2 samples");
  const int K = n_dt, n = n_nodes, m = n_desired, ne = n + 1;
  if (nd == 14)
    for (int j = 0; j < n; ++j)
      if (!(XC[(size_t)14 * j + 6] > 0.0) || !std::isfinite(XC[(size_t)14 * j + 6])) return fail(LTO_EINVAL, "every node mass must be finite and > 0");
  if ((long)K * m * nd > 0x7fffffffL || (long)K * ne * nd > 0x7fffffffL) return fail(LTO_EINVAL, "batch too large");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  // host side: the grids, the sample ranges of every segment, the extended trajectories and the Thomas factors
  lto::HostBuf<double> h_te((size_t)K * ne), h_td((size_t)K * m), h_cp((size_t)m, 0.0), h_xe((size_t)nd * K * ne);
  lto::HostBuf<int> h_fe((size_t)K * n + 1), h_fc((size_t)K * (n - 1) + 1);
  if (!h_te.ok() || !h_td.ok() || !h_cp.ok() || !h_xe.ok() || !h_fe.ok() || !h_fc.ok()) return fail(LTO_ENOMEM, "out of host memory");
  const double t0 = t[0];
  // the sample ranges (segment_samples): the last segment also takes the last sample (t_end itself: the lane steps onto it exactly
  // as the final-state store of lto_indirect_densify does)
  for (int b = 0; b < K; ++b) {
    const double te = t[n - 1] + dt[b];
    double* tb = &h_te[(size_t)b * ne];
    std::memcpy(tb, t, sizeof(double) * n);
    tb[n] = te;
    double* tdb = &h_td[(size_t)b * m];
    linrange(t0, te, m, tdb);
    double* tnb = t_out + (size_t)b * n;
    linrange(t0, te, n, tnb);
    segment_samples(tb, ne, tdb, m, &h_fe[(size_t)b * n], b * m);
    segment_samples(tnb, n, tdb, m, &h_fc[(size_t)b * (n - 1)], b * m);
    double* xb = &h_xe[(size_t)nd * ne * b];
    std::memcpy(xb, XC, sizeof(double) * nd * n);
    for (int q = nd / 2; q < nd; ++q) xb[nd * (n - 1) + q] = 0.0;        // :199 (on a copy); 14 rows: lambda_r, lambda_v, lambda_m
    std::memcpy(xb + nd * n, xb + nd * (n - 1), sizeof(double) * nd);    // the tail's end node: never read by the sweep
  }
  h_fe[(size_t)K * n] = K * m;
  h_fc[(size_t)K * (n - 1)] = K * m;
  for (int i = 1; i < m - 1; ++i) h_cp[i] = 1.0 / (4.0 - h_cp[i - 1]);
  // device side: one block of the call's own (the solve loop below lays the arena out afresh)
  const long Je = (long)K * ne, Jn = (long)K * n, Jm = (long)K * m;
  double *d_xa, *d_xe, *d_te, *d_tn, *d_td, *d_cp, *d_y, *d_mom, *d_g, *d_ga, *d_xc, *d_tau, *d_cost;
  int *d_fe, *d_fc;
  ArenaLayout scratch;
  scratch.add((size_t)nd * Je, d_xa, d_xe);
  scratch.add((size_t)Je, d_te);
  scratch.add((size_t)Jn, d_tn);
  scratch.add((size_t)Jm, d_td);
  scratch.add((size_t)m, d_cp);
  scratch.add((size_t)Jn + 1, d_fe);
  scratch.add((size_t)(Jn - K) + 1, d_fc);
  scratch.add((size_t)nd * Jm, d_y, d_mom);
  scratch.add((size_t)nd * Jn, d_g, d_ga, d_xc);
  scratch.add((size_t)K, d_tau, d_cost);
  lto_direct_orbits arr = *orbits;                 // the upload builds both tables: the departure side gets the arrival's
  arr.n0 = arr.nf; arr.t0 = arr.tf; arr.X0 = arr.Xf;
  DevOrbits dob;
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = orbits_upload(c, &arr, dob, st);
  if (rc) return rc;
  rc = scratch.reserve_block(c, call.block[0], who);
  if (rc) return rc;
  rc = plan_build(c, nd, ne, K, prm, 1, integ, &call.plan[0]);
  if (rc) return rc;
  const auto dense = nd == 14 ? lto_indirect_dense_mass_dev : lto_indirect_dense_dev;
  hipError_t e = hipMemcpyAsync(d_xa, h_xe.data(), sizeof(double) * nd * Je, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_te, h_te.data(), sizeof(double) * Je, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_tn, t_out, sizeof(double) * Jn, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_td, h_td.data(), sizeof(double) * Jm, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_cp, h_cp.data(), sizeof(double) * m, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_fe, h_fe.data(), sizeof(int) * (Jn + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_fc, h_fc.data(), sizeof(int) * (Jn - K + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_pack_soa(d_xa, nd, Je, d_xe, Je, st);
  if (e != hipSuccess) return fail(LTO_EHIP, "stage in", e);
  // 1-2: the extended trajectories' dense output, Y [nd][K m]
  rc = dense(call.plan[0], st, d_xe, Je, d_te, K, d_fe, d_td, d_y, Jm, nullptr);
  if (rc) return rc;
  // 3-4: re-mesh, then the end snapped onto the arrival orbit; the guesses G [nd][K n] in the solve's layout
  RemeshArgs ra;
  ra.Y = d_y; ra.ldy = Jm; ra.td = d_td; ra.tn = d_tn; ra.cp = d_cp; ra.mom = d_mom; ra.G = d_g; ra.ldg = Jn;
  ra.m = m; ra.n = n; ra.K = K;
  e = launch_remesh_spline(nd, ra, st);
  if (e == hipSuccess) e = launch_find_tau(dob.o, d_g, Jn, n, K, d_tau, st);
  if (e == hipSuccess) e = hipMemcpyAsync(tau_out, d_tau, sizeof(double) * K, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && XC_guess) {
    e = launch_unpack_soa(d_g, Jn, nd, Jn, d_ga, st);
    if (e == hipSuccess) e = hipMemcpyAsync(XC_guess, d_ga, sizeof(double) * nd * Jn, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return fail(LTO_EHIP, "re-mesh", e);
  if (!XC_out) return LTO_OK;
  // 5: the Newton loop on the new grids (:236-237), started from G (12 rows: fixed ends; 14: m0 fixed, the final mass free)
  rc = indirect_solve_impl(c, nd, n, K, nullptr, d_g, t_out, K, prm, 1, integ, flag_adjointsOnly, maxIter, XC_out, cost ? d_xc : nullptr,
                           defect, status_flag, iterations, history);
  if (rc) return rc;
  if (nd == 14 && propellant)
    for (int b = 0; b < K; ++b) propellant[b] = XC[6] - XC_out[(size_t)14 * n * b + (size_t)14 * (n - 1) + 6];
  if (!cost) return rc;
  // the cost of every result: its dense output at the same LinRange(t[0], t_end, n_desired), trapezoid of umag
  call.idle = false;
  rc = plan_build(c, nd, n, K, prm, 1, integ, &call.plan[1]);
  if (rc == LTO_OK) rc = dense(call.plan[1], st, d_xc, Jn, d_tn, K, d_fc, d_td, d_y, Jm, nullptr);
  if (rc) return rc;
  if (nd == 14) {
    const double cT = prm->thrustLimit / 1e3 * (prm->TU * prm->TU) / prm->DU;                // aL = cT / m, the sample's own mass
    e = launch_dense_cost_mass(d_y, Jm, d_td, m, K, cT, prm->p, prm->rho, d_cost, st);
  } else {
    const double aL = prm->thrustLimit / prm->mass / 1e3 * (prm->TU * prm->TU) / prm->DU;   // stateCostate_deriv.jl:33
    e = launch_dense_cost(d_y, Jm, d_td, m, K, aL, prm->p, prm->rho, d_cost, st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(cost, d_cost, sizeof(double) * K, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return fail(LTO_EHIP, "cost", e);
  return LTO_OK;
}

extern "C" {

int lto_indirect_add_time_batch(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                                const lto_integrator* integ, const lto_direct_orbits* orbits, int n_dt, const double* dt, int n_desired,
                                int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out, double* tau_out,
                                double* defect, int* status_flag, int* iterations, double* history, double* cost) {
  return add_time_rows(12, "lto_indirect_add_time_batch", c, ndim, n_nodes, XC, t, prm, integ, orbits, n_dt, dt, n_desired,
                       flag_adjointsOnly, maxIter, XC_guess, XC_out, t_out, tau_out, defect, status_flag, iterations, history, cost,
                       nullptr);
}

int lto_indirect_add_time(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                          const lto_integrator* integ, const lto_direct_orbits* orbits, double dt, int n_desired, int flag_adjointsOnly,
                          int maxIter, double* XC_guess, double* XC_out, double* t_out, double* tau_out, double* defect, int* status_flag,
                          int* iterations, double* history, double* cost) {
  return lto_indirect_add_time_batch(c, ndim, n_nodes, XC, t, prm, integ, orbits, 1, &dt, n_desired, flag_adjointsOnly, maxIter,
                                     XC_guess, XC_out, t_out, tau_out, defect, status_flag, iterations, history, cost);
}

/* The same for the 14-row variable-mass system. */
int lto_indirect_add_time_mass_batch(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                                     const lto_integrator* integ, const lto_direct_orbits* orbits, int n_dt, const double* dt,
                                     int n_desired, int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out,
                                     double* tau_out, double* defect, int* status_flag, int* iterations, double* history, double* cost,
                                     double* propellant) {
  return add_time_rows(14, "lto_indirect_add_time_mass_batch", c, 14, n_nodes, XC, t, prm, integ, orbits, n_dt, dt, n_desired,
                       flag_adjointsOnly, maxIter, XC_guess, XC_out, t_out, tau_out, defect, status_flag, iterations, history, cost,
                       propellant);
}

int lto_indirect_add_time_mass(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                               const lto_integrator* integ, const lto_direct_orbits* orbits, double dt, int n_desired,
                               int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out, double* tau_out,
                               double* defect, int* status_flag, int* iterations, double* history, double* cost, double* propellant) {
  return lto_indirect_add_time_mass_batch(c, n_nodes, XC, t, prm, integ, orbits, 1, &dt, n_desired, flag_adjointsOnly, maxIter,
                                          XC_guess, XC_out, t_out, tau_out, defect, status_flag, iterations, history, cost, propellant);
}

}  // extern "C"

/* Mesh equidistribution of converged solutions of nd = 12 or 14 rows (`who` names the entry in the error texts),
 * every phase on the device: per pass the monitor (the caller's
 * weights, or the trial-step counts of a one-lane defect sweep of the current trajectories), the new grids (k_remesh_grid) and the
 * current trajectories' own states on them (k_remesh_nodes); then, if XC_out is set, the Newton loop of lto_indirect_solve_batch
 * started from the last pass's nodes in HBM.  Between the upload of XC, t and weights and the download of the results only the new
 * grids (once per pass: the host checks them, and the solve loop takes its grids from the host) and the step counts come down. */
static int remesh_rows(const int nd, const char* who, lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                       int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, int n_new, const double* weights,
                       int passes, int flag_adjointsOnly, int maxIter, double* t_out, double* XC_guess, double* XC_out,
                       double* defect, int* status_flag, int* iterations, double* history, int* steps_before, int* steps_after) {
  if (!c) return LTO_ENULL;
  const auto fail = [&](int code, const char* what, hipError_t q = hipSuccess) {
    char text[384];
    std::snprintf(text, sizeof text, "%s: %s", who, what);
    return set_err(c, code, text, q);
  };
  if (!XC || !t || !prm || !integ || !t_out || (XC_out && !status_flag))
    return fail(LTO_ENULL, "a required argument is NULL");
  if (ndim != nd) return fail(LTO_EUNSUPPORTED, "ndim must be 12 (dense output)");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE)
    return fail(LTO_EUNSUPPORTED, "dense output is built for LTO_RK4 and LTO_DOP853_ADAPTIVE");
  const bool adaptive = integ->method == LTO_DOP853_ADAPTIVE;
  if (n_batch < 1 || n_nodes < 2 || n_new < 2 || maxIter < 0 || passes < 1)
    return fail(LTO_EINVAL, "need n_batch >= 1, n_nodes >= 2, n_new >= 2, maxIter >= 0, passes >= 1");
  if ((n_tgrids != 1 && n_tgrids != n_batch) || (n_prm != 1 && n_prm != n_batch))
    return fail(LTO_EINVAL, "n_tgrids / n_prm must be 1 or n_batch");
  if (!weights && !adaptive) return fail(LTO_EINVAL, "a fixed-step integrator has no step counts: pass weights");
  if (weights && passes > 1) return fail(LTO_EINVAL, "passes > 1 needs the step counts as the monitor (weights == NULL)");
  const int B = n_batch, n0 = n_nodes, nn = n_new, nmax = n0 > nn ? n0 : nn;
  if (nmax - 1 > kRemeshMaxSegs) return fail(LTO_EINVAL, "more than 262144 segments per trajectory");
  if ((long)B * nmax * nd > 0x7fffffffL) return fail(LTO_EINVAL, "batch too large");
  const auto increasing = [](const double* g, int n, int count) {
    for (int b = 0; b < count; ++b)
      for (int i = 0; i + 1 < n; ++i)
        if (!(g[(size_t)b * n + i] < g[(size_t)b * n + i + 1]) || !std::isfinite(g[(size_t)b * n + i + 1] - g[(size_t)b * n + i])) return false;
    return true;
  };
  if (!increasing(t, n0, n_tgrids)) return fail(LTO_EINVAL, "t must be finite and strictly increasing");
  const long J0 = (long)B * n0, Jn = (long)B * nn, S0 = J0 - B, Sn = Jn - B, Smax = (long)B * (nmax - 1);
  if (weights)
    for (long i = 0; i < S0; ++i)
      if (!(weights[i] > 0.0) || !std::isfinite(weights[i])) return fail(LTO_EINVAL, "every weight must be finite and > 0");
  int rc = bind_device(c);
  if (rc) return rc;
  CallTimer call_timer(c);
  lto::HostBuf<int> h_cnt((size_t)2 * Smax);                // step counters on their way out (the stream copies into it)
  if (!h_cnt.ok()) return fail(LTO_ENOMEM, "out of host memory");
  // device side: one block of the call's own (the solve loop below lays the arena out afresh); the second of a pair, the final
  // trajectories, the weights, the defect and the monitor's scratch only where they are used
  const long Jmax = J0 > Jn ? J0 : Jn;
  const size_t c_stride = nmax - 1 > kRemeshLdsSegs ? remesh_scratch_doubles(nmax) : 0;
  const bool want_final = XC_out && steps_after && adaptive;
  double *d_xa, *d_x0, *d_g[2], *d_xf, *d_t0, *d_tn[2], *d_w, *d_def, *d_c;
  int* d_seg;
  ArenaLayout scratch;
  scratch.add((size_t)nd * Jmax, d_xa);
  scratch.add((size_t)nd * J0, d_x0);
  scratch.add((size_t)nd * Jn, d_g[0]);
  scratch.add(passes > 1 ? (size_t)nd * Jn : 0, d_g[1]);
  scratch.add(want_final ? (size_t)nd * Jn : 0, d_xf);
  scratch.add((size_t)n0 * n_tgrids, d_t0);
  scratch.add((size_t)Jn, d_tn[0]);
  scratch.add(passes > 1 ? (size_t)Jn : 0, d_tn[1]);
  scratch.add((size_t)Jn, d_seg);
  scratch.add(weights ? (size_t)S0 : 0, d_w);
  scratch.add(adaptive ? (size_t)nd * Smax : 0, d_def);
  scratch.add(c_stride * B, d_c);
  HostCall call(c);
  hipStream_t st = c->stream;
  rc = scratch.reserve_block(c, call.block[0], who);
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(d_xa, XC, sizeof(double) * nd * J0, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t0, t, sizeof(double) * n0 * n_tgrids, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && weights) e = hipMemcpyAsync(d_w, weights, sizeof(double) * S0, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_pack_soa(d_xa, nd, J0, d_x0, J0, st);
  if (e != hipSuccess) return fail(LTO_EHIP, "stage in", e);
  // trial steps of a defect sweep of X on tg, one lane per segment whatever the batch size (a batch's counts are its singles'):
  // left in the plan's counters; host_out (if set) = accepted + rejected once the stream has been waited for
  int* pending_out = nullptr;
  long pending_S = 0;
  auto count_sweep = [&](lto_indirect_plan* p, const double* X, long J, const double* tg, int ntg, int* host_out) -> int {
    p->defect_lanes = 1;
    int r = lto_indirect_defect_dev(p, st, X, J, tg, ntg, d_def, p->S, nullptr);
    if (r || !host_out) return r;
    hipError_t q = hipMemcpyAsync(h_cnt.data(), p->d_nacc, sizeof(int) * (size_t)p->S, hipMemcpyDeviceToHost, st);
    if (q == hipSuccess) q = hipMemcpyAsync(h_cnt.data() + p->S, p->d_nrej, sizeof(int) * (size_t)p->S, hipMemcpyDeviceToHost, st);
    if (q != hipSuccess) return fail(LTO_EHIP, "step counters", q);
    pending_out = host_out; pending_S = p->S;
    return LTO_OK;
  };
  auto counts_land = [&]() {
    for (long i = 0; pending_out && i < pending_S; ++i) pending_out[i] = h_cnt[(size_t)i] + h_cnt[(size_t)(pending_S + i)];
    pending_out = nullptr;
  };
  const double* d_xc = d_x0;
  const double* d_tc = d_t0;
  long Jc = J0;
  int nc = n0, ntgc = n_tgrids;
  for (int pass = 0; pass < passes; ++pass) {
    call.idle = false;
    rc = plan_build(c, nd, nc, B, prm, n_prm, integ, &call.plan[0]);
    if (rc) return rc;
    lto_indirect_plan* p = call.plan[0];
    const bool swept = adaptive && (!weights || (pass == 0 && steps_before));
    if (swept) rc = count_sweep(p, d_xc, Jc, d_tc, ntgc, pass == 0 ? steps_before : nullptr);
    if (rc) return rc;
    RemeshGridArgs ga;
    ga.t = d_tc; ga.t_stride = ntgc == 1 ? 0 : nc; ga.n = nc; ga.n_new = nn; ga.n_batch = B;
    ga.w = weights ? d_w : nullptr; ga.nacc = p->d_nacc; ga.nrej = p->d_nrej;
    ga.C = c_stride ? d_c : nullptr; ga.c_stride = (long)c_stride;
    ga.t_out = d_tn[pass & 1]; ga.seg_of = d_seg;
    e = launch_remesh_grid(ga, st);
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_remesh_grid", e);
    IndirectArgs a;
    rc = fill_indirect_args(p, d_xc, Jc, d_tc, ntgc, &a);
    if (rc) return rc;
    RemeshNodeArgs na;
    na.tn = d_tn[pass & 1]; na.seg_of = d_seg; na.G = d_g[pass & 1]; na.ldg = Jn; na.n_new = nn; na.n_batch = B;
    e = launch_remesh_nodes(nd, p->pm, p->integ.method, a, na, st);
    if (e == hipSuccess) e = hipMemcpyAsync(t_out, d_tn[pass & 1], sizeof(double) * Jn, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) return fail(LTO_EHIP, "re-mesh", e);
    counts_land();
    plan_free(p);                                            // (the stream is idle)
    call.plan[0] = nullptr;
    if (!increasing(t_out, nn, B))
      return fail(LTO_EINVAL, "the new grid is not strictly increasing (n_new beyond the grid's resolution, or a NaN trajectory)");
    d_xc = d_g[pass & 1]; d_tc = d_tn[pass & 1]; Jc = Jn; nc = nn; ntgc = B;
  }
  if (steps_before && !adaptive) for (long i = 0; i < S0; ++i) steps_before[i] = integ->steps;
  if (XC_guess) {
    call.idle = false;
    e = launch_unpack_soa(d_xc, Jn, nd, Jn, d_xa, st);
    if (e == hipSuccess) e = hipMemcpyAsync(XC_guess, d_xa, sizeof(double) * nd * Jn, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) return fail(LTO_EHIP, "guess", e);
  }
  if (XC_out) {
    rc = indirect_solve_impl(c, nd, nn, B, nullptr, d_xc, t_out, B, prm, n_prm, integ, flag_adjointsOnly, maxIter, XC_out,
                             want_final ? d_xf : nullptr, defect, status_flag, iterations, history);
    if (rc) return rc;
  }
  if (!steps_after) return LTO_OK;
  if (!adaptive) {
    for (long i = 0; i < Sn; ++i) steps_after[i] = integ->steps;
    return LTO_OK;
  }
  call.idle = false;
  rc = plan_build(c, nd, nn, B, prm, n_prm, integ, &call.plan[0]);
  if (rc == LTO_OK) rc = count_sweep(call.plan[0], XC_out ? d_xf : d_xc, Jn, d_tc, B, steps_after);
  if (rc) return rc;
  e = call.wait();
  if (e != hipSuccess) return fail(LTO_EHIP, "step counters", e);
  counts_land();
  return LTO_OK;
}

extern "C" {

int lto_indirect_remesh_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                              const lto_params* prm, int n_prm, const lto_integrator* integ, int n_new, const double* weights,
                              int passes, int flag_adjointsOnly, int maxIter, double* t_out, double* XC_guess, double* XC_out,
                              double* defect, int* status_flag, int* iterations, double* history, int* steps_before,
                              int* steps_after) {
  return remesh_rows(12, "lto_indirect_remesh_batch", c, ndim, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, n_new, weights, passes,
                     flag_adjointsOnly, maxIter, t_out, XC_guess, XC_out, defect, status_flag, iterations, history, steps_before,
                     steps_after);
}

/* The same for the 14-row variable-mass system: the re-solve is the 14-row loop (m0 pinned, final mass free, mass
 * costate of the last node 0). */
int lto_indirect_remesh_mass_batch(lto_ctx* c, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                   const lto_params* prm, int n_prm, const lto_integrator* integ, int n_new, const double* weights,
                                   int passes, int flag_adjointsOnly, int maxIter, double* t_out, double* XC_guess, double* XC_out,
                                   double* defect, int* status_flag, int* iterations, double* history, int* steps_before,
                                   int* steps_after) {
  return remesh_rows(14, "lto_indirect_remesh_mass_batch", c, 14, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, n_new, weights,
                     passes, flag_adjointsOnly, maxIter, t_out, XC_guess, XC_out, defect, status_flag, iterations, history,
                     steps_before, steps_after);
}

int lto_indirect_remesh_mass(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                             const lto_integrator* integ, int n_new, const double* weights, int passes, int flag_adjointsOnly,
                             int maxIter, double* t_out, double* XC_guess, double* XC_out, double* defect, int* status_flag,
                             int* iterations, double* history, int* steps_before, int* steps_after) {
  return lto_indirect_remesh_mass_batch(c, n_nodes, 1, XC, t, 1, prm, 1, integ, n_new, weights, passes, flag_adjointsOnly, maxIter, t_out,
                                        XC_guess, XC_out, defect, status_flag, iterations, history, steps_before, steps_after);
}

int lto_indirect_remesh(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                        const lto_integrator* integ, int n_new, const double* weights, int passes, int flag_adjointsOnly, int maxIter,
                        double* t_out, double* XC_guess, double* XC_out, double* defect, int* status_flag, int* iterations,
                        double* history, int* steps_before, int* steps_after) {
  return lto_indirect_remesh_batch(c, ndim, n_nodes, 1, XC, t, 1, prm, 1, integ, n_new, weights, passes, flag_adjointsOnly, maxIter,
                                   t_out, XC_guess, XC_out, defect, status_flag, iterations, history, steps_before, steps_after);
}

}  // extern "C"
