// lto_host_sweeps.hip -- the host-pointer sweeps: staging in and out, the context's cached plans, one Newton step, densify.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lto_host.hpp"

/* ------------------------------------------------------------------------------ host-pointer API
 * H2D (Julia layout) -> pack to SoA -> sweep -> unpack -> D2H, all on the context's stream, then one
 * stream synchronise.  The caller's buffers are only touched inside the call.  Pass buffers from lto_host_alloc
 * (page-locked) and the copies are plain DMA at link speed; pageable buffers are staged by the HIP runtime. */

// host AoS [ndim x count] -> device SoA rows of pitch ld.  Page-locked source: the pack kernel reads it over the link;
// otherwise a copy into d_aos first.
hipError_t stage_in(lto_ctx* c, const double* host, int ndim, long count, double* d_aos, double* d_soa, long ld,
                           hipStream_t st) {
  if (const double* z = pinned_view(c, host, sizeof(double) * (size_t)ndim * count)) return launch_pack_soa(z, ndim, count, d_soa, ld, st);
  hipError_t e = hipMemcpyAsync(d_aos, host, sizeof(double) * (size_t)ndim * count, hipMemcpyHostToDevice, st);
  return e == hipSuccess ? launch_pack_soa(d_aos, ndim, count, d_soa, ld, st) : e;
}
// device SoA -> host AoS [ndim x count]; the unpack kernel writes a page-locked destination directly.
hipError_t stage_out(lto_ctx* c, const double* d_soa, long ld, int ndim, long count, double* d_aos, double* host,
                            hipStream_t st) {
  if (double* z = pinned_view(c, host, sizeof(double) * (size_t)ndim * count)) return launch_unpack_soa(d_soa, ld, ndim, count, z, st);
  hipError_t e = launch_unpack_soa(d_soa, ld, ndim, count, d_aos, st);
  return e == hipSuccess ? hipMemcpyAsync(host, d_aos, sizeof(double) * (size_t)ndim * count, hipMemcpyDeviceToHost, st) : e;
}
// plain vectors (time grids, per-segment error estimates): a one-row pack / unpack is a copy kernel
hipError_t vec_in(lto_ctx* c, const double* host, long count, double* dev, hipStream_t st) {
  if (const double* z = pinned_view(c, host, sizeof(double) * (size_t)count)) return launch_pack_soa(z, 1, count, dev, count, st);
  return hipMemcpyAsync(dev, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, st);
}
static hipError_t vec_out(lto_ctx* c, const double* dev, long count, double* host, hipStream_t st) {
  if (double* z = pinned_view(c, host, sizeof(double) * (size_t)count)) return launch_unpack_soa(dev, count, 1, count, z, st);
  return hipMemcpyAsync(host, dev, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st);
}

// The plan of a host-pointer call: looked up in the context's small cache by (shape, integrator, parameter values),
// built on a miss (least recently used entry replaced).  Owned by the context.
int host_plan_acquire(lto_ctx* c, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm,
                             const lto_integrator* integ, lto_indirect_plan** out) {
  *out = nullptr;
  if (!prm || !integ) return set_err(c, LTO_ENULL, "prm or integrator is NULL");
  if (n_prm != 1 && n_prm != n_batch) return set_err(c, LTO_EINVAL, "n_prm must be 1 or n_batch");
  lto_ctx::HostPlan* slot = nullptr;               // an empty entry, else the least recently used one
  // the key compares the integrator field by field (the struct has padding a caller need not initialise) with the
  // max_steps default applied, so that 0 and 100000 share a plan
  const int want_max = integ->max_steps <= 0 ? 100000 : integ->max_steps;
  for (auto& h : c->host_plans) {
    const bool same_integ = h.plan && h.integ.method == integ->method && h.integ.steps == integ->steps && h.integ.rtol == integ->rtol &&
                            h.integ.atol == integ->atol && (h.integ.max_steps <= 0 ? 100000 : h.integ.max_steps) == want_max;
    if (h.plan && h.ndim == ndim && h.n_nodes == n_nodes && h.n_batch == n_batch && h.n_prm == n_prm && same_integ &&
        std::memcmp(h.prm, prm, sizeof(lto_params) * (size_t)n_prm) == 0) {
      h.stamp = ++c->stamp;
      *out = h.plan;
      return LTO_OK;
    }
    if (!slot || (slot->plan && (!h.plan || h.stamp < slot->stamp))) slot = &h;
  }
  lto_ctx::HostPlan* lru = slot;
  lto_indirect_plan* p = nullptr;
  int rc = plan_build(c, ndim, n_nodes, n_batch, prm, n_prm, integ, &p);
  if (rc) return rc;
  lto_params* key = (lto_params*)std::malloc(sizeof(lto_params) * (size_t)n_prm);
  if (!key) { plan_free(p); return set_err(c, LTO_EHIP, "host allocation failed"); }
  std::memcpy(key, prm, sizeof(lto_params) * (size_t)n_prm);
  if (lru->plan) {                                  // the evicted plan's blocks are recycled: nothing of it may be in flight
    (void)hipStreamSynchronize(c->stream);
    plan_free(lru->plan);
    std::free(lru->prm);
  }
  lru->plan = p; lru->prm = key; lru->ndim = ndim; lru->n_nodes = n_nodes; lru->n_batch = n_batch; lru->n_prm = n_prm;
  lru->integ = *integ; lru->stamp = ++c->stamp;
  *out = p;
  return LTO_OK;
}

// LinRange(t0, te, m) into out[0..m)
void linrange(double t0, double te, int m, double* out) {
  for (int k = 0; k < m; ++k) {
    const double tau = (double)k / (double)(m - 1);
    out[k] = (1.0 - tau) * t0 + tau * te;
  }
}
// samples of segment i of a grid g[0..nn-1]: td[0..m) in [g_i, g_{i+1}), the first of them into first[i] (+ base); the last sample
// is left to the caller's closing entry
void segment_samples(const double* g, int nn, const double* td, int m, int* first, int base) {
  int j = 0;
  for (int i = 0; i < nn - 1; ++i) {
    first[i] = base + j;
    while (j < m - 1 && td[j] < g[i + 1]) ++j;
  }
}

// densify for one trajectory, for lto_indirect_densify (any ndim a plan can be built for; the 12-row dense entry then decides) and
// lto_indirect_densify_mass (mass = true: 14 rows through lto_indirect_dense_mass_dev)
static int densify_host(lto_ctx* c, bool mass, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                        const lto_integrator* integ, int n_desired, double* XC_dense, double* t_dense) {
  lto::HostBuf<int> h_first;
  HostCall call(c);
  int rc = plan_build(c, ndim, n_nodes, 1, prm, 1, integ, &call.plan[0]);
  if (rc) return rc;
  lto_indirect_plan* p = call.plan[0];
  const int S = p->S;
  if (!h_first.alloc((size_t)S + 1)) return set_err(c, LTO_EHIP, "host allocation failed");
  linrange(t[0], t[n_nodes - 1], n_desired, t_dense);
  // samples of segment i: t_dense in [t_i, t_{i+1}); the last grid point (== t_n) is served by the final state
  segment_samples(t, n_nodes, t_dense, n_desired, h_first.data(), 0);
  h_first[S] = n_desired - 1;
  const long J = n_nodes;
  double *d_aos, *d_X, *d_t, *d_td, *d_Y, *d_Yaos;
  int* d_first;
  ArenaLayout scratch;
  scratch.add((size_t)ndim * J, d_aos, d_X);
  scratch.add((size_t)n_nodes, d_t);
  scratch.add((size_t)S + 1, d_first);
  scratch.add((size_t)n_desired, d_td);
  scratch.add((size_t)ndim * n_desired, d_Y, d_Yaos);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = hipMemcpyAsync(d_aos, XC, sizeof(double) * ndim * J, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t, t, sizeof(double) * n_nodes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_first, h_first.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_td, t_dense, sizeof(double) * n_desired, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_pack_soa(d_aos, ndim, J, d_X, J, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  // the final state lands in the last column of Y: final_state[c * n_batch + traj] with ld = n_desired, offset n_desired-1
  // is not expressible through the [ND][n_batch] layout, so take it into the tail of d_Yaos and splice on the host side
  double* d_final = d_Yaos;   // [ndim] (n_batch = 1); overwritten by the unpack afterwards, so copy it out first
  rc = mass ? lto_indirect_dense_mass_dev(p, st, d_X, J, d_t, 1, d_first, d_td, d_Y, n_desired, d_final)
            : lto_indirect_dense_dev(p, st, d_X, J, d_t, 1, d_first, d_td, d_Y, n_desired, d_final);
  if (rc == LTO_OK) {
    // splice: Y[c][n_desired-1] = final[c]
    for (int cc = 0; cc < ndim && e == hipSuccess; ++cc)
      e = hipMemcpyAsync(d_Y + (size_t)cc * n_desired + (n_desired - 1), d_final + cc, sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = launch_unpack_soa(d_Y, n_desired, ndim, n_desired, d_Yaos, st);
    if (e == hipSuccess) e = hipMemcpyAsync(XC_dense, d_Yaos, sizeof(double) * ndim * n_desired, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
  }
  return rc;
}

static int direct_host(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                       int n_tgrids, int nsteps, const lto_direct_params* prm, double* Jac_temp, double* ddefect_dtf,
                       double* defect, double* errors, bool want_jac, double* x_mid = nullptr) {
  CallTimer call_timer(c);
  HostCall call(c);
  int rc = direct_plan_build(c, nstate, n_nodes, n_batch, nsteps, prm, &call.dplan[0]);
  if (rc) return rc;
  lto_direct_plan* p = call.dplan[0];
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  const long J = (long)n_nodes * n_batch, S = p->S;
  const int nvar = 2 * (nstate + 3), nj = nstate * nvar;
  double *d_xa, *d_X, *d_ua, *d_U, *d_t, *d_def, *d_def_aos, *d_dtf, *d_dtf_aos, *d_err, *d_jac = nullptr, *d_jac_aos = nullptr;
  ArenaLayout scratch;
  scratch.add((size_t)nstate * J, d_xa, d_X);
  scratch.add((size_t)3 * J, d_ua, d_U);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)nstate * S, d_def, d_def_aos, d_dtf, d_dtf_aos);
  scratch.add((size_t)S, d_err);
  if (want_jac) scratch.add((size_t)nj * S, d_jac, d_jac_aos);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, X, nstate, J, d_xa, d_X, J, st);
  if (e == hipSuccess) e = stage_in(c, U, 3, J, d_ua, d_U, J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)n_nodes * n_tgrids, d_t, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  if (want_jac)
    rc = lto_direct_jacobian_dev(p, st, d_X, J, d_U, J, d_t, n_tgrids, d_jac, S, d_dtf, d_def, S, d_err);
  else   // the dtf staging buffers are free on this path: they carry the mid-point states
    rc = direct_defect_launch(p, st, d_X, J, d_U, J, d_t, n_tgrids, d_def, S, d_err, x_mid ? d_dtf : nullptr, S);
  if (rc == LTO_OK) {
    if (x_mid) e = stage_out(c, d_dtf, S, nstate, S, d_dtf_aos, x_mid, st);
    if (e == hipSuccess && defect) e = stage_out(c, d_def, S, nstate, S, d_def_aos, defect, st);
    if (e == hipSuccess && errors) e = vec_out(c, d_err, S, errors, st);
    if (e == hipSuccess && want_jac) {
      e = stage_out(c, d_jac, S, nj, S, d_jac_aos, Jac_temp, st);
      if (e == hipSuccess && ddefect_dtf) e = stage_out(c, d_dtf, S, nstate, S, d_dtf_aos, ddefect_dtf, st);
    }
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
  }
  return rc;
}

extern "C" {

int lto_indirect_defect(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                        const lto_params* prm, int n_prm, const lto_integrator* integ, double* defect, double* errors) {
  CallTimer call_timer(c);
  if (!c) return LTO_ENULL;
  if (!XC || !t || !defect) return set_err(c, LTO_ENULL, "XC, t or defect is NULL");
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  lto_indirect_plan* p = nullptr;
  int rc = host_plan_acquire(c, ndim, n_nodes, n_batch, prm, n_prm, integ, &p);   // cached between calls, owned by the context
  if (rc) return rc;
  const long J = (long)n_nodes * n_batch, S = p->S;
  double *d_aos, *d_X, *d_t, *d_def, *d_def_aos, *d_err;
  ArenaLayout scratch;
  scratch.add((size_t)ndim * J, d_aos, d_X);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)ndim * S, d_def, d_def_aos);
  scratch.add((size_t)S, d_err);
  rc = scratch.reserve(c);
  if (rc) return rc;
  HostCall call(c);
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, XC, ndim, J, d_aos, d_X, J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)n_nodes * n_tgrids, d_t, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  host_order_adopt(c, p, false);
  rc = lto_indirect_defect_dev(p, st, d_X, J, d_t, n_tgrids, d_def, S, errors ? d_err : nullptr);
  if (rc == LTO_OK) host_order_refresh(c, p, false, st);
  if (rc == LTO_OK) {
    e = stage_out(c, d_def, S, ndim, S, d_def_aos, defect, st);
    if (e == hipSuccess && errors) e = vec_out(c, d_err, S, errors, st);
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
  }
  return rc;
}

int lto_indirect_jacobian(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                          const lto_params* prm, int n_prm, const lto_integrator* integ, double* Phi, double* defect) {
  CallTimer call_timer(c);
  if (!c) return LTO_ENULL;
  if (!XC || !t || !Phi) return set_err(c, LTO_ENULL, "XC, t or Phi is NULL");
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  lto_indirect_plan* p = nullptr;
  int rc = host_plan_acquire(c, ndim, n_nodes, n_batch, prm, n_prm, integ, &p);   // cached between calls, owned by the context
  if (rc) return rc;
  const long J = (long)n_nodes * n_batch, S = p->S;
  const int nn = ndim * ndim;
  double *d_aos, *d_X, *d_t, *d_def, *d_def_aos, *d_phi, *d_phi_aos;
  ArenaLayout scratch;
  scratch.add((size_t)ndim * J, d_aos, d_X);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)ndim * S, d_def, d_def_aos);
  scratch.add((size_t)nn * S, d_phi, d_phi_aos);
  rc = scratch.reserve(c);
  if (rc) return rc;
  HostCall call(c);
  hipStream_t st = c->stream;
  // all operands page-locked: node array and time grid come in with one launch, STM and defect leave with one
  const long nt = (long)n_nodes * n_tgrids;
  const double* zX = pinned_view(c, XC, sizeof(double) * (size_t)ndim * J);
  const double* zt = pinned_view(c, t, sizeof(double) * (size_t)nt);
  double* zPhi = pinned_view(c, Phi, sizeof(double) * (size_t)nn * S);
  double* zdef = defect ? pinned_view(c, defect, sizeof(double) * (size_t)ndim * S) : nullptr;
  hipError_t e;
  if (zX && zt) {
    e = launch_pack_soa2(zX, ndim, J, d_X, J, zt, 1, nt, d_t, nt, st);
  } else {
    e = stage_in(c, XC, ndim, J, d_aos, d_X, J, st);
    if (e == hipSuccess) e = vec_in(c, t, nt, d_t, st);
  }
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  host_order_adopt(c, p, true);
  rc = lto_indirect_jacobian_dev(p, st, d_X, J, d_t, n_tgrids, d_phi, S, d_def, S);
  if (rc == LTO_OK) host_order_refresh(c, p, true, st);
  if (rc == LTO_OK) {
    if (zPhi && zdef) {
      e = launch_unpack_soa2(d_phi, S, nn, S, zPhi, d_def, S, ndim, S, zdef, st);
    } else {
      e = stage_out(c, d_phi, S, nn, S, d_phi_aos, Phi, st);
      if (e == hipSuccess && defect) e = stage_out(c, d_def, S, ndim, S, d_def_aos, defect, st);
    }
    if (e == hipSuccess) e = call.wait();
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
  }
  return rc;
}

/* densify of src/HelperFunctions.jl:51-101 for one trajectory: t_dense = LinRange(t[1], t[end], n_desired); every
 * segment is re-propagated and sampled at the t_dense points inside [t_i, t_{i+1}); the final propagated state is
 * appended (:94-97).  XC_dense [ndim x n_desired], t_dense [n_desired]. */
int lto_indirect_densify(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                         const lto_integrator* integ, int n_desired, double* XC_dense, double* t_dense) {
  if (!c) return LTO_ENULL;
  if (!XC || !t || !XC_dense || !t_dense) return set_err(c, LTO_ENULL, "XC, t, XC_dense or t_dense is NULL");
  if (n_desired < 2) return set_err(c, LTO_EINVAL, "n_desired must be >= 2");
  return densify_host(c, false, ndim, n_nodes, XC, t, prm, integ, n_desired, XC_dense, t_dense);
}

/* densify for one trajectory of the variable-mass system: XC [14 x n_nodes], Isp in prm->mass; XC_dense
 * [14 x n_desired].  The contract of lto_indirect_densify otherwise. */
int lto_indirect_densify_mass(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                              const lto_integrator* integ, int n_desired, double* XC_dense, double* t_dense) {
  if (!c) return LTO_ENULL;
  if (!XC || !t || !prm || !integ || !XC_dense || !t_dense) return set_err(c, LTO_ENULL, "lto_indirect_densify_mass: a required argument is NULL");
  if (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE)
    return set_err(c, LTO_EUNSUPPORTED, "lto_indirect_densify_mass: dense output is built for LTO_RK4 and LTO_DOP853_ADAPTIVE");
  if (n_desired < 2 || n_nodes < 2) return set_err(c, LTO_EINVAL, "lto_indirect_densify_mass: need n_nodes >= 2 and n_desired >= 2");
  return densify_host(c, true, 14, n_nodes, XC, t, prm, integ, n_desired, XC_dense, t_dense);
}

/* One Newton iteration of multiShoot_CRTBP_indirect on the device (indirect.jl:290-296; both settings of flag_adjointsOnly):
 * jacobianCalc + the least-squares step of optimizeTraj_OLS (:181-182) + its second-order correction (:190-214).
 * Only XC, t go up and xc_update, defect come down; Phi never leaves HBM. */
int lto_indirect_newton_step(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                             const lto_params* prm, int n_prm, const lto_integrator* integ, int flag_adjointsOnly,
                             double soc_threshold, double* xc_update, double* defect) {
  if (!c) return LTO_ENULL;
  if (!XC || !t || !xc_update) return set_err(c, LTO_ENULL, "XC, t or xc_update is NULL");
  if (ndim != 12 && ndim != 14) return set_err(c, LTO_EUNSUPPORTED, "device Newton step is built for ndim = 12 and 14");
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  lto_indirect_plan* p = nullptr;
  int rc = host_plan_acquire(c, ndim, n_nodes, n_batch, prm, n_prm, integ, &p);   // cached between calls, owned by the context
  if (rc) return rc;
  const int nd = ndim;
  const long J = (long)n_nodes * n_batch, S = p->S;
  double *d_aos, *d_X, *d_X2, *d_del, *d_del2, *d_t, *d_def, *d_def2, *d_def_aos, *d_phi;
  ArenaLayout scratch;
  scratch.add((size_t)nd * J, d_aos, d_X, d_X2, d_del, d_del2);
  scratch.add((size_t)n_nodes * n_tgrids, d_t);
  scratch.add((size_t)nd * S, d_def, d_def2, d_def_aos);
  scratch.add((size_t)nd * nd * S, d_phi);
  rc = scratch.reserve(c);
  if (rc) return rc;
  lto::HostBuf<double> h_del;
  HostCall call(c);
  hipStream_t st = c->stream;
  hipError_t e = hipMemcpyAsync(d_aos, XC, sizeof(double) * nd * J, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_t, t, sizeof(double) * n_nodes * n_tgrids, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_pack_soa(d_aos, nd, J, d_X, J, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "stage in", e);
  host_order_adopt(c, p, true);
  rc = lto_indirect_jacobian_dev(p, st, d_X, J, d_t, n_tgrids, d_phi, S, d_def, S);
  if (rc == LTO_OK) host_order_refresh(c, p, true, st);
  if (rc == LTO_OK) rc = lto_indirect_newton_solve_dev(p, st, d_phi, S, d_def, S, flag_adjointsOnly, d_del, J);
  if (rc == LTO_OK && !h_del.alloc((size_t)nd * J)) rc = set_err(c, LTO_EHIP, "host allocation failed");
  if (rc == LTO_OK) {
    e = hipMemcpyAsync(h_del.data(), d_del, sizeof(double) * nd * J, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "newton step", e);
  }
  if (rc == LTO_OK) {
    double mx = 0.0;
    bool finite = true;
    for (long k = 0; k < nd * J; ++k) { const double v = std::fabs(h_del[k]); if (!(v == v)) finite = false; if (v > mx) mx = v; }
    if (finite && mx < soc_threshold) {   // :190  norm(xc_update, Inf) < 1e-1
      e = launch_axpy(d_X, d_del, 1.0, d_X2, nd * J, st);
      if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "axpy", e);
      if (rc == LTO_OK) rc = lto_indirect_defect_dev(p, st, d_X2, J, d_t, n_tgrids, d_def2, S, nullptr);
      if (rc == LTO_OK) rc = lto_indirect_newton_solve_dev(p, st, nullptr, 0, d_def2, S, flag_adjointsOnly, d_del2, J);
      if (rc == LTO_OK) {
        e = launch_axpy(d_del, d_del2, 1.0, d_del, nd * J, st);
        if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "axpy", e);
      }
    }
  }
  if (rc == LTO_OK) {
    e = launch_unpack_soa(d_del, J, nd, J, d_aos, st);
    if (e == hipSuccess) e = hipMemcpyAsync(xc_update, d_aos, sizeof(double) * nd * J, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && defect) {
      e = launch_unpack_soa(d_def, S, nd, S, d_def_aos, st);
      if (e == hipSuccess) e = hipMemcpyAsync(defect, d_def_aos, sizeof(double) * nd * S, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    call.idle = e == hipSuccess;
    if (e != hipSuccess) rc = set_err(c, LTO_EHIP, "stage out", e);
  }
  return rc;
}

int lto_direct_defect(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                      int n_tgrids, int nsteps, const lto_direct_params* prm, double* defect, double* errors) {
  if (!c) return LTO_ENULL;
  if (!X || !U || !t || !defect) return set_err(c, LTO_ENULL, "X, U, t or defect is NULL");
  return direct_host(c, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, nullptr, nullptr, defect, errors, false);
}

int lto_direct_jacobian(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                        int n_tgrids, int nsteps, const lto_direct_params* prm, double* Jac_temp, double* ddefect_dtf,
                        double* defect, double* errors) {
  if (!c) return LTO_ENULL;
  if (!X || !U || !t || !Jac_temp) return set_err(c, LTO_ENULL, "X, U, t or Jac_temp is NULL");
  return direct_host(c, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, Jac_temp, ddefect_dtf, defect, errors, true);
}

int lto_direct_midpoints(lto_ctx* c, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                         int n_tgrids, int nsteps, const lto_direct_params* prm, double* x_mid, double* defect, double* errors) {
  if (!c) return LTO_ENULL;
  if (!X || !U || !t || !x_mid) return set_err(c, LTO_ENULL, "X, U, t or x_mid is NULL");
  return direct_host(c, nstate, n_nodes, n_batch, X, U, t, n_tgrids, nsteps, prm, nullptr, nullptr, defect, errors, false, x_mid);
}

}  // extern "C"
