// lto_indirect_events.hip -- switch times, burn arcs and dv of indirect solutions: the device-resident entry on a
// plan, and the host-pointer calls, which stage the trajectories in, run it on a plan of their own and bring the lists back.
// The _mass entries are the same calls for the 14-row variable-mass system, with the mass budget added; one body
// serves both, `nd` = 12 or 14 = the rows the entry is built for.
#include <cmath>

#include "lto_host.hpp"

namespace {

int events_supported(lto_ctx* c, int nd, int ndim, const lto_integrator* integ) {
  if (ndim != nd || (integ->method != LTO_RK4 && integ->method != LTO_DOP853_ADAPTIVE))
    return set_err(c, LTO_EUNSUPPORTED, nd == 12 ? "thrust events are built for ndim = 12 with LTO_RK4 or LTO_DOP853_ADAPTIVE"
                                                 : "the _mass thrust events are built for 14-row plans with LTO_RK4 or LTO_DOP853_ADAPTIVE");
  return LTO_OK;
}

int events_dev(int nd, lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
               int max_events, int* n_events, double* t_event, int* kind, int* on0, double* dv, double* burn_time,
               double* dv_seg, double* propellant, double* dm_seg, int* status) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!n_events || !t_event || !kind || !on0 || !dv || !burn_time || !status || (nd == 14 && !propellant))
    return set_err(c, LTO_ENULL, nd == 12 ? "lto_indirect_events_dev: n_events, t_event, kind, on0, dv, burn_time or status is NULL"
                                          : "lto_indirect_events_mass_dev: n_events, t_event, kind, on0, dv, burn_time, propellant or status is NULL");
  int rc = events_supported(c, nd, p->ndim, &p->integ);
  if (rc) return rc;
  if (max_events < 1) return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_dev: max_events must be >= 1");
  const int swept = p->swept;
  IndirectArgs a;
  rc = fill_indirect_args(p, X, ldx, t, n_tgrids, &a);
  p->swept = swept;                              // this sweep does not fill the plan's step counters
  if (rc) return rc;
  rc = bind_device(c);
  if (rc) return rc;
  const long S = p->S;
  if (!p->d_events) {
    const hipError_t e = pool_alloc(c, &p->d_events, events_record_bytes(S, p->ndim));
    if (e != hipSuccess) { p->d_events = nullptr; return set_err(c, LTO_EHIP, "lto_indirect_events[_mass]_dev: segment records", e); }
  }
  EventsArgs ev{};
  ev.tev = (double*)p->d_events;
  ev.q = ev.tev + (size_t)kEventsPerSeg * S;
  ev.ont = ev.q + S;
  double* recs_end = ev.ont + S;
  if (nd == 14) { ev.dm = recs_end; recs_end += S; ev.dm_seg = dm_seg; ev.propellant = propellant; }
  ev.nev = (int*)recs_end;
  ev.on_s = ev.nev + S;
  ev.on_e = ev.on_s + S;
  ev.max_events = max_events;
  ev.n_events = n_events; ev.t_event = t_event; ev.kind = kind; ev.on0 = on0; ev.dv = dv; ev.burn = burn_time;
  ev.dv_seg = dv_seg; ev.status = status;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  hipError_t e = launch_indirect_events(nd, p->pm, p->integ.method, a, ev, st);
  if (e == hipSuccess) e = launch_events_compact(a, ev, p->n_batch, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_indirect_events", e);
  return LTO_OK;
}

int events_batch(int nd, lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                 const lto_params* prm, int n_prm, const lto_integrator* integ, int max_events, int* n_events, double* t_event,
                 int* kind, int* on0, double* dv, double* burn_time, double* dv_seg, double* propellant, double* dm_seg, int* status) {
  if (!c) return LTO_ENULL;
  CallTimer call_timer(c);
  if (!XC || !t || !prm || !integ || !n_events || !t_event || !kind || !on0 || !dv || !burn_time || !status || (nd == 14 && !propellant))
    return set_err(c, LTO_ENULL, nd == 12 ? "lto_indirect_events_batch: XC, t, prm, integ, n_events, t_event, kind, on0, dv, burn_time or status is NULL"
                                          : "lto_indirect_events_mass_batch: XC, t, prm, integ, n_events, t_event, kind, on0, dv, burn_time, propellant or status is NULL");
  int rc = events_supported(c, nd, ndim, integ);
  if (rc) return rc;
  if (max_events < 1) return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_batch: max_events must be >= 1");
  if (n_nodes < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_batch: need n_nodes >= 2 and n_batch >= 1");
  if (n_tgrids != 1 && n_tgrids != n_batch) return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_batch: n_tgrids must be 1 or n_batch");
  if ((long)max_events * n_batch > 0x7fffffffL) return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_batch: max_events * n_batch beyond 2^31 - 1");
  for (int g = 0; g < n_tgrids; ++g) {
    const double* tb = t + (size_t)g * n_nodes;
    for (int i = 0; i + 1 < n_nodes; ++i)
      if (!(tb[i] < tb[i + 1]) || !std::isfinite(tb[i + 1] - tb[i]))
        return set_err(c, LTO_EINVAL, "lto_indirect_events[_mass]_batch: t must be finite and strictly increasing");
  }
  const int B = n_batch, M = max_events;
  const size_t J = (size_t)n_nodes * B, S = (size_t)(n_nodes - 1) * B, nt = (size_t)n_nodes * n_tgrids;
  HostCall call(c);
  rc = plan_build(c, ndim, n_nodes, n_batch, prm, n_prm, integ, &call.plan[0]);
  if (rc) return rc;
  double *d_aos, *d_X, *d_t, *d_tev, *d_dv, *d_bt, *d_dvseg, *d_prop, *d_dmseg;
  int *d_nev, *d_kind, *d_on0, *d_status;
  ArenaLayout scratch;
  scratch.add((size_t)nd * J, d_aos, d_X);
  scratch.add(nt, d_t);
  scratch.add((size_t)M * B, d_tev);
  scratch.add((size_t)M * B, d_kind);
  scratch.add((size_t)B, d_dv, d_bt);
  scratch.add((size_t)B, d_nev, d_on0, d_status);
  scratch.add(dv_seg ? S : 0, d_dvseg);
  scratch.add(nd == 14 ? (size_t)B : 0, d_prop);
  scratch.add(dm_seg ? S : 0, d_dmseg);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = c->stream;
  hipError_t e = stage_in(c, XC, nd, (long)J, d_aos, d_X, (long)J, st);
  if (e == hipSuccess) e = vec_in(c, t, (long)nt, d_t, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_indirect_events[_mass]_batch: stage in", e);
  rc = events_dev(nd, call.plan[0], st, d_X, (long)J, d_t, n_tgrids, M, d_nev, d_tev, d_kind, d_on0, d_dv, d_bt,
                  dv_seg ? d_dvseg : nullptr, nd == 14 ? d_prop : nullptr, dm_seg ? d_dmseg : nullptr, d_status);
  if (rc) return rc;
  e = hipMemcpyAsync(n_events, d_nev, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_event, d_tev, sizeof(double) * M * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(kind, d_kind, sizeof(int) * M * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(on0, d_on0, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dv, d_dv, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(burn_time, d_bt, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dv_seg) e = hipMemcpyAsync(dv_seg, d_dvseg, sizeof(double) * S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nd == 14) e = hipMemcpyAsync(propellant, d_prop, sizeof(double) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && dm_seg) e = hipMemcpyAsync(dm_seg, d_dmseg, sizeof(double) * S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = call.wait();
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "lto_indirect_events[_mass]_batch: stage out", e);
  return LTO_OK;
}

}  // namespace

extern "C" {

int lto_indirect_events_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                            int max_events, int* n_events, double* t_event, int* kind, int* on0, double* dv, double* burn_time,
                            double* dv_seg, int* status) {
  return events_dev(12, p, stream, X, ldx, t, n_tgrids, max_events, n_events, t_event, kind, on0, dv, burn_time, dv_seg, nullptr,
                    nullptr, status);
}

int lto_indirect_events_batch(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                              const lto_params* prm, int n_prm, const lto_integrator* integ, int max_events, int* n_events,
                              double* t_event, int* kind, int* on0, double* dv, double* burn_time, double* dv_seg, int* status) {
  return events_batch(12, c, ndim, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, max_events, n_events, t_event, kind, on0,
                      dv, burn_time, dv_seg, nullptr, nullptr, status);
}

int lto_indirect_events(lto_ctx* c, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                        const lto_integrator* integ, int max_events, int* n_events, double* t_event, int* kind, int* on0,
                        double* dv, double* burn_time, double* dv_seg, int* status) {
  return lto_indirect_events_batch(c, ndim, n_nodes, 1, XC, t, 1, prm, 1, integ, max_events, n_events, t_event, kind, on0, dv,
                                   burn_time, dv_seg, status);
}

int lto_indirect_events_mass_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                                 int max_events, int* n_events, double* t_event, int* kind, int* on0, double* dv, double* burn_time,
                                 double* dv_seg, double* propellant, double* dm_seg, int* status) {
  return events_dev(14, p, stream, X, ldx, t, n_tgrids, max_events, n_events, t_event, kind, on0, dv, burn_time, dv_seg, propellant,
                    dm_seg, status);
}

int lto_indirect_events_mass_batch(lto_ctx* c, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                   const lto_params* prm, int n_prm, const lto_integrator* integ, int max_events, int* n_events,
                                   double* t_event, int* kind, int* on0, double* dv, double* burn_time, double* dv_seg,
                                   double* propellant, double* dm_seg, int* status) {
  return events_batch(14, c, 14, n_nodes, n_batch, XC, t, n_tgrids, prm, n_prm, integ, max_events, n_events, t_event, kind, on0, dv,
                      burn_time, dv_seg, propellant, dm_seg, status);
}

int lto_indirect_events_mass(lto_ctx* c, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                             const lto_integrator* integ, int max_events, int* n_events, double* t_event, int* kind, int* on0,
                             double* dv, double* burn_time, double* dv_seg, double* propellant, double* dm_seg, int* status) {
  return lto_indirect_events_mass_batch(c, n_nodes, 1, XC, t, 1, prm, 1, integ, max_events, n_events, t_event, kind, on0, dv,
                                        burn_time, dv_seg, propellant, dm_seg, status);
}

}  // extern "C"
