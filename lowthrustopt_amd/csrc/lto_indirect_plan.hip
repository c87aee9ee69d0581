// lto_indirect_plan.hip -- indirect plans: construction, setters and getters, lane order, record staging, warm start, the
// device-resident sweeps with the choice of their kernel form, and kernel calibration.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "lto_host.hpp"

namespace {

// Reference validity rule for p (stateCostate_deriv.jl:36-53): p == 0, p == 1 or p > 1.
bool p_valid(double p) { return p == 0.0 || p == 1.0 || p > 1.0; }

int make_traj_params(lto_ctx* c, int ndim, const lto_params* prm, int n, TrajParams* out, int* pm_out) {
  int pm = 0;
  for (int i = 0; i < n; ++i) {
    const lto_params& q = prm[i];
    if (!p_valid(q.p)) return set_err(c, LTO_EBADP, "Invalid value of p!");
    TrajParams t;
    // ndim = 12: `mass` is the constant spacecraft mass.  ndim = 14: mass is state[7] and the slot carries Isp.
    t.accel_limit = (ndim == 12) ? q.thrustLimit / q.mass / 1e3 * (q.TU * q.TU) / q.DU : 0.0;  // stateCostate_deriv.jl:33
    t.cT = q.thrustLimit / 1e3 * (q.TU * q.TU) / q.DU;
    t.kappa_td = (ndim == 14) ? q.time_direction * 1e3 * q.DU / (q.TU * q.mass * 9.81) : 0.0;
    t.inv_2rho = 1.0 / (2.0 * q.rho);
    t.inv_rho = 1.0 / q.rho;
    t.p = q.p;
    t.inv_p = (q.p != 0.0) ? 1.0 / q.p : 0.0;
    t.inv_pm1 = (q.p > 1.0) ? 1.0 / (q.p - 1.0) : 0.0;
    t.omega = q.time_direction;
    t.MU = q.MU;
    out[i] = t;
    pm |= 1 << p_class(q.p);
  }
  *pm_out = pm;                                  // bit mask of the control-law classes present
  return LTO_OK;
}

int check_integ(lto_ctx* c, const lto_integrator* ig) {
  if (!ig) return set_err(c, LTO_ENULL, "integrator is NULL");
  switch (ig->method) {
    case LTO_RK4:
    case LTO_RKF78_FIXED:
      if (ig->steps < 1) return set_err(c, LTO_EINVAL, "fixed-step integrator needs steps >= 1");
      return LTO_OK;
    case LTO_RKF78_ADAPTIVE:
      if (!(ig->rtol > 0.0)) return set_err(c, LTO_EINVAL, "adaptive integrator needs rtol > 0");
      return LTO_OK;
    case LTO_DOP853_ADAPTIVE:
      if (!(ig->rtol > 0.0) || !(ig->atol >= 0.0)) return set_err(c, LTO_EINVAL, "adaptive integrator needs rtol > 0, atol >= 0");
      return LTO_OK;
  }
  return set_err(c, LTO_EINVAL, "unknown integrator method");
}

}  // namespace

/* ------------------------------------------------------------------------------ indirect plans */

void plan_free(lto_indirect_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  pool_free(p->ctx, p->d_tp, sizeof(TrajParams) * (size_t)p->n_prm);
  pool_free(p->ctx, p->d_nacc, sizeof(int) * (size_t)p->S);
  pool_free(p->ctx, p->d_nrej, sizeof(int) * (size_t)p->S);
  if (!p->order_borrowed) pool_free(p->ctx, p->d_order, order_bytes(p->S));
  pool_free(p->ctx, p->d_bvp, p->bvp_bytes);
  for (int k = 0; k < 2; ++k) pool_free(p->ctx, p->d_hfirst[k], sizeof(double) * (size_t)p->S);
  if (p->h_stats) (void)hipHostFree(p->h_stats);
  if (p->stats_ev) (void)hipEventDestroy(p->stats_ev);
  pool_free(p->ctx, p->d_stats_acc, sizeof(unsigned long long) * 4);
  pool_free(p->ctx, p->d_xa, sizeof(double) * NODE_REC * (size_t)p->n_nodes * p->n_batch);
  pool_free(p->ctx, p->d_da, sizeof(double) * 12 * (size_t)p->S);
  pool_free(p->ctx, p->d_pa, sizeof(double) * 144 * (size_t)p->S);
  pool_free(p->ctx, p->d_events, events_record_bytes(p->S, p->ndim));
  delete p;
}

// plan construction without lifetime bookkeeping (the library's own short-lived and cached plans)
int plan_build(lto_ctx* c, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm,
                      const lto_integrator* integ, lto_indirect_plan** out) {
  if (!c || !out) return LTO_ENULL;
  *out = nullptr;
  if (!prm) return set_err(c, LTO_ENULL, "prm is NULL");
  if (ndim != 12 && ndim != 14) return set_err(c, LTO_EINVAL, "ndim must be 12 (or 14: mass + mass costate extension)");
  if (n_nodes < 2 || n_batch < 1) return set_err(c, LTO_EINVAL, "need n_nodes >= 2 and n_batch >= 1");
  if (n_prm != 1 && n_prm != n_batch) return set_err(c, LTO_EINVAL, "n_prm must be 1 or n_batch");
  if ((long)(n_nodes - 1) * n_batch > 0x7fffffffL) return set_err(c, LTO_EINVAL, "too many segments");
  int rc = check_integ(c, integ);
  if (rc) return rc;
  rc = bind_device(c);
  if (rc) return rc;
  lto::HostBuf<TrajParams> h((size_t)n_prm);
  if (!h.ok()) return set_err(c, LTO_EHIP, "host allocation failed");
  int pm = 0;
  rc = make_traj_params(c, ndim, prm, n_prm, h.data(), &pm);
  if (rc) return rc;
  lto_indirect_plan* p = new (std::nothrow) lto_indirect_plan();
  if (!p) return set_err(c, LTO_EHIP, "host allocation failed");
  std::memset(p, 0, sizeof *p);
  p->ctx = c; p->ndim = ndim; p->n_nodes = n_nodes; p->n_batch = n_batch; p->S = (n_nodes - 1) * n_batch;
  p->pm = pm; p->n_prm = n_prm; p->integ = *integ; p->bvp_variant = -1;
  if (p->integ.max_steps <= 0) p->integ.max_steps = 100000;
  hipError_t e = pool_alloc(c, (void**)&p->d_tp, sizeof(TrajParams) * (size_t)n_prm);
  if (e == hipSuccess) e = hipMemcpy(p->d_tp, h.data(), sizeof(TrajParams) * (size_t)n_prm, hipMemcpyHostToDevice);
  const bool adaptive = integ->method == LTO_RKF78_ADAPTIVE || integ->method == LTO_DOP853_ADAPTIVE;
  if (e == hipSuccess && adaptive) {
    e = pool_alloc(c, (void**)&p->d_nacc, sizeof(int) * (size_t)p->S);
    if (e == hipSuccess) e = pool_alloc(c, (void**)&p->d_nrej, sizeof(int) * (size_t)p->S);
  }
  if (e != hipSuccess) {
    plan_free(p);
    return set_err(c, LTO_EHIP, "plan allocation", e);
  }
  // Page-locked landing place of the trial-step statistics that steer AUTO's lanes per segment (lto_indirect_defect_dev): here, not
  // in the first sweep that wants it -- a sweep may be inside a caller's graph capture, where nothing may be allocated.
  if (defect_stats_wanted(ndim, integ->method, LTO_KERNEL_AUTO, 0, p->S, c->cu_count)) {
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess &&
        pool_alloc(c, (void**)&p->d_stats_acc, sizeof(unsigned long long) * 4) == hipSuccess &&
        hipMemset(p->d_stats_acc, 0, sizeof(unsigned long long) * 4) == hipSuccess) {
      std::memset(hp, 0, 64);
      p->h_stats = (long long*)hp; p->h_stats_dev = (long long*)dp;
      if (hipEventCreateWithFlags(&p->stats_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError(); (void)hipHostFree(hp);
        p->h_stats = nullptr; p->stats_ev = nullptr;
      }
    } else {                       // no statistics: AUTO keeps its size thresholds
      (void)hipGetLastError();
      if (hp) (void)hipHostFree(hp);
      p->h_stats = nullptr;
    }
  }
  *out = p;
  return LTO_OK;
}

// Lane order of the adaptive sweeps.  Round 5: ordered inside windows of consecutive segments, the windows dealt to the XCDs
// (kernels.hpp LTO_ORDER_WINDOW) -- the sweeps then gather from and scatter to the caller's arrays inside one L2 and need no record
// staging.  LTO_ORDER_MODE=global in the environment (development switch, read once per process): the global order of round 4 with
// its record staging.
// A plan that runs STM sweeps keeps the global order and its records: with sixteen workgroup-rounds per CU the sweep's time is the
// sum of its rounds, longest-processing-time-first over ALL workgroups is what keeps that sum short, and the windowed order costs
// 17 % of time there (1.75 against 1.50 ms at C5 + STM) for its 2.6 x less traffic.  A defect-only plan (C5 itself, the line
// search's trial plan) takes the windowed order: same time, a third of the traffic, no record passes.
static int order_kind_for(bool stm) {
  static const int forced = [] {
    const char* e = std::getenv("LTO_ORDER_MODE");
    return !e ? 0 : std::strcmp(e, "global") == 0 ? 1 : std::strcmp(e, "windowed") == 0 ? 2 : 0;
  }();
  return forced ? forced : (stm ? 1 : 2);
}
static int order_weave() {
  static const int w = [] { const char* e = std::getenv("LTO_ORDER_WEAVE"); const int v = e ? std::atoi(e) : 0; return (v >= 1 && v <= 255) ? v : 0; }();      // 0 = the kernel's choice
  return w;
}
static hipError_t segment_order(int kind, const int* nacc, const int* nrej, long S, int* work, int* order, hipStream_t st) {
  return kind == 2 ? launch_segment_order_windowed(nacc, nrej, (int)S, order_weave(), work, order, st)
                   : launch_segment_order(nacc, nrej, (int)S, work, order, st);
}

// Record staging (12-dim plans with the reference's integrator setting): the buffers come with the lane order, outside any sweep.
static bool stage_capable(const lto_indirect_plan* p) { return indirect_records_available(p->ndim, p->integ.method); }
// need_phi: the plan runs STM sweeps, so the [S][144] Phi records are wanted too.  A defect-only plan (the line search's S x 20
// trial plan) never gets them: at 256 x 1 024 x 20 segments they would pin 6 GB nothing reads (advisor finding, round 4).  An
// allocation that fails switches staging off for what it was for -- the sweeps then gather from the caller's arrays as before --
// and is reported: lto_indirect_plan_staging() carries the bit, lto_last_error() the text (the call still returns LTO_OK).
static int stage_alloc(lto_indirect_plan* p, bool need_phi) {
  if (!stage_capable(p)) return LTO_OK;
  lto_ctx* c = p->ctx;
  const bool own = !p->out_blocks;       // LTO_LAYOUT_BLOCKS: the caller's Phi / defect arrays ARE the records
  struct { double** ptr; size_t n; bool want; } want[3] = {{&p->d_xa, (size_t)NODE_REC * p->n_nodes * p->n_batch, true},
                                                           {&p->d_da, (size_t)12 * p->S, own}, {&p->d_pa, (size_t)144 * p->S, need_phi && own}};
  for (auto& w : want) {
    if (*w.ptr || !w.want) continue;
    hipError_t e = pool_alloc(c, (void**)w.ptr, sizeof(double) * w.n);
    if (e != hipSuccess) {
      *w.ptr = nullptr; (void)hipGetLastError();
      p->stage_failed = 1;
      std::snprintf(c->err, sizeof c->err, "note: record staging of ordered sweeps is off for this plan (%zu bytes: %s); results are unaffected",
                    sizeof(double) * w.n, hipGetErrorString(e));
      return LTO_OK;
    }
  }
  return LTO_OK;
}

// The h_first array of sweep kind `which` (0 STM, 1 defect-only); args get it with the warm flag.  The caller marks the array valid
// (warm_filled) only once the sweep that fills it has been launched successfully.
static int warm_args(lto_indirect_plan* p, int which, bool kernel_records, IndirectArgs* a) {
  a->h_first = nullptr; a->warm = 0;
  if (!p->warm_start || !kernel_records || !p->d_hfirst[which]) return LTO_OK;
  a->h_first = p->d_hfirst[which];
  a->warm = p->hfirst_valid[which];
  return LTO_OK;
}
static void warm_filled(lto_indirect_plan* p, int which, const IndirectArgs& a) {
  if (a.h_first) p->hfirst_valid[which] = 1;          // stream order: the next sweep of this kind reads what this one wrote
}

int fill_indirect_args(lto_indirect_plan* p, const double* X, long ldx, const double* t, int n_tgrids,
                              IndirectArgs* a) {
  lto_ctx* c = p->ctx;
  if (!X || !t) return set_err(c, LTO_ENULL, "X or t is NULL");
  const long J = (long)p->n_nodes * p->n_batch;
  if (ldx < J) return set_err(c, LTO_EINVAL, "ldx smaller than n_nodes*n_batch");
  if (n_tgrids != 1 && n_tgrids != p->n_batch) return set_err(c, LTO_EINVAL, "n_tgrids must be 1 or n_batch");
  std::memset(a, 0, sizeof *a);
  a->X = X; a->ldx = ldx; a->t = t; a->t_stride = (n_tgrids == 1) ? 0 : p->n_nodes;
  a->tp = p->d_tp; a->tp_stride = (p->n_prm == 1) ? 0 : 1;
  a->n_nodes = p->n_nodes; a->seg_per_traj = p->n_nodes - 1; a->S = p->S;
  a->steps = p->integ.steps; a->rtol = p->integ.rtol; a->atol = p->integ.atol; a->max_steps = p->integ.max_steps;
  a->nacc = p->d_nacc; a->nrej = p->d_nrej;
  a->order = p->use_order ? p->d_order : nullptr;
  a->xcd_ranges = (p->use_order && p->order_kind == 2) ? 1 : 0;
  a->stm_scale = std::pow(3.0, -(double)(p->integ.steps > 0 ? p->integ.steps % 256 : 0));   // pipe_common.hpp COL_RESCALE_EVERY
  p->swept = 1;                                    // every caller launches a sweep right after a successful fill
  return LTO_OK;
}

// Record staging of a sweep, for both entries below.  kernel_records: the form that runs reads node records and writes per-segment
// records.  Balanced lane order (the global kind): nodes in, Phi / defects out as records (IndirectArgs::Xa / Pa / Da), coalesced
// transposes either side of the sweep (records_out).  LTO_LAYOUT_BLOCKS: the caller's Phi / defect arrays ARE the records the kernel
// writes -- no record arrays of the plan's own and no transposes behind the sweep, with or without a lane order.
static int records_in(lto_indirect_plan* p, bool kernel_records, IndirectArgs* a, hipStream_t st, bool* staged) {
  const bool blocks = p->out_blocks != 0;
  *staged = a->order && p->order_kind == 1 && kernel_records && p->d_xa && (blocks || (p->d_da && (!a->Phi || p->d_pa)));
  if (*staged) {
    hipError_t q = launch_node_records(a->X, a->ldx, a->t, a->t_stride, p->n_nodes, (long)p->n_nodes * p->n_batch, p->d_xa, st);
    if (q != hipSuccess) return set_err(p->ctx, LTO_EHIP, "launch_node_records", q);
    a->Xa = p->d_xa;
    if (a->Phi) a->Pa = p->d_pa;
    if (a->defect) a->Da = p->d_da;
  }
  if (blocks && a->Phi) a->Pa = a->Phi;
  if (blocks && a->defect) a->Da = a->defect;
  return LTO_OK;
}
static hipError_t records_out(const lto_indirect_plan* p, bool staged, const IndirectArgs& a, hipStream_t st) {
  if (!staged || p->out_blocks) return hipSuccess;
  hipError_t e = a.Phi ? launch_pack_soa(p->d_pa, 144, p->S, a.Phi, a.ldp, st) : hipSuccess;
  if (e == hipSuccess && a.Da) e = launch_pack_soa(p->d_da, 12, p->S, a.defect, a.ldd, st);
  return e;
}

static hipError_t launch_defect(int lanes, const lto_indirect_plan* p, const IndirectArgs& a, hipStream_t st) {
  if (lanes == 4) return launch_indirect_defect4(p->ndim, p->pm, a, st);
  if (lanes == 2) return launch_indirect_defect2(p->pm, a, st);
  return launch_indirect_defect(p->ndim, p->pm, p->integ.method, a, st);
}

static hipError_t launch_stm(const StmChoice& ch, const lto_indirect_plan* p, const IndirectArgs& a, hipStream_t st) {
  switch (ch.kernel) {
    case LTO_KERNEL_COOP: return launch_indirect_stm_coop(p->ndim, p->pm, p->integ.method, a, st);
    case LTO_KERNEL_COOP2: return launch_indirect_stm_coop2(p->ndim, p->pm, a, st);
    case LTO_KERNEL_PIPE8: return launch_indirect_stm_pipe8(p->ndim, p->pm, a, st);
    case LTO_KERNEL_PIPE48: return launch_indirect_stm_pipe48(p->ndim, p->pm, a, ch.seg44, st);
    case LTO_KERNEL_PIPE32: return launch_indirect_stm_pipe32(p->ndim, p->pm, a, st);
    case LTO_KERNEL_LANE: return launch_indirect_stm_lane(p->pm, a, st);
  }
  return ch.stream ? launch_indirect_stm_stream(p->ndim, p->pm, a, st)
                   : launch_indirect_stm(p->ndim, p->pm, p->integ.method, p->cols_per_lane, a, st);
}

/* Host-pointer API: adopt / refresh the context's cached lane order (see lto_ctx::order_cache).  Below these sizes
 * one round of wavefronts / workgroups covers the chip and the order cannot matter. */
// Round 4: defect-only sweeps from 16 384 segments (was 131 072).  Every wavefront of such a sweep is resident at once, but a
// wavefront lasts as long as its slowest segment and holds its registers and issue slots until then: with the lanes ordered, the
// line search's 20 x 4 096 segments take 69 instead of 152 us, 20 x 1 024 take 50 instead of 63 (tools/probe_linesearch_lanes.py).
static const long kOrderMinStm = 8192, kOrderMinDefect = 16384;

bool host_order_wanted(const lto_indirect_plan* p, bool stm) {
  return p->d_nacc && p->S >= (stm ? kOrderMinStm : kOrderMinDefect);
}

void host_order_adopt(lto_ctx* c, lto_indirect_plan* p, bool stm) {
  c->last_call_order = 0;
  if (p->order_borrowed) { p->d_order = nullptr; p->use_order = 0; p->order_borrowed = 0; }   // cached plan: the context's order may have moved
  const int kind = order_kind_for(stm);
  if (!host_order_wanted(p, stm) || !c->order_cache[kind] || c->order_S[kind] != p->S || c->order_ndim[kind] != p->ndim) return;
  p->d_order = c->order_cache[kind]; p->order_borrowed = 1; p->use_order = 1; p->order_kind = kind;
  c->last_call_order = kind;
  if (kind == 1) (void)stage_alloc(p, stm);
}

void host_order_refresh(lto_ctx* c, lto_indirect_plan* p, bool stm, hipStream_t st) {
  if (!host_order_wanted(p, stm)) return;
  const int kind = order_kind_for(stm);
  if (!c->order_cache[kind] || c->order_S[kind] != p->S) {
    if (p->use_order) return;                      // (cannot happen: adoption requires a matching cache)
    if (c->order_cache[kind]) { (void)hipStreamSynchronize(st); (void)hipFree(c->order_cache[kind]); c->order_cache[kind] = nullptr; }
    if (hipMalloc((void**)&c->order_cache[kind], order_bytes(p->S)) != hipSuccess) {
      c->order_cache[kind] = nullptr; (void)hipGetLastError();
      return;                                      // balancing is an optimisation: carry on without it
    }
    c->order_S[kind] = p->S;
  }
  c->order_ndim[kind] = p->ndim;
  if (segment_order(kind, p->d_nacc, p->d_nrej, p->S, c->order_cache[kind] + p->S, c->order_cache[kind], st) != hipSuccess) {
    (void)hipGetLastError();
    c->order_S[kind] = 0;                          // never adopt a half-written order
  }
}

extern "C" {

int lto_indirect_plan_create(lto_ctx* c, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm,
                             const lto_integrator* integ, lto_indirect_plan** out) {
  const int rc = plan_build(c, ndim, n_nodes, n_batch, prm, n_prm, integ, out);
  if (rc == LTO_OK) ctx_plan_added(c);
  return rc;
}

// The caller may have launched sweeps of this plan on its own streams: the plan's device blocks go back to the
// context's block cache (pool_free) and may be handed to the next plan at once, so everything in flight on the device
// has to finish first.  Destroying a plan is rare; the library's own short-lived plans are freed by HostCall, behind a
// drain of the one stream they used.
void lto_indirect_plan_destroy(lto_indirect_plan* p) {
  if (!p) return;
  lto_ctx* c = p->ctx;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  plan_free(p);
  if (ctx_release(c, OWNER_PLAN)) ctx_free(c);
}

const int* lto_indirect_plan_steps_accepted(const lto_indirect_plan* p) { return p ? p->d_nacc : nullptr; }
const int* lto_indirect_plan_steps_rejected(const lto_indirect_plan* p) { return p ? p->d_nrej : nullptr; }

int lto_indirect_plan_copy_steps(lto_indirect_plan* p, void* stream, int* accepted, int* rejected) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!p->d_nacc || !p->d_nrej) return set_err(c, LTO_EINVAL, "fixed-step plan has no step counters");
  int rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  if (accepted) e = hipMemcpyAsync(accepted, p->d_nacc, sizeof(int) * (size_t)p->S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rejected) e = hipMemcpyAsync(rejected, p->d_nrej, sizeof(int) * (size_t)p->S, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "copy step counters", e);
  return LTO_OK;
}

int lto_indirect_plan_staging(const lto_indirect_plan* p) {
  if (!p) return 0;
  if (p->out_blocks) return (p->d_xa ? 3 : 0) | (p->stage_failed ? 4 : 0);      // node records only: results go straight to the caller's blocks
  return ((p->d_xa && p->d_da) ? 1 : 0) | (p->d_pa ? 2 : 0) | (p->stage_failed ? 4 : 0);
}

int lto_indirect_plan_set_output_layout(lto_indirect_plan* p, int layout) {
  if (!p) return LTO_ENULL;
  if (layout != LTO_LAYOUT_SOA && layout != LTO_LAYOUT_BLOCKS) return set_err(p->ctx, LTO_EINVAL, "layout must be LTO_LAYOUT_SOA or LTO_LAYOUT_BLOCKS");
  if (layout == LTO_LAYOUT_BLOCKS && !stage_capable(p))
    return set_err(p->ctx, LTO_EUNSUPPORTED, "LTO_LAYOUT_BLOCKS is built for 12-dim DOP853_ADAPTIVE plans (the kernels that write per-segment records)");
  p->out_blocks = layout == LTO_LAYOUT_BLOCKS;
  return LTO_OK;
}

int lto_indirect_plan_rebalance(lto_indirect_plan* p, void* stream) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!p->d_nacc || !p->d_nrej) return set_err(c, LTO_EINVAL, "fixed-step plan: every segment takes the same number of steps");
  if (!p->swept) return set_err(c, LTO_EINVAL, "no sweep has run on this plan yet: there are no step counts to balance by");
  int rc = bind_device(c);
  if (rc) return rc;
  if (!p->d_order) {
    hipError_t e = pool_alloc(c, (void**)&p->d_order, order_bytes(p->S));
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "order allocation", e);
  }
  const int kind = order_kind_for(p->stm_swept != 0);
  hipError_t e = segment_order(kind, p->d_nacc, p->d_nrej, p->S, p->d_order + p->S, p->d_order, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_segment_order", e);
  p->use_order = 1;
  p->order_kind = kind;
  return kind == 2 ? LTO_OK : stage_alloc(p, p->stm_swept != 0);
}

int lto_indirect_plan_reset_order(lto_indirect_plan* p) {
  if (!p) return LTO_ENULL;
  p->use_order = 0;
  return LTO_OK;
}

int lto_indirect_plan_copy_order(lto_indirect_plan* p, void* stream, int* order_host, int* kind_out) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (!kind_out) return set_err(c, LTO_ENULL, "kind_out is NULL");
  const int kind = (p->use_order && p->d_order) ? p->order_kind : 0;       // what fill_indirect_args hands the next sweep
  if (kind != 0) {
    if (!order_host) return set_err(c, LTO_ENULL, "order_host is NULL and the plan has a lane order");
    int rc = bind_device(c);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(order_host, p->d_order, sizeof(int) * (size_t)p->S, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "copy lane order", e);
  }
  *kind_out = kind;
  return LTO_OK;
}

int lto_indirect_plan_set_kernel(lto_indirect_plan* p, int kernel) {
  if (!p) return LTO_ENULL;
  // (selectors 3 and 4 are not indirect families: 3 = LTO_KERNEL_DIRECT_PIPE, the direct plans' pipelined Jacobian kernel; 4 is unassigned)
  if (kernel != LTO_KERNEL_AUTO && kernel != LTO_KERNEL_PER_LANE && kernel != LTO_KERNEL_COOP && kernel != LTO_KERNEL_LANE &&
      kernel != LTO_KERNEL_PIPE8 && kernel != LTO_KERNEL_COOP2 && kernel != LTO_KERNEL_PIPE48 && kernel != LTO_KERNEL_PIPE32)
    return set_err(p->ctx, LTO_EINVAL, "kernel must be LTO_KERNEL_AUTO, _PER_LANE, _COOP, _PIPE8, _COOP2, _PIPE48, _PIPE32 or _LANE");
  if (kernel == LTO_KERNEL_LANE && !indirect_stm_lane_available(p->ndim, p->integ.method, p->S))
    return set_err(p->ctx, LTO_EINVAL, "LTO_KERNEL_LANE is built for 12-dim RK4 plans");
  if (kernel == LTO_KERNEL_COOP2 && !indirect_stm_coop2_available(p->ndim, p->integ.method, p->pm))
    return set_err(p->ctx, LTO_EINVAL, "LTO_KERNEL_COOP2 is built for DOP853_ADAPTIVE plans: 12-dim, and 14-dim with p = 0 or p = 1");
  if ((kernel == LTO_KERNEL_PIPE8 || kernel == LTO_KERNEL_PIPE48 || kernel == LTO_KERNEL_PIPE32) && !indirect_stm_pipeline_available(p->integ.method))
    return set_err(p->ctx, LTO_EINVAL, "the pipeline kernels are built for fixed-step RK4 plans");
  if (kernel == LTO_KERNEL_PIPE32 && !indirect_stm_pipe32_available(p->ndim, p->pm))
    return set_err(p->ctx, LTO_EINVAL, "LTO_KERNEL_PIPE32 is built for 12-dim plans and for 14-dim plans with p = 0 or p = 1");
  p->kernel = kernel;
  return LTO_OK;
}

int lto_indirect_plan_last_kernel(const lto_indirect_plan* p) { return p ? p->last_kernel : LTO_KERNEL_AUTO; }

int lto_indirect_plan_set_defect_lanes(lto_indirect_plan* p, int lanes) {
  if (!p) return LTO_ENULL;
  if (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 4) return set_err(p->ctx, LTO_EINVAL, "defect lanes must be 0 (choose), 1, 2 or 4");
  if ((lanes == 2 && !indirect_defect2_available(p->ndim, p->integ.method)) || (lanes == 4 && !indirect_defect4_available(p->ndim, p->integ.method, p->pm)))
    return set_err(p->ctx, LTO_EINVAL, "two and four lanes per segment are built for 12-dim DOP853_ADAPTIVE plans (the reference's integrator setting); "
                                       "four also for 14-dim DOP853_ADAPTIVE plans with p = 0 or p = 1");
  p->defect_lanes = lanes;
  return LTO_OK;
}

int lto_indirect_plan_set_warm_start(lto_indirect_plan* p, int on) {
  if (!p) return LTO_ENULL;
  if (on && !indirect_warm_start_available(p->ndim, p->integ.method))
    return set_err(p->ctx, LTO_EINVAL, "warm start is built for 12-dim DOP853_ADAPTIVE plans (the reference's integrator setting)");
  if (on) {
    // Both arrays are allocated and zeroed HERE, not inside the first warm sweep (advisor finding, round 3): a sweep may be part
    // of a caller's graph capture, where nothing may be allocated, and a segment a sweep skips (zero span, another launch's
    // control-law class) must leave a value the next sweep recognises as "none" -- 0 -- not whatever the pool handed out.
    int rc = bind_device(p->ctx);
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {
      if (p->d_hfirst[k]) continue;
      hipError_t e = pool_alloc(p->ctx, (void**)&p->d_hfirst[k], sizeof(double) * (size_t)p->S);
      if (e == hipSuccess) e = hipMemset(p->d_hfirst[k], 0, sizeof(double) * (size_t)p->S);
      if (e != hipSuccess) { p->d_hfirst[k] = nullptr; return set_err(p->ctx, LTO_EHIP, "warm-start array", e); }
      p->hfirst_valid[k] = 0;
    }
  }
  p->warm_start = on ? 1 : 0;
  if (!on) { p->hfirst_valid[0] = 0; p->hfirst_valid[1] = 0; }
  return LTO_OK;
}

int lto_indirect_plan_set_cols_per_lane(lto_indirect_plan* p, int cols) {
  if (!p) return LTO_ENULL;
  if (cols == 12 || cols == 14) {
    if (cols != p->ndim || !indirect_stm_stream_available(p->ndim, p->integ.method, p->integ.steps, p->S))
      return set_err(p->ctx, LTO_EINVAL, "cols_per_lane = ndim (12 or 14: the whole STM in the segment's lane) is built for RK4 plans with ONE step per segment");
  } else if (cols != 0 && cols != 1 && cols != 2 && cols != 3) return set_err(p->ctx, LTO_EINVAL, "cols_per_lane must be 0, 1, 2, 3 or the plan's dimension");
  if (p->ndim == 14 && cols == 3) return set_err(p->ctx, LTO_EUNSUPPORTED, "14 STM columns do not split into groups of 3: use 0 (auto), 1 or 2");
  if (p->ndim == 12 && cols == 2) return set_err(p->ctx, LTO_EUNSUPPORTED, "two columns per lane are not built for 12-dim plans (removed in round 6: one column wins up to 8 192 segments, three above): use 0 (auto), 1 or 3");
  p->cols_per_lane = cols;
  return LTO_OK;
}

// Fill args -> decide (sweep_policy.hpp defect_lanes) -> stage in -> launch -> stage out.
int lto_indirect_defect_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t,
                            int n_tgrids, double* defect, long ldd, double* errors) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  IndirectArgs a;
  int rc = fill_indirect_args(p, X, ldx, t, n_tgrids, &a);
  if (rc) return rc;
  if (!defect) return set_err(c, LTO_ENULL, "defect is NULL");
  if (ldd < p->S && !p->out_blocks) return set_err(c, LTO_EINVAL, "ldd smaller than the segment count");
  a.defect = defect; a.ldd = ldd; a.errors = errors;
  rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  const bool stats = defect_stats_wanted(p->ndim, p->integ.method, p->kernel, p->defect_lanes, p->S, c->cu_count);
  if (stats && p->h_stats && p->stats_pending) {
    // The verdict is the same in every run of the same call sequence (advisor finding, round 4: it used to be "whatever has
    // arrived by then", read while the kernel might still be writing): statistics are consumed only behind the event recorded
    // after k_step_stats -- the host waits for it here, i.e. for the EARLIER sweep that launched it, which a Newton loop has
    // long read back -- then latched in the plan until the next statistics launch is consumed.  Inside a graph capture nothing
    // may be waited for: the latched verdict stands.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
    if (cap == hipStreamCaptureStatusNone && hipEventSynchronize(p->stats_ev) == hipSuccess) {
      p->stats_pending = 0;
      p->stats_lanes = defect_stats_verdict(p->h_stats[0], p->h_stats[1], p->h_stats[2], p->S, c->cu_count);
    }
  }
  const int lanes = defect_lanes(p->ndim, p->integ.method, p->pm, p->S, p->kernel, p->defect_lanes, (stats && p->h_stats) ? p->stats_lanes : 0,
                                 p->out_blocks != 0, c->cu_count);
  rc = warm_args(p, 1, lanes > 1, &a);
  if (rc) return rc;
  bool staged = false;
  rc = records_in(p, lanes > 1, &a, st, &staged);
  if (rc) return rc;
  hipError_t e = launch_defect(lanes, p, a, st);
  if (e == hipSuccess) e = records_out(p, staged, a, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_indirect_defect", e);
  warm_filled(p, 1, a);
  if (stats) {
    // statistics for the next sweep's choice (a few us, stream-ordered, written by the kernel itself into page-locked memory)
    // not after every sweep (the extra launch and its host write cost ~10 us): after the first two, then every sixteenth
    const int age = p->stats_age++;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;        // (an event recorded inside a capture cannot be waited for later)
    if (p->h_stats && (age < 2 || (age & 15) == 0) && hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone &&
        launch_step_stats(p->d_nacc, p->d_nrej, p->S, p->d_stats_acc, p->h_stats_dev, st) == hipSuccess &&
        hipEventRecord(p->stats_ev, st) == hipSuccess)
      p->stats_pending = 1;
  }
  p->swept = 1;
  return LTO_OK;
}

int lto_indirect_auto_kernel(int ndim, int method, int steps, double p, long n_segments, int n_cus, int ordered) {
  if ((ndim != 12 && ndim != 14) || method < LTO_RK4 || method > LTO_DOP853_ADAPTIVE || n_segments < 1 || n_cus < 1) return LTO_EINVAL;
  if (!(p == 0.0 || p >= 1.0)) return LTO_EINVAL;           // the reference's error("Invalid value of p!") is a run-time code; here: not a plan
  const int pm = 1 << p_class(p);
  return auto_stm_kernel(ndim, method, steps, pm, n_segments, n_cus, ordered != 0, 0, kRoundCostDefault[ndim == 14 ? 1 : 0], kRoundCostDefault[0][2], kLaneRoundUs);
}

// Fill args -> decide (sweep_policy.hpp resolve_stm) -> stage in -> launch -> stage out.
int lto_indirect_jacobian_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t,
                              int n_tgrids, double* Phi, long ldp, double* defect, long ldd) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  IndirectArgs a;
  int rc = fill_indirect_args(p, X, ldx, t, n_tgrids, &a);
  if (rc) return rc;
  if (!Phi) return set_err(c, LTO_ENULL, "Phi is NULL");
  if (!p->out_blocks && (ldp < p->S || (defect && ldd < p->S))) return set_err(c, LTO_EINVAL, "ldp/ldd smaller than the segment count");
  a.Phi = Phi; a.ldp = ldp; a.defect = defect; a.ldd = ldd;
  rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  const StmChoice ch = resolve_stm(p->ndim, p->integ.method, p->integ.steps, p->pm, p->S, p->kernel, p->cols_per_lane, p->use_order != 0, p->p48_form,
                                   c->cu_count > 0 ? c->cu_count : 256, c->round_cost, c->lane_round_us);
  const bool kernel_records = ch.kernel == LTO_KERNEL_COOP2;
  p->last_kernel = ch.kernel;
  rc = warm_args(p, 0, kernel_records, &a);
  if (rc) return rc;
  p->stm_swept = 1;
  const bool blocks = p->out_blocks != 0;
  if (blocks && !kernel_records) return set_err(c, LTO_EUNSUPPORTED, "LTO_LAYOUT_BLOCKS needs the two-lanes-per-state cooperative kernel (LTO_KERNEL_AUTO or _COOP2)");
  if (!blocks && a.order && p->order_kind == 1 && kernel_records && p->d_xa && p->d_da && !p->d_pa && !p->stage_failed) {
    // the lane order was made before this plan's first STM sweep: the Phi records come now -- unless the stream is being captured
    // (an allocation may not happen there; this sweep then runs unstaged and a later one outside a capture allocates)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) (void)stage_alloc(p, true);
    else (void)hipGetLastError();
  }
  bool staged = false;
  rc = records_in(p, kernel_records, &a, st, &staged);
  if (rc) return rc;
  hipError_t e = launch_stm(ch, p, a, st);
  if (e == hipSuccess) e = records_out(p, staged, a, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_indirect_stm", e);
  warm_filled(p, 0, a);
  p->swept = 1;
  return LTO_OK;
}

/* ------------------------------------------------------------------------------ device Newton solve */
int lto_indirect_newton_solve_dev(lto_indirect_plan* p, void* stream, const double* Phi, long ldp, const double* defect,
                                  long ldd, int adjoints_only, double* delta, long ldx) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  if (p->out_blocks) return set_err(c, LTO_EUNSUPPORTED, "device Newton solve reads struct-of-arrays Phi / defect: use a plan with LTO_LAYOUT_SOA");
  if (!defect || !delta) return set_err(c, LTO_ENULL, "defect or delta is NULL");
  if (ldd < p->S || (Phi && ldp < p->S) || ldx < (long)p->n_nodes * p->n_batch) return set_err(c, LTO_EINVAL, "leading dimension too small");
  int rc = bind_device(c);
  if (rc) return rc;
  if (!p->d_bvp) {
    if (!Phi) return set_err(c, LTO_EINVAL, "no factorisation yet: the first solve needs Phi");
    p->bvp_bytes = sizeof(double) * bvp_workspace_doubles(p->ndim, p->n_nodes, p->n_batch);
    hipError_t e = pool_alloc(c, (void**)&p->d_bvp, p->bvp_bytes);
    if (e != hipSuccess) { p->d_bvp = nullptr; return set_err(c, LTO_EHIP, "newton workspace", e); }
  }
  const int variant = adjoints_only ? 1 : 0;
  if (!Phi && p->bvp_variant != variant) return set_err(c, LTO_EINVAL, "re-solve requested for a variant that was not factored");
  hipError_t e = launch_bvp_solve(p->ndim, Phi, ldp, defect, ldd, p->n_nodes, p->n_batch, variant, p->d_bvp, delta, ldx, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_bvp_solve", e);
  if (Phi) p->bvp_variant = variant;
  return LTO_OK;
}

/* ------------------------------------------------------------------------------ dense output */
// One body for both entries; `rows` is the row count the entry is declared for (12: lto_indirect_dense_dev, 14:
// lto_indirect_dense_mass_dev).  A plan of another row count is refused before anything is launched.
static int dense_dev_rows(int rows, lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                          const int* first, const double* t_samples, double* Y, long ldy, double* final_state) {
  if (!p) return LTO_ENULL;
  lto_ctx* c = p->ctx;
  IndirectArgs a;
  int rc = fill_indirect_args(p, X, ldx, t, n_tgrids, &a);
  if (rc) return rc;
  if (!first || !t_samples || !Y) return set_err(c, LTO_ENULL, "first, t_samples or Y is NULL");
  // dense output is built for what densify needs (HelperFunctions.jl:51-101 re-propagates with the solver of the sweep: the 12-dim
  // system, DOP853 for Vern8) and for the contract's RK4; round 6 removed the 24 other instantiations, which nothing ran
  // (DESIGN 4.20 brought the 14-row RK4 / DOP853 forms back, behind an entry of their own)
  if (p->ndim != rows || (p->integ.method != LTO_RK4 && p->integ.method != LTO_DOP853_ADAPTIVE))
    return set_err(c, LTO_EUNSUPPORTED, rows == 12 ? "dense output is built for ndim = 12 with LTO_RK4 or LTO_DOP853_ADAPTIVE"
                                                   : "lto_indirect_dense_mass_dev takes a 14-row plan with LTO_RK4 or LTO_DOP853_ADAPTIVE");
  rc = bind_device(c);
  if (rc) return rc;
  DenseArgs d;
  d.first = first; d.td = t_samples; d.Y = Y; d.ldy = ldy; d.final_state = final_state;
  hipStream_t st = (hipStream_t)stream;
  timing_begin(c, st);
  hipError_t e = launch_indirect_dense(p->ndim, p->pm, p->integ.method, a, d, st);
  timing_end(c, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_indirect_dense", e);
  p->swept = 1;
  return LTO_OK;
}

int lto_indirect_dense_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                           const int* first, const double* t_samples, double* Y, long ldy, double* final_state) {
  return dense_dev_rows(12, p, stream, X, ldx, t, n_tgrids, first, t_samples, Y, ldy, final_state);
}

int lto_indirect_dense_mass_dev(lto_indirect_plan* p, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                                const int* first, const double* t_samples, double* Y, long ldy, double* final_state) {
  return dense_dev_rows(14, p, stream, X, ldx, t, n_tgrids, first, t_samples, Y, ldy, final_state);
}

/* AUTO's cost table measured on this device: one full round of every RK4 STM family and dimension (16 / 48 / 64 x CUs segments,
 * 64 RK4 steps, one state near the L2 halo orbits in every segment -- fixed-step kernels do the same work whatever the data), after 30 ms of
 * sweeps so that the clocks have settled; the median of five launches. */
int lto_calibrate_kernels(lto_ctx* c) {
  if (!c) return LTO_ENULL;
  int rc = bind_device(c);
  if (rc) return rc;
  const long cus = c->cu_count > 0 ? c->cu_count : 256;
  const long per_round[5] = {16 * cus, 48 * cus, 64 * cus, 44 * cus, 32 * cus};
  const int family_kernel[5] = {LTO_KERNEL_PIPE8, LTO_KERNEL_PIPE48, LTO_KERNEL_PER_LANE, LTO_KERNEL_PIPE48, LTO_KERNEL_PIPE32};
  const long lane_round = 256 * cus;                 // the whole-segment lanes' round (12-dim): the largest batch measured
  const long Smax = lane_round, nmax = Smax + 1;
  hipStream_t st = c->stream;
  LTO_HIP(c, hipStreamSynchronize(st));
  double *d_X, *d_t, *d_phi, *d_def;
  ArenaLayout scratch;
  scratch.add((size_t)14 * nmax, d_X);
  scratch.add((size_t)nmax, d_t);
  scratch.add((size_t)196 * Smax, d_phi);
  scratch.add((size_t)14 * Smax, d_def);
  rc = scratch.reserve(c);
  if (rc) return rc;
  // a state near the Earth-Moon L2 halo family (0.17 DU from the Moon), small costates; 1 000 kg / lambda_m = 0.1 for the 14-row layout
  const double x12[12] = {1.1599795702248494, 0.0097200000000000, -0.1240184140575570, 0.0087153964800000, -0.2085329310256100, 0.0105833000000000,
                          0.01, -0.02, 0.015, 0.02, 0.01, -0.01};
  lto::HostBuf<double> hX((size_t)14 * nmax), ht((size_t)nmax);
  if (!hX.ok() || !ht.ok()) return set_err(c, LTO_ENOMEM, "lto_calibrate_kernels: out of host memory");
  for (long k = 0; k < nmax; ++k) ht[k] = 0.02 * (double)k;
  hipEvent_t e0, e1;
  LTO_HIP(c, hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return set_err(c, LTO_EHIP, "hipEventCreate"); }
  lto_params prm = {0.012150585609624, 384400.0, 375190.25852, 0.05, 1000.0, 1.0, 1.0, 1.0};
  lto_integrator integ; std::memset(&integ, 0, sizeof integ);
  integ.method = LTO_RK4; integ.steps = 64;
  double measured[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 1e300, 1e300, 0}};
  double measured_lane = 0.0;
  for (int di = 0; di < 2 && rc == LTO_OK; ++di) {
    const int nd = di ? 14 : 12;
    for (long k = 0; k < nmax; ++k)
      for (int r = 0; r < nd; ++r) {
        double v;
        if (nd == 12) v = x12[r];
        else v = (r < 6) ? x12[r] : (r == 6) ? 1000.0 : (r < 13) ? x12[r - 1] : 0.1;
        hX[(size_t)r * nmax + k] = v;
      }
    prm.mass = di ? 3000.0 : 1000.0;                 // 14-row layout: the slot carries Isp
    hipError_t e = hipMemcpyAsync(d_X, hX.data(), sizeof(double) * nd * nmax, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_t, ht.data(), sizeof(double) * nmax, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { rc = set_err(c, LTO_EHIP, "calibration upload", e); break; }
    for (int f = 0; f < 6 && rc == LTO_OK; ++f) {     // f = 5: the whole-segment lanes (12-dim only)
      if (nd == 14 && (f == 2 || f == 3 || f == 5)) continue;
      const long S = (f == 5) ? lane_round : per_round[f];      // one full round: with 44 x CUs segments the 44-form is the cheaper one, with 48 x CUs the 48-form
      HostCall call(c);                             // owns the family's plan
      rc = plan_build(c, nd, (int)(S + 1), 1, &prm, 1, &integ, &call.plan[0]);
      if (rc) break;
      lto_indirect_plan* p = call.plan[0];
      p->kernel = (f == 5) ? LTO_KERNEL_LANE : family_kernel[f];
      p->p48_form = (f == 3) ? 44 : 48;
      if (f == 2) p->cols_per_lane = 3;
      auto sweep = [&]() { return lto_indirect_jacobian_dev(p, st, d_X, nmax, d_t, 1, d_phi, S, d_def, S); };
      if (di == 0 && f == 0) {                      // let the clocks settle: ~30 ms of sweeps
        const auto t0 = std::chrono::steady_clock::now();
        while (rc == LTO_OK && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 0.03) {
          for (int q = 0; q < 16 && rc == LTO_OK; ++q) rc = sweep();
          if (rc == LTO_OK && hipStreamSynchronize(st) != hipSuccess) rc = set_err(c, LTO_EHIP, "calibration warm-up");
        }
      }
      double ms[5];
      for (int q = 0; q < 2 && rc == LTO_OK; ++q) rc = sweep();
      for (int q = 0; q < 5 && rc == LTO_OK; ++q) {
        float m = 0.0f;
        if (hipEventRecord(e0, st) != hipSuccess) { rc = set_err(c, LTO_EHIP, "hipEventRecord"); break; }
        rc = sweep();
        if (rc == LTO_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&m, e0, e1) != hipSuccess))
          rc = set_err(c, LTO_EHIP, "calibration timing");
        ms[q] = m;
      }
      call.idle = rc == LTO_OK;                     // e1 was waited for behind the last sweep
      if (rc == LTO_OK) {
        std::sort(ms, ms + 5);
        if (f == 5) measured_lane = ms[2] * 1e3 * (64.0 / integ.steps);
        else measured[di][f] = ms[2] * 1e3 * (64.0 / integ.steps);
      }
    }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (rc != LTO_OK) return rc;
  for (int di = 0; di < 2; ++di)
    for (int f = 0; f < 5; ++f)
      if (!(measured[di][f] > 0.0)) return set_err(c, LTO_EHIP, "calibration returned a non-positive time");
  if (!(measured_lane > 0.0)) return set_err(c, LTO_EHIP, "calibration returned a non-positive time");
  std::memcpy(c->round_cost, measured, sizeof measured);
  c->lane_round_us = measured_lane;
  c->calibrated = true;
  return LTO_OK;
}

double lto_kernel_lane_round_us(const lto_ctx* c) { return c ? c->lane_round_us : 0.0; }

int lto_kernel_round_costs(const lto_ctx* c, int ndim, double* us_per_round, int* calibrated) {
  if (!c || !us_per_round) return LTO_ENULL;
  if (ndim != 12 && ndim != 14) return LTO_EINVAL;
  for (int f = 0; f < 5; ++f) us_per_round[f] = c->round_cost[ndim == 14 ? 1 : 0][f];
  if (ndim == 14) us_per_round[2] = us_per_round[3] = -1.0;           // not candidates
  if (calibrated) *calibrated = c->calibrated ? 1 : 0;
  return LTO_OK;
}

}  // extern "C"
