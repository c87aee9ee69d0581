// lto_host.hpp -- the one internal header of the host units (lto_*.hip but lto_group.hip and lto_comm.hip, which reach the context
// through include/lto.h alone): the context and the two plan types, the small classes every host-pointer call is built from, and one
// declaration of every helper that one unit defines and another calls.  Nothing here is part of the ABI.
// No container that throws here either (hostbuf.hpp has the ones that do not).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>

#include "../../include/lto.h"
#include "kernels.hpp"
#include "hostbuf.hpp"

using namespace lto;

struct lto_ctx {
  int device;
  int cu_count;    // compute units of the device: the kernel choice works in rounds of workgroups per CU
  hipStream_t stream;
  bool timing;
  hipEvent_t ev0, ev1;
  bool ev_valid;
  // grow-only device arena for the host-pointer API
  char* arena;
  size_t arena_bytes;
  // small cache of device blocks for plan-owned buffers: the host-pointer API builds a plan per call, and a
  // hipMalloc/hipFree pair costs more than a 29-segment sweep
  struct { void* ptr; size_t bytes; } pool[8];
  // lane order of the last large adaptive sweep made through the host-pointer API (which builds a plan per call):
  // consecutive Newton iterations sweep the same problem, so the previous call's step counts balance this one.
  // A stale order is still a valid permutation -- it can only cost speed, never correctness.
  // One slot per kind of order (round 6; advisor finding: defect sweeps want the windowed order, STM sweeps / Newton steps the global
  // one, and a loop that alternates defectCalc and jacobianCalc at the same size evicted the other call's order every time).
  int* order_cache[3];   // [kind]: [order_S + workspace] (kernels.hpp order_bytes); kind 1 global, 2 windowed (slot 0 unused)
  long order_S[3];
  int order_ndim[3];
  // plans of the host-pointer API, kept between calls (a Newton iteration calls with the same shapes and parameters
  // every time: no parameter upload, no device allocation per call); owned by the context
  struct HostPlan {
    lto_indirect_plan* plan;
    int ndim, n_nodes, n_batch, n_prm;
    lto_integrator integ;
    lto_params* prm;       // [n_prm] copy of the caller's parameters (the key)
    unsigned long stamp;   // last use
  } host_plans[4];
  unsigned long stamp;
  // lifetime: plans handed to the caller keep the context alive.  lto_destroy with such plans outstanding (a garbage
  // collector runs finalizers in any order) only marks the context; the last lto_*_plan_destroy frees it.
  int live_plans;
  bool closing;
  bool free_claimed = false;   // somebody is freeing this context (ctx_release)
  // page-locked blocks handed out by lto_host_alloc.  The GPU addresses them directly, so the host-pointer API reads and
  // writes a caller's buffer that lies inside one of them in place: the AoS <-> SoA kernels are the transfer, and no
  // copy-engine operation (about 10 us of latency each) is queued.
  // A block keeps its context alive the way a plan does (lto_destroy defers while any is outstanding); `dev` is null for a
  // block the device cannot address directly (still page-locked: the copy engine moves it).  The list has its own lock:
  // a garbage collector may free a block from another thread while a sweep looks one up.
  struct Pinned { char* host; char* dev; size_t bytes; };
  lto::HostList<Pinned> pinned;
  std::mutex pinned_mu;
  double last_call_ms;     // wall time of the last host-pointer call, entry to return (lto_last_call_ms)
  int last_call_order;     // lane order the last host-pointer indirect call swept with: 0 natural, 1 global, 2 windowed (lto_last_call_order)
  // landing block of the Newton loop's per-iteration scalars (lto_indirect_solve_batch): page-locked, mapped, written by
  // k_iter_report; word 0 is the sequence number the host polls, the values follow.  Grow-only; absent = copy + synchronise.
  // AUTO's cost table: microseconds per ROUND of each RK4 STM family at 64 steps, [ndim == 14][family] with family 0 = eight-wave
  // pipeline (rounds of 16 x CUs segments), 1 = 48-segment pipeline (48 x CUs), 2 = per-lane with three columns (64 x CUs; 12-dim
  // only), 3 = 44-segment form of the large-batch pipeline (44 x CUs; 12-dim only), 4 = 32-segment / twelve-wave pipeline (32 x CUs).
  // Defaults: MI355X, profiles/r04z; lto_calibrate_kernels replaces them with this device's own.
  double round_cost[2][5];
  double lane_round_us;    // the whole-segment lanes (kernels_indirect_lane.hip, 12-dim): us per round of 256 x CUs segments at 64 steps
  bool calibrated;
  double* rep_host;
  double* rep_dev;
  size_t rep_doubles;
  long long rep_seq;
  char err[512];
};

struct lto_indirect_plan {
  lto_ctx* ctx;
  int ndim, n_nodes, n_batch, S;
  int pm;           // bit mask of the PMode classes present in the batch
  int n_prm;        // 1 or n_batch
  lto_integrator integ;
  TrajParams* d_tp;
  int* d_nacc;
  int* d_nrej;
  int* d_order;     // [S] lane -> segment map of adaptive sweeps + LTO_ORDER_BINS ints of sort workspace (lazily allocated)
  int use_order;
  int order_kind;      // what d_order holds: 1 = the global order (record staging), 2 = the windowed order (kernels.hpp LTO_ORDER_WINDOW)
  int order_borrowed;  // d_order belongs to the context's cache
  int swept;           // an adaptive sweep has filled the step counters
  int cols_per_lane;
  int kernel;       // LTO_KERNEL_*
  int last_kernel;  // family the last STM sweep ran (AUTO resolved)
  int p48_form;     // large-batch pipeline, 12-dim: 0 = the form with the cheaper rounds, 44 / 48 = that form (calibration)
  double* d_bvp;    // workspace of the device Newton solve (lazily allocated)
  size_t bvp_bytes;
  int bvp_variant;  // -1 none, 0 square system, 1 adjoints-only least squares: what the stored factorisation is
  // warm start of the adaptive controllers (lto_indirect_plan_set_warm_start): first accepted step size of every segment in the
  // last STM sweep / defect-only sweep (they control different error norms, hence two arrays; lazily allocated)
  int warm_start;
  int defect_lanes;         // lanes per segment of the defect-only sweep with the reference's setting: 0 = choose, 1, 2, 4
  double* d_hfirst[2];      // [0] STM sweeps, [1] defect-only sweeps
  int hfirst_valid[2];
  // record staging of rebalanced sweeps (kernels.hpp, IndirectArgs::Xa / Da / Pa): allocated with the lane order
  // trial-step statistics of the last defect-only sweep (k_step_stats): [sum, max, S] in page-locked host memory the kernel writes
  long long* h_stats;       // host view (nullptr: not available)
  long long* h_stats_dev;   // device view of the same block
  unsigned long long* d_stats_acc;   // [3] device scratch
  int stats_age;            // qualifying sweeps so far
  hipEvent_t stats_ev;      // recorded behind every k_step_stats launch
  int stats_pending;        // a k_step_stats launch has not been consumed yet
  int stats_lanes;          // the statistics' verdict, latched when they are consumed: 0 none (size thresholds), 1 or 2 lanes per segment
  double* d_xa;             // [n_nodes n_batch][NODE_REC]
  double* d_da;             // [S][12]
  double* d_pa;             // [S][144]: only for plans that run STM sweeps (stage_alloc's need_phi)
  int stm_swept;            // an STM sweep has run on this plan
  int stage_failed;         // an allocation of record staging failed: the sweeps gather from the caller's arrays (lto_indirect_plan_staging)
  int out_blocks;           // LTO_LAYOUT_BLOCKS: Phi [S][144] and defect [S][12] per-segment blocks instead of struct-of-arrays (lto_indirect_plan_set_output_layout)
  void* d_events;           // per-segment records of lto_indirect_events_dev (kernels.hpp events_record_bytes), allocated at its first call
};

struct lto_direct_plan {
  lto_ctx* ctx;
  int nstate, n_nodes, n_batch, S, nsteps;
  lto_direct_params prm;
  int kernel;       // LTO_KERNEL_*
  void* qp_ws;      // workspace of the QP step (kernels_direct_qp.hip), allocated at the plan's first step
  int qp_ws_nr;     // right-hand sides the workspace is sized for: 1 (frozen ends) or 3 (free ends, grown at the first free step)
  double* qp_singular_out;   // lto_direct_solve_batch: where the QP step also reports singular systems (device, [n_batch])
  int qp_last_nr;   // right-hand sides of the last QP step on this plan (0: none yet): the workspace holds that variant's layout
  void* cs_acc;     // reduction scratch of the costates kernel (lto_direct_costates.hip), allocated at its first call
};

#define LTO_HIP(c, call)                                              \
  do {                                                                \
    hipError_t e_ = (call);                                           \
    if (e_ != hipSuccess) return set_err((c), LTO_EHIP, #call, e_);   \
  } while (0)

// the two orbit tables on the device with the natural-spline second derivatives (a tridiagonal solve on the host, once per call)
struct DevOrbits {
  EndOrbitsDev o;
  double* buf = nullptr;
  ~DevOrbits() { if (buf) (void)hipFree(buf); }
};

// Helpers shared between the host units, by the unit that defines them.  They were file-static while the host side was one unit; all
// of them, and ArenaLayout, have hidden visibility: the library exports include/lto.h and nothing of this.
#pragma GCC visibility push(hidden)

// lto_ctx.hip
int set_err(lto_ctx* c, int code, const char* what, hipError_t e = hipSuccess);
int bind_device(lto_ctx* c);
int arena_reserve(lto_ctx* c, size_t bytes);
hipError_t pool_alloc(lto_ctx* c, void** out, size_t bytes);
void pool_free(lto_ctx* c, void* ptr, size_t bytes);
void timing_begin(lto_ctx* c, hipStream_t st);
void timing_end(lto_ctx* c, hipStream_t st);
hipError_t stream_wait(hipStream_t st);
enum CtxOwner { OWNER_HANDLE, OWNER_PLAN, OWNER_BLOCK };
void ctx_plan_added(lto_ctx* c);
bool ctx_release(lto_ctx* c, CtxOwner what);
void ctx_free(lto_ctx* c);
double* pinned_view(lto_ctx* c, const double* host, size_t bytes);

// lto_indirect_plan.hip
int plan_build(lto_ctx* c, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm, const lto_integrator* integ,
               lto_indirect_plan** out);
void plan_free(lto_indirect_plan* p);
int fill_indirect_args(lto_indirect_plan* p, const double* X, long ldx, const double* t, int n_tgrids, IndirectArgs* a);
bool host_order_wanted(const lto_indirect_plan* p, bool stm);
void host_order_adopt(lto_ctx* c, lto_indirect_plan* p, bool stm);
void host_order_refresh(lto_ctx* c, lto_indirect_plan* p, bool stm, hipStream_t st);

// lto_direct_plan.hip
int direct_plan_build(lto_ctx* c, int nstate, int n_nodes, int n_batch, int nsteps, const lto_direct_params* prm, lto_direct_plan** out);
void direct_plan_free(lto_direct_plan* p);
int direct_qp_workspace(lto_direct_plan* p, int nr);
int direct_defect_launch(lto_direct_plan* p, void* stream, const double* X, long ldx, const double* U, long ldu, const double* t,
                         int n_tgrids, double* defect, long ldd, double* errors, double* mid, long ldm);
int direct_qp_launch(lto_direct_plan* p, hipStream_t st, int nr, const double* Jac, long ldj, const double* defect, long ldd,
                     const double* X, long ldx, const double* U, long ldu, const double* t, int n_tgrids,
                     const lto_direct_targets* targets, int allow_impulsive, double* dX, double* dU, double* dV, double* cost,
                     const lto_direct_end_model* model = nullptr, const double* beta = nullptr, double* pout = nullptr,
                     const double* dtf = nullptr, const double* tfb = nullptr, const double* tf = nullptr);

// lto_direct_costates.hip
int direct_costates_launch(lto_direct_plan* p, hipStream_t st, const double* Jac, long ldj, double* Lambda, long ldl, double* mult,
                           long ldm, double* kkt_res, const double* X = nullptr, long ldx = 0, double* XC = nullptr, long ldxc = 0);

// lto_util.hip
bool report_reserve(lto_ctx* c, size_t doubles);
int read_scalars(lto_ctx* c, hipStream_t st, const double* a, int na, const double* b, int nb, double* out);

// lto_host_sweeps.hip
hipError_t stage_in(lto_ctx* c, const double* host, int ndim, long count, double* d_aos, double* d_soa, long ld, hipStream_t st);
hipError_t stage_out(lto_ctx* c, const double* d_soa, long ld, int ndim, long count, double* d_aos, double* host, hipStream_t st);
hipError_t vec_in(lto_ctx* c, const double* host, long count, double* dev, hipStream_t st);
int host_plan_acquire(lto_ctx* c, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm, const lto_integrator* integ,
                      lto_indirect_plan** out);
void linrange(double t0, double te, int m, double* out);
void segment_samples(const double* g, int nn, const double* td, int m, int* first, int base);

// lto_indirect_solve.hip
int indirect_solve_impl(lto_ctx* c, int ndim, int n_nodes, int n_batch, const double* XC_in, const double* d_Xin, const double* t,
                        int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, int flag_adjointsOnly, int maxIter,
                        double* XC_out, double* d_Xout, double* defect, int* status_flag, int* iterations, double* history);

// lto_direct_solve.hip
int orbits_upload(lto_ctx* c, const lto_direct_orbits* ob, DevOrbits& d, hipStream_t st);

// lto_halo.hip
int halo_integrator_check(lto_ctx* c, const lto_integrator* integ, const char* unsupported, const char* steps);

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// The scratch of one host-pointer call: every buffer is declared once with its element count (add); the layout is then
// materialised in the order of declaration, every buffer on a 256-B boundary, and the pointers are filled in.  reserve() places it
// in the context's arena, grown to the exact sum of the aligned sizes.  reserve_block() places it in one hipMalloc block of that
// sum and hands the block to `slot` (a HostCall's block[k], which frees it): for the calls that run indirect_solve_impl in their
// middle, which lays the arena out afresh.  A buffer of zero elements takes no bytes; its pointer is valid (the next buffer's
// start, or the end) and nothing may be read through it.  (reserve_block of a layout with no bytes at all gets no block from
// hipMalloc: every pointer is then null.)
class ArenaLayout {
  static constexpr int kMax = 24;
  struct Slot { void* ptr; void (*set)(void*, char*); size_t bytes; };
  Slot slot_[kMax];
  int n_ = 0;
  template <class T> void add1(T*& p, size_t count) {
    if (n_ < kMax) slot_[n_] = {&p, [](void* q, char* at) { *(T**)q = (T*)at; }, al256(sizeof(T) * count)};
    ++n_;
  }
  size_t total() const {
    size_t sum = 0;
    for (int k = 0; k < n_; ++k) sum += slot_[k].bytes;
    return sum;
  }
  void place(char* base) {
    size_t off = 0;
    for (int k = 0; k < n_; ++k) { slot_[k].set(slot_[k].ptr, base + off); off += slot_[k].bytes; }
  }
 public:
  template <class... T> void add(size_t count, T*&... p) { (add1(p, count), ...); }   // buffers of `count` elements each
  int reserve(lto_ctx* c) {
    if (n_ > kMax) return set_err(c, LTO_EINVAL, "internal: too many scratch buffers");
    const int rc = arena_reserve(c, total());
    if (rc) return rc;
    place(c->arena);
    return LTO_OK;
  }
  int reserve_block(lto_ctx* c, void*& slot, const char* who) {   // `who`: the error text of a failed allocation
    if (n_ > kMax) return set_err(c, LTO_EINVAL, "internal: too many scratch buffers");
    const hipError_t e = hipMalloc(&slot, total());
    if (e != hipSuccess) { slot = nullptr; return set_err(c, LTO_EHIP, who, e); }
    place((char*)slot);
    return LTO_OK;
  }
};

#pragma GCC visibility pop

// CallTimer, HostCall and NewtonBatch are outside the hidden block by an accident this cut preserves: as one unit they had default
// visibility, and the weak copies of their inline members are in the library's dynamic list.  A follow-up should hide them.

// entry-to-return wall time of a host-pointer call, kept in the context
struct CallTimer {
  lto_ctx* c;
  std::chrono::steady_clock::time_point t0;
  explicit CallTimer(lto_ctx* ctx) : c(ctx), t0(std::chrono::steady_clock::now()) {}
  ~CallTimer() { if (c) c->last_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// What a host-pointer call owns on the context's stream: the short-lived plans it builds ([0] the trajectories', [1] the line
// search's) and the device blocks it allocates.  At scope exit the stream is drained first -- unless the call has waited for it
// since its last launch (`idle`, set by wait()) -- and only then is anything freed: a plan's blocks go back to the context's block
// cache (pool_free) and may be handed to the next plan at once.  Host buffers the stream copies from or into are declared ahead of
// it, so that they outlive the drain.  Plans of the context (host_plan_acquire, lto_*_plan_create) are never given to it.
struct HostCall {
  hipStream_t st;
  bool idle = false;
  lto_indirect_plan* plan[2] = {};
  lto_direct_plan* dplan[2] = {};
  void* block[2] = {};
  explicit HostCall(lto_ctx* c) : st(c->stream) {}
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  hipError_t wait() { const hipError_t e = stream_wait(st); idle = e == hipSuccess; return e; }
  ~HostCall() {
    if (!idle) (void)hipStreamSynchronize(st);
    for (int k = 1; k >= 0; --k) {
      if (plan[k]) plan_free(plan[k]);
      if (dplan[k]) direct_plan_free(dplan[k]);
      if (block[k]) (void)hipFree(block[k]);
    }
  }
};

/* The per-trajectory bookkeeping of the two batched device Newton loops (lto_indirect_solve_batch, direct_solve_impl): who is still
 * in its loop, the iteration counts, the status flags and the last max |defect| on the host; the trial step lengths
 * LinRange(0.1, 1, n_alpha); and the flags the device reads per trajectory (1 = still in the loop, 1 = line search on), uploaded
 * when they change.  The tolerance, the first line-search iteration and what the counts report stay with each loop. */
struct NewtonBatch {
  const int B;
  lto::HostBuf<char> active;
  lto::HostBuf<int> it, status;
  lto::HostBuf<double> h_er, h_act, h_search, alphas;     // h_act / h_search: the flags last uploaded (-1: none yet)
  NewtonBatch(int n_batch, int n_alpha)
      : B(n_batch), active(B, 1), it(B, 0), status(B, 0), h_er(B, 1.0), h_act(B, -1.0), h_search(B, -1.0), alphas(n_alpha) {
    if (!alphas.ok()) return;
    for (int a = 0; a < n_alpha; ++a) alphas[a] = 0.1 + (1.0 - 0.1) / (n_alpha - 1) * a;
    alphas[n_alpha - 1] = 1.0;
  }
  bool ok() const { return active.ok() && it.ok() && status.ok() && h_er.ok() && h_act.ok() && h_search.ok() && alphas.ok(); }
  bool any_active() const { for (int b = 0; b < B; ++b) if (active[b]) return true; return false; }
  // `while er > tol` and the iteration limit, trajectory by trajectory; false once none is left in its loop.  A trajectory that
  // reaches the limit leaves with status 1 and its count past maxIter.
  bool next(double tol, int maxIter) {
    for (int b = 0; b < B; ++b) {
      if (!active[b]) continue;
      if (!(h_er[b] > tol)) { active[b] = 0; continue; }            // converged, or NaN (the comparison is false)
      if (++it[b] > maxIter) { status[b] = 1; active[b] = 0; }
    }
    return any_active();
  }
  // the device's flags of this iteration, the line search on past iteration `search_after`
  hipError_t upload_flags(int search_after, double* d_act, double* d_search, hipStream_t st) {
    bool changed = false;
    for (int b = 0; b < B; ++b) {
      const double fa = active[b] ? 1.0 : 0.0, fs = (active[b] && it[b] > search_after) ? 1.0 : 0.0;
      if (fa != h_act[b] || fs != h_search[b]) { h_act[b] = fa; h_search[b] = fs; changed = true; }
    }
    if (!changed) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(d_act, h_act.data(), sizeof(double) * B, hipMemcpyHostToDevice, st);
    return e == hipSuccess ? hipMemcpyAsync(d_search, h_search.data(), sizeof(double) * B, hipMemcpyHostToDevice, st) : e;
  }
  void copy_out(int* status_flag, int* iterations) const {
    for (int b = 0; b < B; ++b) { status_flag[b] = status[b]; if (iterations) iterations[b] = it[b]; }
  }
};
