// lto_util.hip -- the small device-resident entry points: axpy, trial points, line-search pick, scalars to the host, lane order and
// step statistics read back, AoS <-> SoA, defect norms.
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>

#include "lto_host.hpp"

// Scalars of the Newton loop to the host: a[0..na) then b[0..nb) into out.  With the mapped landing block one small kernel
// writes them and the host polls the sequence word (a few microseconds after the kernel); a stream that has drained without
// the word arriving is an error.  Without the block: two copies and a stream synchronisation (about 30 us).
bool report_reserve(lto_ctx* c, size_t doubles) {
  if (c->rep_host && c->rep_doubles >= doubles) return true;
  if (c->rep_host) { (void)hipDeviceSynchronize(); (void)hipHostFree(c->rep_host); c->rep_host = nullptr; c->rep_doubles = 0; }   // (any stream may have carried the last report)
  void* hp = nullptr; void* dp = nullptr;
  const size_t want = doubles + 64;
  if (hipHostMalloc(&hp, sizeof(double) * (want + 1), hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
    (void)hipGetLastError();
    if (hp) (void)hipHostFree(hp);
    return false;
  }
  std::memset(hp, 0, sizeof(double) * (want + 1));
  c->rep_host = (double*)hp; c->rep_dev = (double*)dp; c->rep_doubles = want; c->rep_seq = 0;
  return true;
}
int read_scalars(lto_ctx* c, hipStream_t st, const double* a, int na, const double* b, int nb, double* out) {
  hipError_t e;
  if (c->rep_host && c->rep_doubles >= (size_t)(na + nb)) {
    const long long seq = ++c->rep_seq;
    e = launch_iter_report(a, na, b, nb, c->rep_dev + 1, (long long*)c->rep_dev, seq, st);
    if (e != hipSuccess) return set_err(c, LTO_EHIP, "report", e);
    volatile long long* w = (volatile long long*)c->rep_host;
    // busy poll (a look at the stream every 16 k reads) for the first 5 ms -- the usual case is microseconds behind the last kernel of
    // an iteration the host enqueued in a fraction of its run time -- then a look and a short sleep per read, so that a sweep that
    // takes seconds does not hold a core at 100 %.  (Counting reads instead of time sent a 0.45 ms iteration into the sleeps: a
    // cached read takes a nanosecond.)
    const auto t_start = std::chrono::steady_clock::now();
    bool slow = false;
    for (unsigned long spin = 1;; ++spin) {
      if (*w == seq) break;
      if (slow || (spin & 0x3fff) == 0) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipErrorNotReady) {
          if (slow) std::this_thread::sleep_for(std::chrono::microseconds(20));
          else slow = std::chrono::steady_clock::now() - t_start > std::chrono::milliseconds(5);
          continue;
        }
        if (q == hipSuccess && *w == seq) break;
        return set_err(c, LTO_EHIP, "report: the stream drained without the iteration's scalars", q);
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    std::memcpy(out, c->rep_host + 1, sizeof(double) * (size_t)(na + nb));
    return LTO_OK;
  }
  e = hipMemcpyAsync(out, a, sizeof(double) * (size_t)na, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nb > 0) e = hipMemcpyAsync(out + na, b, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? LTO_OK : set_err(c, LTO_EHIP, "norm", e);
}

extern "C" {

int lto_axpy_dev(lto_ctx* c, void* stream, const double* x, const double* d, double alpha, double* y, long count) {
  if (!c) return LTO_ENULL;
  if (!x || !d || !y) return set_err(c, LTO_ENULL, "x, d or y is NULL");
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = launch_axpy(x, d, alpha, y, count, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_axpy", e);
  return LTO_OK;
}

int lto_trial_points_dev(lto_ctx* c, void* stream, const double* X, const double* delta, long ld, int ndim, int n_nodes, int n_batch,
                         int n_alpha, const double* alphas, double* Xt, long ldt) {
  if (!c) return LTO_ENULL;
  if (!X || !delta || !alphas || !Xt) return set_err(c, LTO_ENULL, "X, delta, alphas or Xt is NULL");
  if (ndim < 1 || n_nodes < 1 || n_batch < 1 || n_alpha < 1) return set_err(c, LTO_EINVAL, "ndim, n_nodes, n_batch and n_alpha must be positive");
  if (ld < (long)n_nodes * n_batch || ldt < (long)n_nodes * n_batch * n_alpha) return set_err(c, LTO_EINVAL, "leading dimension too small");
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = launch_trial_points(X, delta, ld, ndim, n_nodes, n_batch, n_alpha, alphas, Xt, ldt, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_trial_points", e);
  return LTO_OK;
}

int lto_line_search_pick_dev(lto_ctx* c, void* stream, const double* sumsq, const double* maxabs, const double* alphas, int n_alpha,
                             const double* trial_defect, long ldt, int ndim, int seg_per_traj, int n_batch, double* step,
                             double* maxabs_out, double* defect, long ldd) {
  if (!c) return LTO_ENULL;
  if (!sumsq || !alphas || !step) return set_err(c, LTO_ENULL, "sumsq, alphas or step is NULL");
  if ((maxabs == nullptr) != (maxabs_out == nullptr) || (trial_defect == nullptr) != (defect == nullptr))
    return set_err(c, LTO_ENULL, "maxabs / maxabs_out and trial_defect / defect come in pairs");
  if (n_alpha < 1 || n_batch < 1 || ndim < 1 || seg_per_traj < 1) return set_err(c, LTO_EINVAL, "n_alpha, n_batch, ndim and seg_per_traj must be positive");
  if (defect && (ldt < (long)seg_per_traj * n_batch * n_alpha || ldd < (long)seg_per_traj * n_batch)) return set_err(c, LTO_EINVAL, "leading dimension too small");
  int rc = bind_device(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = defect ? launch_take_trial(trial_defect, ldt, sumsq, nullptr, nullptr, n_alpha, seg_per_traj, ndim, n_batch, defect, ldd, alphas,
                                            step, maxabs, maxabs_out, st)
                        : launch_pick_alpha(sumsq, alphas, n_alpha, nullptr, nullptr, step, n_batch, maxabs, maxabs_out, st);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "line search pick", e);
  return LTO_OK;
}

int lto_read_scalars_dev(lto_ctx* c, void* stream, const double* a, int na, const double* b, int nb, double* out) {
  if (!c) return LTO_ENULL;
  if (!a || !out || (nb > 0 && !b)) return set_err(c, LTO_ENULL, "a, b or out is NULL");
  if (na < 1 || nb < 0 || (long)na + nb > (1L << 20)) return set_err(c, LTO_EINVAL, "need 1 <= na, 0 <= nb, na + nb <= 2^20");
  int rc = bind_device(c);
  if (rc) return rc;
  (void)report_reserve(c, (size_t)na + nb);
  return read_scalars(c, (hipStream_t)stream, a, na, b, nb, out);
}

/* ------------------------------------------------------------------------------ lane order and step statistics, read back */
// The launchers lto_indirect_plan_rebalance runs, on step counts of the caller's choosing.  The workspace is the context's arena,
// which the next host-pointer call lays out afresh: the stream is drained before the call returns.
int lto_segment_order_dev(lto_ctx* c, int kind, int weave, int n_segments, const int* accepted_dev, const int* rejected_dev,
                          int* order_dev, void* stream) {
  if (!c) return LTO_ENULL;
  if (!accepted_dev || !rejected_dev || !order_dev) return set_err(c, LTO_ENULL, "accepted_dev, rejected_dev or order_dev is NULL");
  if (kind != 1 && kind != 2) return set_err(c, LTO_EINVAL, "kind must be 1 (global order) or 2 (windowed order)");
  if (weave < 0 || weave > 255) return set_err(c, LTO_EINVAL, "weave must be 0 (choose) .. 255");
  if (n_segments < 1) return set_err(c, LTO_EINVAL, "need n_segments >= 1");
  int rc = bind_device(c);
  if (rc) return rc;
  int* work;
  ArenaLayout scratch;
  scratch.add(order_workspace_ints(n_segments), work);
  rc = scratch.reserve(c);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = kind == 2 ? launch_segment_order_windowed(accepted_dev, rejected_dev, n_segments, weave, work, order_dev, st)
                           : launch_segment_order(accepted_dev, rejected_dev, n_segments, work, order_dev, st);
  const hipError_t q = hipStreamSynchronize(st);
  if (e == hipSuccess) e = q;
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_segment_order", e);
  return LTO_OK;
}

// k_step_stats as a defect sweep launches it: a zeroed device scratch, a page-locked landing block (here the call's own).  The
// kernel's last workgroup must leave the scratch zeroed for the next launch; the call reads it back and says so if it did not.
int lto_step_stats_dev(lto_ctx* c, int n_segments, const int* accepted_dev, const int* rejected_dev, long long* out_host, void* stream) {
  if (!c) return LTO_ENULL;
  if (!accepted_dev || !rejected_dev || !out_host) return set_err(c, LTO_ENULL, "accepted_dev, rejected_dev or out_host is NULL");
  if (n_segments < 1) return set_err(c, LTO_EINVAL, "need n_segments >= 1");
  int rc = bind_device(c);
  if (rc) return rc;
  unsigned long long* acc;
  ArenaLayout scratch;
  scratch.add(4, acc);
  rc = scratch.reserve(c);
  if (rc) return rc;
  void* hp = nullptr; void* dp = nullptr;
  if (hipHostMalloc(&hp, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
    const hipError_t e = hipGetLastError();
    if (hp) (void)hipHostFree(hp);
    return set_err(c, LTO_EHIP, "page-locked block of the step statistics", e);
  }
  long long* land = (long long*)hp;
  for (int k = 0; k < 8; ++k) land[k] = -1;                 // a word the kernel does not write shows
  unsigned long long left[3] = {1, 1, 1};
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(acc, 0, sizeof(unsigned long long) * 4, st);
  if (e == hipSuccess) e = launch_step_stats(accepted_dev, rejected_dev, n_segments, acc, (long long*)dp, st);
  if (e == hipSuccess) e = hipMemcpyAsync(left, acc, sizeof left, hipMemcpyDeviceToHost, st);
  const hipError_t q = hipStreamSynchronize(st);
  if (e == hipSuccess) e = q;
  const long long got[3] = {land[0], land[1], land[2]};
  (void)hipHostFree(hp);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_step_stats", e);
  if (left[0] || left[1] || left[2]) return set_err(c, LTO_EHIP, "k_step_stats left its device scratch non-zero: the next launch would add to it");
  for (int k = 0; k < 3; ++k) out_host[k] = got[k];
  return LTO_OK;
}

/* ------------------------------------------------------------------------------ utilities */
int lto_pack_soa_dev(lto_ctx* c, void* stream, const double* aos, int ndim, long count, double* soa, long ld) {
  if (!c) return LTO_ENULL;
  if (!aos || !soa) return set_err(c, LTO_ENULL, "aos or soa is NULL");
  if (ndim < 1 || count < 0 || ld < count) return set_err(c, LTO_EINVAL, "bad pack dimensions");
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = launch_pack_soa(aos, ndim, count, soa, ld, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_pack_soa", e);
  return LTO_OK;
}

int lto_unpack_soa_dev(lto_ctx* c, void* stream, const double* soa, long ld, int ndim, long count, double* aos) {
  if (!c) return LTO_ENULL;
  if (!aos || !soa) return set_err(c, LTO_ENULL, "aos or soa is NULL");
  if (ndim < 1 || count < 0 || ld < count) return set_err(c, LTO_EINVAL, "bad unpack dimensions");
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = launch_unpack_soa(soa, ld, ndim, count, aos, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_unpack_soa", e);
  return LTO_OK;
}

int lto_defect_norms_dev(lto_ctx* c, void* stream, const double* defect, long ldd, int ndim, int seg_per_traj,
                         int n_batch, double* sumsq, double* maxabs) {
  if (!c) return LTO_ENULL;
  if (!defect) return set_err(c, LTO_ENULL, "defect is NULL");
  if (ndim < 1 || seg_per_traj < 1 || n_batch < 1 || ldd < (long)seg_per_traj * n_batch)
    return set_err(c, LTO_EINVAL, "bad norm dimensions");
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = launch_defect_norms(defect, ldd, ndim, seg_per_traj, n_batch, sumsq, maxabs,
                                     (hipStream_t)stream);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "launch_defect_norms", e);
  return LTO_OK;
}

}  // extern "C"
