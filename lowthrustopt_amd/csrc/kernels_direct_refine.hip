// kernels_direct_refine.hip -- errors-driven mesh refinement of the direct transcription on the device:
// meshRefine_direct (src/multiShoot_CRTBP_direct.jl:597-680 as drivers.meshRefine_direct re-specifies it), batched, with the
// trajectories resident in HBM between the upload and the download.
//
// A segment's RKF7(8) estimate depends on its own two nodes, controls and times only (direct.jl:77-105), so
//   removal    deleting a node changes ONE estimate, the merged segment's: one workgroup per trajectory keeps the estimates and a
//              doubly linked list of the nodes alive, and loops arg-min -> unlink -> one lane pair re-evaluates the merged segment;
//   insertion  splitting a segment never changes the decision for another: a pass is mark, exclusive scan, scatter (one workgroup
//              per trajectory) and then, over the split segments of the whole batch, mid-point + the estimates of the two halves.
// Every evaluation is direct_segment (direct_segment.hpp), the body of the defect sweep: estimates and mid-points are the sweep's.
//
// Working layout: node-major, as the caller's arrays -- X [B][M][NS], U [B][M][3], t [B][M], E [B][M] (E_i = estimate of segment i)
// with M = max_nodes, twice (a pass scatters from one copy into the other; ctl's `cur` says per trajectory which one is current, so
// a finished trajectory is never touched again).
#include "direct_segment.hpp"

namespace lto {

constexpr int kRefineBlock = 256;

__device__ __forceinline__ DirectConsts refine_consts(const DirectRefineArgs& a) { return DirectConsts{a.MU, a.kk, a.isp_g0, a.TU}; }

// ---- the estimates of the input mesh: lane pair = segment, as k_direct_defect, on the caller's node-major arrays
template <int NS>
__global__ __launch_bounds__(64) void k_refine_errors(const DirectRefineArgs a) {
  const int m = a.n_in - 1;
  const long S = (long)m * a.B;
  const long gid = (long)blockIdx.x * 64 + threadIdx.x;
  const long s = gid >> 1;
  const int dir = (int)(gid & 1);
  const long sc = s < S ? s : S - 1;             // inactive lanes shadow the last segment (keeps the exchange defined)
  const int b = (int)(sc / m), i = (int)(sc - (long)b * m);
  const long node = (long)b * a.n_in + i + dir;
  const double* t = a.t_in + (long)b * a.t_in_stride;
  const double hhalf = 0.5 * (t[i + 1] - t[i]);
  double x[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) x[c] = a.X_in[node * NS + c];
  const double e = refine_segment<NS>(refine_consts(a), dir, x, a.U_in[node * 3], a.U_in[node * 3 + 1], a.U_in[node * 3 + 2], hhalf,
                                      a.half_steps);
  if (s < S && dir == 0) a.E0[(long)b * a.n_in + i] = e;
}

// ---- workgroup helpers
// (value, index) of the minimum with numpy's rules: a NaN wins over every number, and among equals (or NaNs) the first index
struct MinAt { double v; int i; };
__device__ __forceinline__ MinAt min_at(const MinAt p, const MinAt q) {
  const bool pn = p.v != p.v, qn = q.v != q.v;
  bool take_q;
  if (pn || qn) take_q = qn && (!pn || q.i < p.i);
  else take_q = q.v < p.v || (q.v == p.v && q.i < p.i);
  return take_q ? q : p;
}
__device__ __forceinline__ MinAt wave_min_at(MinAt p) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    MinAt q;
    q.v = __shfl_xor(p.v, off, 64);
    q.i = __shfl_xor(p.i, off, 64);
    p = min_at(p, q);
  }
  return p;
}

// inclusive scan of one integer per thread over the workgroup, in thread order: a tile of 64 by six shift-and-add steps in its
// wavefront (the radix-64 tile scan of kernels_remesh.hip; integer counts are exact in any order), the four tile totals through LDS.
// `total` = the workgroup's sum.  sw: four ints of LDS; two barriers.
__device__ __forceinline__ int block_scan_incl(int v, int* sw, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  __syncthreads();                               // the previous call's readers of sw are done
  if (lane == 63) sw[w] = v;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int q = 0; q < kRefineBlock / 64; ++q) { const int tq = sw[q]; if (q < w) before += tq; sum += tq; }
  total = sum;
  return v + before;
}

// ---- removal: one workgroup per trajectory, no host round trip.  est[i] = estimate of the segment whose LEFT node is i (+inf: no
// such segment -- the last node, a removed node); nxt / prv = the neighbours alive (nxt < 0: removed).  Up to kRefineLdsNodes
// nodes these live in LDS, above that in the call's global scratch (this workgroup's slice, between its own barriers).
template <int NS, bool IN_LDS>
__global__ __launch_bounds__(kRefineBlock) void k_refine_remove(const DirectRefineArgs a) {
  __shared__ double s_est[IN_LDS ? kRefineLdsNodes : 1];
  __shared__ int s_nxt[IN_LDS ? kRefineLdsNodes : 1], s_prv[IN_LDS ? kRefineLdsNodes : 1];
  __shared__ double s_wv[kRefineBlock / 64];
  __shared__ int s_wi[kRefineBlock / 64], s_scan[kRefineBlock / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = a.n_in;
  double* est = IN_LDS ? s_est : a.rm_est + (long)b * n0;
  int* nxt = IN_LDS ? s_nxt : a.rm_link + 2L * b * n0;
  int* prv = IN_LDS ? s_prv : nxt + n0;
  const double* Xi = a.X_in + (long)b * n0 * NS;
  const double* Ui = a.U_in + (long)b * n0 * 3;
  const double* ti = a.t_in + (long)b * a.t_in_stride;
  const double inf = __builtin_inf();
  for (int i = tid; i < n0; i += kRefineBlock) {
    est[i] = (i < n0 - 1) ? a.E0[(long)b * n0 + i] : inf;
    nxt[i] = i + 1;
    prv[i] = i - 1;
  }
  __syncthreads();
  const DirectConsts k = refine_consts(a);
  int n = n0, nan_seen = 0;
  for (;;) {
    MinAt best{inf, 0x7fffffff};
    for (int i = tid; i < n0; i += kRefineBlock) best = min_at(best, MinAt{est[i], i});
    best = wave_min_at(best);
    if (lane == 0) { s_wv[wave] = best.v; s_wi[wave] = best.i; }
    __syncthreads();
    best = MinAt{s_wv[0], s_wi[0]};
#pragma unroll
    for (int q = 1; q < kRefineBlock / 64; ++q) best = min_at(best, MinAt{s_wv[q], s_wi[q]});
    if (best.v != best.v) nan_seen = 1;
    if (!(n > 2 && best.v < a.tol_min)) break;   // uniform: every thread read the same four candidates
    // node k of the arg-min segment k goes, and k == 0 becomes 1 (direct.jl:616-618): the left node unless it is the first
    const int del = (prv[best.i] < 0) ? nxt[best.i] : best.i;
    const int p = prv[del], q = nxt[del];
    __syncthreads();                             // everybody has read the links and the candidates
    if (wave == 0) {
      // the merged segment (p, q): every lane pair of this wavefront evaluates it (no divergence), lane 0 stores
      const int dir = lane & 1;
      const int node = dir ? q : p;
      double x[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) x[c] = Xi[(long)node * NS + c];
      const double hhalf = 0.5 * (ti[q] - ti[p]);
      const double e = refine_segment<NS>(k, dir, x, Ui[node * 3L], Ui[node * 3L + 1], Ui[node * 3L + 2], hhalf, a.half_steps);
      if (lane == 0) {
        est[p] = e;
        est[del] = inf;
        nxt[p] = q;
        prv[q] = p;
        nxt[del] = -1;
      }
    }
    --n;
    __syncthreads();
  }
  // the nodes alive, compacted in order into copy 0 of the working arrays
  double* Xw = a.X[0] + (long)b * a.M * NS;
  double* Uw = a.U[0] + (long)b * a.M * 3;
  double* tw = a.t[0] + (long)b * a.M;
  double* Ew = a.E[0] + (long)b * a.M;
  int carry = 0;
  for (int base = 0; base < n0; base += kRefineBlock) {
    const int i = base + tid;
    const int alive = (i < n0 && nxt[i] >= 0) ? 1 : 0;
    int total;
    const int pos = carry + block_scan_incl(alive, s_scan, total) - alive;
    carry += total;
    if (alive) {
#pragma unroll
      for (int c = 0; c < NS; ++c) Xw[(long)pos * NS + c] = Xi[(long)i * NS + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) Uw[pos * 3L + c] = Ui[i * 3L + c];
      tw[pos] = ti[i];
      if (i < n0 - 1) Ew[pos] = est[i];
    }
  }
  if (tid == 0) {
    a.ctl[RC_N * a.B + b] = n;
    a.ctl[RC_CUR * a.B + b] = 0;
    a.ctl[RC_ACTIVE * a.B + b] = nan_seen ? 0 : 1;
    a.ctl[RC_STATUS * a.B + b] = nan_seen ? 2 : 0;
    a.ctl[RC_NSPLIT * a.B + b] = 0;
    a.ctl[RC_REMOVED * a.B + b] = n0 - n;
    a.ctl[RC_PASSES * a.B + b] = 0;
  }
}

// ---- insertion, first half of a pass: one workgroup per trajectory still in its loop.  `while max(errors) > tol_max and n < max_nodes`;
// in index order every segment with errors > tol_max is split, at most max_nodes - n of them.  The old nodes (and the estimates of
// the segments that stay) are scattered into the other copy, the split segments are listed in order for k_refine_insert.
template <int NS>
__global__ __launch_bounds__(kRefineBlock) void k_refine_split(const DirectRefineArgs a) {
  __shared__ int s_scan[kRefineBlock / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!a.ctl[RC_ACTIVE * a.B + b]) {             // frozen: nothing of it is read or written again
    if (tid == 0) a.ctl[RC_NSPLIT * a.B + b] = 0;
    return;
  }
  const int n = a.ctl[RC_N * a.B + b], cur = a.ctl[RC_CUR * a.B + b], m = n - 1, room = a.M - n;
  const double* Eo = a.E[cur] + (long)b * a.M;
  int nan_l = 0, mark_l = 0;
  for (int i = tid; i < m; i += kRefineBlock) {
    const double e = Eo[i];
    nan_l |= (e != e);
    mark_l |= (e > a.tol_max);
  }
  const int any_nan = __syncthreads_or(nan_l), any_mark = __syncthreads_or(mark_l);
  if (any_nan || !any_mark || room <= 0) {       // uniform
    if (tid == 0) {
      a.ctl[RC_ACTIVE * a.B + b] = 0;
      a.ctl[RC_STATUS * a.B + b] = any_nan ? 2 : (any_mark ? 1 : 0);
      a.ctl[RC_NSPLIT * a.B + b] = 0;
    }
    return;
  }
  const double* Xo = a.X[cur] + (long)b * a.M * NS;
  const double* Uo = a.U[cur] + (long)b * a.M * 3;
  const double* to = a.t[cur] + (long)b * a.M;
  double* Xn = a.X[cur ^ 1] + (long)b * a.M * NS;
  double* Un = a.U[cur ^ 1] + (long)b * a.M * 3;
  double* tn = a.t[cur ^ 1] + (long)b * a.M;
  double* En = a.E[cur ^ 1] + (long)b * a.M;
  int* list = a.list + (long)b * a.M;
  int carry = 0;
  for (int base = 0; base < n; base += kRefineBlock) {
    const int i = base + tid;
    const int mark = (i < m && Eo[i] > a.tol_max) ? 1 : 0;
    int total;
    const int rank = carry + block_scan_incl(mark, s_scan, total) - mark;   // marked segments before i
    carry += total;
    if (i < n) {
      const int before = rank < room ? rank : room;                         // of them split: the first `room`
      const int split = mark && rank < room;
      const long slot = (long)i + before;
#pragma unroll
      for (int c = 0; c < NS; ++c) Xn[slot * NS + c] = Xo[(long)i * NS + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) Un[slot * 3 + c] = Uo[i * 3L + c];
      tn[slot] = to[i];
      if (split) list[rank] = i;
      else if (i < m) En[slot] = Eo[i];
    }
  }
  if (tid == 0) {
    const int ns = carry < room ? carry : room;
    a.ctl[RC_NSPLIT * a.B + b] = ns;
    a.ctl[RC_N * a.B + b] = n + ns;
    a.ctl[RC_CUR * a.B + b] = cur ^ 1;
    a.ctl[RC_PASSES * a.B + b] += 1;
  }
}

// ---- insertion, second half: lane pair = split segment r of trajectory blockIdx.y (old segment i = list[r]; its nodes sit at slots
// i + r and i + r + 2 of the new mesh, the new node between them).  Three evaluations: the old segment with one RKF7(8) step per
// half-arc -- lto_direct_midpoints at nsteps = 2, the reference's ode7 (direct.jl:651-656) -- for the new state, then the two halves
// with the call's nsteps for their estimates.
template <int NS>
__global__ __launch_bounds__(64) void k_refine_insert(const DirectRefineArgs a) {
  const int b = blockIdx.y;
  const int ns = a.ctl[RC_NSPLIT * a.B + b];
  if ((int)blockIdx.x * 32 >= ns) return;        // wave-uniform (also every frozen trajectory: ns = 0)
  const int lane = threadIdx.x, dir = lane & 1;
  const int r_raw = blockIdx.x * 32 + (lane >> 1);
  const int r = r_raw < ns ? r_raw : ns - 1;     // shadow pairs repeat the last split, store nothing
  const int cur = a.ctl[RC_CUR * a.B + b];       // k_refine_split has switched: cur = the new mesh
  const int i = a.list[(long)b * a.M + r];
  const double* Xo = a.X[cur ^ 1] + (long)b * a.M * NS;
  const double* Uo = a.U[cur ^ 1] + (long)b * a.M * 3;
  const double* to = a.t[cur ^ 1] + (long)b * a.M;
  double* Xn = a.X[cur] + (long)b * a.M * NS;
  double* Un = a.U[cur] + (long)b * a.M * 3;
  double* tn = a.t[cur] + (long)b * a.M;
  double* En = a.E[cur] + (long)b * a.M;
  const DirectConsts k = refine_consts(a);
  const long slot = (long)i + r;
  const double t0 = to[i], t1 = to[i + 1];
  const double tm = t0 + (t1 - t0) / 2;          // direct.jl:644, in that order
  double um[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) um[c] = (Uo[i * 3L + c] + Uo[(i + 1) * 3L + c]) / 2;   // :659
  const long mine = (long)i + dir;               // this lane's end of the old segment
  double x[NS], xm[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) x[c] = Xo[mine * NS + c];
  (void)refine_segment<NS>(k, dir, x, Uo[mine * 3], Uo[mine * 3 + 1], Uo[mine * 3 + 2], 0.5 * (t1 - t0), 1);
#pragma unroll
  for (int c = 0; c < NS; ++c) { const double o = xchg1(x[c]); xm[c] = dir ? o : x[c]; }   // the forward lane's end state
  // left half (node i, new node), then right half (new node, node i + 1); the new mesh's times as the sweep reads them
  double e_half[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bool at_new = (dir == 1 - h);          // which of the pair starts from the new node
    double xs[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) xs[c] = at_new ? xm[c] : Xo[mine * NS + c];
    const double ux = at_new ? um[0] : Uo[mine * 3], uy = at_new ? um[1] : Uo[mine * 3 + 1], uz = at_new ? um[2] : Uo[mine * 3 + 2];
    const double hhalf = h ? 0.5 * (t1 - tm) : 0.5 * (tm - t0);
    e_half[h] = refine_segment<NS>(k, dir, xs, ux, uy, uz, hhalf, a.half_steps);
  }
  if (r_raw < ns && dir == 0) {
#pragma unroll
    for (int c = 0; c < NS; ++c) Xn[(slot + 1) * NS + c] = xm[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) Un[(slot + 1) * 3 + c] = um[c];
    tn[slot + 1] = tm;
    En[slot] = e_half[0];
    En[slot + 1] = e_half[1];
  }
}

// ---- the outputs: the current copy of every trajectory, NaN from its node count on
template <int NS>
__global__ __launch_bounds__(kRefineBlock) void k_refine_finish(const DirectRefineArgs a) {
  const long j = (long)blockIdx.x * kRefineBlock + threadIdx.x;
  if (j >= (long)a.M * a.B) return;
  const int b = (int)(j / a.M), i = (int)(j - (long)b * a.M);
  const int n = a.ctl[RC_N * a.B + b], cur = a.ctl[RC_CUR * a.B + b];
  const double nan = __builtin_nan("");
  const bool in = i < n;
#pragma unroll
  for (int c = 0; c < NS; ++c) a.X_out[j * NS + c] = in ? a.X[cur][j * NS + c] : nan;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.U_out[j * 3 + c] = in ? a.U[cur][j * 3 + c] : nan;
  a.t_out[j] = in ? a.t[cur][j] : nan;
  if (i < a.M - 1) a.E_out[(long)b * (a.M - 1) + i] = (i < n - 1) ? a.E[cur][j] : nan;
}

template <int NS>
static hipError_t refine_begin(const DirectRefineArgs& a, hipStream_t st) {
  const long S = (long)(a.n_in - 1) * a.B;
  hipLaunchKernelGGL((k_refine_errors<NS>), dim3((unsigned)((2 * S + 63) / 64)), dim3(64), 0, st, a);
  if (a.n_in <= kRefineLdsNodes) hipLaunchKernelGGL((k_refine_remove<NS, true>), dim3(a.B), dim3(kRefineBlock), 0, st, a);
  else {
    if (!a.rm_est || !a.rm_link) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_refine_remove<NS, false>), dim3(a.B), dim3(kRefineBlock), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_direct_refine_begin(int nstate, const DirectRefineArgs& a, hipStream_t st) {
  if (a.B < 1 || a.n_in < 2 || a.M < a.n_in) return hipErrorInvalidValue;
  return nstate == 6 ? refine_begin<6>(a, st) : nstate == 7 ? refine_begin<7>(a, st) : hipErrorInvalidValue;
}

hipError_t launch_direct_refine_pass(int nstate, const DirectRefineArgs& a, int max_split, hipStream_t st) {
  if (nstate != 6 && nstate != 7) return hipErrorInvalidValue;
  if (nstate == 6) hipLaunchKernelGGL((k_refine_split<6>), dim3(a.B), dim3(kRefineBlock), 0, st, a);
  else hipLaunchKernelGGL((k_refine_split<7>), dim3(a.B), dim3(kRefineBlock), 0, st, a);
  if (max_split > 0) {
    const dim3 grid((max_split + 31) / 32, a.B);
    if (nstate == 6) hipLaunchKernelGGL((k_refine_insert<6>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_refine_insert<7>), grid, dim3(64), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_direct_refine_finish(int nstate, const DirectRefineArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)(((long)a.M * a.B + kRefineBlock - 1) / kRefineBlock));
  if (nstate == 6) hipLaunchKernelGGL((k_refine_finish<6>), grid, dim3(kRefineBlock), 0, st, a);
  else if (nstate == 7) hipLaunchKernelGGL((k_refine_finish<7>), grid, dim3(kRefineBlock), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lto
