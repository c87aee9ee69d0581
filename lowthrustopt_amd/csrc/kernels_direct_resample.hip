// kernels_direct_resample.hip -- a batch of direct solutions resampled onto one common node count: the new grid
// equidistributes the transcription's own RKF7(8) estimates, the new nodes lie on the transcription's own piecewise trajectory.
//
// The input may be ragged, as lto_direct_refine_batch writes it: trajectory b owns the first n[b] of `cap` columns, anything behind
// them is never read into a result.  Per pass
//   k_resample_errors   the estimates of the current meshes: lane pair = segment through direct_segment, as the defect sweep;
//   k_resample_grid     weights r_i = e_i^(1/8) with their floor, the running sum in scan64.hpp's order, the new times;
//   k_direct_resample_nodes   lane = new node: the half-arc of the old segment it falls into, or a bit copy of an old node.
// All arrays node-major, as the caller's: X [B][cap][NS], U [B][cap][3], t [B][cap].
#include "direct_segment.hpp"
#include "scan64.hpp"

namespace lto {

__device__ __forceinline__ DirectConsts resample_consts(const DirectResampleArgs& a) { return DirectConsts{a.MU, a.kk, a.isp_g0, a.TU}; }
__device__ __forceinline__ int resample_nodes_of(const DirectResampleArgs& a, const int b) { return a.n ? a.n[b] : a.cap; }

// ---- the estimates: lane pair = segment i = 32 blockIdx.x + lane / 2 of trajectory blockIdx.y.  E [B][cap - 1]: the estimate of
// every segment of the valid part, NaN behind it.
template <int NS>
__global__ __launch_bounds__(64) void k_resample_errors(const DirectResampleArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x, dir = lane & 1;
  const int m = resample_nodes_of(a, b) - 1;
  const int i_raw = blockIdx.x * 32 + (lane >> 1);
  double* E = a.E + (long)b * (a.cap - 1);
  const double nan = __builtin_nan("");
  if ((int)blockIdx.x * 32 >= m) {               // wave-uniform: nothing but padding here
    if (dir == 0 && i_raw < a.cap - 1) E[i_raw] = nan;
    return;
  }
  const int i = i_raw < m ? i_raw : m - 1;       // shadow pairs repeat the last valid segment (keeps the exchange defined)
  const long node = (long)b * a.cap + i + dir;
  const double* t = a.t + (long)b * a.cap;
  const double hhalf = 0.5 * (t[i + 1] - t[i]);  // as direct_setup (kernels_direct.hip)
  double x[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) x[c] = a.X[node * NS + c];
  const double e = refine_segment<NS>(resample_consts(a), dir, x, a.U[node * 3], a.U[node * 3 + 1], a.U[node * 3 + 2], hhalf,
                                      a.half_steps);
  if (dir == 0 && i_raw < a.cap - 1) E[i_raw] = i_raw < m ? e : nan;
}

// ---- the grid.  One workgroup per trajectory: weights, running sum, new times, as k_remesh_grid with the node count n[b].
// from_E: W_i = max(r_i, w_floor max_j r_j), r_i = E_i^(1/8) as three square roots (correctly rounded: the host restatement has the
// same weights bit for bit); all weights 1 if every r_j is 0; else W holds the caller's weights.  t_new [B][n_new]: g_k = k W /
// (n_new - 1) on the piecewise-linear running sum, end points the old ones bit for bit.
// status [B] is sticky: a trajectory that arrives with status != 0 is left alone, its times NaN.  Here it becomes 2 on a NaN
// estimate and 1 if the new times are not strictly increasing (n_new beyond what the grid resolves); its times are NaN then.
__device__ __forceinline__ void resample_give_up(const DirectResampleArgs& a, const int b, const int status) {
  double* tn = a.t_new + (long)b * a.n_new;
  for (int k = threadIdx.x; k < a.n_new; k += kRemeshBlock) tn[k] = __builtin_nan("");
  if (threadIdx.x == 0) a.status[b] = status;
}

template <bool IN_LDS>
__global__ __launch_bounds__(kRemeshBlock) void k_resample_grid(const DirectResampleArgs a) {
#pragma clang fp contract(off)       // floor and t'_k in the order the restatement writes them: no fused multiply-add
  __shared__ double s1[IN_LDS ? kRemeshLdsSegs : 1], s2[IN_LDS ? kRemeshLdsSegs / 64 : 1], s3[64], s4[1];
  __shared__ double s_max[kRemeshBlock / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int prior = a.status[b];
  if (prior != 0) { resample_give_up(a, b, prior); return; }   // uniform
  const int n = resample_nodes_of(a, b), m = n - 1, n_new = a.n_new;
  const int m1 = (m + 63) >> 6, m2 = (m1 + 63) >> 6;
  double* c1 = IN_LDS ? s1 : a.C + (long)b * a.c_stride;
  double* c2 = IN_LDS ? s2 : c1 + (((long)m + 63) & ~63L);
  const double* t = a.t + (long)b * a.cap;
  double* w = a.W + (long)b * (a.cap - 1);
  if (a.from_E) {
    const double* E = a.E + (long)b * (a.cap - 1);
    double mx = 0.0;
    int nan_l = 0;
    for (int i = tid; i < m; i += kRemeshBlock) {
      const double e = E[i];
      const double r = sqrt(sqrt(sqrt(e)));
      nan_l |= (r != r);
      mx = fmax(mx, r);
      w[i] = r;                                  // this thread reads it back below
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = mx;
    if (__syncthreads_or(nan_l)) { resample_give_up(a, b, 2); return; }   // uniform
    double rmax = s_max[0];
#pragma unroll
    for (int q = 1; q < kRemeshBlock / 64; ++q) rmax = fmax(rmax, s_max[q]);
    const double floor_w = a.w_floor * rmax;
    for (int i = tid; i < m; i += kRemeshBlock) w[i] = (rmax == 0.0) ? 1.0 : fmax(w[i], floor_w);
  }
  for (int i = tid; i < m; i += kRemeshBlock) c1[i] = w[i];
  __syncthreads();
  scan_tiles(c1, m, c2, tid);
  scan_tiles(c2, m1, s3, tid);
  scan_tiles(s3, m2, s4, tid);
  add_tile_offsets(c2, m1, s3, tid);
  add_tile_offsets(c1, m, c2, tid);
  // c1[i] = C_{i+1}
  const double W = c1[m - 1];
  double* tn = a.t_new + (long)b * n_new;
  for (int k = tid; k < n_new; k += kRemeshBlock) {
    if (k == 0) { tn[0] = t[0]; continue; }
    if (k == n_new - 1) { tn[k] = t[n - 1]; continue; }
    const double g = (double)k * W / (double)(n_new - 1);
    int lo = 0, hi = m - 1;                     // the largest i in [0, m-1] with C_i <= g (a NaN g: i = 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (c1[mid - 1] <= g) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    const double Ci = i ? c1[i - 1] : 0.0;
    const double ti = t[i];
    tn[k] = ti + (g - Ci) / w[i] * (t[i + 1] - ti);
  }
  __syncthreads();                               // the new times of the whole trajectory are written
  int bad = 0;
  for (int k = tid; k < n_new - 1; k += kRemeshBlock) bad |= !(tn[k] < tn[k + 1]);
  if (__syncthreads_or(bad)) resample_give_up(a, b, 1);
}

// u_i + s (u_{i+1} - u_i) in two roundings, as the restatement
__device__ __forceinline__ double resample_control(const double u0, const double u1, const double s) {
#pragma clang fp contract(off)
  return u0 + s * (u1 - u0);
}

// ---- the nodes.  Lane = new node k = 64 blockIdx.x + lane of trajectory blockIdx.y.  i = the largest old index with t_i <= t'_k,
// t_mid = t_i + (t_{i+1} - t_i)/2 (direct.jl:70):
//   t'_k == t_i, or the last node     a bit copy of that old node's state and control;
//   t_i < t'_k <= t_mid                forward from x_i with u_i over t'_k - t_i;
//   t'_k > t_mid                       backward from x_{i+1}, velocity reversed, u_{i+1}, over t_{i+1} - t'_k (direct.jl:90-98);
// half_steps equal RKF7(8) steps over that span.  At t'_k == t_mid the span is the sweep's own 0.5 (t_{i+1} - t_i) -- the
// difference t_mid - t_i may be an ulp off it -- so the node is lto_direct_midpoints' at the same nsteps bit for bit.
// Control: u_i + s (u_{i+1} - u_i), s = (t'_k - t_i)/(t_{i+1} - t_i).  A trajectory with status != 0: NaN.
template <int NS>
__global__ __launch_bounds__(64) void k_direct_resample_nodes(const DirectResampleArgs a) {
  const int b = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  if (k >= a.n_new) return;
  const long j = (long)b * a.n_new + k;
  double* xo = a.X_new + j * NS;
  double* uo = a.U_new + j * 3;
  if (a.status[b] != 0) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < NS; ++c) xo[c] = nan;
#pragma unroll
    for (int c = 0; c < 3; ++c) uo[c] = nan;
    return;
  }
  const int n = resample_nodes_of(a, b);
  const double* t = a.t + (long)b * a.cap;
  const double* Xb = a.X + (long)b * a.cap * NS;
  const double* Ub = a.U + (long)b * a.cap * 3;
  const double tk = a.t_new[j];
  int lo = 0, hi = n - 1;                        // the largest i in [0, n-1] with t_i <= t'_k
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= tk) lo = mid; else hi = mid - 1;
  }
  const int i = (k == a.n_new - 1) ? n - 1 : lo;
  if ((i == n - 1) || (tk == t[i])) {            // the last node, or an old node: bit copies, never a propagation
#pragma unroll
    for (int c = 0; c < NS; ++c) xo[c] = Xb[(long)i * NS + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) uo[c] = Ub[i * 3L + c];
    return;
  }
  const double t0 = t[i], t1 = t[i + 1];
  const double tm = t0 + (t1 - t0) / 2;          // direct.jl:70, in that order
  const double s = (tk - t0) / (t1 - t0);
  int src = i, dir = 0;
  double span;
  if (tk <= tm) span = (tk == tm) ? 0.5 * (t1 - t0) : tk - t0;
  else { dir = 1; src = i + 1; span = t1 - tk; }
  double x[NS];
#pragma unroll
  for (int c = 0; c < NS; ++c) x[c] = Xb[(long)src * NS + c];
  SysDirect<NS> sys;
  double nc;
  direct_lane(resample_consts(a), dir, Ub[src * 3L], Ub[src * 3L + 1], Ub[src * 3L + 2], sys.L, nc);
  if (dir) { x[3] = -x[3]; x[4] = -x[4]; x[5] = -x[5]; }     // reverse velocity (direct.jl:92)
  const double h = span / (double)a.half_steps;              // as direct_segment
  for (int q = 0; q < a.half_steps; ++q) {
    double xn[NS];
    (void)rkf78_step<SysDirect<NS>, NS>(sys, h, x, xn);
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c] = xn[c];
  }
  if (dir) { x[3] = -x[3]; x[4] = -x[4]; x[5] = -x[5]; }     // direct.jl:98
#pragma unroll
  for (int c = 0; c < NS; ++c) xo[c] = x[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) uo[c] = resample_control(Ub[i * 3L + c], Ub[(i + 1) * 3L + c], s);
}

static bool resample_args_ok(int nstate, const DirectResampleArgs& a) {
  return (nstate == 6 || nstate == 7) && a.B >= 1 && a.B <= 65535 && a.cap >= 2 && a.half_steps >= 1;
}

hipError_t launch_direct_resample_errors(int nstate, const DirectResampleArgs& a, hipStream_t st) {
  if (!resample_args_ok(nstate, a) || !a.E) return hipErrorInvalidValue;
  const dim3 grid((a.cap - 1 + 31) / 32, a.B);
  if (nstate == 6) hipLaunchKernelGGL((k_resample_errors<6>), grid, dim3(64), 0, st, a);
  else hipLaunchKernelGGL((k_resample_errors<7>), grid, dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_direct_resample_grid(const DirectResampleArgs& a, hipStream_t st) {
  if (a.B < 1 || a.cap < 2 || a.n_new < 2 || a.cap - 1 > kRemeshMaxSegs || !a.W || !a.t_new || !a.status || (a.from_E && !a.E))
    return hipErrorInvalidValue;
  if (a.cap - 1 <= kRemeshLdsSegs) hipLaunchKernelGGL(k_resample_grid<true>, dim3(a.B), dim3(kRemeshBlock), 0, st, a);
  else {
    if (!a.C || a.c_stride < (long)remesh_scratch_doubles(a.cap)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resample_grid<false>, dim3(a.B), dim3(kRemeshBlock), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_direct_resample_nodes(int nstate, const DirectResampleArgs& a, hipStream_t st) {
  if (!resample_args_ok(nstate, a) || a.n_new < 2 || !a.X_new || !a.U_new || !a.t_new || !a.status) return hipErrorInvalidValue;
  const dim3 grid((a.n_new + 63) / 64, a.B);
  if (nstate == 6) hipLaunchKernelGGL((k_direct_resample_nodes<6>), grid, dim3(64), 0, st, a);
  else hipLaunchKernelGGL((k_direct_resample_nodes<7>), grid, dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace lto
