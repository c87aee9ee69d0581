// kernels_remesh.hip -- mesh equidistribution of a converged indirect solution: the new grid from a per-segment
// monitor (k_remesh_grid) and the nodes of the input's own piecewise trajectory on it (k_remesh_nodes, remesh_nodes.hpp).
#include "remesh_nodes.hpp"
#include "scan64.hpp"

namespace lto {

// ---- the grid.  One workgroup per trajectory.  Monitor w_i > 0 of old segment i (the caller's weights, or the trial-step counts
// nacc + nrej of a defect sweep), C_0 = 0, C_{i+1} = C_i + w_i, W = C_{n-1}; new node k sits where the piecewise-linear C(t) reaches
// g_k = k W / (n_new - 1).
//
// The running sum is scan64.hpp's: one summation order whatever the size (tests/remesh_reference.scan64 restates it).
// The partial sums of up to kRemeshLdsSegs segments stay in LDS; above that the same code runs on a global scratch block
// (`C`, written and read by this workgroup only, between its own barriers).
template <bool IN_LDS>
__global__ __launch_bounds__(kRemeshBlock) void k_remesh_grid(const RemeshGridArgs r) {
#pragma clang fp contract(off)       // t'_k in the order the restatement writes it: no fused multiply-add
  __shared__ double s1[IN_LDS ? kRemeshLdsSegs : 1], s2[IN_LDS ? kRemeshLdsSegs / 64 : 1], s3[64], s4[1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = r.n, m = n - 1, n_new = r.n_new;
  const int m1 = (m + 63) >> 6, m2 = (m1 + 63) >> 6;
  double* c1 = IN_LDS ? s1 : r.C + (long)b * r.c_stride;
  double* c2 = IN_LDS ? s2 : c1 + (((long)m + 63) & ~63L);
  const double* t = r.t + (long)b * r.t_stride;
  const double* w = r.w ? r.w + (long)b * m : nullptr;
  const int* na = r.nacc ? r.nacc + (long)b * m : nullptr;
  const int* nr = r.nrej ? r.nrej + (long)b * m : nullptr;
  const auto monitor = [&](const int i) { return w ? w[i] : (double)(na[i] + nr[i]); };
  for (int i = tid; i < m; i += kRemeshBlock) c1[i] = monitor(i);
  __syncthreads();
  scan_tiles(c1, m, c2, tid);
  scan_tiles(c2, m1, s3, tid);
  scan_tiles(s3, m2, s4, tid);
  add_tile_offsets(c2, m1, s3, tid);
  add_tile_offsets(c1, m, c2, tid);
  // c1[i] = C_{i+1}
  const double W = c1[m - 1];
  double* tn = r.t_out + (long)b * n_new;
  int* seg = r.seg_of + (long)b * n_new;
  for (int k = tid; k < n_new; k += kRemeshBlock) {
    if (k == 0) { tn[0] = t[0]; seg[0] = 0; continue; }
    if (k == n_new - 1) { tn[k] = t[n - 1]; seg[k] = n - 1; continue; }
    const double g = (double)k * W / (double)(n_new - 1);
    int lo = 0, hi = m - 1;                     // the largest i in [0, m-1] with C_i <= g (a NaN g: i = 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (c1[mid - 1] <= g) lo = mid; else hi = mid - 1;
    }
    int i = lo;
    const double Ci = i ? c1[i - 1] : 0.0;
    const double ti = t[i];
    const double tk = ti + (g - Ci) / monitor(i) * (t[i + 1] - ti);
    // the node the new one is propagated from: the largest i with t_i <= t'_k (t'_k may round onto t_{i+1}: a copy of that node)
    while (i < n - 1 && t[i + 1] <= tk) ++i;
    tn[k] = tk;
    seg[k] = i;
  }
}

hipError_t launch_remesh_grid(const RemeshGridArgs& r, hipStream_t st) {
  if (r.n_batch <= 0) return hipSuccess;
  if (r.n < 2 || r.n_new < 2 || r.n - 1 > kRemeshMaxSegs) return hipErrorInvalidValue;
  if (r.n - 1 <= kRemeshLdsSegs) hipLaunchKernelGGL(k_remesh_grid<true>, dim3(r.n_batch), dim3(kRemeshBlock), 0, st, r);
  else {
    if (!r.C || r.c_stride < (long)remesh_scratch_doubles(r.n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_remesh_grid<false>, dim3(r.n_batch), dim3(kRemeshBlock), 0, st, r);
  }
  return hipGetLastError();
}

// ---- the nodes: k_remesh_nodes<ND, PM, METHOD> (remesh_nodes.hpp).  The 12-row family lives here.
hipError_t launch_remesh_nodes(int ndim, int pm, int method, const IndirectArgs& a, const RemeshNodeArgs& r, hipStream_t st) {
  if (ndim == 14) return launch_remesh_nodes14(pm, method, a, r, st);
  if (ndim != 12) return hipErrorInvalidValue;
  return launch_remesh_nodes_method<12>(pm, method, a, r, st);
}

}  // namespace lto
