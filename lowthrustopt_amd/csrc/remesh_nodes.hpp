// remesh_nodes.hpp -- the node kernel of the mesh equidistribution, a template of the row count: <12> is
// instantiated in kernels_remesh.hip, <14> (state + mass + costates + mass costate) in kernels_indirect14.hip.
#pragma once
#include "indirect_kernel.hpp"

namespace lto {

// ---- the nodes.  Lane = NEW node j = b n_new + k: it gathers old node seg_of[j] of its trajectory, integrates over its own span
// t'_k - t_seg with the plan's integrator (advance<>, as the sweeps and k_indirect_dense) and stores struct-of-arrays in the solve
// loop's node layout.  The new nodes inside one heavy old segment run side by side; no lane integrates further than one old
// segment.  A zero span (the first and the last node always) stores the gathered node bit for bit.
template <int ND, int PM, int METHOD>
__global__ __launch_bounds__(64) void k_remesh_nodes(const IndirectArgs a, const RemeshNodeArgs r) {
  const long j = (long)blockIdx.x * 64 + threadIdx.x;
  if (j >= (long)r.n_new * r.n_batch) return;
  const int traj = (int)(j / r.n_new);
  using Sys = SysIndirect<ND, PM, 0>;
  Sys sys;
  sys.tp = a.tp[(long)traj * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;
  sys.w2 = 2.0 * sys.tp.omega;
  const int i = r.seg_of[j];
  const long node = (long)traj * a.n_nodes + i;
  double y[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c) y[c] = a.X[c * a.ldx + node];
  const double span = r.tn[j] - a.t[(long)traj * a.t_stride + i];
  int nacc = 0, nrej = 0;
  double maxErr = 0.0;
  if (span > 0.0) advance<Sys, ND, METHOD>(sys, span, a, y, nacc, nrej, maxErr);
#pragma unroll
  for (int c = 0; c < ND; ++c) r.G[c * r.ldg + j] = y[c];
}

template <int ND, int METHOD>
static hipError_t launch_remesh_nodes_pm(int pm, const IndirectArgs& a0, const RemeshNodeArgs& r, hipStream_t st) {
  dim3 grid((unsigned)(((long)r.n_new * r.n_batch + 63) / 64));
  (void)for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) {
    hipLaunchKernelGGL((k_remesh_nodes<ND, decltype(cls)::value, METHOD>), grid, dim3(64), 0, st, a, r);
    return hipSuccess;
  });
  return hipGetLastError();
}

template <int ND>
static hipError_t launch_remesh_nodes_method(int pm, int method, const IndirectArgs& a, const RemeshNodeArgs& r, hipStream_t st) {
  if ((long)r.n_new * r.n_batch <= 0) return hipSuccess;
  switch (method) {
    case M_RK4: return launch_remesh_nodes_pm<ND, M_RK4>(pm, a, r, st);
    case M_DOP853_ADAPTIVE: return launch_remesh_nodes_pm<ND, M_DOP853_ADAPTIVE>(pm, a, r, st);
  }
  return hipErrorInvalidValue;
}

// the 14-row family (kernels_indirect14.hip); launch_remesh_nodes (kernels_remesh.hip) switches on the row count
hipError_t launch_remesh_nodes14(int pm, int method, const IndirectArgs& a, const RemeshNodeArgs& r, hipStream_t st);

}  // namespace lto
