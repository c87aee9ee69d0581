// direct_segment.hpp -- one segment of the direct transcription on a lane pair: the forward half-arc from node i and the backward
// half-arc from node i+1 (lane parity = direction) meet through the xchg1 exchange.  The defect sweep (kernels_direct.hip), the
// mesh refinement (kernels_direct_refine.hip) and the resampling (kernels_direct_resample.hip) evaluate segments through these
// functions alone, so an estimate or a mid-point of theirs is the sweep's, bit for bit.
#pragma once
#include "kernels.hpp"
#include "rk.hpp"

namespace lto {

template <int NS>
struct SysDirect {
  static constexpr int DIM = NS;
  DirectLane L;
  __device__ __forceinline__ void rhs(const double (&x)[NS], double (&k)[NS]) const {
    VarCoef6 vc;
    rhs_direct<NS, false>(x, L, k, vc);
  }
};

// physical constants of a direct sweep as the lanes use them
struct DirectConsts {
  double MU, kk, isp_g0, TU;       // kk = TU^2/DU/1e3; isp_g0 = Isp * 9.81
};

// the lane's half-arc: control (cx, cy, cz) of its node and the time direction; nc = |control|
__device__ __forceinline__ void direct_lane(const DirectConsts& k, const int dir, const double cx, const double cy, const double cz,
                                            DirectLane& L, double& nc) {
  const double td = dir ? -1.0 : 1.0;
  L.MU = k.MU;
  L.w2 = 2.0 * td;
  L.cx = cx; L.cy = cy; L.cz = cz;
  L.kk = k.kk;
  { const double k6 = L.kk * 1e-3; L.tx = L.cx * k6; L.ty = L.cy * k6; L.tz = L.cz * k6; }   // NS = 6: control * kk / 1000.0
  nc = sqrt(__builtin_fma(L.cx, L.cx, __builtin_fma(L.cy, L.cy, L.cz * L.cz)));
  L.mdot = -td * nc / k.isp_g0 * k.TU;                       // prop_EP_deriv.jl:42
}

__device__ __forceinline__ double xchg1(double v) { return __shfl_xor(v, 1); }

// The segment of this lane pair.  x: in, the lane's node state (velocity already reversed on the backward lane, direct.jl:92); out, the
// half-arc's end state in forward orientation -- on the forward lane the mid-point state meshRefine_direct inserts (direct.jl:651-660).
// d: forward end - backward end (the defect on the forward lane, :101).  e: the larger RKF7(8) estimate of the two half-arcs (:104).
// Both lanes of the pair must call it together.
template <int NS>
__device__ __forceinline__ void direct_segment(const SysDirect<NS>& sys, const int dir, const double hhalf, const int half_steps,
                                               double (&x)[NS], double (&d)[NS], double& e) {
  const double h = hhalf / (double)half_steps;
  double maxErr = 0.0;
  for (int k = 0; k < half_steps; ++k) {
    double xn[NS];
    const double delta = rkf78_step<SysDirect<NS>, NS>(sys, h, x, xn);
    maxErr = fmax(maxErr, delta);
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c] = xn[c];
  }
  if (dir) { x[3] = -x[3]; x[4] = -x[4]; x[5] = -x[5]; }     // direct.jl:98
#pragma unroll
  for (int c = 0; c < NS; ++c) d[c] = x[c] - xchg1(x[c]);    // fwd lane: state_for - stateF_back  (:101)
  e = fmax(maxErr, xchg1(maxErr));                           // :104
}

// The estimate the mesh tools decide on (the refinement, kernels_direct_refine.hip; the resampling, kernels_direct_resample.hip).
// The sweep's fmax drops a NaN (rk.hpp), so a NaN node would read as a perfect segment and be "removed" together with its
// neighbours, or weigh nothing in a monitor; here a segment whose end states are not numbers has a NaN estimate, which ends the
// work on its trajectory (numpy's min / max propagate it and both comparisons are false).  Finite data: exactly e.
template <int NS>
__device__ __forceinline__ double refine_estimate(const double (&d)[NS], const double e) {
  double bad = e;
#pragma unroll
  for (int c = 0; c < NS; ++c) bad += d[c];
  return (bad != bad) ? bad : e;
}

// One segment on this lane pair from explicit operands: xs = this lane's node state (as stored), (ux, uy, uz) its control, hhalf
// the half span.  Returns the estimate; xs becomes the half-arc's end state (forward lane: the mid-point state).
template <int NS>
__device__ __forceinline__ double refine_segment(const DirectConsts& k, const int dir, double (&xs)[NS], const double ux,
                                                 const double uy, const double uz, const double hhalf, const int half_steps) {
  SysDirect<NS> sys;
  double nc;
  direct_lane(k, dir, ux, uy, uz, sys.L, nc);
  if (dir) { xs[3] = -xs[3]; xs[4] = -xs[4]; xs[5] = -xs[5]; }   // reverse velocity (direct.jl:92)
  double d[NS], e;
  direct_segment<NS>(sys, dir, hhalf, half_steps, xs, d, e);
  return refine_estimate<NS>(d, e);
}

}  // namespace lto
