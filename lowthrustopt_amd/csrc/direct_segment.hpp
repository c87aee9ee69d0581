// direct_segment.hpp -- one segment of the direct transcription on a lane pair: the forward half-arc from node i and the backward
// half-arc from node i+1 (lane parity = direction) meet through the xchg1 exchange.  The defect sweep (kernels_direct.hip) and the
// mesh refinement (kernels_direct_refine.hip) evaluate segments through these functions alone, so an estimate or a mid-point of the
// refinement is the sweep's, bit for bit.
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

}  // namespace lto
