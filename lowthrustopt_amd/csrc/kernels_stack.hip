// kernels_stack.hip -- the trajectory-stacking initial guess (CRTBP_Multishoot_direct_demo.jl:116-157) for B starts side by side
// (DESIGN 4.15): a ballistic coast on the departure halo, find_tau (HelperFunctions.jl:38-48) for the closest point of the arrival
// halo, a coast from there, and the snap of the last node onto the arrival orbit.  Three kernels: the table work every start of a
// call shares (k_stack_prepare), one coast (k_stack_arc, launched once per arc) and one search (k_stack_find, once per search).
#include "kernels.hpp"
#include "indirect_kernel.hpp"     // run_dop853
#include "orbit_spline.hpp"

namespace lto {

// The CRTBP without thrust: y = (r, v).  The state rows of rhs12 (dynamics.hpp) with the control taken out at compile time.
struct SysBallistic {
  static constexpr int DIM = 6;
  double MU;
  __device__ __forceinline__ void rhs(const double (&y)[6], double (&k)[6]) const {
    const double x = y[0], yy = y[1], z = y[2];
    const double a = x + MU, b = a - 1.0;
    const double yz2 = __builtin_fma(yy, yy, z * z);
    const double d1 = __builtin_fma(a, a, yz2), d2 = __builtin_fma(b, b, yz2);
    const double i1 = rsqrt_nr(d1), i2 = rsqrt_nr(d2);
    const double c1 = (1.0 - MU) * (i1 * i1 * i1), c2 = MU * (i2 * i2 * i2);
    const double cs = c1 + c2;
    k[0] = y[3]; k[1] = y[4]; k[2] = y[5];
    k[3] = __builtin_fma(-c1, a, __builtin_fma(-c2, b, __builtin_fma(2.0, y[4], x)));
    k[4] = __builtin_fma(-cs, yy, __builtin_fma(-2.0, y[3], yy));
    k[5] = -cs * z;
  }
};

// ---- what the starts of a call share: the candidates' states, once, and every start's state on the departure table.
// Thread g < kStackCand: candidate g of the arrival table; thread kStackCandLd + b: start b.
__global__ __launch_bounds__(64) void k_stack_prepare(const EndOrbitsDev o, const double* tau1, int B, double* cand, double* y0) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g < kStackCand) {
    const double tj = (double)g / 1000.0;
    for (int q = 0; q < 6; ++q) cand[q * kStackCandLd + g] = end_spline(o, 1, q, tj);
  } else if (g >= kStackCandLd && g - kStackCandLd < B) {
    const int b = g - kStackCandLd;
    const double x = tau1[b];
    for (int q = 0; q < 6; ++q) y0[(long)q * B + b] = end_spline(o, 0, q, x);
  }
}

hipError_t launch_stack_prepare(const EndOrbitsDev& o, const double* tau1, int B, double* cand, double* y0, hipStream_t st) {
  hipLaunchKernelGGL(k_stack_prepare, dim3((kStackCandLd + B + 63) / 64), dim3(64), 0, st, o, tau1, B, cand, y0);
  return hipGetLastError();
}

// ---- one coast: lane = start.  Every advance starts the integrator afresh (as k_indirect_dense), so a stored node is the flow of
// the stored node before it; a node at the lane's current time is stored as it is.
template <int METHOD>
__device__ __forceinline__ void stack_advance(const SysBallistic& sys, const double span, const StackArcArgs& a, double (&y)[6]) {
  if (METHOD == M_RK4) {
    const double h = span / (double)a.steps;
    for (int k = 0; k < a.steps; ++k) rk4_step(sys, h, y);
  } else {
    int na = 0, nr = 0;
    run_dop853<SysBallistic, 6>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr);
  }
}

template <int METHOD>
__global__ __launch_bounds__(64) void k_stack_arc(const StackArcArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const long B = a.B;
  SysBallistic sys;
  sys.MU = a.MU;
  double y[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) y[q] = a.y0[q * B + b];
  double tcur = a.t_start ? a.t_start[b] : 0.0;
  const int k0 = a.k0 ? a.k0[b] : 0, k1 = a.k1 ? a.k1[b] : a.n;
  for (int k = k0; k < k1; ++k) {
    const double ts = a.t[k * B + b];
    if (ts > tcur) { stack_advance<METHOD>(sys, ts - tcur, a, y); tcur = ts; }
#pragma unroll
    for (int q = 0; q < 6; ++q) a.X[((long)q * a.n + k) * B + b] = y[q];
  }
  if (a.t_end) {
    const double te = a.t_end[b];
    if (te > tcur) stack_advance<METHOD>(sys, te - tcur, a, y);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) a.xe[q * B + b] = y[q];
}

hipError_t launch_stack_arc(int method, const StackArcArgs& a, hipStream_t st) {
  return launch_by_method(method, k_stack_arc<M_RK4>, k_stack_arc<M_DOP853_ADAPTIVE>, a.B, a, st);
}

// ---- find_tau as a scan of the candidate table: one workgroup per start, the rule of k_find_tau (kernels_addtime.hip) -- the first
// j of the smallest |s(j / 1000) - x|_2 as a (distance, index) lexicographic minimum, the same whatever the reduction order; a NaN
// distance never wins, and if every one is NaN, j = 0 (its gap is then NaN).
constexpr int kStackBlock = 256;

__device__ __forceinline__ void stack_min(double& d, int& j, const double d2, const int j2) {
  if (d2 < d || (d2 == d && j2 < j)) { d = d2; j = j2; }
}

__global__ __launch_bounds__(kStackBlock) void k_stack_find(const StackFindArgs f) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long B = f.B;
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = f.x[q * B + b];
  double best = __builtin_inf();
  int jbest = kStackCand;
  for (int j = tid; j < kStackCand; j += kStackBlock) {
    double s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double dq = f.cand[q * kStackCandLd + j] - x[q];
      s2 += dq * dq;
    }
    const double d = sqrt(s2);
    stack_min(best, jbest, d == d ? d : __builtin_inf(), j);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double d2 = __shfl_xor(best, off, 64);
    const int j2 = __shfl_xor(jbest, off, 64);
    stack_min(best, jbest, d2, j2);
  }
  __shared__ double sd[kStackBlock / 64];
  __shared__ int sj[kStackBlock / 64];
  __shared__ double ssnap[6];
  __shared__ int sbad;
  if (tid == 0) sbad = 0;
  if ((tid & 63) == 0) { sd[tid >> 6] = best; sj[tid >> 6] = jbest; }
  __syncthreads();
  if (tid < 6) {
    double d = sd[0];
    int j = sj[0];
    for (int w = 1; w < kStackBlock / 64; ++w) stack_min(d, j, sd[w], sj[w]);
    const bool none = !(d < __builtin_inf());          // every distance NaN (or infinite): candidate 0, and no gap to report
    if (j >= kStackCand) j = 0;
    const double ts = (double)j / 1000.0;
    const double s = end_spline(f.o, 1, tid, ts);
    ssnap[tid] = s;
    if (f.snap) f.snap[tid * B + b] = s;
    if (tid == 0) { f.tau[b] = ts; f.gap[b] = none ? __builtin_nan("") : d; }
  }
  if (!f.X_out) return;
  __syncthreads();
  // the start's nodes in the caller's layout, the last one on the arrival orbit
  const int n = f.n, tot = 6 * n;
  int bad = 0;
  for (int i = tid; i < tot; i += kStackBlock) {
    const int k = i / 6, q = i - 6 * k;
    const double v = (k == n - 1) ? ssnap[q] : f.X[((long)q * n + k) * B + b];
    f.X_out[(long)b * tot + i] = v;
    bad |= !(fabs(v) < __builtin_inf());
  }
  if (bad) atomicOr(&sbad, 1);
  __syncthreads();
  if (tid == 0) f.status[b] = sbad ? 2 : 0;
}

hipError_t launch_stack_find(const StackFindArgs& f, hipStream_t st) {
  hipLaunchKernelGGL(k_stack_find, dim3(f.B), dim3(kStackBlock), 0, st, f);
  return hipGetLastError();
}

}  // namespace lto
