// kernels_addtime.hip -- addTimeFinal (src/HelperFunctions.jl:196-250) re-specified for a batch of K time-of-flight changes
// (DESIGN 4.12): the re-mesh of the densified, extended trajectories onto the new grids (:211-224), the snap of their last
// node onto the arrival orbit (find_tau, :38-48, then :227-230), and the cost of a converged trajectory's control law.
// The extended trajectories themselves are integrated by k_indirect_dense (indirect_kernel.hpp); nothing here integrates.
#include "kernels.hpp"
#include "orbit_spline.hpp"

namespace lto {

// ---- re-mesh: natural cubic spline through each of the ROWS x K sample rows (12: state and costate; 14: the variable-mass system,
// DESIGN 4.21 -- the mass and its costate are rows like any other), evaluated at the n new nodes.
// Lane = (component, trajectory) pair, pair = c * K + b.  The knots of a trajectory are LinRange(t0, t_end, m): uniform, so the
// moment system M_{i-1} + 4 M_i + M_{i+1} = 6 / h^2 (y_{i+1} - 2 y_i + y_{i-1}), M_0 = M_{m-1} = 0, has constant coefficients and
// its Thomas factors cp[] are the same for every lane (computed on the host).  The forward sweep keeps d' in mom[j * P + pair]
// (coalesced over the lanes), the backward sweep turns it into the moments in place, then the lane evaluates its row at the new
// nodes with the knots' own spacing -- the form of drivers._natural_spline.  Nodes 0 and n-1 coincide with knots 0 and m-1: the
// sample itself is returned there, bit for bit.
template <int ROWS>
__global__ __launch_bounds__(64) void k_remesh_spline(const RemeshArgs r) {
  const int P = ROWS * r.K;
  const int pair = blockIdx.x * 64 + threadIdx.x;
  if (pair >= P) return;
  const int c = pair / r.K, b = pair - c * r.K;
  const int m = r.m;
  const double* y = r.Y + (long)c * r.ldy + (long)b * m;
  const double* td = r.td + (long)b * m;
  const double* tn = r.tn + (long)b * r.n;
  double* mom = r.mom;
  const double h = (td[m - 1] - td[0]) / (double)(m - 1);
  const double s6 = 6.0 / (h * h);
  // forward sweep: d'_i = (r_i - d'_{i-1}) cp_i, cp_i = 1 / (4 - cp_{i-1}), cp_0 = 0
  double dprev = 0.0, y0 = y[0], y1 = y[1];
  for (int i = 1; i < m - 1; ++i) {
    const double y2 = y[i + 1];
    const double ri = s6 * ((y2 - y1) - (y1 - y0));
    dprev = (ri - dprev) * r.cp[i];
    mom[(long)i * P + pair] = dprev;
    y0 = y1; y1 = y2;
  }
  // backward sweep: M_{m-2} = d'_{m-2}, M_i = d'_i - cp_i M_{i+1}
  double mnext = 0.0;
  for (int i = m - 2; i >= 1; --i) {
    mnext = mom[(long)i * P + pair] - r.cp[i] * mnext;
    mom[(long)i * P + pair] = mnext;
  }
  double* out = r.G + (long)c * r.ldg + (long)b * r.n;
  out[0] = y[0];
  out[r.n - 1] = y[m - 1];
  int i = 0;
  for (int k = 1; k < r.n - 1; ++k) {
    const double x = tn[k];
    // the last knot i with td[i] <= x, clipped to [0, m-2] (searchsorted(side = right) - 1); x grows with k
    while (i < m - 2 && td[i + 1] <= x) ++i;
    const double t0 = td[i], t1 = td[i + 1], hi = t1 - t0, a = t1 - x, bb = x - t0;
    const double Mi = (i == 0) ? 0.0 : mom[(long)i * P + pair];
    const double Mj = (i + 1 == m - 1) ? 0.0 : mom[(long)(i + 1) * P + pair];
    out[k] = (Mi * a * a * a + Mj * bb * bb * bb) / (6.0 * hi) + (y[i] - Mi * hi * hi / 6.0) * a / hi +
             (y[i + 1] - Mj * hi * hi / 6.0) * bb / hi;
  }
}

hipError_t launch_remesh_spline(int rows, const RemeshArgs& r, hipStream_t st) {
  if (rows == 12) hipLaunchKernelGGL(k_remesh_spline<12>, dim3((12 * r.K + 63) / 64), dim3(64), 0, st, r);
  else if (rows == 14) hipLaunchKernelGGL(k_remesh_spline<14>, dim3((14 * r.K + 63) / 64), dim3(64), 0, st, r);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- find_tau: one workgroup per trajectory.  Candidate j = 0..1000 has tau_j = j / 1000 and d_j = |s(tau_j) - x|_2 with x the
// position and velocity of the trajectory's last node; the first j of the smallest d_j wins (the reference's
// tau_trial[d .== minimum(d)][1]) -- a (distance, index) lexicographic minimum, the same whatever the reduction order.  A NaN
// distance never wins; if every one is NaN, j = 0.  The winner's s(tau*) replaces the node's first six rows, tau* goes to tau.
constexpr int kTauCand = 1001;
constexpr int kTauBlock = 256;

__device__ __forceinline__ void tau_min(double& d, int& j, const double d2, const int j2) {
  if (d2 < d || (d2 == d && j2 < j)) { d = d2; j = j2; }
}

__global__ __launch_bounds__(kTauBlock) void k_find_tau(const EndOrbitsDev o, double* G, long ldg, int n, double* tau) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long node = (long)b * n + (n - 1);
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = G[q * ldg + node];
  double best = __builtin_inf();
  int jbest = kTauCand;
  for (int j = tid; j < kTauCand; j += kTauBlock) {
    const double tj = (double)j / 1000.0;
    double s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double dq = end_spline(o, 1, q, tj) - x[q];
      s2 += dq * dq;
    }
    const double d = sqrt(s2);
    tau_min(best, jbest, d == d ? d : __builtin_inf(), j);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double d2 = __shfl_xor(best, off, 64);
    const int j2 = __shfl_xor(jbest, off, 64);
    tau_min(best, jbest, d2, j2);
  }
  __shared__ double sd[kTauBlock / 64];
  __shared__ int sj[kTauBlock / 64];
  if ((tid & 63) == 0) { sd[tid >> 6] = best; sj[tid >> 6] = jbest; }
  __syncthreads();
  if (tid < 6) {
    double d = sd[0];
    int j = sj[0];
    for (int w = 1; w < kTauBlock / 64; ++w) tau_min(d, j, sd[w], sj[w]);
    if (j >= kTauCand) j = 0;
    const double ts = (double)j / 1000.0;
    G[tid * ldg + node] = end_spline(o, 1, tid, ts);
    if (tid == 0) tau[b] = ts;
  }
}

hipError_t launch_find_tau(const EndOrbitsDev& o, double* G, long ldg, int n, int K, double* tau, hipStream_t st) {
  hipLaunchKernelGGL(k_find_tau, dim3(K), dim3(kTauBlock), 0, st, o, G, ldg, n, tau);
  return hipGetLastError();
}

// ---- cost of the control law along K dense outputs: trapezoid over t_dense of umag(|lambda_v|) in DU/TU (controlLaw_cart's
// magnitude before the conversion to N, indirect.jl:389-440; a NaN magnitude counts 0 as there).  One lane per trajectory.
__global__ __launch_bounds__(64) void k_dense_cost(const double* Y, long ldy, const double* td, int m, int K, double aL, double p,
                                                   double rho, double* cost) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= K) return;
  const long o = (long)b * m;
  double acc = 0.0, uprev = 0.0, tprev = 0.0;
  for (int j = 0; j < m; ++j) {
    const double lx = Y[9 * ldy + o + j], ly = Y[10 * ldy + o + j], lz = Y[11 * ldy + o + j];
    const double nv = sqrt(lx * lx + ly * ly + lz * lz);
    double u;
    if (p == 0.0) u = aL;
    else if (p == 1.0) u = 0.5 * (1.0 + tanh((nv - 1.0) / (2.0 * rho))) * aL;
    else { u = pow(nv / p, 1.0 / (p - 1.0)); if (u > aL) u = aL; }   // np.minimum: a NaN stays NaN
    if (u != u) u = 0.0;
    const double tj = td[o + j];
    if (j > 0) acc += 0.5 * (tj - tprev) * (uprev + u);
    uprev = u; tprev = tj;
  }
  cost[b] = acc;
}

hipError_t launch_dense_cost(const double* Y, long ldy, const double* td, int m, int K, double aL, double p, double rho, double* cost,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_dense_cost, dim3((K + 63) / 64), dim3(64), 0, st, Y, ldy, td, m, K, aL, p, rho, cost);
  return hipGetLastError();
}

// ---- the same for the 14-row variable-mass system: lambda_v is rows 10..12, and the acceleration limit is the
// sample's own, aL_j = cT / m_j with m_j row 6 and cT = thrustLimit / 1e3 TU^2 / DU.  The expression forms are k_dense_cost's.
// A sample whose mass is not positive (a re-solve that did not converge can leave one) counts 0, as a NaN does.
__global__ __launch_bounds__(64) void k_dense_cost_mass(const double* Y, long ldy, const double* td, int m, int K, double cT, double p,
                                                        double rho, double* cost) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= K) return;
  const long o = (long)b * m;
  double acc = 0.0, uprev = 0.0, tprev = 0.0;
  for (int j = 0; j < m; ++j) {
    const double lx = Y[10 * ldy + o + j], ly = Y[11 * ldy + o + j], lz = Y[12 * ldy + o + j];
    const double nv = sqrt(lx * lx + ly * ly + lz * lz);
    const double ms = Y[6 * ldy + o + j];
    const double aL = cT / ms;
    double u;
    if (p == 0.0) u = aL;
    else if (p == 1.0) u = 0.5 * (1.0 + tanh((nv - 1.0) / (2.0 * rho))) * aL;
    else { u = pow(nv / p, 1.0 / (p - 1.0)); if (u > aL) u = aL; }   // np.minimum: a NaN stays NaN
    if (u != u || !(ms > 0.0)) u = 0.0;
    const double tj = td[o + j];
    if (j > 0) acc += 0.5 * (tj - tprev) * (uprev + u);
    uprev = u; tprev = tj;
  }
  cost[b] = acc;
}

hipError_t launch_dense_cost_mass(const double* Y, long ldy, const double* td, int m, int K, double cT, double p, double rho,
                                  double* cost, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_cost_mass, dim3((K + 63) / 64), dim3(64), 0, st, Y, ldy, td, m, K, cT, p, rho, cost);
  return hipGetLastError();
}

}  // namespace lto
