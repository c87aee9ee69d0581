// kernels_stationkeep.hip -- station-keeping on periodic orbits of the CRTBP, gfx950: the Floquet-mode feedback gains
// from the hyperbolic directions the manifold seeds carry round the orbit, and batched flights under any impulsive linear feedback.
//
// k_stationkeep_gains   one lane per (phase, orbit).  With S = [2 Omega, -I; I, 0] (A^T S + S A = 0 for the variational system, so
//                       Phi^T S Phi = S) w = S v_s is a left eigenvector of the monodromy matrix for lambda_u at every phase: W = w /
//                       (w . v_u), G = -w_v W^T / |w_v|^2 the minimum-norm velocity change that zeroes the unstable component,
//                       alpha = |w_v| / |W|.  No fused multiply-add: every product and every sum rounded on its own, in the order
//                       include/lto.h states, so the host reproduces the outputs bit for bit.
// k_stationkeep_flight  one lane per run, 6 components, span by span under run_dop853 (or `steps` RK4 steps) over SysCrtbpDir
//                       (crtbp_ballistic.hpp): at every burn epoch the deviation from the reference point, the lost test, the
//                       commanded burn G (d + nav), dead band and clip, the execution error, the impulse, then the ballistic span.
//                       The loop counter is the same for every lane of a wave (a lost or failed lane leaves the loop, nothing is
//                       synchronised), so with n_orb = 1 the reference points and the spans come through scalar loads and the gains
//                       from one address for the wave.
//                       nav / exe stay run-major as the caller passes them: 80 bytes per span against hundreds of right-hand sides.
//
// No LDS, no atomics, plain vector stores; per-lane flags are doubles (DESIGN "Compiler hazards").
#include "kernels.hpp"
#include "crtbp_ballistic.hpp"

namespace lto {

__global__ __launch_bounds__(64) void k_stationkeep_gains(const StationGainsArgs a) {
#pragma clang fp contract(off)                 // the order of include/lto.h, every operation rounded on its own
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n) return;
  double vu[6], vs[6];
  double fin = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) { vu[i] = a.V[12 * g + i]; vs[i] = a.V[12 * g + 6 + i]; fin += vu[i]; fin += vs[i]; }
  double w[6];
  w[0] = 2.0 * vs[1] - vs[3];
  w[1] = -2.0 * vs[0] - vs[4];
  w[2] = -vs[5];
  w[3] = vs[0]; w[4] = vs[1]; w[5] = vs[2];
  double p = w[0] * vu[0], ns2 = w[0] * w[0], nu2 = vu[0] * vu[0];
#pragma unroll
  for (int i = 1; i < 6; ++i) {
    const double q = w[i] * vu[i], qs = w[i] * w[i], qu = vu[i] * vu[i];
    p = p + q; ns2 = ns2 + qs; nu2 = nu2 + qu;
  }
  const double ns = __dsqrt_rn(ns2), nu = __dsqrt_rn(nu2);
  double W[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) W[i] = w[i] / p;
  double wn2 = W[0] * W[0];
#pragma unroll
  for (int i = 1; i < 6; ++i) { const double q = W[i] * W[i]; wn2 = wn2 + q; }
  const double q3 = W[3] * W[3], q4 = W[4] * W[4], q5 = W[5] * W[5];
  const double wv2 = (q3 + q4) + q5;
  const double alpha = __dsqrt_rn(wv2) / __dsqrt_rn(wn2);
  const double lim = (a.sing_tol * ns) * nu;
  double st = 0.0;
  if (!((fin - fin) == 0.0)) st = 2.0;
  else if (fabs(p) <= lim || !(alpha > a.sing_tol)) st = 3.0;
  const double nan = __builtin_nan("");
  if (a.W) {
#pragma unroll
    for (int i = 0; i < 6; ++i) a.W[6 * g + i] = (st != 0.0) ? nan : W[i];
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double q = W[3 + r] * W[c];
      a.G[18 * g + 3 * c + r] = (st != 0.0) ? nan : (-q) / wv2;
    }
  }
  if (a.alpha) a.alpha[g] = (st != 0.0) ? nan : alpha;
  a.status[g] = (int)st;
}

hipError_t launch_stationkeep_gains(const StationGainsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_stationkeep_gains, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

namespace {

__device__ __forceinline__ double norm3(const double x, const double y, const double z) {
  return sqrt(__builtin_fma(x, x, __builtin_fma(y, y, z * z)));
}

// One double of the orbit records X_ref and dt.  SHARED (n_orb = 1): every lane of a wave reads the same address, and nothing writes
// the records while the kernel runs, so the read goes through the constant address space -- a scalar load into SGPRs when the index
// is wave-uniform, which the loop counter is.  Otherwise a plain per-lane load.  The 18 doubles of G stay on vector loads (one
// address for the wave when SHARED): as scalars they are 36 more SGPRs, and the DOP853 kernel, already spilling SGPRs to VGPR
// lanes, then spills to scratch memory (68 bytes).
template <bool SHARED>
__device__ __forceinline__ double orbit_read(const double* p, const long i) {
  if constexpr (SHARED) return ((const __attribute__((address_space(4))) double*)p)[i];
  else return p[i];
}

}  // namespace

template <int METHOD, bool SHARED>
__global__ __launch_bounds__(64) void k_stationkeep_flight(const StationFlightArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int n_man = a.n_man, n_upd = a.n_man * a.n_rev;
  const long ob = SHARED ? 0L : (long)b * n_man;             // the first record of the run's orbit
  const double* navb = a.nav ? a.nav + 6L * n_upd * b : nullptr;
  const double* exeb = a.exe ? a.exe + 4L * n_upd * b : nullptr;
  double* devb = a.dev ? a.dev + 2L * n_upd * b : nullptr;
  double* histb = a.dv_hist ? a.dv_hist + (long)n_upd * b : nullptr;
  SysCrtbpDir sys;
  sys.MU = a.MU;
  sys.sgn = 1.0;
  double y[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) y[q] = a.x0[6L * b + q];
  // per-lane flags are doubles (dop853_lane.hpp)
  double st = finite_all(y) ? 0.0 : 2.0;       // 0 in flight, 1 lost, 2 failed
  double total = 0.0, dev_r = 0.0, dev_v = 0.0;
  int nb = 0, nacc = 0, nrej = 0;
  int end_u = (st != 0.0) ? 0 : n_upd;         // the update at which the run ended
  if (st == 0.0) {
    // u and j are the same in every lane that is still in the loop: the orbit's records are at wave-uniform addresses when SHARED
    for (int u = 0, j = 0; u < n_upd; ++u, j = (j + 1 == n_man) ? 0 : j + 1) {
      const long rec = ob + j;
      double d[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) d[q] = y[q] - orbit_read<SHARED>(a.X_ref, 6 * rec + q);
      dev_r = norm3(d[0], d[1], d[2]);
      dev_v = norm3(d[3], d[4], d[5]);
      if (!(((dev_r + dev_v) - (dev_r + dev_v)) == 0.0)) { st = 2.0; end_u = u; break; }
      if (devb) { devb[2 * u] = dev_r; devb[2 * u + 1] = dev_v; }
      if (a.r_lost > 0.0 && dev_r > a.r_lost) { st = 1.0; end_u = u; break; }
      if (navb) {
#pragma unroll
        for (int q = 0; q < 6; ++q) d[q] += navb[6 * u + q];
      }
      double c[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) acc = __builtin_fma(a.G[18 * rec + 3 * q + r], d[q], acc);
        c[r] = acc;
      }
      const double m = norm3(c[0], c[1], c[2]);
      if (!((m - m) == 0.0)) { st = 2.0; end_u = u; break; }
      double burn = 0.0;
      if (!(m < a.dv_min)) {
        if (a.dv_max > 0.0 && m > a.dv_max) {
          const double s = a.dv_max / m;
          c[0] *= s; c[1] *= s; c[2] *= s;
        }
        if (exeb) {
          const double s = 1.0 + exeb[4 * u];
#pragma unroll
          for (int r = 0; r < 3; ++r) c[r] = __builtin_fma(s, c[r], exeb[4 * u + 1 + r]);
        }
        burn = norm3(c[0], c[1], c[2]);
        if (!((burn - burn) == 0.0)) { st = 2.0; end_u = u; break; }
        y[3] += c[0]; y[4] += c[1]; y[5] += c[2];
        total += burn;
        ++nb;
      }
      if (histb) histb[u] = burn;
      const double span = orbit_read<SHARED>(a.dt, rec);
      if (METHOD == M_RK4) {
        const double h = span / (double)a.steps;
        for (int k = 0; k < a.steps; ++k) rk4_step(sys, h, y);
        nacc += a.steps;
      } else {
        int na = 0, nr = 0;
        run_dop853<SysCrtbpDir, 6>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr);
        nacc += na; nrej += nr;
      }
      if (!finite_all(y)) { st = 2.0; end_u = u; break; }
    }
  }
  const double nan = __builtin_nan("");
  if (st == 0.0) {
    double d[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) d[q] = y[q] - orbit_read<SHARED>(a.X_ref, 6 * ob + q);
    dev_r = norm3(d[0], d[1], d[2]);
    dev_v = norm3(d[3], d[4], d[5]);
  }
  // the history past the run's end: a lost run keeps the deviation that lost it, a failed run nothing of its last update
  for (int u = end_u; u < n_upd; ++u) {
    if (devb && (st == 2.0 || u > end_u)) { devb[2 * u] = nan; devb[2 * u + 1] = nan; }
    if (histb) histb[u] = nan;
  }
  const bool fail = st == 2.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) a.x_final[6L * b + q] = fail ? nan : y[q];
  a.dv_total[b] = fail ? nan : total;
  if (a.dev_final) { a.dev_final[2L * b] = fail ? nan : dev_r; a.dev_final[2L * b + 1] = fail ? nan : dev_v; }
  if (a.n_burn) a.n_burn[b] = nb;
  if (a.accepted) a.accepted[b] = nacc;
  if (a.rejected) a.rejected[b] = nrej;
  if (a.lost_at) a.lost_at[b] = (st == 1.0) ? end_u : -1;
  a.status[b] = (int)st;
}

template <int METHOD>
static hipError_t launch_stationkeep_method(const StationFlightArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.B + 63) / 64));
  if (a.n_orb == 1) hipLaunchKernelGGL((k_stationkeep_flight<METHOD, true>), grid, dim3(64), 0, st, a);
  else hipLaunchKernelGGL((k_stationkeep_flight<METHOD, false>), grid, dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_stationkeep_flight(int method, const StationFlightArgs& a, hipStream_t st) {
  if (method == M_RK4) return launch_stationkeep_method<M_RK4>(a, st);
  if (method == M_DOP853_ADAPTIVE) return launch_stationkeep_method<M_DOP853_ADAPTIVE>(a, st);
  return hipErrorInvalidValue;
}

}  // namespace lto
