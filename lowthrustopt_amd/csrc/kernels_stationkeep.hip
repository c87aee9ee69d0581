// kernels_stationkeep.hip -- station-keeping on periodic orbits of the CRTBP, gfx950: the Floquet-mode feedback gains
// from the hyperbolic directions the manifold seeds carry round the orbit, and batched flights under any impulsive linear feedback.
//
// k_stationkeep_gains   one lane per (phase, orbit).  With S = [2 Omega, -I; I, 0] (A^T S + S A = 0 for the variational system, so
//                       Phi^T S Phi = S) w = S v_s is a left eigenvector of the monodromy matrix for lambda_u at every phase: W = w /
//                       (w . v_u), G = -w_v W^T / |w_v|^2 the minimum-norm velocity change that zeroes the unstable component,
//                       alpha = |w_v| / |W|.  No fused multiply-add: every product and every sum rounded on its own, in the order
//                       include/lto.h states, so the host reproduces the outputs bit for bit.
// k_stationkeep_target_gains  one lane per record: the target-point law of Howell & Pernicka from the phase-to-phase
//                       STMs of k_halo_stm, G = -H^-1 N with H = q I + sum_k r_k B_k^T B_k, N = sum_k r_k B_k^T [A_k | B_k], by a 3 x 3
//                       Cholesky factorisation.  The same rule: no fused multiply-add, the order of include/lto.h.
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

__global__ __launch_bounds__(64) void k_stationkeep_target_gains(const StationTargetGainsArgs a) {
#pragma clang fp contract(off)                 // the order of include/lto.h, every operation rounded on its own
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n) return;
  const double* Pg = a.Phi + 36 * (long)a.K * g;
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // the lower triangle: 00, 10, 11, 20, 21, 22
  double N[3][6];
  double bad = 0.0;
  for (int k = 0; k < a.K; ++k) {
    const double* Pk = Pg + 36 * (long)k;
    const double rk = a.r[k];
    double T[3][6];                            // T = [A_k | B_k], the position rows of Phi_k; B_k = its columns 3..5
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const double v = Pk[6 * c + r];
        bad += ((v - v) == 0.0) ? 0.0 : 1.0;
        if (r < 3) T[r][c] = v;
      }
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j, ++e) {
        double s = T[0][3 + i] * T[0][3 + j];
        s = s + T[1][3 + i] * T[1][3 + j];
        s = s + T[2][3 + i] * T[2][3 + j];
        const double t = rk * s;
        H[e] = (k == 0) ? t : H[e] + t;
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double s = T[0][3 + i] * T[0][c];
        s = s + T[1][3 + i] * T[1][c];
        s = s + T[2][3 + i] * T[2][c];
        const double t = rk * s;
        N[i][c] = (k == 0) ? t : N[i][c] + t;
      }
    }
  }
  const double h00 = a.q + H[0], h10 = H[1], h11 = a.q + H[2], h20 = H[3], h21 = H[4], h22 = a.q + H[5];
  const double hmax = fmax(fmax(h00, h11), h22);
  const double lim = a.sing_tol * hmax;
  // Cholesky H = L L^T: d_i the squared pivots
  const double d0 = h00;
  const double l00 = __dsqrt_rn(d0);
  const double l10 = h10 / l00, l20 = h20 / l00;
  const double d1 = h11 - l10 * l10;
  const double l11 = __dsqrt_rn(d1);
  const double l21 = (h21 - l20 * l10) / l11;
  const double d2 = (h22 - l20 * l20) - l21 * l21;
  const double l22 = __dsqrt_rn(d2);
  double st = 0.0;
  if (bad != 0.0) st = 2.0;
  else if (!(d0 > lim) || !(d1 > lim) || !(d2 > lim)) st = 3.0;
  const double nan = __builtin_nan("");
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double z0 = N[0][c] / l00;
    const double z1 = (N[1][c] - l10 * z0) / l11;
    const double z2 = ((N[2][c] - l20 * z0) - l21 * z1) / l22;
    const double x2 = z2 / l22;
    const double x1 = (z1 - l21 * x2) / l11;
    const double x0 = ((z0 - l10 * x1) - l20 * x2) / l00;
    a.G[18 * g + 3 * c + 0] = (st != 0.0) ? nan : -x0;
    a.G[18 * g + 3 * c + 1] = (st != 0.0) ? nan : -x1;
    a.G[18 * g + 3 * c + 2] = (st != 0.0) ? nan : -x2;
  }
  if (a.pivot) a.pivot[g] = (st != 0.0) ? nan : fmin(fmin(d0, d1), d2) / hmax;
  a.status[g] = (int)st;
}

hipError_t launch_stationkeep_target_gains(const StationTargetGainsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_stationkeep_target_gains, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
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

hipError_t launch_stationkeep_flight(int method, const StationFlightArgs& a, hipStream_t st) {
  if (a.n_orb == 1) return launch_by_method(method, k_stationkeep_flight<M_RK4, true>, k_stationkeep_flight<M_DOP853_ADAPTIVE, true>, a.B, a, st);
  return launch_by_method(method, k_stationkeep_flight<M_RK4, false>, k_stationkeep_flight<M_DOP853_ADAPTIVE, false>, a.B, a, st);
}

}  // namespace lto
