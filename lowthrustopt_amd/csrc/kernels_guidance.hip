// kernels_guidance.hip -- neighbouring-extremal guidance (DESIGN 4.23, and 4.24 for the variable-mass system), gfx950.
//
// k_guidance_gains<NX>: one wavefront per trajectory, lanes 0 .. NX^2 - 1 one element (row r = e % NX, column c = e / NX) of an
// NX x NX block each; NX = 6 for 12-row solutions, 7 for the 14-row variable-mass ones (x = (r, v, m), lambda = (l_r, l_v, l_m)).
// With Phi_k = d y(t_{k+1}) / d y(t_k) = [A B; C D] and d lambda_k = K_k d x_k keeping the linearised arrival conditions:
//   K_{n-2} = -M^-1 N,    K_k = (D - K_{k+1} B)^-1 (K_{k+1} A - C),  k = n-3 .. 0.
// NX = 6: the arrival state is fixed, M = B, N = A.  NX = 7: r_f, v_f and lambda_m(t_f) = 0 are fixed and m_f is free: M is rows
// 0..5 of B over row 6 of D, N rows 0..5 of A over row 6 of C.
// Every node is one NX x NX system M X = R with NX right-hand sides, solved by LU with partial (row) pivoting: lane (r, c) holds
// M[r][c] and R[r][c], rows and columns move between lanes by __shfl, every lane runs the same pivot search on the same NX
// values, so there is no LDS and no barrier, and nothing is shared between wavefronts: a trajectory's gains do not depend on its
// batch.  pivot[k] = min |u_ii| / max |M|, M as it stands (no scaling); below sing_tol the node and every earlier one get NaN gains
// (status 3), a non-finite block or gain does the same with status 2.
//
// k_guided_flight<NX>: lane = start.  The lane carries (x, lambda, q), q' = umag -- SysEvents, 13 components, or SysEventsMass, 15,
// all in DOP853's error norm -- node interval by node interval, each a span of its own (run_dop853, or `steps` RK4 steps).  At node
// k with k % update_every == 0 the costate is reset to lambda_nom,k + K_k (x - x_nom,k + e_j), for NX = 7 with the measured mass
// among the seven rows; otherwise it runs on.  NX = 7 carries the mass over a span as m_k + y[6] (kernels_events.hip) and fails a
// lane whose mass at a span's start is not positive.  The nominal, the gains and the grid are laid out [row][n_nom]: one address
// for all lanes when n_nom = 1, coalesced over the lanes when every start has its own.  Starts, navigation errors and every output
// are [row][B].  One launch per control-law class, per-lane flags as doubles, no atomics.
//
// k_rows_to_lanes / k_lanes_to_rows: the caller's column-major [rows x count] arrays <-> [row][count]; the row counts here
// (36 (n - 1) or 49 (n - 1) for the gains) are beyond what the tiled pack kernels of kernels_util.hip take.
#include <hip/hip_runtime.h>

#include "indirect_kernel.hpp"
#include "wave_reduce.hpp"

namespace lto {

namespace {

__global__ __launch_bounds__(256) void k_rows_to_lanes(const double* aos, const long rows, const long count, double* soa) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // i = row * count + j: the stores coalesce
  if (i >= rows * count) return;
  const long row = i / count, j = i - row * count;
  soa[i] = aos[row + rows * j];
}

__global__ __launch_bounds__(256) void k_lanes_to_rows(const double* soa, const long rows, const long count, double* aos) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // the loads coalesce
  if (i >= rows * count) return;
  const long row = i / count, j = i - row * count;
  aos[row + rows * j] = soa[i];
}

template <int NX>
__global__ __launch_bounds__(64) void k_guidance_gains(const GainsArgs g) {
  constexpr int ND = 2 * NX, NE = NX * NX;
  static_assert(NE <= 64, "one element per lane of one wavefront");
  const int b = blockIdx.x;
  const int e = threadIdx.x;
  const bool el = e < NE;                        // the lanes behind the block carry zeros through every shuffle
  const int r = el ? e % NX : 0, c = el ? e / NX : 0;
  const int segs = g.n_nodes - 1;
  const double nan = __builtin_nan("");
  double kn = 0.0;                               // K_{k+1}[r][c]
  double dead = 0.0;                             // 2 or 3 once a node has failed: wave-uniform
  for (int k = segs - 1; k >= 0; --k) {
    const long s = (long)b * segs + k;
    double* Kout = g.K + NE * s;
    if (dead != 0.0) {
      if (el) Kout[e] = nan;
      if (g.pivot && e == 0) g.pivot[s] = nan;
      continue;
    }
    // Phi [ND ND][ldp], entry col * ND + row
    double A = 0.0, Bm = 0.0, Cm = 0.0, D = 0.0;
    if (el) {
      A = g.Phi[(long)(c * ND + r) * g.ldp + s];
      Bm = g.Phi[(long)((c + NX) * ND + r) * g.ldp + s];
      Cm = g.Phi[(long)(c * ND + r + NX) * g.ldp + s];
      D = g.Phi[(long)((c + NX) * ND + r + NX) * g.ldp + s];
    }
    double m, x;
    if (k == segs - 1) {
      if (NX == 7 && r == 6) {                   // the arrival condition d lambda_m = 0 in place of d m = 0
        m = D; x = -Cm;
      } else {
        m = Bm; x = -A;
      }
    } else {
      double kb = 0.0, ka = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        const double krj = __shfl(kn, r + NX * j, 64);
        kb = __builtin_fma(krj, __shfl(Bm, j + NX * c, 64), kb);
        ka = __builtin_fma(krj, __shfl(A, j + NX * c, 64), ka);
      }
      m = D - kb; x = ka - Cm;
    }
    if (!el) { m = 0.0; x = 0.0; }
    const double fin_in = wave_sum((m - m) + (x - x));
    const double mmax = wave_max(fabs(m));
    // LU with row pivoting, the right-hand sides carried along
    double umin = __builtin_huge_val();
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      int piv = p;
      double best = fabs(__shfl(m, p + NX * p, 64));
#pragma unroll
      for (int i = p + 1; i < NX; ++i) {
        const double v = fabs(__shfl(m, i + NX * p, 64));
        if (v > best) { best = v; piv = i; }
      }
      umin = fmin(umin, best);
      const int src = (r == p) ? piv : ((r == piv) ? p : r);
      m = __shfl(m, src + NX * c, 64);
      x = __shfl(x, src + NX * c, 64);
      const double upp = __shfl(m, p + NX * p, 64);
      const double l = __shfl(m, r + NX * p, 64) / upp;
      const double mp = __shfl(m, p + NX * c, 64), xp = __shfl(x, p + NX * c, 64);
      if (el && r > p) {
        m = (c > p) ? __builtin_fma(-l, mp, m) : 0.0;
        x = __builtin_fma(-l, xp, x);
      }
    }
    // back substitution, row by row from the last
#pragma unroll
    for (int i = NX - 1; i >= 0; --i) {
      double acc = __shfl(x, i + NX * c, 64);
#pragma unroll
      for (int j = NX - 1; j > i; --j) acc = __builtin_fma(-__shfl(m, i + NX * j, 64), __shfl(x, j + NX * c, 64), acc);
      const double uii = __shfl(m, i + NX * i, 64);
      if (el && r == i) x = acc / uii;
    }
    const double ratio = umin / mmax;
    const double fin_out = wave_sum(el ? (x - x) : 0.0);
    if (!(fin_in == 0.0)) dead = 2.0;                               // Phi (or the gain it is multiplied with) is not finite
    else if (!(ratio >= g.sing_tol)) dead = 3.0;
    else if (!(fin_out == 0.0)) dead = 2.0;
    if (g.pivot && e == 0) g.pivot[s] = (dead == 2.0 && !(fin_in == 0.0)) ? nan : ratio;
    if (el) Kout[e] = (dead != 0.0) ? nan : x;
    kn = x;
  }
  if (e == 0) g.status[b] = (int)dead;
}

template <int NX, int PM, int METHOD>
__global__ __launch_bounds__(64) void k_guided_flight(const IndirectArgs a, const GuidedArgs g) {
  constexpr int ND = 2 * NX, NE = NX * NX, DIM = ND + 1;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int B = g.n_batch;
  if (b >= B) return;
  using Sys = typename AugmentedSys<ND, PM>::type;
  static_assert(Sys::DIM == DIM, "state, costate and the quadrature of umag");
  Sys sys;
  sys.tp = a.tp[(long)b * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;
  const long nn = g.n_nom;
  const long h = (nn == 1) ? 0 : b;
  const double* nom = g.nom + h;                 // [(k ND + c)][n_nom]
  const double* Kd = g.K + h;                    // [(k NE + r + NX c)][n_nom]
  const double* tg = g.t + h;                    // [k][n_nom]
  const int n = g.n_nodes, every = g.every;
  double y[DIM];
#pragma unroll
  for (int c = 0; c < NX; ++c) y[c] = g.x0[(long)c * B + b];
#pragma unroll
  for (int c = 0; c < NX; ++c) y[NX + c] = nom[(long)(NX + c) * nn];
  y[ND] = 0.0;
  // per-lane flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler hazards")
  double failed = 0.0;
  int nacc = 0, nrej = 0;
  double dv = 0.0;
  if (g.nodes) {                                  // node 0: the start itself, bit for bit
#pragma unroll
    for (int c = 0; c < NX; ++c) g.nodes[(long)c * B + b] = y[c];
  }
  int k = 0, j = 0, next_upd = (every > 0) ? 0 : -1;
  for (; k < n - 1; ++k) {
    if (k == next_upd) {
      const double* nk = nom + (long)k * ND * nn;
      const double* Kk = Kd + (long)k * NE * nn;
      double dx[NX];
#pragma unroll
      for (int c = 0; c < NX; ++c) {
        dx[c] = y[c] - nk[(long)c * nn];
        if (g.nav) dx[c] += g.nav[((long)j * NX + c) * B + b];
      }
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NX; ++c) acc = __builtin_fma(Kk[(long)(r + NX * c) * nn], dx[c], acc);
        y[NX + r] = nk[(long)(NX + r) * nn] + acc;
      }
      ++j;
      next_upd += every;
    }
    const double span = tg[(long)(k + 1) * nn] - tg[(long)k * nn];
    double insum = span;                          // the start, the nominal's costate and the applied gain have to be finite
#pragma unroll
    for (int c = 0; c < ND; ++c) insum += y[c];
    if (!((insum - insum) == 0.0)) { failed = 1.0; break; }
    if constexpr (NX == 7) {                      // the span starts from the mass it has: m_k + y[6], y[6] = 0
      if (!(y[6] > 0.0)) { failed = 1.0; break; }
      sys.m_i = y[6];
      y[6] = 0.0;
    }
    y[ND] = 0.0;
    if (METHOD == M_RK4) {
      const double hs = span / (double)a.steps;
      for (int s = 0; s < a.steps; ++s) rk4_step(sys, hs, y);
      nacc += a.steps;
    } else {
      int na = 0, nr = 0;
      run_dop853<Sys, DIM>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr);
      nacc += na; nrej += nr;
    }
    if constexpr (NX == 7) y[6] = sys.m_i + y[6];
    double fin = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) fin += y[c];
    if (!((fin - fin) == 0.0)) { failed = 1.0; break; }
    dv += y[ND];
    if (g.nodes) {
#pragma unroll
      for (int c = 0; c < NX; ++c) g.nodes[((long)(k + 1) * NX + c) * B + b] = y[c];
    }
  }
  const double nan = __builtin_nan("");
  if (failed != 0.0 && g.nodes) {                 // the nodes from the failed span on
    for (int kk = k + 1; kk < n; ++kk) {
#pragma unroll
      for (int c = 0; c < NX; ++c) g.nodes[((long)kk * NX + c) * B + b] = nan;
    }
  }
#pragma unroll
  for (int c = 0; c < NX; ++c) g.x_final[(long)c * B + b] = (failed != 0.0) ? nan : y[c];
  if (g.lam_final) {
#pragma unroll
    for (int c = 0; c < NX; ++c) g.lam_final[(long)c * B + b] = (failed != 0.0) ? nan : y[NX + c];
  }
  g.dv[b] = (failed != 0.0) ? nan : dv;
  g.status[b] = (failed != 0.0) ? 2 : 0;
  g.nacc[b] = nacc;
  g.nrej[b] = nrej;
}

template <int NX, int METHOD>
hipError_t launch_guided_pm(int pm, const IndirectArgs& a0, const GuidedArgs& g, hipStream_t st) {
  dim3 grid((g.n_batch + 63) / 64);
  // every class is launched and the error state read once, behind the last launch (as launch_dense_pm)
  (void)for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) {
    hipLaunchKernelGGL((k_guided_flight<NX, decltype(cls)::value, METHOD>), grid, dim3(64), 0, st, a, g);
    return hipSuccess;
  });
  return hipGetLastError();
}

template <int NX>
hipError_t launch_guided_nx(int pm, int method, const IndirectArgs& a, const GuidedArgs& g, hipStream_t st) {
  if (method == M_RK4) return launch_guided_pm<NX, M_RK4>(pm, a, g, st);
  if (method == M_DOP853_ADAPTIVE) return launch_guided_pm<NX, M_DOP853_ADAPTIVE>(pm, a, g, st);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_rows_to_lanes(const double* aos, long rows, long count, double* soa, hipStream_t st) {
  const long total = rows * count;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rows_to_lanes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, aos, rows, count, soa);
  return hipGetLastError();
}

hipError_t launch_lanes_to_rows(const double* soa, long rows, long count, double* aos, hipStream_t st) {
  const long total = rows * count;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_lanes_to_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, soa, rows, count, aos);
  return hipGetLastError();
}

hipError_t launch_guidance_gains(const GainsArgs& g, hipStream_t st) {
  if (g.nx == 6) hipLaunchKernelGGL(k_guidance_gains<6>, dim3((unsigned)g.n_batch), dim3(64), 0, st, g);
  else if (g.nx == 7) hipLaunchKernelGGL(k_guidance_gains<7>, dim3((unsigned)g.n_batch), dim3(64), 0, st, g);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_guided_flight(int pm, int method, const IndirectArgs& a, const GuidedArgs& g, hipStream_t st) {
  if (g.nx == 6) return launch_guided_nx<6>(pm, method, a, g, st);
  if (g.nx == 7) return launch_guided_nx<7>(pm, method, a, g, st);
  return hipErrorInvalidValue;
}

}  // namespace lto
