// kernels_replay.hip -- control replay: the 6- or 7-state flown under the control law of the indirect method with
// lambda_v(t) given as a natural cubic spline over an even time grid, from many starts at once.  The reference's
// CRTBP_prop_EP_NNControl_deriv! (src/CRTBP_prop_EP_deriv.jl:128-215) re-specified: the mass of :142 is lto_params.mass (6 states) or
// the current mass (7 states), and the flow rate of :195 is -kappa umag m, the law of the 14-row system.
//
// k_replay_moments: lane = (component, history).  The knots are LinRange(t0, t1, n_knots), so the moment system
// M_{i-1} + 4 M_i + M_{i+1} = 6 / h^2 (y_{i+1} - 2 y_i + y_{i-1}), M_0 = M_last = 0 has the host's Thomas factors cp[] for every
// lane (k_remesh_spline's sweeps).  Out: vm[(k * 6 + c * 2 + 0) * n_hist + hist] = the knot's value, [.. + 1] its moment.
//
// k_control_replay: lane = trajectory.  The lane integrates knot interval by knot interval -- inside one the control is ONE cubic,
// so the integrand is smooth and no step spans a knot -- every interval a span of its own with the start rule, trial step and step
// decision of every other DOP853 kernel here (run_dop853), or `steps` RK4 steps.  The system is autonomous: the interval's local
// time is one more state (s' = 1) behind the quadrature q' = umag, outside the error norm.  The interval's twelve cubic
// coefficients are formed once per interval from the two knots' values and moments: coalesced loads over the lanes when every
// start has its own history, one address for all lanes when there is one history.  No atomics, nothing shared between lanes: a
// trajectory's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include "indirect_kernel.hpp"

namespace lto {

namespace {

__global__ __launch_bounds__(64) void k_replay_moments(const double* lamv, const double* cp, double* mom, double* vm, const int m,
                                                      const int n_hist, const double h) {
  const int P = 3 * n_hist;
  const int pair = blockIdx.x * 64 + threadIdx.x;
  if (pair >= P) return;
  const int c = pair / n_hist, hist = pair - c * n_hist;
  const double* y = lamv + (long)hist * 3 * m + c;            // knot k at y[3 k]
  const double s6 = 6.0 / (h * h);
  // forward sweep: d'_i = (r_i - d'_{i-1}) cp_i, cp_i = 1 / (4 - cp_{i-1}), cp_0 = 0
  double dprev = 0.0, y0 = y[0], y1 = y[3];
  for (int i = 1; i < m - 1; ++i) {
    const double y2 = y[3 * (long)(i + 1)];
    const double ri = s6 * ((y2 - y1) - (y1 - y0));
    dprev = (ri - dprev) * cp[i];
    mom[(long)i * P + pair] = dprev;
    y0 = y1; y1 = y2;
  }
  // backward sweep: M_{m-2} = d'_{m-2}, M_i = d'_i - cp_i M_{i+1}; the values and moments go out knot by knot
  double mnext = 0.0;
  vm[((long)(m - 1) * 6 + c * 2) * n_hist + hist] = y[3 * (long)(m - 1)];
  vm[((long)(m - 1) * 6 + c * 2 + 1) * n_hist + hist] = 0.0;
  for (int i = m - 2; i >= 1; --i) {
    mnext = mom[(long)i * P + pair] - cp[i] * mnext;
    vm[((long)i * 6 + c * 2) * n_hist + hist] = y[3 * (long)i];
    vm[((long)i * 6 + c * 2 + 1) * n_hist + hist] = mnext;
  }
  vm[(long)(c * 2) * n_hist + hist] = y[0];
  vm[(long)(c * 2 + 1) * n_hist + hist] = 0.0;
}

// y = (x[NS], q, s): the state, the quadrature of umag and the interval's local time.  lambda_v(s) per component, with a = h - s and
// b = s:  a (A3 a^2 + A1) + b (B3 b^2 + B1),  A3 = M_i / (6 h), A1 = (y_i - M_i h^2 / 6) / h, B3 and B1 from knot i + 1 -- the form
// of k_remesh_spline with the divisions done once per interval.  NS = 7 carries the mass as m_i + y[6], y[6] = 0 at the interval's
// start (kernels_events.hip: a propagated mass near 1000 kg would be rounded to 1e-13 kg in every step).
template <int NS, int PM>
struct SysReplay {
  static constexpr int DIM = NS + 2;
  TrajParams tp;
  double h;
  double m_i;
  double A3[3], A1[3], B3[3], B1[3];
  __device__ __forceinline__ void rhs(const double (&y)[DIM], double (&k)[DIM]) const {
    const double MU = tp.MU;
    const double x = y[0], yy = y[1], z = y[2];
    const double w2 = 2.0 * tp.omega;
    const double a = x + MU, b = a - 1.0;
    const double yz2 = __builtin_fma(yy, yy, z * z);
    const double d1 = __builtin_fma(a, a, yz2), d2 = __builtin_fma(b, b, yz2);
    const double i1 = rsqrt_nr(d1), i2 = rsqrt_nr(d2);
    const double c1 = (1.0 - MU) * (i1 * i1 * i1), c2 = MU * (i2 * i2 * i2);
    const double cs = c1 + c2;
    const double sb = y[NS + 1], sa = h - sb;
    const double sa2 = sa * sa, sb2 = sb * sb;
    double l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) l[c] = __builtin_fma(sa, __builtin_fma(A3[c], sa2, A1[c]), sb * __builtin_fma(B3[c], sb2, B1[c]));
    const double n2 = __builtin_fma(l[0], l[0], __builtin_fma(l[1], l[1], l[2] * l[2]));
    const double inv_n = inv_norm_guarded(n2);
    const double n = n2 * inv_n;
    double aL = tp.accel_limit, mass = 0.0;
    if constexpr (NS == 7) { mass = m_i + y[6]; aL = tp.cT * rcp_nr(mass); }
    double m, ua, ub, un;
    bool tlim;
    control_dispatch<PM, false, true>(tp, aL, n, inv_n, m, ua, ub, un, tlim);
    k[0] = y[3]; k[1] = y[4]; k[2] = y[5];
    k[3] = __builtin_fma(-ua, l[0], __builtin_fma(-c1, a, __builtin_fma(-c2, b, __builtin_fma(w2, y[4], x))));
    k[4] = __builtin_fma(-ua, l[1], __builtin_fma(-cs, yy, __builtin_fma(-w2, y[3], yy)));
    k[5] = __builtin_fma(-ua, l[2], -cs * z);
    if constexpr (NS == 7) k[6] = (-tp.kappa_td * m) * mass;
    k[NS] = m;
    k[NS + 1] = 1.0;
  }
};

template <int NS, int PM, int METHOD>
__global__ __launch_bounds__(64) void k_control_replay(const IndirectArgs a, const ReplayArgs r) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int B = r.n_batch;
  if (b >= B) return;
  using Sys = SysReplay<NS, PM>;
  constexpr int D = Sys::DIM;
  Sys sys;
  sys.tp = a.tp[(long)b * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;
  const double h = r.h;
  sys.h = h;
  sys.m_i = 0.0;
  const double inv_h = 1.0 / h, h26 = h * h / 6.0, inv_6h = 1.0 / (6.0 * h);
  const long nh = r.n_hist;
  const double* vm = r.vm + (nh == 1 ? 0 : b);
  double y[D];
  double insum = 0.0;
#pragma unroll
  for (int c = 0; c < NS; ++c) { y[c] = r.x0[(long)c * B + b]; insum += y[c]; }
  y[NS] = 0.0;
  // per-lane flags are doubles (dop853_lane.hpp, DESIGN.md "Compiler hazards")
  double failed = ((insum - insum) == 0.0) ? 0.0 : 1.0;
  if (NS == 7 && !(y[NS - 1] > 0.0)) failed = 1.0;
  int nacc = 0, nrej = 0;
  const int ns = r.n_samples, every = r.sample_every;
  double* smp = r.samples ? r.samples + (long)b * ns : nullptr;      // [NS][ld_s], column b ns + j
  int j = 0;
  if (smp) {                                                          // knot 0: the start itself, bit for bit
#pragma unroll
    for (int c = 0; c < NS; ++c) smp[(long)c * r.ld_s] = y[c];
    j = 1;
  }
  const int last = r.n_knots - 1;
  double dv = 0.0;
  int i = 0;
  for (; i < last && failed == 0.0; ++i) {
    const double* v0 = vm + (long)i * 6 * nh;
    const double* v1 = v0 + 6 * nh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double yi = v0[(long)(2 * c) * nh], Mi = v0[(long)(2 * c + 1) * nh];
      const double yj = v1[(long)(2 * c) * nh], Mj = v1[(long)(2 * c + 1) * nh];
      sys.A3[c] = Mi * inv_6h;
      sys.B3[c] = Mj * inv_6h;
      sys.A1[c] = __builtin_fma(-Mi, h26, yi) * inv_h;
      sys.B1[c] = __builtin_fma(-Mj, h26, yj) * inv_h;
    }
    if constexpr (NS == 7) { sys.m_i = y[6]; y[6] = 0.0; }
    y[NS] = 0.0;
    y[NS + 1] = 0.0;
    if (METHOD == M_RK4) {
      const double hs = h / (double)a.steps;
      for (int k = 0; k < a.steps; ++k) rk4_step(sys, hs, y);
      nacc += a.steps;
    } else {
      int na = 0, nr = 0;
      run_dop853<Sys, NS + 1>(sys, h, a.rtol, a.atol, a.max_steps, y, na, nr);
      nacc += na; nrej += nr;
    }
    if constexpr (NS == 7) y[6] = sys.m_i + y[6];
    double fin = 0.0;
#pragma unroll
    for (int c = 0; c <= NS; ++c) fin += y[c];
    if (!((fin - fin) == 0.0)) failed = 1.0;
    if (NS == 7 && !(y[NS - 1] > 0.0)) failed = 1.0;
    if (failed != 0.0) break;
    dv += y[NS];
    const int knot = i + 1;
    if (smp && (knot == last || knot % every == 0)) {
#pragma unroll
      for (int c = 0; c < NS; ++c) smp[(long)c * r.ld_s + j] = y[c];
      ++j;
    }
  }
  const double nan = __builtin_nan("");
  if (failed != 0.0 && smp) {                                         // the samples from the failed interval on
    for (; j < ns; ++j) {
#pragma unroll
      for (int c = 0; c < NS; ++c) smp[(long)c * r.ld_s + j] = nan;
    }
  }
#pragma unroll
  for (int c = 0; c < NS; ++c) r.x_final[(long)c * B + b] = (failed != 0.0) ? nan : y[c];
  r.dv[b] = (failed != 0.0) ? nan : dv;
  r.status[b] = (failed != 0.0) ? 2 : 0;
  r.nacc[b] = nacc;
  r.nrej[b] = nrej;
}

template <int NS, int METHOD>
hipError_t launch_replay_pm(int pm, const IndirectArgs& a0, const ReplayArgs& r, hipStream_t st) {
  dim3 grid((r.n_batch + 63) / 64);
  // every class is launched and the error state read once, behind the last launch (as launch_dense_pm)
  (void)for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) {
    hipLaunchKernelGGL((k_control_replay<NS, decltype(cls)::value, METHOD>), grid, dim3(64), 0, st, a, r);
    return hipSuccess;
  });
  return hipGetLastError();
}

}  // namespace

hipError_t launch_replay_moments(const double* lamv, const double* cp, double* mom, double* vm, int n_knots, int n_hist, double h,
                                 hipStream_t st) {
  hipLaunchKernelGGL(k_replay_moments, dim3((3 * n_hist + 63) / 64), dim3(64), 0, st, lamv, cp, mom, vm, n_knots, n_hist, h);
  return hipGetLastError();
}

hipError_t launch_control_replay(int nstate, int pm, int method, const IndirectArgs& a, const ReplayArgs& r, hipStream_t st) {
  if (nstate == 6 && method == M_RK4) return launch_replay_pm<6, M_RK4>(pm, a, r, st);
  if (nstate == 6 && method == M_DOP853_ADAPTIVE) return launch_replay_pm<6, M_DOP853_ADAPTIVE>(pm, a, r, st);
  if (nstate == 7 && method == M_RK4) return launch_replay_pm<7, M_RK4>(pm, a, r, st);
  if (nstate == 7 && method == M_DOP853_ADAPTIVE) return launch_replay_pm<7, M_DOP853_ADAPTIVE>(pm, a, r, st);
  return hipErrorInvalidValue;
}

}  // namespace lto
