// kernels_events.hip -- switch times, burn arcs and dv of indirect solutions, gfx950.
//
// k_indirect_events: lane = segment.  The lane integrates the augmented state (y[12], q), q' = umag(|lambda_v|), q(t_i) = 0, over
// [t_i, t_{i+1}] with the plan's integrator (RK4 x steps, or DOP853 with all 13 components in the error norm), compares the engine's
// on-state at the two ends of every accepted step and, where it differs, brackets the crossing by trial steps of the same formula
// from the step's start state with length theta h: bisection in theta until the bracket's ends are adjacent doubles in absolute
// time, at most 60 halvings; t_event is the bracket's upper end (the first time on the new side).  Integration goes on from the
// accepted step unchanged -- the law is continuous, nothing restarts.  TWO crossings inside one accepted step leave the on-state
// at its ends equal and are not seen.  One launch per control-law class (kernels.hpp for_classes), per-segment records
// struct-of-arrays.
//
// k_events_compact: one wavefront per trajectory over its segments, 64 at a time: an exclusive scan of the per-segment counts (the
// joins included: where the on-state at the end of segment i differs from the one at the start of segment i+1, an event at
// t_{i+1}), an ordered gather into the trajectory's list, dv and burn_time as lane-strided partial sums closed by a butterfly.  No
// atomics: a trajectory's result does not depend on its batch.
//
// k_indirect_events<14>: the same lane for the 14-row variable-mass system, (y[14], q) with q' = umag as rhs14_base
// forms it, DOP853 with all 15 components in the error norm.  The threshold of p > 1 is formed from the state's CURRENT mass, and the
// lane leaves dm = m_i - m(t_{i+1}) with its records; k_events_compact sums it into `propellant` in the order of dv.
#include <hip/hip_runtime.h>

#include "indirect_kernel.hpp"
#include "wave_reduce.hpp"

namespace lto {

namespace {

// SysEvents, the augmented system (y[12], q), is in indirect_kernel.hpp: the guided flight (kernels_guidance.hip) integrates it too.

// Threshold of the event function g = |lambda_v| - thr: p = 1: 1 (more than half thrust); p > 1: p aL^(p-1) (clamped at the limit)
template <int PM>
__device__ __forceinline__ double event_threshold(const TrajParams& tp) {
  if (PM == PM_P1) return 1.0;
  if (PM == PM_P2) return 2.0 * tp.accel_limit;
  if (PM == PM_PGEN) return tp.p * pow(tp.accel_limit, tp.p - 1.0);
  return 0.0;
}
// the engine is on iff g > 0 (g == 0, and a NaN, are off); p = 0: always on.  A double, not a bool (dop853_lane.hpp).
template <int PM>
__device__ __forceinline__ double on_state(const double (&y)[13], const double thr) {
  if (PM == PM_P0) return 1.0;
  const double n2 = __builtin_fma(y[9], y[9], __builtin_fma(y[10], y[10], y[11] * y[11]));
  const double n = n2 * inv_norm_guarded(n2);
  return (n - thr > 0.0) ? 1.0 : 0.0;
}

// What a lane keeps of its segment while it steps.
struct SegEvents {
  double on;          // current on-state
  double tmark;       // since when it is on
  double ont;         // on-time so far
  double e0, e1, e2, e3;
  int nev;
  __device__ __forceinline__ void crossing(const double tev, const double on_new) {
    e0 = (nev == 0) ? tev : e0;
    e1 = (nev == 1) ? tev : e1;
    e2 = (nev == 2) ? tev : e2;
    e3 = (nev == 3) ? tev : e3;
    ++nev;
    if (on != 0.0) ont += tev - tmark;
    else tmark = tev;
    on = on_new;
  }
};

// The step from absolute time t0 over h changed the on-state from on_prev: bracket the crossing in theta.  trial(theta h, yt): the
// state one step of length theta h from the step's start state; on(yt): its on-state.
template <int D, class On, class Trial>
__device__ __forceinline__ double locate_crossing(const double t0, const double h, const double on_prev, On&& on, Trial&& trial) {
  double lo = 0.0, hi = 1.0;
  double t_hi = t0 + h;
  for (int k = 0; k < 60; ++k) {
    const double mid = 0.5 * (lo + hi);
    double yt[D];
    trial(mid * h, yt);
    if (on(yt) == on_prev) lo = mid;
    else hi = mid;
    const double t_lo = __builtin_fma(lo, h, t0);
    t_hi = __builtin_fma(hi, h, t0);
    if (!(t_hi > nextafter(t_lo, __builtin_huge_val()))) break;     // adjacent doubles (or the same one)
  }
  return t_hi;
}

// ---------------------------------------------------------------------------------------- the variable-mass system
// The lane carries the mass as m_i + y[6], y[6](t_i) = 0: a segment burns 1e-5 .. 1e-2 of the mass, and a propagated m near
// 1000 kg is rounded to eps m = 1.1e-13 kg in every step, so m_i - m(t_{i+1}) formed from it is good to eps m / dm only (measured:
// 2.6e-12 relative on 0.04 kg).  The RHS and the event function see m_i + y[6]; the propagated mass is m(t_{i+1}) = m_i + y[6],
// and dm = m_i - m(t_{i+1}) is -y[6] with the digits that sum would round away -- unless the sum IS m_i: a segment that does not
// move the mass by half a unit of its last place has burned nothing, dm = 0 (Isp -> infinity: the constant-mass system).
// SysEventsMass itself lives in indirect_kernel.hpp beside SysEvents: the guided flight of 14-row solutions carries it too.

// g = |lambda_v| - thr(m) > 0 with the state's own mass: p = 1: thr = 1; p > 1: thr = p (cT / m)^(p-1).  A NaN (a mass of 0 makes
// one) is off.
template <int PM>
__device__ __forceinline__ double on_state_mass(const double (&y)[15], const TrajParams& tp, const double m_i) {
  if (PM == PM_P0) return 1.0;
  const double mass = m_i + y[6];
  const double n2 = __builtin_fma(y[10], y[10], __builtin_fma(y[11], y[11], y[12] * y[12]));
  const double n = n2 * inv_norm_guarded(n2);
  double thr = 1.0;
  if (PM == PM_P2) thr = 2.0 * (tp.cT * rcp_nr(mass));
  if (PM == PM_PGEN) thr = tp.p * pow(tp.cT * rcp_nr(mass), tp.p - 1.0);
  return (n - thr > 0.0) ? 1.0 : 0.0;
}

// ND = 12: (y[12], q) under SysEvents.  ND = 14: (y[14], q) under SysEventsMass, the on-state from the current mass, and dm.
template <int ND, int PM, int METHOD>
__global__ __launch_bounds__(64) void k_indirect_events(const IndirectArgs a, const EventsArgs ev) {
  constexpr int D = ND + 1;
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= a.S) return;
  const int traj = s / a.seg_per_traj;
  const int i = s - traj * a.seg_per_traj;
  const long node = (long)traj * a.n_nodes + i;
  const long tg = (long)traj * a.t_stride + i;
  using Sys = typename AugmentedSys<ND, PM>::type;
  static_assert(Sys::DIM == D, "state, costate and the quadrature of umag");
  Sys sys;
  sys.tp = a.tp[(long)traj * a.tp_stride];
  if (a.class_filter && p_class(sys.tp.p) != PM) return;
  double thr = 0.0;
  if constexpr (ND == 12) thr = event_threshold<PM>(sys.tp);
  const auto on_of = [&](const double (&yt)[D]) {
    if constexpr (ND == 12) return on_state<PM>(yt, thr);
    else return on_state_mass<PM>(yt, sys.tp, sys.m_i);
  };
  double y[D];
  double next_sum = 0.0;                          // node i + 1 only has to be finite (and its mass positive, below)
#pragma unroll
  for (int c = 0; c < ND; ++c) { y[c] = a.X[c * a.ldx + node]; next_sum += a.X[c * a.ldx + node + 1]; }
  y[ND] = 0.0;
  if constexpr (ND == 14) { sys.m_i = y[6]; y[6] = 0.0; }
  const double ta = a.t[tg], tb = a.t[tg + 1];
  const double span = tb - ta;
  SegEvents se;
  se.on = on_of(y);
  se.tmark = ta; se.ont = 0.0; se.nev = 0;
  se.e0 = se.e1 = se.e2 = se.e3 = __builtin_nan("");
  const double on_start = se.on;

  if (METHOD == M_RK4) {
    const double h = span / (double)a.steps;
    for (int k = 0; k < a.steps; ++k) {
      double y0[D];
#pragma unroll
      for (int c = 0; c < D; ++c) y0[c] = y[c];
      rk4_step(sys, h, y);
      if (PM != PM_P0) {
        const double on1 = on_of(y);
        if (on1 != se.on) {
          const double tev = locate_crossing<D>(__builtin_fma((double)k, h, ta), h, se.on, on_of, [&](const double th, double (&yt)[D]) {
#pragma unroll
            for (int c = 0; c < D; ++c) yt[c] = y0[c];
            rk4_step(sys, th, yt);
          });
          se.crossing(tev, on1);
        }
      }
    }
  } else {
    int nacc = 0, nrej = 0;
    run_dop853_stop<Sys, D>(sys, span, a.rtol, a.atol, a.max_steps, y, nacc, nrej,
                            [&](const double t, const double h, const double (&y0)[D], double (&K)[13][D], const double (&yn)[D]) {
      if (PM == PM_P0) return 0.0;
      const double on1 = on_of(yn);
      if (on1 != se.on) {
        const double tev = locate_crossing<D>(ta + t, h, se.on, on_of, [&](const double th, double (&yt)[D]) {
          double E5, E3;
          (void)dop853_try<Sys, D>(sys, th, a.rtol, a.atol, y0, K, yt, E5, E3);
        });
        se.crossing(tev, on1);
      }
      return 0.0;
    });
  }
  if (se.on != 0.0) se.ont += tb - se.tmark;
  double fin = next_sum;
#pragma unroll
  for (int c = 0; c < D; ++c) fin += y[c];
  fin += se.ont;
  bool finite;
  double dm = 0.0;
  if constexpr (ND == 14) {
    // the masses of the segment's two nodes, read again here instead of a flag kept across the integration: finite and positive
    // (a NaN fails the comparison, an infinity the finite sum)
    const double m_i = a.X[6 * a.ldx + node], m_n = a.X[6 * a.ldx + node + 1];
    finite = ((fin + m_i) - (fin + m_i)) == 0.0 && m_i > 0.0 && m_n > 0.0;
    dm = (m_i + y[6] == m_i) ? 0.0 : -y[6];
  } else {
    finite = (fin - fin) == 0.0;
  }
  const long S = a.S;
  ev.tev[0 * S + s] = se.e0; ev.tev[1 * S + s] = se.e1; ev.tev[2 * S + s] = se.e2; ev.tev[3 * S + s] = se.e3;
  ev.q[s] = finite ? y[ND] : __builtin_nan("");
  ev.ont[s] = finite ? se.ont : __builtin_nan("");
  if constexpr (ND == 14) ev.dm[s] = finite ? dm : __builtin_nan("");
  ev.nev[s] = se.nev;
  ev.on_s[s] = (on_start != 0.0) ? 1 : 0;
  ev.on_e[s] = (se.on != 0.0) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_events_compact(const IndirectArgs a, const EventsArgs ev, const int n_batch) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_batch) return;
  const int nseg = a.seg_per_traj, M = ev.max_events;
  const long s0 = (long)b * nseg, S = a.S;
  const double* tg = a.t + (long)b * a.t_stride;
  double* t_out = ev.t_event + (long)b * M;
  int* k_out = ev.kind + (long)b * M;
  // dv and burn_time: lane l sums the segments l, l + 64, .. in order, then the butterfly
  double pq = 0.0, pt = 0.0;
  for (int i = lane; i < nseg; i += 64) { pq += ev.q[s0 + i]; pt += ev.ont[s0 + i]; }
  const double dv = wave_sum(pq), bt = wave_sum(pt);
  double pm = 0.0;                               // the variable-mass form: the segments' dm, summed as q is
  if (ev.dm)
    for (int i = lane; i < nseg; i += 64) pm += ev.dm[s0 + i];
  const double prop = wave_sum(pm);
  const bool bad = !((dv - dv) == 0.0 && (bt - bt) == 0.0 && (prop - prop) == 0.0);
  int base = 0, limit = M, over = 0;
  if (!bad) {
    for (int c0 = 0; c0 < nseg; c0 += 64) {
      const int i = c0 + lane;
      const bool valid = i < nseg;
      const long s = s0 + (valid ? i : 0);
      const int nv = valid ? ev.nev[s] : 0;
      const int os = valid ? ev.on_s[s] : 0;
      const int join = (valid && i + 1 < nseg && ev.on_e[s] != ev.on_s[s + 1]) ? 1 : 0;
      const int cnt = nv + join;
      const int incl = wave_scan_incl(cnt, lane);
      const int first = base + incl - cnt;
      // a segment with more crossings than it keeps: the list ends ahead of the first one that is missing
      const int hole = wave_min(nv > kEventsPerSeg ? first + kEventsPerSeg : 0x7fffffff);
      if (hole < limit) limit = hole;
      if (hole != 0x7fffffff) over = 1;
      const int kept = nv < kEventsPerSeg ? nv : kEventsPerSeg;
      for (int k = 0; k < kept; ++k) {
        const int pos = first + k;
        if (pos < limit) { t_out[pos] = ev.tev[(long)k * S + s]; k_out[pos] = ((os + k) & 1) ? -1 : 1; }
      }
      if (join) {
        const int pos = first + nv;
        if (pos < limit) { t_out[pos] = tg[i + 1]; k_out[pos] = ev.on_s[s + 1] ? 1 : -1; }
      }
      base += __shfl(incl, 63, 64);
    }
  }
  const int listed = bad ? 0 : (base < limit ? base : limit);
  for (int p = listed + lane; p < M; p += 64) { t_out[p] = __builtin_nan(""); k_out[p] = 0; }
  if (ev.dv_seg)
    for (int i = lane; i < nseg; i += 64) ev.dv_seg[s0 + i] = bad ? __builtin_nan("") : ev.q[s0 + i];
  if (ev.dm_seg)
    for (int i = lane; i < nseg; i += 64) ev.dm_seg[s0 + i] = bad ? __builtin_nan("") : ev.dm[s0 + i];
  if (lane == 0) {
    if (ev.propellant) ev.propellant[b] = bad ? __builtin_nan("") : prop;
    ev.n_events[b] = bad ? 0 : base;
    ev.on0[b] = bad ? 0 : ev.on_s[s0];
    ev.dv[b] = bad ? __builtin_nan("") : dv;
    ev.burn[b] = bad ? __builtin_nan("") : bt;
    ev.status[b] = bad ? 2 : ((base > M || over) ? 1 : 0);
  }
}

template <int ND, int METHOD>
hipError_t launch_events_pm(int pm, const IndirectArgs& a0, const EventsArgs& e, hipStream_t st) {
  dim3 grid((a0.S + 63) / 64);
  // every class is launched and the error state read once, behind the last launch (as launch_dense_pm)
  (void)for_classes<PM_P0, PM_P1, PM_P2, PM_PGEN>(pm, a0, [&](auto cls, const IndirectArgs& a) {
    hipLaunchKernelGGL((k_indirect_events<ND, decltype(cls)::value, METHOD>), grid, dim3(64), 0, st, a, e);
    return hipSuccess;
  });
  return hipGetLastError();
}

template <int ND>
hipError_t launch_events_nd(int pm, int method, const IndirectArgs& a, const EventsArgs& e, hipStream_t st) {
  if (method == M_RK4) return launch_events_pm<ND, M_RK4>(pm, a, e, st);
  if (method == M_DOP853_ADAPTIVE) return launch_events_pm<ND, M_DOP853_ADAPTIVE>(pm, a, e, st);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_indirect_events(int nd, int pm, int method, const IndirectArgs& a, const EventsArgs& e, hipStream_t st) {
  if (nd == 12) return launch_events_nd<12>(pm, method, a, e, st);
  if (nd == 14 && e.dm && e.propellant) return launch_events_nd<14>(pm, method, a, e, st);
  return hipErrorInvalidValue;
}

hipError_t launch_events_compact(const IndirectArgs& a, const EventsArgs& e, int n_batch, hipStream_t st) {
  hipLaunchKernelGGL(k_events_compact, dim3(n_batch), dim3(64), 0, st, a, e, n_batch);
  return hipGetLastError();
}

}  // namespace lto
