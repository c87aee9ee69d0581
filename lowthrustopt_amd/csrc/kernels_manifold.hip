// kernels_manifold.hip -- invariant manifolds of periodic orbits of the CRTBP, gfx950: the hyperbolic pair of the
// monodromy matrix and its eigenvectors carried round the orbit (the seeds), ballistic arcs flown to a Poincare section (the hot
// path), and the nearest partner of every state of one set in another.
//
// k_manifold_eigen      one lane per orbit.  lambda_u and v_u by power iteration on M (Rayleigh quotient, the iterate's sign aligned
//                       with the one before it, so a negative lambda_u converges), v_s by inverse iteration on M - I / lambda_u (a
//                       6 x 6 LU with partial pivoting, rows exchanged by selects: every index is a compile-time constant and the
//                       matrix stays in registers), lambda_s the Rayleigh quotient of v_s.
// k_manifold_transport  one lane per (orbit, phase, kind): the base state with ONE variational vector, 12 components, the error
//                       norm over all of them (run_dop853).  The unstable vector flies forward over tau P, the stable one
//                       backward over (1 - tau) P as the time-reversed system over a positive span.
// k_manifold_starts     one lane per (orbit, phase): the orbit's status from the flags of all its flights, the starts X +- eps V
//                       (the product rounded, then the sum: what the host forms from the outputs), NaN for an orbit without result.
// k_section_flight      one lane per arc, 6 components, run_dop853_stop (dop853_lane.hpp) with a hook that counts the section's
//                       crossings, locates the last one asked for (the bisection of kernels_halo.hip's halo_crossing) and ends the
//                       flight there or at a step end inside r_min.
// k_state_match         one workgroup per state of A: a (distance, index) lexicographic minimum over Bs (the rule of k_stack_find).
//
// No LDS but the match's two reduction arrays, no atomics, plain vector stores; per-lane flags are doubles (DESIGN "Compiler hazards").
#include "kernels.hpp"
#include "crtbp_ballistic.hpp"

namespace lto {

namespace {

// The CRTBP without thrust and one variational vector, y = (r, v, c_r, c_v), c' = [0 I; G 2W] c (the expressions of kernels_halo.hip's
// SysHaloVar), times sgn = +-1: sgn = -1 is the time-reversed system, flown over a positive span.
struct SysCrtbpVarDir {
  static constexpr int DIM = 12;
  double MU, sgn;
  __device__ __forceinline__ void rhs(const double (&y)[12], double (&k)[12]) const {
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
    const double q1 = 3.0 * c1 * (i1 * i1), q2 = 3.0 * c2 * (i2 * i2), qs = q1 + q2;
    const double qa = __builtin_fma(q1, a, q2 * b);
    const double gxx = __builtin_fma(q1 * a, a, __builtin_fma(q2 * b, b, 1.0 - cs));
    const double gyy = __builtin_fma(qs * yy, yy, 1.0 - cs);
    const double gzz = __builtin_fma(qs * z, z, -cs);
    const double gxy = qa * yy, gxz = qa * z, gyz = qs * yy * z;
    k[6] = y[9]; k[7] = y[10]; k[8] = y[11];
    k[9] = __builtin_fma(gxx, y[6], __builtin_fma(gxy, y[7], __builtin_fma(gxz, y[8], 2.0 * y[10])));
    k[10] = __builtin_fma(gxy, y[6], __builtin_fma(gyy, y[7], __builtin_fma(gyz, y[8], -2.0 * y[9])));
    k[11] = __builtin_fma(gxz, y[6], __builtin_fma(gyz, y[7], gzz * y[8]));
#pragma unroll
    for (int i = 0; i < 12; ++i) k[i] *= sgn;
  }
};

// The ballistic CRTBP, y = (r, v), times sgn = +-1: SysCrtbpDir of crtbp_ballistic.hpp, with finite_all.

// Jacobi constant C = x^2 + y^2 + 2 (1 - MU) / r1 + 2 MU / r2 - v^2
__device__ __forceinline__ double jacobi6(const double MU, const double (&y)[6]) {
  const double a = y[0] + MU, b = a - 1.0;
  const double yz2 = __builtin_fma(y[1], y[1], y[2] * y[2]);
  const double r1 = sqrt(__builtin_fma(a, a, yz2)), r2 = sqrt(__builtin_fma(b, b, yz2));
  const double v2 = __builtin_fma(y[3], y[3], __builtin_fma(y[4], y[4], y[5] * y[5]));
  return __builtin_fma(y[0], y[0], y[1] * y[1]) + 2.0 * (1.0 - MU) / r1 + 2.0 * MU / r2 - v2;
}

// ---------------------------------------------------------------------------------------------------------------- 6 x 6 algebra
__device__ __forceinline__ void mat6_vec(const double (&A)[6][6], const double (&v)[6], double (&w)[6]) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s = __builtin_fma(A[r][c], v[c], s);
    w[r] = s;
  }
}
__device__ __forceinline__ double dot6(const double (&a)[6], const double (&b)[6]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) s = __builtin_fma(a[i], b[i], s);
  return s;
}
// w <- sign w / |w|_2 with the sign that makes w . v >= 0; returns max |w - v| and takes w over into v
__device__ __forceinline__ double unit6_step(double (&w)[6], double (&v)[6]) {
  const double n = sqrt(dot6(w, w));
  const double s = (dot6(w, v) < 0.0) ? -1.0 : 1.0;
  double move = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double u = s * (w[i] / n);
    const double d = fabs(u - v[i]);
    move = (d > move || d != d) ? d : move;     // a NaN stays
    v[i] = u;
  }
  return move;
}
// v_x > 0; v_x = 0 exactly: the component of largest magnitude positive (the first of equals)
__device__ __forceinline__ void sign_rule6(double (&v)[6]) {
  double big = v[0], s = v[0];
#pragma unroll
  for (int i = 1; i < 6; ++i) {
    if (fabs(v[i]) > fabs(big)) big = v[i];
  }
  if (s == 0.0) s = big;
  if (s < 0.0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = -v[i];
  }
}

// LU of C with partial pivoting, in place (L below the diagonal, unit diagonal implied); piv[k] = the row exchanged with row k.
// The exchange runs over the rows below k with a predicate, so no index depends on data.  Only the columns from k on are
// exchanged: the multipliers already stored left of them stay with the step that made them, which is what lu6_solve needs, since
// it exchanges and eliminates step by step (exchanging them too would ask for all exchanges of x before the first elimination).
// A pivot that is exactly 0 (the shift is an eigenvalue to the last bit) is replaced by `tiny`: inverse iteration wants the
// direction, not the size.
__device__ __forceinline__ void lu6(double (&C)[6][6], int (&piv)[6], const double tiny) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k;
    double best = fabs(C[k][k]);
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const double m = fabs(C[r][k]);
      if (m > best) { best = m; p = r; }
    }
    piv[k] = p;
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const bool ex = (r == p);
#pragma unroll
      for (int c = k; c < 6; ++c) {
        const double u = C[k][c], l = C[r][c];
        C[k][c] = ex ? l : u;
        C[r][c] = ex ? u : l;
      }
    }
    if (C[k][k] == 0.0) C[k][k] = tiny;
    const double d = C[k][k];
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const double l = C[r][k] / d;
      C[r][k] = l;
#pragma unroll
      for (int c = k + 1; c < 6; ++c) C[r][c] = __builtin_fma(-l, C[k][c], C[r][c]);
    }
  }
}
__device__ __forceinline__ void lu6_solve(const double (&C)[6][6], const int (&piv)[6], double (&x)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const bool ex = (r == piv[k]);
      const double u = x[k], l = x[r];
      x[k] = ex ? l : u;
      x[r] = ex ? u : l;
    }
#pragma unroll
    for (int r = k + 1; r < 6; ++r) x[r] = __builtin_fma(-C[r][k], x[k], x[r]);
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    double s = x[k];
#pragma unroll
    for (int c = k + 1; c < 6; ++c) s = __builtin_fma(-C[k][c], x[c], s);
    x[k] = s / C[k][k];
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ the eigen step
__global__ __launch_bounds__(64) void k_manifold_eigen(const ManifoldSeedArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  double A[6][6];
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
#pragma unroll
    for (int r = 0; r < 6; ++r) { A[r][c] = a.M[36 * (long)b + 6 * c + r]; sum += A[r][c]; }
  }
  double bad = ((sum - sum) == 0.0) ? 0.0 : 1.0;
  double vu[6] = {1.0, 0.9, 0.8, 0.7, 0.6, 0.5}, vs[6], w[6];
  double lu = __builtin_nan(""), ls = __builtin_nan("");
  if (bad == 0.0) {
    {
      const double n = sqrt(dot6(vu, vu));
#pragma unroll
      for (int i = 0; i < 6; ++i) vu[i] /= n;
    }
    double conv = 0.0;
    for (int it = 0; it < LTO_MANIFOLD_POWER_CAP && conv == 0.0; ++it) {
      mat6_vec(A, vu, w);
      if (unit6_step(w, vu) < 1e-15) conv = 1.0;
    }
    mat6_vec(A, vu, w);
    lu = dot6(vu, w);
    if (conv == 0.0 || !(fabs(lu) > 1.0)) bad = 1.0;
  }
  if (bad == 0.0) {
    const double sigma = 1.0 / lu;
    double Cm[6][6];
    int piv[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = 0; c < 6; ++c) Cm[r][c] = (r == c) ? A[r][c] - sigma : A[r][c];
    }
    lu6(Cm, piv, 2.220446049250313e-16 * fabs(lu));
    // the start: v_u mirrored in the xz-plane with time reversed -- the stable vector itself on a symmetric orbit, as good as any
    // other vector elsewhere
#pragma unroll
    for (int i = 0; i < 6; ++i) vs[i] = (i & 1) ? -vu[i] : vu[i];
    double conv = 0.0;
    for (int it = 0; it < LTO_MANIFOLD_INVERSE_CAP && conv == 0.0; ++it) {
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = vs[i];
      lu6_solve(Cm, piv, w);
      if (unit6_step(w, vs) < 1e-15) conv = 1.0;
    }
    mat6_vec(A, vs, w);
    ls = dot6(vs, w);
    if (!finite_all(vs) || !((ls - ls) == 0.0)) bad = 1.0;
  }
  sign_rule6(vu);
  sign_rule6(vs);
  const double nan = __builtin_nan("");
  double* v0 = a.vec0 + 12 * (long)b;
#pragma unroll
  for (int i = 0; i < 6; ++i) { v0[i] = (bad != 0.0) ? nan : vu[i]; v0[6 + i] = (bad != 0.0) ? nan : vs[i]; }
  a.lambda[2 * (long)b] = (bad != 0.0) ? nan : lu;
  a.lambda[2 * (long)b + 1] = (bad != 0.0) ? nan : ls;
  a.eig_flag[b] = bad;
}

// ------------------------------------------------------------------------------------------------------------------- the transport
template <int METHOD>
__global__ __launch_bounds__(64) void k_manifold_transport(const ManifoldSeedArgs a) {
  const long L = (long)blockIdx.x * 64 + threadIdx.x;
  if (L >= 2L * a.P * a.B) return;
  const int kind = (int)(L & 1);
  const long jb = L >> 1;
  const int b = (int)(jb / a.P), j = (int)(jb - (long)b * a.P);
  double y[12];
#pragma unroll
  for (int i = 0; i < 6; ++i) { y[i] = a.state0[6 * (long)b + i]; y[6 + i] = a.vec0[12 * (long)b + 6 * kind + i]; }
  const double Pb = a.period[b], tau = a.tau[j];
  double flag = 0.0;
  if (a.eig_flag[b] == 0.0) {
    if (!(Pb > 0.0) || !((Pb - Pb) == 0.0)) flag = 2.0;
    const double span = (tau == 0.0) ? 0.0 : ((kind == 0) ? tau * Pb : (1.0 - tau) * Pb);
    if (flag == 0.0 && span > 0.0) {
      SysCrtbpVarDir sys;
      sys.MU = a.MU;
      sys.sgn = (kind == 0) ? 1.0 : -1.0;
      if (METHOD == M_RK4) {
        const double h = span / (double)a.steps;
        for (int k = 0; k < a.steps; ++k) rk4_step(sys, h, y);
      } else {
        int na = 0, nr = 0;
        run_dop853<SysCrtbpVarDir, 12>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr);
      }
      // both vectors are unit vectors again at the phase
      const double n = sqrt(__builtin_fma(y[6], y[6], __builtin_fma(y[7], y[7], __builtin_fma(y[8], y[8],
                            __builtin_fma(y[9], y[9], __builtin_fma(y[10], y[10], y[11] * y[11]))))));
#pragma unroll
      for (int i = 6; i < 12; ++i) y[i] /= n;
    }
    if (!finite_all(y)) flag = 2.0;
  }
  a.fly_flag[L] = flag;
#pragma unroll
  for (int i = 0; i < 6; ++i) { a.X[6 * L + i] = y[i]; a.V[6 * L + i] = y[6 + i]; }
}

__global__ __launch_bounds__(64) void k_manifold_starts(const ManifoldSeedArgs a) {
#pragma clang fp contract(off)                 // X +- eps V as the host forms it: the product rounded, then the sum
  const long g = (long)blockIdx.x * 64 + threadIdx.x;
  if (g >= (long)a.P * a.B) return;
  const int b = (int)(g / a.P), j = (int)(g - (long)b * a.P);
  double st = (a.eig_flag[b] != 0.0) ? 1.0 : 0.0;
  if (st == 0.0) {
    const double* ff = a.fly_flag + 2L * a.P * b;
    for (int q = 0; q < 2 * a.P; ++q)
      if (ff[q] != 0.0) st = 2.0;
  }
  const double nan = __builtin_nan("");
  double* Xo = a.X + 12 * g;
  double* Vo = a.V + 12 * g;
  double* So = a.starts + 24 * g;
#pragma unroll
  for (int kind = 0; kind < 2; ++kind) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double x = (st != 0.0) ? nan : Xo[6 * kind + i], v = (st != 0.0) ? nan : Vo[6 * kind + i];
      const double ev = a.eps * v;
      So[6 * (2 * kind) + i] = x + ev;
      So[6 * (2 * kind + 1) + i] = x - ev;
      if (st != 0.0) { Xo[6 * kind + i] = nan; Vo[6 * kind + i] = nan; }
    }
  }
  if (j == 0) {
    a.status[b] = (int)st;
    if (st != 0.0) { a.lambda[2 * (long)b] = nan; a.lambda[2 * (long)b + 1] = nan; }
  }
}

hipError_t launch_manifold_seeds(int method, const ManifoldSeedArgs& a, hipStream_t st) {
  if (method != M_RK4 && method != M_DOP853_ADAPTIVE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_manifold_eigen, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_by_method(method, k_manifold_transport<M_RK4>, k_manifold_transport<M_DOP853_ADAPTIVE>, 2L * a.P * a.B, a, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_manifold_starts, dim3((unsigned)(((long)a.P * a.B + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- section flights
namespace {

// Component `axis` of y without a data-dependent index.  On the bit patterns: a chain of selects on the values is turned back into an
// indexed load by the compiler, which puts y into scratch memory.
__device__ __forceinline__ double pick6(const double (&y)[6], const int axis) {
  long long bits = 0;
#pragma unroll
  for (int q = 0; q < 6; ++q) bits |= __double_as_longlong(y[q]) & -(long long)(axis == q);
  return __longlong_as_double(bits);
}

// What an arc carries from step to step and from sample interval to sample interval.
struct ArcState {
  double side;      // the sign of g at the last point where g != 0; 0: none yet
  double status;    // -1 in flight; 0 / 3 set by the step that ended the arc
  double tc;        // the end, relative to the span's start
  double yc[6];
  int count;
};

// After an accepted step from time t over h to yn.  trial(th, yt): the state one step of length th from the step's start.
// Returns non-zero when the arc ends in this step (st.status, st.tc, st.yc set).
template <class Trial>
__device__ __forceinline__ double section_after_step(const SectionFlightArgs& a, ArcState& st, const double t, const double h,
                                                     const double (&yn)[6], Trial&& trial) {
  const double ge = pick6(yn, a.axis) - a.value;
  if (a.n_cross > 0 && (ge > 0.0 || ge < 0.0)) {
    const double sg = (ge > 0.0) ? 1.0 : -1.0;
    const double from = st.side;
    st.side = sg;
    if (from != 0.0 && sg != from && (a.dir == 0 || (double)a.dir == sg)) {
      ++st.count;
      if (st.count == a.n_cross) {
        // halo_crossing's bisection (kernels_halo.hip) on g: the bracket's ends down to adjacent doubles in time, the state from
        // one more trial step to its far end
        // (one call site for the trial step: the pass after the last halving is the one to the far end)
        double lo = 0.0, hi = 1.0, th = 0.5, closing = 0.0;
        double yt[6];
        for (int k = 0; k <= 60; ++k) {
          trial(th * h, yt);
          if (closing != 0.0) break;
          if (from * (pick6(yt, a.axis) - a.value) > 0.0) lo = th;
          else hi = th;
          const double t_lo = __builtin_fma(lo, h, t), t_hi = __builtin_fma(hi, h, t);
          if (k == 59 || !(t_hi > nextafter(t_lo, __builtin_huge_val()))) { closing = 1.0; th = hi; }
          else th = 0.5 * (lo + hi);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) st.yc[q] = yt[q];
        st.tc = __builtin_fma(hi, h, t);
        st.status = 0.0;
        return 1.0;
      }
    }
  }
  const double ax = yn[0] + a.MU, bx = ax - 1.0;
  const double yz2 = __builtin_fma(yn[1], yn[1], yn[2] * yn[2]);
  const double d1 = __builtin_fma(ax, ax, yz2), d2 = __builtin_fma(bx, bx, yz2);
  if (d1 < a.rmin1 * a.rmin1 || d2 < a.rmin2 * a.rmin2) {
#pragma unroll
    for (int q = 0; q < 6; ++q) st.yc[q] = yn[q];
    st.tc = t + h;
    st.status = 3.0;
    return 1.0;
  }
  return 0.0;
}

}  // namespace

template <int METHOD>
__global__ __launch_bounds__(64) void k_section_flight(const SectionFlightArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.N) return;
  SysCrtbpDir sys;
  sys.MU = a.MU;
  const double T = a.t_max[b];
  sys.sgn = (T < 0.0) ? -1.0 : 1.0;
  const double Tabs = fabs(T);
  double y[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) y[q] = a.y0[6 * (long)b + q];
  const double nan = __builtin_nan("");
  ArcState st;
  st.status = finite_all(y) ? -1.0 : 2.0;
  st.count = 0;
  st.tc = 0.0;
  {
    const double g0 = pick6(y, a.axis) - a.value;
    st.side = (g0 > 0.0) ? 1.0 : ((g0 < 0.0) ? -1.0 : 0.0);
  }
  const double C0 = jacobi6(a.MU, y);
  const int n = a.n_samples;
  const int nint = (n >= 2) ? n - 1 : 1;
  double* Xb = (n >= 2) ? a.X + 6 * (long)n * b : nullptr;
  if (n >= 2) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Xb[q] = y[q];
  }
  const double dt = Tabs / (double)nint;
  double tprev = 0.0, t_end = Tabs;
  for (int i = 1; i <= nint; ++i) {
    double reached = 0.0;                               // this interval's end was reached in flight
    if (st.status < 0.0) {
      const double ti = (i == nint) ? Tabs : (double)i * dt;
      const double span = ti - tprev;
      double done;
      if (METHOD == M_RK4) {
        done = (span > 0.0) ? 1.0 : 0.0;
        const double h = span / (double)a.steps;
        for (int k = 0; k < a.steps && done == 1.0; ++k) {
          double ys[6];
#pragma unroll
          for (int q = 0; q < 6; ++q) ys[q] = y[q];
          rk4_step(sys, h, y);
          const double stop = section_after_step(a, st, (double)k * h, h, y, [&](const double th, double (&yt)[6]) {
#pragma unroll
            for (int q = 0; q < 6; ++q) yt[q] = ys[q];
            rk4_step(sys, th, yt);
          });
          if (stop != 0.0) done = 2.0;
        }
      } else {
        int na = 0, nr = 0;
        done = run_dop853_stop<SysCrtbpDir, 6>(sys, span, a.rtol, a.atol, a.max_steps, y, na, nr,
            [&](const double t, const double h, const double (&ys)[6], double (&K)[13][6], const double (&yn)[6]) -> double {
          return section_after_step(a, st, t, h, yn, [&](const double th, double (&yt)[6]) {
            double E5, E3;
            (void)dop853_try<SysCrtbpDir, 6>(sys, th, a.rtol, a.atol, ys, K, yt, E5, E3);
          });
        });
      }
      if (done == 2.0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) y[q] = st.yc[q];
        t_end = tprev + st.tc;
      } else if (done == 1.0 && finite_all(y)) {
        tprev = ti;
        reached = 1.0;
      } else {
        st.status = 2.0;
      }
    }
    if (n >= 2) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Xb[6 * (long)i + q] = (reached != 0.0) ? y[q] : nan;
    }
  }
  if (st.status < 0.0) st.status = (a.n_cross == 0) ? 0.0 : 1.0;
  if (!finite_all(y)) st.status = 2.0;
  const bool fail = st.status == 2.0;
  if (fail && n >= 2) {
    for (int i = 0; i < n; ++i) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Xb[6 * (long)i + q] = nan;
    }
  }
  const double dC = fabs(jacobi6(a.MU, y) - C0);
#pragma unroll
  for (int q = 0; q < 6; ++q) a.x_end[6 * (long)b + q] = fail ? nan : y[q];
  a.t_end[b] = fail ? nan : sys.sgn * t_end;
  a.dC[b] = fail ? nan : dC;
  a.count[b] = st.count;
  a.status[b] = (int)st.status;
}

hipError_t launch_section_flight(int method, const SectionFlightArgs& a, hipStream_t st) {
  return launch_by_method(method, k_section_flight<M_RK4>, k_section_flight<M_DOP853_ADAPTIVE>, a.N, a, st);
}

// ------------------------------------------------------------------------------------------------------------------- nearest partner
constexpr int kMatchBlock = 256;
constexpr int kMatchNone = 0x7fffffff;

namespace {

__device__ __forceinline__ void match_min(double& d, int& j, const double d2, const int j2) {
  if (d2 < d || (d2 == d && j2 < j)) { d = d2; j = j2; }
}
// The two squared norms of a pair, every product and every sum rounded on its own, in the order include/lto.h states:
//   dr2 = (dx dx + dy dy) + dz dz,  dv2 = (dvx dvx + dvy dvy) + dvz dvz
__device__ __forceinline__ void match_norms(const double (&x)[6], const double* s, double& dr2, double& dv2) {
#pragma clang fp contract(off)
  double q[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { const double d = x[i] - s[i]; q[i] = d * d; }
  dr2 = (q[0] + q[1]) + q[2];
  dv2 = (q[3] + q[4]) + q[5];
}
// d = sqrt(dr2 + (w w) dv2), the product and the sum rounded on their own, the root correctly rounded
__device__ __forceinline__ double match_dist(const double dr2, const double dv2, const double w2) {
#pragma clang fp contract(off)
  const double p = w2 * dv2;
  return __dsqrt_rn(dr2 + p);
}

}  // namespace

__global__ __launch_bounds__(kMatchBlock) void k_state_match(const StateMatchArgs f) {
  const int ia = blockIdx.x, tid = threadIdx.x;
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = f.A[6 * (long)ia + q];
  const double w2 = f.w * f.w;
  double best = __builtin_inf();
  int jbest = kMatchNone;
  for (int j = tid; j < f.nB; j += kMatchBlock) {
    double dr2, dv2;
    match_norms(x, f.Bs + 6 * (long)j, dr2, dv2);
    const double d = match_dist(dr2, dv2, w2);
    if (d == d) match_min(best, jbest, d, j);            // a NaN distance never wins
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double d2 = __shfl_xor(best, off, 64);
    const int j2 = __shfl_xor(jbest, off, 64);
    match_min(best, jbest, d2, j2);
  }
  __shared__ double sd[kMatchBlock / 64];
  __shared__ int sj[kMatchBlock / 64];
  if ((tid & 63) == 0) { sd[tid >> 6] = best; sj[tid >> 6] = jbest; }
  __syncthreads();
  if (tid == 0) {
    double d = sd[0];
    int j = sj[0];
    for (int k = 1; k < kMatchBlock / 64; ++k) match_min(d, j, sd[k], sj[k]);
    const double nan = __builtin_nan("");
    double dr = nan, dv = nan;
    if (j == kMatchNone) { j = -1; d = nan; }
    else {
      double dr2, dv2;
      match_norms(x, f.Bs + 6 * (long)j, dr2, dv2);
      dr = __dsqrt_rn(dr2); dv = __dsqrt_rn(dv2);
    }
    f.index[ia] = j;
    f.dist[ia] = d;
    if (f.dr) f.dr[ia] = dr;
    if (f.dv) f.dv[ia] = dv;
  }
}

hipError_t launch_state_match(const StateMatchArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_state_match, dim3((unsigned)a.nA), dim3(kMatchBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace lto
