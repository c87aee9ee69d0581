// kernels_direct_qp.hip -- the QP step of direct multiple shooting on the device (optimizeTraj of
// src/multiShoot_CRTBP_direct.jl:248-403 for the reference demo's setting: flagEnd = false, beta = 0, tf fixed).
//
// With the end points frozen, the thrust bound commented out (:305-317) and tf_jump = 0 (:292) the subproblem is a convex QP
// with equality constraints only:
//   min  sum_k w_k |u_k + du_k|^2 + (DU/TU)^2 (|dV1 + d1|^2 + |dV2 + d2|^2)            (:323-326, :377-380)
//   s.t. E_i dx_i + F_i dx_{i+1} + G_i du_i + H_i du_{i+1} = -defect_i                    (:337)
//        x_0[0:6] + dx_0[0:6] + [0; dV1 + d1] = s0,  x_{n-1}[0:6] + dx_{n-1}[0:6] + [0; dV2 + d2] = sf      (:370-375)
//        x_0[6] + dx_0[6] = mass (nstate 7, :269-271);   d1 = d2 = 0 unless allowImpulsive (:298-302).
// Its optimality conditions, WITHOUT eliminating anything, are a square block-bidiagonal two-point BVP in the node vector
// y_k = (dx_k, du_k, lambda_k), NB = 2 ns + 3 unknowns per node (lambda_k = multiplier of defect k, lambda_{n-1} a dummy pinned
// to 0).  Block row i (NB rows) couples y_i and y_{i+1}: defect constraint i, stationarity in du_{i+1}
// (2 w (u + du) + H_i^T l_i + G_{i+1}^T l_{i+1} = 0) and in dx_{i+1} (F_i^T l_i + E_{i+1}^T l_{i+1} = 0); a pinned component's
// stationarity row is its pin instead; with allowImpulsive the impulse is eliminated through the velocity pin and the row carries
// the 2 (DU/TU)^2 term.  Node 0 contributes ns + 3 boundary rows (its stationarity / pins), node n-1 ns rows (lambda = 0).
//
// Solved like the indirect Newton step (kernels_bvp.hip): STRUCTURED ORTHOGONAL cyclic reduction.  At every level adjacent block
// rows are stacked, the 2NB x NB column block of their shared node is triangularised by Householder reflections (one wavefront per
// pair, lane = column, reflector broadcast by v_readlane), the top NB rows are kept for back-substitution and the bottom NB rows
// are the new block row.  The shared node's block [B_top; A_bottom] always has full column rank: B_i is block triangular with
// diagonal blocks F_i, 2 w I and E_{i+1}^T (state-transition derivatives, invertible), and a merged row's B inherits that.  The
// last level leaves one block row on (y_0, y_{n-1}); with the two boundary blocks that is a 2NB x 2NB system, triangularised the
// same way in one wavefront per trajectory.  Orthogonal transformations only -- no products of STMs (kernels_bvp.hip:10-13).
//
// Scaling: rows mix nondimensional states with controls in N (G ~ 1e-5 per N, w ~ 0.1 TU).  Per trajectory, with g = max |G|,|H|
// and w = max dt, the unknowns are du = s_u u~, lambda = s_l l~ and the stationarity rows are multiplied by r_u (du) and r_x = 1/s_l
// (dx): s_u = 1/g, r_u = g/(2w), s_l = 2w/g^2, all rounded to powers of two (exact).  Every block is then O(1).
#include "kernels.hpp"
#include "orbit_spline.hpp"
#include <type_traits>

namespace lto {

// NR right-hand sides: 1 for the frozen-end step, 3 for the free-end step (z0 | dz/dp1 | dz/dp2, kernels below and DESIGN 4.8c),
// 4 for the free-end step with a free time of flight (... | dz/dp3, p3 = tf_jump)
template <int NS, int NR = 1>
struct QpDims {
  static constexpr int NB = 2 * NS + 3;          // unknowns per node: dx (NS), du (3), lambda (NS)
  static constexpr int R2 = 2 * NB;              // rows of a pair's stack
  static constexpr int NCOLS = 3 * NB + NR;      // mid | left | right | rhs (NR)
  static constexpr int ROW = 2 * NB * NB + NR * NB;   // A (NB x NB), B (NB x NB), r (NB x NR), column-major
  static constexpr int REC_R = 0, REC_CA = NB * NB, REC_CB = 2 * NB * NB, REC_G = 3 * NB * NB, REC = 3 * NB * NB + NR * NB;
  static_assert(NCOLS <= 64, "one wavefront per pair");
};

struct QpArgs {
  int n_nodes, n_batch, S_traj;
  const double* Jac; long ldj;       // the Jacobian sweep's SoA outputs: Jac[(col*NS+row)*ldj + s]
  const double* defect; long ldd;
  const double* X; long ldx;
  const double* U; long ldu;
  const double* t; int t_stride;
  const double* tg;                  // targets [n_batch][QP_TARGET]: s0[6], sf[6], mass, dV1[3], dV2[3]
  int impulsive;
  double c2;                         // (DU/TU)^2
  unsigned long long* gw;            // [n_batch][2]: bits of max |G|,|H| and of max dt (non-negative doubles order as integers)
  double* rec;                       // [n_batch][n_nodes][REC]
  double* Y; long ldy;               // solution, scaled unknowns: Y[(m*NB + c)*ldy + b*n_nodes + k], m = right-hand side
  int* status;                       // [n_batch]: 0 ok, 1 singular KKT system
  const double* em;                  // free ends only: end model [n_batch][QP_MODEL]: g0[6], gf[6], |c0|, |cf| (lto_direct_end_model)
  const double* beta;                // free ends only: [n_batch]
};
// free time of flight (NR = 4): the tf column of the sweep and the per-trajectory bounds.  A separate type, so that the kernels of
// NR = 1 and 3 keep their argument layout.
struct QpArgsTf : QpArgs {
  const double* dtf;                 // d defect / d tf [NS][ldd] (the Jacobian sweep's tf column)
  const double* tfb;                 // [n_batch][3]: step, tf_min, tf_max (lto_direct_tf_bounds, TU)
  const double* tf;                  // [n_batch]: the current tf of every trajectory
};
template <int NR>
using QpA = std::conditional_t<NR == 4, QpArgsTf, QpArgs>;
constexpr int QP_TARGET = 19;
constexpr int QP_MODEL = 14;
constexpr double QP_PBOUND = 0.1;    // |p1|, |p2| <= 0.1 (:280-284)

struct QpScale { double su, ru, sl, rx; };
__device__ __forceinline__ double pow2_near(const double v) { return ldexp(1.0, ilogb(v)); }
__device__ __forceinline__ QpScale qp_scale(const QpArgs& a, const int b) {
  double g = __longlong_as_double((long long)a.gw[2 * b]), w = __longlong_as_double((long long)a.gw[2 * b + 1]);
  if (!(g > 0.0) || !(g < 1e300)) g = 1.0;
  if (!(w > 0.0) || !(w < 1e300)) w = 1.0;
  QpScale s;
  s.su = pow2_near(1.0 / g);
  s.ru = pow2_near(g / (2.0 * w));
  s.sl = pow2_near(2.0 * w / (g * g));
  s.rx = 1.0 / s.sl;
  return s;
}
__device__ __forceinline__ double qp_weight(const QpArgs& a, const int b, const int k) {   // trapezoid weight of node k (:323-326)
  const double* t = a.t + (long)b * a.t_stride;
  double w = 0.0;
  if (k > 0) w += 0.5 * (t[k] - t[k - 1]);
  if (k < a.n_nodes - 1) w += 0.5 * (t[k + 1] - t[k]);
  return w;
}

// ---- per-trajectory scale inputs: max |G|,|H| over the segments, max dt
template <int NS>
__global__ __launch_bounds__(256) void k_qp_gmax(QpArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  double g = 0.0, w = 0.0;
  if (i < a.S_traj) {
    const long s = (long)b * a.S_traj + i;
#pragma unroll
    for (int col = 2 * NS; col < 2 * NS + 6; ++col)
#pragma unroll
      for (int r = 0; r < NS; ++r) g = fmax(g, fabs(a.Jac[(long)(col * NS + r) * a.ldj + s]));
    const double* t = a.t + (long)b * a.t_stride;
    w = fabs(t[i + 1] - t[i]);
  }
  for (int off = 32; off > 0; off >>= 1) { g = fmax(g, __shfl_xor(g, off)); w = fmax(w, __shfl_xor(w, off)); }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&a.gw[2 * b], (unsigned long long)__double_as_longlong(g));
    atomicMax(&a.gw[2 * b + 1], (unsigned long long)__double_as_longlong(w));
  }
}

// ---- element (r, cc) of the level-0 block row i of trajectory b: cc < NB column of y_i, cc < 2NB column of y_{i+1}, cc = 2NB rhs
template <int NS>
__device__ double qp_elem0(const QpArgs& a, const QpScale& sc, const int b, const int i, const int r, const int cc) {
  constexpr int NB = QpDims<NS>::NB;
  const long s = (long)b * a.S_traj + i;
  const int k = i + 1;
  const bool last = (k == a.n_nodes - 1);
  const long node = (long)b * a.n_nodes + k;
  const bool isA = cc < NB, isB = (cc >= NB && cc < 2 * NB);
  const int c = isA ? cc : cc - NB;
  auto J = [&](const long seg, const int row, const int col) { return a.Jac[(long)(col * NS + row) * a.ldj + seg]; };
  if (r < NS) {                                   // defect constraint i (:337)
    if (!isA && !isB) return -a.defect[(long)r * a.ldd + s];
    if (c < NS) return J(s, r, isA ? c : NS + c);
    if (c < NS + 3) return sc.su * J(s, r, (isA ? 2 * NS : 2 * NS + 3) + c - NS);
    return 0.0;
  }
  if (r < NS + 3) {                               // stationarity in du_{i+1}, scaled by r_u
    const int q = r - NS;
    if (isA) return (c >= NS + 3) ? sc.ru * sc.sl * J(s, c - NS - 3, 2 * NS + 3 + q) : 0.0;
    const double wk = qp_weight(a, b, k);
    if (isB) {
      if (c == NS + q) return sc.ru * 2.0 * wk * sc.su;
      if (c >= NS + 3 && !last) return sc.ru * sc.sl * J(s + 1, c - NS - 3, 2 * NS + q);
      return 0.0;
    }
    return -sc.ru * 2.0 * wk * a.U[(long)q * a.ldu + node];
  }
  const int j = r - NS - 3;                       // stationarity in dx_{i+1}, scaled by r_x -- or the terminal pin
  const double* tg = a.tg + (long)b * QP_TARGET;
  if (last && (j < 3 || (j < 6 && !a.impulsive))) {
    if (isA) return 0.0;
    if (isB) return (c == j) ? 1.0 : 0.0;
    return tg[6 + j] - a.X[(long)j * a.ldx + node] - (j >= 3 ? tg[16 + j - 3] : 0.0);
  }
  if (isA) return (c >= NS + 3) ? J(s, c - NS - 3, NS + j) : 0.0;
  if (isB) {
    if (!last) return (c >= NS + 3) ? J(s + 1, c - NS - 3, j) : 0.0;
    return (j < 6 && c == j) ? 2.0 * a.c2 * sc.rx : 0.0;            // impulse eliminated through the velocity pin
  }
  return (last && j < 6) ? sc.rx * 2.0 * a.c2 * (tg[6 + j] - a.X[(long)j * a.ldx + node]) : 0.0;
}

// ---- element (r, c) of node 0's boundary block (NS + 3 rows on y_0; c = NB: rhs)
template <int NS>
__device__ double qp_elem_bc0(const QpArgs& a, const QpScale& sc, const int b, const int r, const int c) {
  constexpr int NB = QpDims<NS>::NB;
  const long node = (long)b * a.n_nodes, s = (long)b * a.S_traj;
  auto J = [&](const int row, const int col) { return a.Jac[(long)(col * NS + row) * a.ldj + s]; };
  const double* tg = a.tg + (long)b * QP_TARGET;
  if (r < 3) {                                    // stationarity in du_0
    const double w0 = qp_weight(a, b, 0);
    if (c == NS + r) return sc.ru * 2.0 * w0 * sc.su;
    if (c >= NS + 3 && c < NB) return sc.ru * sc.sl * J(c - NS - 3, 2 * NS + r);
    if (c == NB) return -sc.ru * 2.0 * w0 * a.U[(long)r * a.ldu + node];
    return 0.0;
  }
  const int j = r - 3;
  if (j == 6) {                                   // initial mass (:269-271)
    if (c == NB) return tg[12] - a.X[6 * a.ldx + node];
    return (c == 6) ? 1.0 : 0.0;
  }
  if (j < 3 || !a.impulsive) {
    if (c == NB) return tg[j] - a.X[(long)j * a.ldx + node] - (j >= 3 ? tg[13 + j - 3] : 0.0);
    return (c == j) ? 1.0 : 0.0;
  }
  if (c >= NS + 3 && c < NB) return J(c - NS - 3, j);
  if (c == j) return 2.0 * a.c2 * sc.rx;
  if (c == NB) return sc.rx * 2.0 * a.c2 * (tg[j] - a.X[(long)j * a.ldx + node]);
  return 0.0;
}

// ---- free ends: the extra right-hand sides m = 1 (d/dp1) and m = 2 (d/dp2).  The end targets s0 + g0 p1 and sf + gf p2 enter
// only the pins of node 0 and node n-1 and, with impulses, the velocity rows through which the impulse is eliminated.  With a free
// tf (NR = 4), m = 3 (d/dp3): the defect rows of segment i read J z + dtf_i p3 = -defect_i, so the column is -dtf_i there (unscaled,
// like the defect column) and zero elsewhere -- the end targets do not depend on tf.
template <int NS, int NR>
__device__ double qp_elem0_free(const QpA<NR>& a, const QpScale& sc, const int b, const int i, const int r, const int m) {
  if constexpr (NR == 4) {
    if (m == 3) return (r < NS) ? -a.dtf[(long)r * a.ldd + (long)b * a.S_traj + i] : 0.0;
  }
  const int j = r - NS - 3;
  if (m != 2 || i + 2 != a.n_nodes || j < 0 || j >= 6) return 0.0;
  const double gf = a.em[(long)b * QP_MODEL + 6 + j];
  return (j < 3 || !a.impulsive) ? gf : sc.rx * 2.0 * a.c2 * gf;
}
template <int NS>
__device__ double qp_elem_bc0_free(const QpArgs& a, const QpScale& sc, const int b, const int r, const int m) {
  const int j = r - 3;
  if (m != 1 || j < 0 || j >= 6) return 0.0;
  const double g0 = a.em[(long)b * QP_MODEL + j];
  return (j < 3 || !a.impulsive) ? g0 : sc.rx * 2.0 * a.c2 * g0;
}

template <int K>
__device__ __forceinline__ double qp_bcast(const double x) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), K), hi = __builtin_amdgcn_readlane(__double2hiint(x), K);
  return __hiloint2double(hi, lo);
}
template <int FIRST, int LAST, class F>
__device__ __forceinline__ void qp_static_for(F&& f) {
  if constexpr (FIRST < LAST) {
    f(std::integral_constant<int, FIRST>{});
    qp_static_for<FIRST + 1, LAST>(f);
  }
}

// NK Householder reflections on a ROWS-row stack, lane c = column c (c < NL); the reflector of step k is lane k's column
template <int ROWS, int NK, int NL>
__device__ __forceinline__ void qp_householder(double (&col)[ROWS], const int c) {
  qp_static_for<0, NK>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    double x[ROWS];
#pragma unroll
    for (int r = k + 1; r < ROWS; ++r) x[r] = qp_bcast<k>(col[r]);
    const double alpha = qp_bcast<k>(col[k]);
    double q0 = 0.0, q1 = 0.0;
#pragma unroll
    for (int r = k + 1; r < ROWS; ++r) {
      if (((r - k - 1) & 1) == 0) q0 = __builtin_fma(x[r], x[r], q0);
      else q1 = __builtin_fma(x[r], x[r], q1);
    }
    const double xn2 = q0 + q1;
    const bool trivial = (xn2 == 0.0);
    const double nrm = sqrt(__builtin_fma(alpha, alpha, xn2));
    const double beta = (alpha >= 0.0) ? -nrm : nrm;
    const double vk = alpha - beta;
    const double g = trivial ? 0.0 : 1.0 / (beta * (beta - alpha));
    if (c == k && !trivial) col[k] = beta;
    if (c > k && c < NL) {
      double w0 = vk * col[k], w1 = 0.0;
#pragma unroll
      for (int r = k + 1; r < ROWS; ++r) {
        if (((r - k - 1) & 1) == 0) w0 = __builtin_fma(x[r], col[r], w0);
        else w1 = __builtin_fma(x[r], col[r], w1);
      }
      const double w = (w0 + w1) * g;
      col[k] = __builtin_fma(-w, vk, col[k]);
#pragma unroll
      for (int r = k + 1; r < ROWS; ++r) col[r] = __builtin_fma(-w, x[r], col[r]);
    }
  });
}

// ---- one level of the reduction: pair j of trajectory b stacks rows 2j and 2j+1 of `cur` (FIRST: the level-0 rows, formed from
// the sweep's outputs), eliminates node (2j+1) 2^level and writes the new row j of `nxt`; a row without a partner is carried.
template <int NS, bool FIRST, int NR>
__global__ __launch_bounds__(64) void k_qp_level(QpA<NR> a, const int level, const int M, const double* __restrict__ cur,
                                                 double* __restrict__ nxt) {
  using D = QpDims<NS, NR>;
  constexpr int NB = D::NB;
  const int j = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
  const QpScale sc = qp_scale(a, b);
  const double* rows = cur + (long)b * a.S_traj * D::ROW;
  double* orow = nxt + ((long)b * a.S_traj + j) * D::ROW;
  if (2 * j + 1 >= M) {                           // carried row
    for (int e = c; e < D::ROW; e += 64) {
      double v;
      if (FIRST) {
        const int cc = (e < 2 * NB * NB) ? e / NB : 2 * NB, r = (e < 2 * NB * NB) ? e % NB : (e - 2 * NB * NB) % NB;
        const int m = (e < 2 * NB * NB) ? 0 : (e - 2 * NB * NB) / NB;
        if constexpr (NR == 1) v = qp_elem0<NS>(a, sc, b, 2 * j, r, cc);
        else v = (m == 0) ? qp_elem0<NS>(a, sc, b, 2 * j, r, cc) : qp_elem0_free<NS, NR>(a, sc, b, 2 * j, r, m);
      } else {
        v = rows[(long)(2 * j) * D::ROW + e];
      }
      orow[e] = v;
    }
    return;
  }
  double col[D::R2];
#pragma unroll
  for (int r = 0; r < D::R2; ++r) col[r] = 0.0;
  const double* top = rows + (long)(2 * j) * D::ROW;
  const double* bot = top + D::ROW;
  // columns: shared node [B_top; A_bot] | left node [A_top; 0] | right node [0; B_bot] | rhs
  if (c < NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      col[r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j, r, NB + c) : top[NB * NB + c * NB + r];
      col[NB + r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j + 1, r, c) : bot[c * NB + r];
    }
  } else if (c < 2 * NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) col[r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j, r, c - NB) : top[(c - NB) * NB + r];
  } else if (c < 3 * NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) col[NB + r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j + 1, r, c - NB) : bot[NB * NB + (c - 2 * NB) * NB + r];
  } else if (c == 3 * NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      col[r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j, r, 2 * NB) : top[2 * NB * NB + r];
      col[NB + r] = FIRST ? qp_elem0<NS>(a, sc, b, 2 * j + 1, r, 2 * NB) : bot[2 * NB * NB + r];
    }
  } else if (NR > 1 && c < D::NCOLS) {            // the free-end right-hand sides
    const int m = c - 3 * NB;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      col[r] = FIRST ? qp_elem0_free<NS, NR>(a, sc, b, 2 * j, r, m) : top[2 * NB * NB + m * NB + r];
      col[NB + r] = FIRST ? qp_elem0_free<NS, NR>(a, sc, b, 2 * j + 1, r, m) : bot[2 * NB * NB + m * NB + r];
    }
  }
  qp_householder<D::R2, NB, D::NCOLS>(col, c);
  const int mid = (2 * j + 1) << level;
  double* rec = a.rec + ((long)b * a.n_nodes + mid) * D::REC;
  if (c < NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) rec[D::REC_R + c * NB + r] = (r <= c) ? col[r] : 0.0;
  } else if (c < 2 * NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) { rec[D::REC_CA + (c - NB) * NB + r] = col[r]; orow[(c - NB) * NB + r] = col[NB + r]; }
  } else if (c < 3 * NB) {
#pragma unroll
    for (int r = 0; r < NB; ++r) { rec[D::REC_CB + (c - 2 * NB) * NB + r] = col[r]; orow[NB * NB + (c - 2 * NB) * NB + r] = col[NB + r]; }
  } else if (c >= 3 * NB && c < D::NCOLS) {
    const int m = c - 3 * NB;
#pragma unroll
    for (int r = 0; r < NB; ++r) { rec[D::REC_G + m * NB + r] = col[r]; orow[2 * NB * NB + m * NB + r] = col[NB + r]; }
  }
}

// ---- the last level: the one block row A y_0 + B y_{n-1} = r with node 0's boundary block (NS + 3 rows) and lambda_{n-1} = 0 (NS
// rows): 2NB x 2NB, triangularised in one wavefront (lane = column), back-substituted by lane 0 from LDS.  A pivot below 1e-13 of
// the largest marks the trajectory's KKT system singular (e.g. too few nodes to reach the terminal state).
template <int NS, int NR>
__global__ __launch_bounds__(64) void k_qp_final(QpArgs a, const double* __restrict__ cur) {
  using D = QpDims<NS, NR>;
  constexpr int NB = D::NB, N2 = 2 * NB;
  __shared__ double Rs[N2 + NR][N2];
  __shared__ double ys[NR][N2];
  const int b = blockIdx.x, c = threadIdx.x;
  const QpScale sc = qp_scale(a, b);
  const double* row = cur + (long)b * a.S_traj * D::ROW;
  double col[N2];
#pragma unroll
  for (int r = 0; r < N2; ++r) col[r] = 0.0;
  if (c <= N2) {
    const int rc = (c < N2) ? c : 2 * NB;       // column of the block row: y_0 | y_{n-1} | rhs
#pragma unroll
    for (int r = 0; r < NB; ++r) col[r] = row[(rc < 2 * NB) ? (long)rc * NB + r : 2L * NB * NB + r];
    if (c < NB || c == N2) {
      const int bc = (c < NB) ? c : NB;
#pragma unroll
      for (int r = 0; r < NS + 3; ++r) col[NB + r] = qp_elem_bc0<NS>(a, sc, b, r, bc);
    } else if (c >= NB + NS + 3) {              // lambda_{n-1} = 0
#pragma unroll
      for (int r = NB + NS + 3; r < N2; ++r) col[r] = (r == c) ? 1.0 : 0.0;
    }
  } else if (NR > 1 && c < N2 + NR) {           // the free-end right-hand sides (zero in the lambda_{n-1} rows)
    const int m = c - N2;
#pragma unroll
    for (int r = 0; r < NB; ++r) col[r] = row[2L * NB * NB + m * NB + r];
#pragma unroll
    for (int r = 0; r < NS + 3; ++r) col[NB + r] = qp_elem_bc0_free<NS>(a, sc, b, r, m);
  }
  qp_householder<N2, N2, N2 + NR>(col, c);
  if (c < N2 + NR) {
#pragma unroll
    for (int r = 0; r < N2; ++r) Rs[c][r] = col[r];
  }
  __syncthreads();
  if (c == 0) {
    double dmax = 0.0, dmin = 1e300;
    for (int k = 0; k < N2; ++k) { dmax = fmax(dmax, fabs(Rs[k][k])); dmin = fmin(dmin, fabs(Rs[k][k])); }
    a.status[b] = (dmin <= 1e-13 * dmax) ? 1 : 0;
  }
  if (c < NR) {                                 // lane m back-substitutes right-hand side m
    for (int k = N2 - 1; k >= 0; --k) {
      double s = Rs[N2 + c][k];
      for (int m = k + 1; m < N2; ++m) s -= Rs[m][k] * ys[c][m];
      ys[c][k] = s / Rs[k][k];
    }
  }
  __syncthreads();
  if (c < N2) {
    const long node = (long)b * a.n_nodes + ((c < NB) ? 0 : a.n_nodes - 1);
#pragma unroll
    for (int m = 0; m < NR; ++m) a.Y[(long)(m * NB + c % NB) * a.ldy + node] = ys[m][c];
  }
}

// ---- back-substitution of one level: pair j forms y_mid = R^{-1} (g - Ca y_left - Cb y_right), lane r = row r
template <int NS, int NR>
__global__ __launch_bounds__(64) void k_qp_back(QpArgs a, const int level) {
  using D = QpDims<NS, NR>;
  constexpr int NB = D::NB;
  const int j = blockIdx.x, b = blockIdx.y, r = threadIdx.x;
  const int mid = (2 * j + 1) << level, left = (2 * j) << level;
  int right = (2 * j + 2) << level;
  if (right > a.n_nodes - 1) right = a.n_nodes - 1;
  const double* rec = a.rec + ((long)b * a.n_nodes + mid) * D::REC;
  const long nb = (long)b * a.n_nodes;
  const int rr = r < NB ? r : NB - 1;
  double s[NR], x[NR];
#pragma unroll
  for (int m = 0; m < NR; ++m) {
    const double* Ym = a.Y + (long)m * NB * a.ldy;
    s[m] = rec[D::REC_G + m * NB + rr];
    for (int c = 0; c < NB; ++c)
      s[m] -= rec[D::REC_CA + c * NB + rr] * Ym[(long)c * a.ldy + nb + left] + rec[D::REC_CB + c * NB + rr] * Ym[(long)c * a.ldy + nb + right];
    x[m] = 0.0;
  }
  const double rdiag = 1.0 / rec[D::REC_R + rr * NB + rr];
  qp_static_for<0, NB>([&](auto kc) {
    constexpr int k = NB - 1 - decltype(kc)::value;
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const double xk = qp_bcast<k>(s[m] * rdiag);
      if (rr == k) x[m] = xk;
      if (rr < k) s[m] = __builtin_fma(-rec[D::REC_R + k * NB + rr], xk, s[m]);
    }
  });
  if (r < NB) {
#pragma unroll
    for (int m = 0; m < NR; ++m) a.Y[(long)(m * NB + r) * a.ldy + nb + mid] = x[m];
  }
}

// ---- unscale into the caller's arrays, grid over nodes; per-block partial sums of the control cost (:377-380) in `part`
constexpr int QP_FIN = 256;
template <int NS>
__global__ __launch_bounds__(QP_FIN) void k_qp_unscale(QpArgs a, double* dX, long ldX, double* dU, long ldU, double* part) {
  const int b = blockIdx.y, tid = threadIdx.x, k = blockIdx.x * QP_FIN + tid;
  const QpScale sc = qp_scale(a, b);
  const bool bad = a.status[b] != 0;              // singular: every output of the trajectory is NaN (and the status says why)
  const double nan = __builtin_nan("");
  double acc = 0.0;
  if (k < a.n_nodes) {
    const long node = (long)b * a.n_nodes + k;
#pragma unroll
    for (int c = 0; c < NS; ++c) dX[(long)c * ldX + node] = bad ? nan : a.Y[(long)c * a.ldy + node];
    const double wk = qp_weight(a, b, k);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double du = bad ? nan : sc.su * a.Y[(long)(NS + q) * a.ldy + node];
      dU[(long)q * ldU + node] = du;
      const double u = a.U[(long)q * a.ldu + node] + du;
      acc = __builtin_fma(wk * u, u, acc);
    }
  }
  __shared__ double red[QP_FIN];
  red[tid] = acc;
  __syncthreads();
  for (int h = QP_FIN / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) part[(long)b * gridDim.x + blockIdx.x] = red[0];
}
// ---- the impulses through the pins and the cost, one thread per trajectory (the partial sums added in a fixed order)
__global__ void k_qp_cost(QpArgs a, const double* dX, long ldX, double* dV, double* cost, double* singular, const double* part, int nblk) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.n_batch) return;
  const bool bad = a.status[b] != 0;
  const double nan = __builtin_nan("");
  double acc = 0.0;
  for (int k = 0; k < nblk; ++k) acc += part[(long)b * nblk + k];
  const double* tg = a.tg + (long)b * QP_TARGET;
  const long nb = (long)b * a.n_nodes;
  double ce = 0.0;
  for (int e = 0; e < 2; ++e) {
    const long node = nb + (e ? a.n_nodes - 1 : 0);
    for (int q = 0; q < 3; ++q) {
      const double dv = tg[13 + 3 * e + q];
      // impulse update d = s_v - x_v - dx_v - dV (the velocity pin solved for it); 0 when impulses are off
      const double upd = a.impulsive ? tg[6 * e + 3 + q] - a.X[(long)(3 + q) * a.ldx + node] - dX[(long)(3 + q) * ldX + node] - dv : 0.0;
      dV[(long)b * 6 + 3 * e + q] = bad ? nan : upd;
      ce += (dv + upd) * (dv + upd);
    }
  }
  cost[b] = bad ? nan : acc + a.c2 * ce;
  if (singular) singular[b] = bad ? 1.0 : 0.0;
}

// ---- free ends: the solution is z(p) = z0 + z1 p1 + z2 p2 and the reduced cost
//   phi(p) = phi0 + G.p + p'Hp/2,  phi0 = the frozen cost of z0,
//   G_i = 2 (sum_k w_k (u_k + du0_k).du_ik + c2 sum_e a_e.b_ei),  H_ij = 2 (sum_k w_k du_ik.du_jk + c2 sum_e b_ei.b_ej) + beta |c|_i delta_ij
// with a_e, b_ei the end-point impulse terms dV + d and their p-derivatives.  Per-block partial sums of the node sums in `part`
// [n_batch][nblk][qp_nsum(NR)], in this order: u.u, u.du_m (m = 1 .. NR-1), du_i.du_j (i <= j, row by row), all weighted -- six for
// NR = 3, ten for NR = 4 (p3 = tf_jump adds z3, with no beta term).
constexpr int QP_NSUM = 6;
__host__ __device__ constexpr int qp_nsum(const int nr) { return 1 + (nr - 1) + (nr - 1) * nr / 2; }
template <int NS, int NR>
__global__ __launch_bounds__(QP_FIN) void k_qp_free_sums(QpArgs a, double* part) {
  constexpr int NB = QpDims<NS, NR>::NB, NP = NR - 1, NSUM = qp_nsum(NR);
  const int b = blockIdx.y, tid = threadIdx.x, k = blockIdx.x * QP_FIN + tid;
  const QpScale sc = qp_scale(a, b);
  double acc[NSUM] = {};
  if (k < a.n_nodes) {
    const long node = (long)b * a.n_nodes + k;
    const double wk = qp_weight(a, b, k);
#pragma unroll
    for (int q = 0; q < 3; ++q) {             // straight-line code per q (qp_static_for): the NR = 3 kernel as before this form
      const double u = a.U[(long)q * a.ldu + node] + sc.su * a.Y[(long)(NS + q) * a.ldy + node];
      double d[NP];
      qp_static_for<0, NP>([&](auto m) { d[m] = sc.su * a.Y[(long)((m + 1) * NB + NS + q) * a.ldy + node]; });
      acc[0] = __builtin_fma(wk * u, u, acc[0]);
      qp_static_for<0, NP>([&](auto m) { acc[1 + m] = __builtin_fma(wk * u, d[m], acc[1 + m]); });
      qp_static_for<0, NP>([&](auto i) {
        qp_static_for<i, NP>([&](auto j) {
          constexpr int s = 1 + NP + i * NP - i * (i - 1) / 2 + (j - i);   // row i of the upper triangle starts after rows 0 .. i-1
          acc[s] = __builtin_fma(wk * d[i], d[j], acc[s]);
        });
      });
    }
  }
  __shared__ double red[NSUM][QP_FIN];
#pragma unroll
  for (int m = 0; m < NSUM; ++m) red[m][tid] = acc[m];
  __syncthreads();
  for (int h = QP_FIN / 2; h > 0; h >>= 1) {
    if (tid < h)
#pragma unroll
      for (int m = 0; m < NSUM; ++m) red[m][tid] += red[m][tid + h];
    __syncthreads();
  }
  if (tid < NSUM) part[((long)b * gridDim.x + blockIdx.x) * NSUM + tid] = red[tid][0];
}

__device__ __forceinline__ double qp_phi(const double* G, const double* H, const double phi0, const double p1, const double p2) {
  return phi0 + G[0] * p1 + G[1] * p2 + 0.5 * (H[0] * p1 * p1 + 2.0 * H[1] * p1 * p2 + H[2] * p2 * p2);
}
__device__ __forceinline__ double qp_clamp(const double v) { return fmin(fmax(v, -QP_PBOUND), QP_PBOUND); }

// ---- the exact minimum of a convex 2-D quadratic G.p + p'Hp/2 (H = [H0 H1; H1 H2]) over the box [lo1, hi1] x [lo2, hi2]: every
// candidate is handed to `consider`, in this order: the interior stationary point (H positive definite and the point inside the
// box), the clamped 1-D minimisers on the edges p1 = lo1, hi1, p2 = lo2, hi2, and the four corners.  A coordinate on a bound is the
// bound value itself.
template <class F>
__device__ __forceinline__ void qp_box2(const double* G, const double* H, const double lo1, const double hi1, const double lo2,
                                        const double hi2, F&& consider) {
  const double det = H[0] * H[2] - H[1] * H[1];
  if (H[0] > 0.0 && det > 0.0) {
    const double p1 = (-G[0] * H[2] + G[1] * H[1]) / det, p2 = (-G[1] * H[0] + G[0] * H[1]) / det;
    if (p1 >= lo1 && p1 <= hi1 && p2 >= lo2 && p2 <= hi2) consider(p1, p2);
  }
  for (int s = 0; s < 2; ++s) {                    // edges p1 = lo1, hi1: min over p2
    const double p1 = s ? hi1 : lo1;
    if (H[2] > 0.0) consider(p1, fmin(fmax(-(G[1] + H[1] * p1) / H[2], lo2), hi2));
  }
  for (int s = 0; s < 2; ++s) {                    // edges p2 = lo2, hi2: min over p1
    const double p2 = s ? hi2 : lo2;
    if (H[0] > 0.0) consider(fmin(fmax(-(G[0] + H[1] * p2) / H[0], lo1), hi1), p2);
  }
  consider(lo1, lo2); consider(hi1, lo2); consider(lo1, hi2); consider(hi1, hi2);
}

// ---- the 2 x 2 box QP of every trajectory, one thread each: min phi(p) over |p1|, |p2| <= 0.1 over the candidates of qp_box2.  phi
// is convex, so the smallest phi among them is the minimum; exact ties go to the smaller max|p|, then to the earlier candidate.  Then
// the impulses, p and the cost (with the beta term).
template <int NS>
__global__ void k_qp_free_box(QpArgs a, double* dV, double* pout, double* cost, double* singular, const double* part, int nblk) {
  constexpr int NB = QpDims<NS, 3>::NB;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.n_batch) return;
  const bool bad = a.status[b] != 0;
  const double nan = __builtin_nan("");
  double sum[QP_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < nblk; ++k)
#pragma unroll
    for (int m = 0; m < QP_NSUM; ++m) sum[m] += part[((long)b * nblk + k) * QP_NSUM + m];
  const double* tg = a.tg + (long)b * QP_TARGET;
  const double* em = a.em + (long)b * QP_MODEL;
  const long nb = (long)b * a.n_nodes;
  // end-point impulse terms dV_e + d_e = a_e + b_e1 p1 + b_e2 p2 (d_e = s_v + g_v p_e - x_v - dx_v - dV_e, or 0 without impulses)
  double ae[6], be1[6], be2[6];
  for (int e = 0; e < 2; ++e) {
    const long node = nb + (e ? a.n_nodes - 1 : 0);
    for (int q = 0; q < 3; ++q) {
      const int v = 3 + q, i = 3 * e + q;
      if (a.impulsive) {
        ae[i] = tg[6 * e + v] - a.X[(long)v * a.ldx + node] - a.Y[(long)v * a.ldy + node];
        be1[i] = (e == 0 ? em[v] : 0.0) - a.Y[(long)(NB + v) * a.ldy + node];
        be2[i] = (e == 1 ? em[6 + v] : 0.0) - a.Y[(long)(2 * NB + v) * a.ldy + node];
      } else {
        ae[i] = tg[13 + i];
        be1[i] = be2[i] = 0.0;
      }
    }
  }
  double caa = 0.0, ca1 = 0.0, ca2 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
  for (int i = 0; i < 6; ++i) {
    caa += ae[i] * ae[i]; ca1 += ae[i] * be1[i]; ca2 += ae[i] * be2[i];
    c11 += be1[i] * be1[i]; c12 += be1[i] * be2[i]; c22 += be2[i] * be2[i];
  }
  const double beta = a.beta[b];
  const double phi0 = sum[0] + a.c2 * caa;
  const double G[2] = {2.0 * (sum[1] + a.c2 * ca1), 2.0 * (sum[2] + a.c2 * ca2)};
  const double H[3] = {2.0 * (sum[3] + a.c2 * c11) + beta * em[12], 2.0 * (sum[4] + a.c2 * c12), 2.0 * (sum[5] + a.c2 * c22) + beta * em[13]};
  double best = 0.0, bp1 = 0.0, bp2 = 0.0, bm = 0.0;
  bool have = false;
  auto consider = [&](const double p1, const double p2) {
    const double f = qp_phi(G, H, phi0, p1, p2), m = fmax(fabs(p1), fabs(p2));
    if (!have || f < best || (f == best && m < bm)) { best = f; bp1 = p1; bp2 = p2; bm = m; have = true; }
  };
  // the candidates of qp_box2 at +-d, written out: this kernel's code stays as it was before qp_box2
  const double d = QP_PBOUND, det = H[0] * H[2] - H[1] * H[1];
  if (H[0] > 0.0 && det > 0.0) {
    const double p1 = (-G[0] * H[2] + G[1] * H[1]) / det, p2 = (-G[1] * H[0] + G[0] * H[1]) / det;
    if (fabs(p1) <= d && fabs(p2) <= d) consider(p1, p2);
  }
  for (int s = -1; s <= 1; s += 2) {               // edges p1 = s d: min over p2
    const double p1 = s * d;
    if (H[2] > 0.0) consider(p1, qp_clamp(-(G[1] + H[1] * p1) / H[2]));
  }
  for (int s = -1; s <= 1; s += 2) {               // edges p2 = s d: min over p1
    const double p2 = s * d;
    if (H[0] > 0.0) consider(qp_clamp(-(G[0] + H[1] * p2) / H[0]), p2);
  }
  consider(-d, -d); consider(d, -d); consider(-d, d); consider(d, d);
  for (int e = 0; e < 2; ++e)
    for (int q = 0; q < 3; ++q) {
      const int i = 3 * e + q;
      dV[(long)b * 6 + i] = bad ? nan : (a.impulsive ? ae[i] + be1[i] * bp1 + be2[i] * bp2 - tg[13 + i] : 0.0);
    }
  pout[2 * b] = bad ? nan : bp1;
  pout[2 * b + 1] = bad ? nan : bp2;
  cost[b] = bad ? nan : best;
  if (singular) singular[b] = bad ? 1.0 : 0.0;
}

// ---- free tf: the 3 x 3 box QP in p = (p1, p2, p3 = tf_jump), one thread per trajectory.  Bounds |p1|, |p2| <= 0.1
// and p3 in [lo, hi], lo = max(-step, tf_min - tf), hi = min(step, tf_max - tf) (:286-295).  Candidates, in this order: the interior
// stationary point (H positive definite by its leading minors and the point inside the box), then the exact 2-D box minimum of each
// face p1 = lo, p1 = hi, p2 = lo, p2 = hi, p3 = lo, p3 = hi (qp_box2 on the other two coordinates, in increasing order).  phi is
// convex, so the smallest phi among them is the minimum, also when H is singular.  Ties: the smaller max(|p1|/0.1, |p2|/0.1,
// |p3|/step) (the last term 0 when step = 0), then the earlier candidate.  p [n_batch][3].
// phi(p1, p2, p3) = the free-end step's qp_phi(p1, p2) + the terms of p3, which are exactly 0 at p3 = 0: a trajectory whose tf is
// pinned (step = 0) beside one whose tf moves reports the cost its free-end step reports, to the last bit.
__device__ __forceinline__ double qp_phi3(const double (&G)[3], const double (&H)[3][3], const double phi0, const double (&p)[3]) {
  const double H2[3] = {H[0][0], H[0][1], H[1][1]};
  const double q3 = __builtin_fma(H[2][2] * p[2], p[2], __builtin_fma(2.0 * H[1][2] * p[1], p[2], 2.0 * H[0][2] * p[0] * p[2]));
  return qp_phi(G, H2, phi0, p[0], p[1]) + __builtin_fma(G[2], p[2], 0.5 * q3);
}
template <int NS>
__global__ __launch_bounds__(64) void k_qp_free_box3(QpArgsTf a, double* dV, double* pout, double* cost, double* singular, const double* part, int nblk) {
  constexpr int NB = QpDims<NS, 4>::NB, NSUM = qp_nsum(4);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.n_batch) return;
  const bool bad = a.status[b] != 0;
  const double nan = __builtin_nan("");
  double sum[NSUM];
#pragma unroll
  for (int m = 0; m < NSUM; ++m) sum[m] = 0.0;
  for (int k = 0; k < nblk; ++k)
#pragma unroll
    for (int m = 0; m < NSUM; ++m) sum[m] += part[((long)b * nblk + k) * NSUM + m];
  const double* tg = a.tg + (long)b * QP_TARGET;
  const double* em = a.em + (long)b * QP_MODEL;
  const long nb = (long)b * a.n_nodes;
  // end-point impulse terms dV_e + d_e = a_e + sum_m b_em p_m; tf enters them only through dx at the end nodes
  double ae[6], be[3][6];
  for (int e = 0; e < 2; ++e) {
    const long node = nb + (e ? a.n_nodes - 1 : 0);
    for (int q = 0; q < 3; ++q) {
      const int v = 3 + q, i = 3 * e + q;
      if (a.impulsive) {
        ae[i] = tg[6 * e + v] - a.X[(long)v * a.ldx + node] - a.Y[(long)v * a.ldy + node];
        be[0][i] = (e == 0 ? em[v] : 0.0) - a.Y[(long)(NB + v) * a.ldy + node];
        be[1][i] = (e == 1 ? em[6 + v] : 0.0) - a.Y[(long)(2 * NB + v) * a.ldy + node];
        be[2][i] = -a.Y[(long)(3 * NB + v) * a.ldy + node];
      } else {
        ae[i] = tg[13 + i];
        be[0][i] = be[1][i] = be[2][i] = 0.0;
      }
    }
  }
  double caa = 0.0, ca[3] = {0.0, 0.0, 0.0}, cb[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int i = 0; i < 6; ++i) {
    caa += ae[i] * ae[i];
    for (int m = 0; m < 3; ++m) {
      ca[m] += ae[i] * be[m][i];
      for (int l = m; l < 3; ++l) cb[m][l] += be[m][i] * be[l][i];
    }
  }
  const double beta = a.beta[b];
  const double phi0 = sum[0] + a.c2 * caa;
  double G[3], H[3][3];
  for (int m = 0, s = 4; m < 3; ++m) {
    G[m] = 2.0 * (sum[1 + m] + a.c2 * ca[m]);
    for (int l = m; l < 3; ++l, ++s) H[m][l] = H[l][m] = 2.0 * (sum[s] + a.c2 * cb[m][l]);
  }
  H[0][0] += beta * em[12];
  H[1][1] += beta * em[13];
  const double* tb = a.tfb + (long)b * 3;
  const double step = tb[0], tf = a.tf[b];
  const double lo[3] = {-QP_PBOUND, -QP_PBOUND, fmax(-step, tb[1] - tf)};
  const double hi[3] = {QP_PBOUND, QP_PBOUND, fmin(step, tb[2] - tf)};
  const double inv3 = step > 0.0 ? 1.0 / step : 0.0;
  double best = 0.0, bp[3] = {0.0, 0.0, 0.0}, bm = 0.0;
  bool have = false;
  auto consider = [&](const double (&p)[3]) {
    const double f = qp_phi3(G, H, phi0, p);
    const double m = fmax(fmax(fabs(p[0]), fabs(p[1])) / QP_PBOUND, fabs(p[2]) * inv3);
    if (!have || f < best || (f == best && m < bm)) { best = f; bp[0] = p[0]; bp[1] = p[1]; bp[2] = p[2]; bm = m; have = true; }
  };
  // interior: H p = -G by the adjugate, H positive definite by Sylvester's criterion
  const double A00 = H[1][1] * H[2][2] - H[1][2] * H[1][2], A01 = H[0][2] * H[1][2] - H[0][1] * H[2][2],
               A02 = H[0][1] * H[1][2] - H[0][2] * H[1][1], A11 = H[0][0] * H[2][2] - H[0][2] * H[0][2],
               A12 = H[0][1] * H[0][2] - H[0][0] * H[1][2], A22 = H[0][0] * H[1][1] - H[0][1] * H[0][1];
  const double det = H[0][0] * A00 + H[0][1] * A01 + H[0][2] * A02;
  if (H[0][0] > 0.0 && A22 > 0.0 && det > 0.0) {
    const double p[3] = {-(A00 * G[0] + A01 * G[1] + A02 * G[2]) / det, -(A01 * G[0] + A11 * G[1] + A12 * G[2]) / det,
                         -(A02 * G[0] + A12 * G[1] + A22 * G[2]) / det};
    if (p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2]) consider(p);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {                   // faces p_k = lo_k, hi_k: the exact 2-D minimum over the other two
    const int i = (k == 0) ? 1 : 0, j = (k == 2) ? 1 : 2;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double v = s ? hi[k] : lo[k];
      const double Gf[2] = {G[i] + H[i][k] * v, G[j] + H[j][k] * v};
      const double Hf[3] = {H[i][i], H[i][j], H[j][j]};
      qp_box2(Gf, Hf, lo[i], hi[i], lo[j], hi[j], [&](const double x, const double y) {
        double p[3];
        p[k] = v; p[i] = x; p[j] = y;
        consider(p);
      });
    }
  }
  for (int e = 0; e < 2; ++e)
    for (int q = 0; q < 3; ++q) {
      const int i = 3 * e + q;
      dV[(long)b * 6 + i] = bad ? nan : (a.impulsive ? ae[i] + be[0][i] * bp[0] + be[1][i] * bp[1] + be[2][i] * bp[2] - tg[13 + i] : 0.0);
    }
  for (int m = 0; m < 3; ++m) pout[3 * b + m] = bad ? nan : bp[m];
  cost[b] = bad ? nan : best;
  if (singular) singular[b] = bad ? 1.0 : 0.0;
}

// ---- dX = z0 + sum_m z_m p_m (dx part), dU = s_u (du part), grid over nodes; p [n_batch][NR - 1]
template <int NS, int NR>
__global__ __launch_bounds__(QP_FIN) void k_qp_free_combine(QpArgs a, const double* pout, double* dX, long ldX, double* dU, long ldU) {
  constexpr int NB = QpDims<NS, NR>::NB, NP = NR - 1;
  const int b = blockIdx.y, k = blockIdx.x * QP_FIN + threadIdx.x;
  if (k >= a.n_nodes) return;
  const QpScale sc = qp_scale(a, b);
  double p[NP];
  qp_static_for<0, NP>([&](auto m) { p[m] = pout[NP * b + m]; });    // NaN for a singular system
  const long node = (long)b * a.n_nodes + k;
  auto z = [&](const int c) {          // fma(z_NP, p_NP, ... fma(z_1, p_1, z_0)), loaded outermost term first
    double y[NR];
    qp_static_for<0, NR>([&](auto mm) { y[NP - mm] = a.Y[(long)((NP - mm) * NB + c) * a.ldy + node]; });
    double v = y[0];
    qp_static_for<1, NR>([&](auto m) { v = __builtin_fma(y[m], p[m - 1], v); });
    return v;
  };
#pragma unroll
  for (int c = 0; c < NS; ++c) dX[(long)c * ldX + node] = z(c);
#pragma unroll
  for (int q = 0; q < 3; ++q) dU[(long)q * ldU + node] = sc.su * z(NS + q);
}

// workspace: gw (u64 [2 n_batch]) | status (int [n_batch]) | rows A | rows B | records | Y | partial sums; NR = 1, 3 or 4
static size_t qp_header_bytes(int n_batch) {
  return ((sizeof(unsigned long long) * 2 * n_batch + sizeof(int) * n_batch + 255) / 256) * 256;
}
template <int NS, int NR>
static size_t qp_doubles(int n_nodes, int n_batch) {
  using D = QpDims<NS, NR>;
  const size_t S = (size_t)(n_nodes - 1) * n_batch, J = (size_t)n_nodes * n_batch;
  const size_t nblk = (size_t)(n_nodes + QP_FIN - 1) / QP_FIN;
  return 2 * S * D::ROW + J * D::REC + (size_t)NR * D::NB * J + nblk * n_batch * qp_nsum(NR);
}
size_t direct_qp_workspace_bytes(int nstate, int n_nodes, int n_batch, int nr) {
  const size_t nd = (nstate == 7) ? (nr == 4 ? qp_doubles<7, 4>(n_nodes, n_batch) : nr == 3 ? qp_doubles<7, 3>(n_nodes, n_batch) : qp_doubles<7, 1>(n_nodes, n_batch))
                                  : (nr == 4 ? qp_doubles<6, 4>(n_nodes, n_batch) : nr == 3 ? qp_doubles<6, 3>(n_nodes, n_batch) : qp_doubles<6, 1>(n_nodes, n_batch));
  return qp_header_bytes(n_batch) + sizeof(double) * nd + 4096;
}
int* direct_qp_status(void* workspace, int n_batch) {
  return (int*)((char*)workspace + sizeof(unsigned long long) * 2 * n_batch);
}

template <int NS, int NR>
static hipError_t direct_qp_impl(const DirectQpArgs& q, void* workspace, hipStream_t st) {
  using D = QpDims<NS, NR>;
  QpA<NR> a;
  a.n_nodes = q.n_nodes; a.n_batch = q.n_batch; a.S_traj = q.n_nodes - 1;
  a.Jac = q.Jac; a.ldj = q.ldj; a.defect = q.defect; a.ldd = q.ldd; a.X = q.X; a.ldx = q.ldx; a.U = q.U; a.ldu = q.ldu;
  a.t = q.t; a.t_stride = q.t_stride; a.tg = q.targets; a.impulsive = q.impulsive; a.c2 = q.c2;
  a.em = q.model; a.beta = q.beta;
  if constexpr (NR == 4) { a.dtf = q.dtf; a.tfb = q.tfb; a.tf = q.tf; }
  const size_t S = (size_t)a.S_traj * a.n_batch, J = (size_t)a.n_nodes * a.n_batch;
  a.gw = (unsigned long long*)workspace;
  a.status = direct_qp_status(workspace, a.n_batch);
  double* rowsA = (double*)((char*)workspace + qp_header_bytes(a.n_batch));
  double* rowsB = rowsA + S * D::ROW;
  a.rec = rowsB + S * D::ROW;
  a.Y = a.rec + J * D::REC; a.ldy = (long)J;
  const int nblk = (a.n_nodes + QP_FIN - 1) / QP_FIN;
  double* part = a.Y + (size_t)NR * D::NB * J;
  hipError_t e = hipMemsetAsync(a.gw, 0, sizeof(unsigned long long) * 2 * a.n_batch, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_qp_gmax<NS>), dim3((a.S_traj + 255) / 256, a.n_batch), dim3(256), 0, st, (const QpArgs&)a);
  int M = a.S_traj, level = 0;
  int Ms[40];
  double* cur = rowsA;
  double* nxt = rowsB;
  bool first = true;
  do {                                  // a single segment still passes once: its level-0 row is formed ("carried")
    Ms[level] = M;
    const int groups = (M + 1) / 2;
    if (first) hipLaunchKernelGGL((k_qp_level<NS, true, NR>), dim3(groups, a.n_batch), dim3(64), 0, st, a, level, M, cur, nxt);
    else hipLaunchKernelGGL((k_qp_level<NS, false, NR>), dim3(groups, a.n_batch), dim3(64), 0, st, a, level, M, cur, nxt);
    { double* t = cur; cur = nxt; nxt = t; }
    first = false;
    M = groups;
    ++level;
  } while (M > 1);
  const QpArgs& ab = a;                 // the kernels past the first level read the common arguments only
  hipLaunchKernelGGL((k_qp_final<NS, NR>), dim3(a.n_batch), dim3(64), 0, st, ab, cur);
  for (int l = level - 1; l >= 0; --l) {
    const int pairs = Ms[l] / 2;
    if (pairs > 0) hipLaunchKernelGGL((k_qp_back<NS, NR>), dim3(pairs, a.n_batch), dim3(64), 0, st, ab, l);
  }
  if constexpr (NR >= 3) {
    hipLaunchKernelGGL((k_qp_free_sums<NS, NR>), dim3(nblk, a.n_batch), dim3(QP_FIN), 0, st, ab, part);
    if constexpr (NR == 4)
      hipLaunchKernelGGL((k_qp_free_box3<NS>), dim3((a.n_batch + 63) / 64), dim3(64), 0, st, a, q.dV, q.p, q.cost, q.singular, part, nblk);
    else
      hipLaunchKernelGGL((k_qp_free_box<NS>), dim3((a.n_batch + 63) / 64), dim3(64), 0, st, a, q.dV, q.p, q.cost, q.singular, part, nblk);
    hipLaunchKernelGGL((k_qp_free_combine<NS, NR>), dim3(nblk, a.n_batch), dim3(QP_FIN), 0, st, ab, q.p, q.dX, q.ldX, q.dU, q.ldU);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((k_qp_unscale<NS>), dim3(nblk, a.n_batch), dim3(QP_FIN), 0, st, a, q.dX, q.ldX, q.dU, q.ldU, part);
  hipLaunchKernelGGL(k_qp_cost, dim3((a.n_batch + 63) / 64), dim3(64), 0, st, a, q.dX, q.ldX, q.dV, q.cost, q.singular, part, nblk);
  return hipGetLastError();
}

// the impulses of the solve loop's targets after a step:  dV1 += alpha_b d1, dV2 += alpha_b d2  (:568-569; alpha = 0: frozen)
__global__ void k_qp_update_dv(double* tg, const double* dV, const double* step, int nb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * 6) return;
  const int b = i / 6, q = i % 6;
  if (step[b] != 0.0) tg[(long)b * QP_TARGET + 13 + q] = __builtin_fma(step[b], dV[i], tg[(long)b * QP_TARGET + 13 + q]);
}
hipError_t launch_direct_qp_update_dv(double* targets, const double* dV, const double* step, int n_batch, hipStream_t st) {
  hipLaunchKernelGGL(k_qp_update_dv, dim3((6 * n_batch + 255) / 256), dim3(256), 0, st, targets, dV, step, n_batch);
  return hipGetLastError();
}

// ---- costates from the multipliers of a frozen step: one lane per (trajectory, node), node index fastest, so that
// a wavefront's loads of one Jacobian entry are one contiguous run.  With l_i = s_l l~_i the multiplier of defect i (the lambda part
// of Y, unscaled; s_l is a power of two) and E_i, F_i the blocks d defect_i / d x_i, d defect_i / d x_{i+1}:
//   Lambda_k = E_k^T l_k (k < n-1),  Lambda_{n-1} = -F_{n-2}^T l_{n-2};  interior residual E_k^T l_k + F_{k-1}^T l_{k-1}.
// acc [n_batch][2]: bits of the largest |residual| and of the largest |Lambda| of every trajectory (k_qp_gmax's reduction).  With
// XC (NS = 6 only): XC [12][ldxc] = (X; cc Lambda), the node vector of the indirect method.  A singular trajectory gets NaN.
template <int NS>
__global__ __launch_bounds__(QP_FIN) void k_qp_costates(QpArgs a, DirectCostatesArgs o, unsigned long long* acc) {
  const int b = blockIdx.y, k = blockIdx.x * QP_FIN + threadIdx.x;
  const bool bad = a.status[b] != 0;
  double rmax = 0.0, lmax = 0.0;
  if (k < a.n_nodes) {
    const QpScale sc = qp_scale(a, b);
    const long node = (long)b * a.n_nodes + k, s = (long)b * a.S_traj + k;
    const bool hasE = k < a.n_nodes - 1, hasF = k > 0;
    const double nan = __builtin_nan("");
    double e[NS], f[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) e[c] = f[c] = 0.0;
    if (hasE) {                                   // E_k^T l_k; segment k does not exist at the last node
      double l[NS];
#pragma unroll
      for (int r = 0; r < NS; ++r) l[r] = sc.sl * a.Y[(long)(NS + 3 + r) * a.ldy + node];
#pragma unroll
      for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int r = 0; r < NS; ++r) e[c] = __builtin_fma(a.Jac[(long)(c * NS + r) * a.ldj + s], l[r], e[c]);
      if (o.mult)
#pragma unroll
        for (int r = 0; r < NS; ++r) o.mult[(long)r * o.ldm + s] = bad ? nan : l[r];
    }
    if (hasF) {                                   // F_{k-1}^T l_{k-1}
      double l[NS];
#pragma unroll
      for (int r = 0; r < NS; ++r) l[r] = sc.sl * a.Y[(long)(NS + 3 + r) * a.ldy + node - 1];
#pragma unroll
      for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int r = 0; r < NS; ++r) f[c] = __builtin_fma(a.Jac[(long)((NS + c) * NS + r) * a.ldj + s - 1], l[r], f[c]);
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      const double lam = hasE ? e[c] : -f[c];
      o.Lambda[(long)c * o.ldl + node] = bad ? nan : lam;
      if (!bad) {
        lmax = fmax(lmax, fabs(lam));
        if (hasE && hasF) rmax = fmax(rmax, fabs(e[c] + f[c]));
      }
      if constexpr (NS == 6) {
        if (o.XC) {
          o.XC[(long)c * o.ldxc + node] = o.X[(long)c * o.ldx + node];
          o.XC[(long)(6 + c) * o.ldxc + node] = bad ? nan : o.cc * lam;
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { rmax = fmax(rmax, __shfl_xor(rmax, off)); lmax = fmax(lmax, __shfl_xor(lmax, off)); }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&acc[2 * b], (unsigned long long)__double_as_longlong(rmax));
    atomicMax(&acc[2 * b + 1], (unsigned long long)__double_as_longlong(lmax));
  }
}
// kkt_res = largest |residual| / largest |Lambda| per trajectory: 0 without an interior node, NaN for a singular trajectory
__global__ void k_qp_costates_res(const int* status, const unsigned long long* acc, double* kkt_res, int n_batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_batch) return;
  const double r = __longlong_as_double((long long)acc[2 * b]), l = __longlong_as_double((long long)acc[2 * b + 1]);
  kkt_res[b] = status[b] != 0 ? __builtin_nan("") : (r == 0.0 ? 0.0 : r / l);
}

size_t direct_costates_acc_bytes(int n_batch) { return sizeof(unsigned long long) * 2 * n_batch; }

template <int NS>
static hipError_t direct_costates_impl(const DirectCostatesArgs& o, void* workspace, void* acc, hipStream_t st) {
  using D = QpDims<NS, 1>;                         // the layout of the frozen step's workspace (direct_qp_impl)
  QpArgs a = {};
  a.n_nodes = o.n_nodes; a.n_batch = o.n_batch; a.S_traj = o.n_nodes - 1;
  a.Jac = o.Jac; a.ldj = o.ldj;
  const size_t S = (size_t)a.S_traj * a.n_batch, J = (size_t)a.n_nodes * a.n_batch;
  a.gw = (unsigned long long*)workspace;
  a.status = direct_qp_status(workspace, a.n_batch);
  a.Y = (double*)((char*)workspace + qp_header_bytes(a.n_batch)) + 2 * S * D::ROW + J * D::REC; a.ldy = (long)J;
  const hipError_t e = hipMemsetAsync(acc, 0, direct_costates_acc_bytes(a.n_batch), st);
  if (e != hipSuccess) return e;
  const int nblk = (a.n_nodes + QP_FIN - 1) / QP_FIN;
  hipLaunchKernelGGL((k_qp_costates<NS>), dim3(nblk, a.n_batch), dim3(QP_FIN), 0, st, a, o, (unsigned long long*)acc);
  hipLaunchKernelGGL(k_qp_costates_res, dim3((a.n_batch + 63) / 64), dim3(64), 0, st, (const int*)a.status,
                     (const unsigned long long*)acc, o.kkt_res, a.n_batch);
  return hipGetLastError();
}
hipError_t launch_direct_costates(int nstate, const DirectCostatesArgs& o, void* workspace, void* acc, hipStream_t st) {
  if (nstate == 7) return o.XC ? hipErrorInvalidValue : direct_costates_impl<7>(o, workspace, acc, st);
  return direct_costates_impl<6>(o, workspace, acc, st);
}

hipError_t launch_direct_qp(int nstate, int nr, const DirectQpArgs& q, void* workspace, hipStream_t st) {
  switch (nr) {
    case 1: return (nstate == 7) ? direct_qp_impl<7, 1>(q, workspace, st) : direct_qp_impl<6, 1>(q, workspace, st);
    case 3: return (nstate == 7) ? direct_qp_impl<7, 3>(q, workspace, st) : direct_qp_impl<6, 3>(q, workspace, st);
    case 4: return (nstate == 7) ? direct_qp_impl<7, 4>(q, workspace, st) : direct_qp_impl<6, 4>(q, workspace, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lto

namespace lto {

// ---- free ends: the end states and the end model of every trajectory at its current (tau1, tau2) -- interpEndStates (:434-461)
// at tau and tau +- h, each argument wrapped into [0, 1] on its own, and the finite differences of :339-349.  One thread per
// trajectory and end point; the natural-spline second derivatives of the two tables come from the host (fixed for a call).
__global__ void k_end_states(EndOrbitsDev o, const double* tau, int n_batch, double* s, int s_stride, double* model) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * n_batch) return;
  const int b = g / 2, e = g % 2;
  const double x = tau[g], h = 0.05;               // pert (:340)
  double c2 = 0.0;
  for (int j = 0; j < 6; ++j) {
    const double s0 = end_spline(o, e, j, x), sp = end_spline(o, e, j, x + h), sm = end_spline(o, e, j, x - h);
    s[(long)b * s_stride + 6 * e + j] = s0;
    const double gj = (sp - sm) / (2.0 * h), cj = (sp - 2.0 * s0 + sm) / (h * h);
    model[(long)b * QP_MODEL + 6 * e + j] = gj;
    c2 += cj * cj;
  }
  model[(long)b * QP_MODEL + 12 + e] = sqrt(c2);
}
hipError_t launch_end_states(const EndOrbitsDev& o, const double* tau, int n_batch, double* s, int s_stride, double* model,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_end_states, dim3((2 * n_batch + 63) / 64), dim3(64), 0, st, o, tau, n_batch, s, s_stride, model);
  return hipGetLastError();
}

// tau1 += alpha p1, tau2 += alpha p2 (:564-565), not wrapped; alpha = 0: frozen
__global__ void k_tau_update(double* tau, const double* p, const double* step, int n_batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n_batch) return;
  const double a = step[i / 2];
  if (a != 0.0) tau[i] = tau[i] + p[i] * a;
}
hipError_t launch_tau_update(double* tau, const double* p, const double* step, int n_batch, hipStream_t st) {
  hipLaunchKernelGGL(k_tau_update, dim3((2 * n_batch + 63) / 64), dim3(64), 0, st, tau, p, step, n_batch);
  return hipGetLastError();
}

// free tf: tau1 += alpha p1, tau2 += alpha p2, then tf += alpha p3 (:564-567), p [n_batch][3]; alpha = 0: frozen.  tf is kept in
// [tf_min, tf_max] (tfb [n_batch][3]) against the rounding of tf + alpha (bound - tf).
__global__ void k_tf_update(double* tau, double* tf, const double* p, const double* step, const double* tfb, int n_batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_batch) return;
  const double a = step[b];
  if (a == 0.0) return;
  tau[2 * b] = tau[2 * b] + p[3 * b] * a;
  tau[2 * b + 1] = tau[2 * b + 1] + p[3 * b + 1] * a;
  tf[b] = fmin(fmax(tf[b] + p[3 * b + 2] * a, tfb[3 * b + 1]), tfb[3 * b + 2]);
}
// the grid of every trajectory from its tf: t = t0 + (tau_grid + 1) / 2 (tf - t0) (:582), evaluated as written (no contraction, so
// that it equals the host's formula bit for bit), and the copies of the line search's na trial trajectories per trajectory
__global__ void k_tf_grid(const double* taug, const double* t0, const double* tf, int n, int n_batch, double* t, double* tl, int na) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * n_batch) return;
  const int b = (int)(i / n), k = (int)(i % n);
  const double v = t0[b] + (taug[i] + 1.0) / 2.0 * (tf[b] - t0[b]);
  t[i] = v;
  for (int a = 0; a < na; ++a) tl[((long)b * na + a) * n + k] = v;
}
hipError_t launch_tf_update(double* tau, double* tf, const double* p, const double* step, const double* tfb, int n_batch,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_tf_update, dim3((n_batch + 63) / 64), dim3(64), 0, st, tau, tf, p, step, tfb, n_batch);
  return hipGetLastError();
}
hipError_t launch_tf_grid(const double* taug, const double* t0, const double* tf, int n, int n_batch, double* t, double* tl, int na,
                          hipStream_t st) {
  const long tot = (long)n * n_batch;
  hipLaunchKernelGGL(k_tf_grid, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, taug, t0, tf, n, n_batch, t, tl, na);
  return hipGetLastError();
}

}  // namespace lto
