// kernels_guidance_cov.hip -- linear covariance of the guided flight, gfx950.
//
// k_guidance_covariance<NX>: the forward pass of include/lto.h over the segment STMs Phi_k and the gains K_k that the gains sweep
// left in HBM.  One workgroup of four wavefronts per (trajectory, four cases): blockIdx.x the trajectory, blockIdx.y the group of
// cases, one wavefront per case.  Phi_k (ND^2 values, ND = 2 NX) and K_k (NX^2) are shared by all cases of a trajectory: thread t
// of the workgroup fetches one value of node k + 1 into a register while node k is worked on, and the 256 threads write them to
// LDS once per node.  Every wavefront keeps the covariance Z of z = (dx, dlambda) of its case in an LDS tile of its own, column
// major, with two more tiles for T = Phi Z and for T Phi^T ahead of the symmetrisation; lane l works on the elements l, l + 64, ..
// of a tile (three for NX = 6, four for NX = 7).  No per-lane array, no scratch.  The phases of a node are separated by workgroup
// barriers that every wavefront reaches whatever its case does: a case that has failed, or a wavefront behind the last case, only
// skips the arithmetic.  Nothing is shared between cases or between trajectories but the read-only Phi_k and K_k, so a
// (trajectory, case) pair's outputs do not depend on the batch or on the case list.
//
// Arithmetic: the order of include/lto.h, every product and every sum rounded on its own (no contraction), every dot product from
// its first product over j = 0, 1, ..  tests/covariance_reference.py restates it; the GPU test holds the outputs to it bit for bit.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace lto {

namespace {

constexpr int kCovWaves = 4;

template <int NX>
__global__ __launch_bounds__(64 * kCovWaves) void k_guidance_covariance(const CovArgs a) {
#pragma clang fp contract(off)                 // the order of include/lto.h, every operation rounded on its own
  constexpr int ND = 2 * NX, NE = NX * NX, NZ = ND * ND, PER = (NZ + 63) / 64;
  static_assert(NZ + NE <= 64 * kCovWaves, "one staged value of Phi_k or K_k per thread");
  static_assert(3 * NE <= NZ, "U, V and P + R share one tile");
  __shared__ double sPhi[NZ];                    // Phi_k[r][c] at c ND + r
  __shared__ double sK[NE];                      // K_k[r][c] at c NX + r
  __shared__ double sZ[kCovWaves][NZ];           // Z[r][c] at c ND + r
  __shared__ double sT[kCovWaves][NZ];           // T = Phi Z
  __shared__ double sW[kCovWaves][NZ];           // T Phi^T; at an update U, V and P + R, NE values each
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const long b = blockIdx.x;
  const int cs = blockIdx.y * kCovWaves + w;
  const bool live = cs < a.n_cases;              // wave-uniform
  const int segs = a.n_nodes - 1, n_cases = a.n_cases;
  const double nan = __builtin_nan("");
  double* Z = sZ[w];
  double* T = sT[w];
  double* W = sW[w];
  const bool el = lane < NE;                     // lane (r, c) of an NX x NX block
  const int r6 = el ? lane % NX : 0, c6 = el ? lane / NX : 0;
  // the first node's Phi and K
  const long s0 = b * segs;
  double stage = 0.0;
  if (tid < NZ) stage = a.Phi[(long)tid * a.ldp + s0];
  else if (tid < NZ + NE) stage = a.K[(long)NE * s0 + (tid - NZ)];
  // the case: P0 and R symmetrised on load
  const int every = live ? a.every[cs] : 0;
  bool bad = false;
  double rr = 0.0, pk = 0.0;                     // R[r6][c6];  the last P[r6][c6] stored
  if (live) {
    const double* P0 = a.P0 + (long)NE * cs;
    const double* R = a.R + (long)NE * cs;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + 64 * i;
      if (e < NZ) {
        const int r = e % ND, c = e / ND;
        double v = 0.0;
        if (r < NX && c < NX) {
          v = 0.5 * (P0[r + NX * c] + P0[c + NX * r]);
          bad = bad || !((v - v) == 0.0);
        }
        Z[e] = v;
      }
    }
    if (el) {
      rr = 0.5 * (R[r6 + NX * c6] + R[c6 + NX * r6]);
      bad = bad || !((rr - rr) == 0.0);
      pk = 0.5 * (P0[r6 + NX * c6] + P0[c6 + NX * r6]);
    }
  }
  int dead = (live && __any(bad)) ? 2 : 0;       // wave-uniform
  double* Pn = (a.P_nodes && live) ? a.P_nodes + ((b * n_cases + cs) * (long)a.n_nodes) * NE : nullptr;
  if (Pn && el) Pn[lane] = pk;                   // node 0: the symmetrised P0 as it is
  for (int k = 0; k < segs; ++k) {
    if (tid < NZ) sPhi[tid] = stage;
    else if (tid < NZ + NE) sK[tid - NZ] = stage;
    if (k + 1 < segs) {                          // node k + 1 is on its way while node k is worked on
      const long s = s0 + k + 1;
      if (tid < NZ) stage = a.Phi[(long)tid * a.ldp + s];
      else if (tid < NZ + NE) stage = a.K[(long)NE * s + (tid - NZ)];
    }
    __syncthreads();
    const bool upd = every > 0 && k % every == 0;
    bad = false;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int e = lane + 64 * i;
      if (e < NZ) {
        const double v = sPhi[e];
        bad = bad || !((v - v) == 0.0);
      }
    }
    if (upd && el) {                             // a gain that is not applied is not looked at
      const double v = sK[lane];
      bad = bad || !((v - v) == 0.0);
    }
    if (live && __any(bad)) dead = 2;
    const bool run = live && dead == 0;
    const bool upd_run = run && upd;
    if (upd_run && el) W[2 * NE + lane] = Z[c6 * ND + r6] + rr;       // P + R first, element by element
    __syncthreads();
    double u = 0.0;
    if (upd_run && el) {                         // U = K P,  V = K (P + R)
      const double* S = W + 2 * NE;
      u = sK[r6] * Z[c6 * ND];
      double v = sK[r6] * S[NX * c6];
#pragma unroll
      for (int j = 1; j < NX; ++j) {
        u = u + sK[r6 + NX * j] * Z[c6 * ND + j];
        v = v + sK[r6 + NX * j] * S[j + NX * c6];
      }
      W[NE + lane] = v;
    }
    __syncthreads();
    if (upd_run && el) {                         // Z_lx = U,  Z_xl = U^T copied,  Z_ll = V K^T;  Z_xx stays
      const double* V = W + NE;
      double l = V[r6] * sK[c6];
#pragma unroll
      for (int j = 1; j < NX; ++j) l = l + V[r6 + NX * j] * sK[c6 + NX * j];
      Z[c6 * ND + NX + r6] = u;
      Z[(NX + r6) * ND + c6] = u;
      Z[(NX + c6) * ND + NX + r6] = l;
    }
    __syncthreads();
    if (run) {                                   // T = Phi Z
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int e = lane + 64 * i;
        if (e < NZ) {
          const int r = e % ND, c = e / ND;
          double t = sPhi[r] * Z[c * ND];
#pragma unroll
          for (int j = 1; j < ND; ++j) t = t + sPhi[j * ND + r] * Z[c * ND + j];
          T[e] = t;
        }
      }
    }
    __syncthreads();
    if (run) {                                   // T Phi^T
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int e = lane + 64 * i;
        if (e < NZ) {
          const int r = e % ND, c = e / ND;
          double z = T[r] * sPhi[c];
#pragma unroll
          for (int j = 1; j < ND; ++j) z = z + T[j * ND + r] * sPhi[j * ND + c];
          W[e] = z;
        }
      }
    }
    __syncthreads();
    if (run) {                                   // the symmetric part; P_{k+1} = Z_xx
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int e = lane + 64 * i;
        if (e < NZ) {
          const int r = e % ND, c = e / ND;
          Z[e] = 0.5 * (W[e] + W[r * ND + c]);
        }
      }
      if (el) pk = 0.5 * (W[c6 * ND + r6] + W[r6 * ND + c6]);
    }
    if (Pn && el) Pn[(long)(k + 1) * NE + lane] = (dead != 0) ? nan : pk;
  }
  if (live) {
    if (el) a.P_final[(b * n_cases + cs) * (long)NE + lane] = (dead != 0) ? nan : pk;
    if (lane == 0) a.status[b * n_cases + cs] = dead;
  }
}

}  // namespace

hipError_t launch_guidance_covariance(const CovArgs& a, hipStream_t st) {
  if (a.n_nodes < 2 || a.n_batch < 1 || a.n_cases < 1) return hipErrorInvalidValue;
  const long groups = ((long)a.n_cases + kCovWaves - 1) / kCovWaves;
  if (groups > 65535) return hipErrorInvalidValue;                    // blockIdx.y
  const dim3 grid((unsigned)a.n_batch, (unsigned)groups), block(64 * kCovWaves);
  if (a.nx == 6) hipLaunchKernelGGL(k_guidance_covariance<6>, grid, block, 0, st, a);
  else if (a.nx == 7) hipLaunchKernelGGL(k_guidance_covariance<7>, grid, block, 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace lto
