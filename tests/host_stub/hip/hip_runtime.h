// Host stub of <hip/hip_runtime.h>: lets g++ compile lowthrustopt_amd/csrc/dynamics.hpp, rk.hpp and dop853_lane.hpp so the CPU
// test-suite can check the PRODUCT's device formulas (RHS, variational coefficients, fused column path, the adaptive DOP853 lane
// driver) against the oracle without a GPU.  The reduced-precision seeds mimic v_rsq_f64 / v_rcp_f64 (~2^-23) so the refinement
// steps are exercised too.
#pragma once
#include <cmath>
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__ const
using std::fabs; using std::fmax; using std::fmin; using std::sqrt; using std::exp; using std::pow; using std::cbrt;
static inline double __builtin_amdgcn_rsq(double x) { return (double)(float)(1.0 / std::sqrt(x)); }
static inline double __builtin_amdgcn_rcp(double x) { return (double)(float)(1.0 / x); }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __ddiv_rn(double a, double b) { return a / b; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __shfl_xor(double v, int, int) { return v; }      // one lane: only there so that the group form parses
static inline double __shfl(double v, int, int) { return v; }
// What kernels.hpp and halo_common.hpp name beside the arithmetic, as declarations: one lane, nothing is launched.  They let all of
// kernels.hpp parse; launch_by_method is never instantiated on the host (hipGetLastError has no definition here, and the launch
// macro drops its arguments).
#define __global__
#define __launch_bounds__(n)
typedef int hipError_t;
typedef void* hipStream_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1;
struct dim3 { unsigned x, y, z; constexpr dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
constexpr dim3 blockIdx(0, 0, 0), threadIdx(0, 0, 0);
hipError_t hipGetLastError();
#define hipLaunchKernelGGL(k, grid, block, lds, stream, ...) ((void)(k))
#include <cstring>
static inline long long __double_as_longlong(double x) { long long r; std::memcpy(&r, &x, 8); return r; }
static inline double __longlong_as_double(long long x) { double r; std::memcpy(&r, &x, 8); return r; }
static inline int __double2hiint(double x) { return (int)(__double_as_longlong(x) >> 32); }
static inline int __double2loint(double x) { return (int)(__double_as_longlong(x) & 0xffffffffll); }
static inline double __hiloint2double(int hi, int lo) { return __longlong_as_double(((long long)hi << 32) | (unsigned)lo); }
