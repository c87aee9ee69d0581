// pipe_hooks.hpp (probe version) -- same interface as lowthrustopt_amd/csrc/hooks/pipe_hooks.hpp, with the counters behind it.
// Used by `make probe` only (build/liblto_probe.so; tools/probe_pipe_roles.py, tools/probe_coop2.py): the probe scripts pass a
// defect buffer with spare rows, and the hooks write their figures there.
#pragma once
#include <hip/hip_runtime.h>

namespace lto {
namespace hook {

constexpr bool kProbeBuild = true;

struct BarrierWait {
  long long waited = 0;
  // edges of a phase loop (report_edges): ticks from the wave's first hook to leaving the first barrier (fill), from leaving the
  // second-to-last barrier to arriving at the last (drain), and from leaving the last barrier to the report (epilogue)
  long long born = clock64(), first_leave = 0, prev_leave = 0, last_arrive = 0, last_leave = 0;
  int nsync = 0;
  // stamps inside the epilogue (ticks since leaving the last barrier): 0 = before the first Phi store, 1 = after the last one is
  // issued, 2 = after the wave's global stores have drained; drained() waits for them (probe build only) and takes stamp 2
  long long mark[3] = {0, 0, 0};
  __device__ __forceinline__ void stamp(int i) { mark[i] = clock64() - last_leave; }
  __device__ __forceinline__ void drained() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(2); }
  __device__ __forceinline__ void sync() {
    const long long t = clock64(); __syncthreads(); const long long t2 = clock64();
    waited += t2 - t;
    if (nsync++ == 0) first_leave = t2;
    prev_leave = last_leave; last_arrive = t; last_leave = t2;
  }
  __device__ __forceinline__ int sync_or(const int pred) { const long long t = clock64(); const int r = __syncthreads_or(pred); waited += clock64() - t; return r; }
  __device__ __forceinline__ void report(double* rows, long ld, int row, long col) const { if (rows) rows[row * ld + col] = (double)waited; }
  __device__ __forceinline__ void report_edges(double* rows, long ld, int row0, long col) const {
    if (!rows) return;
    rows[row0 * ld + col] = (double)(first_leave - born);
    rows[(row0 + 1) * ld + col] = (double)(nsync > 1 ? last_arrive - prev_leave : 0);
    rows[(row0 + 2) * ld + col] = (double)(clock64() - last_leave);
    rows[(row0 + 3) * ld + col] = (double)nsync;
    for (int i = 0; i < 3; ++i) rows[(row0 + 4 + i) * ld + col] = (double)mark[i];
  }
};
struct RegionClock {
  long long c0 = 0, w0 = 0;
  __device__ __forceinline__ void start() { c0 = clock64(); w0 = wall_clock64(); }
  __device__ __forceinline__ void report(double* rows, long ld, int row_ticks, int row_wall, long col) const {
    if (rows) { rows[row_ticks * ld + col] = (double)(clock64() - c0); rows[row_wall * ld + col] = (double)(wall_clock64() - w0); }
  }
  __device__ __forceinline__ void report_ticks(double* rows, long ld, int row, long col) const { if (rows) rows[row * ld + col] = (double)(clock64() - c0); }
};
struct Counter {
  int n = 0;
  __device__ __forceinline__ void bump() { ++n; }
  __device__ __forceinline__ void report(double* rows, long ld, int row, long col) const { if (rows) rows[row * ld + col] = (double)n; }
};
// 100 MHz wall-clock stamps 0 .. 3 into rows row0 .. row0 + 3, and the hardware id of the compute unit (XCC, SE, CU) into row0 + 4
struct Stamps {
  long long t[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void mark(int i) { t[i] = wall_clock64(); }
  __device__ __forceinline__ void report(double* rows, long ld, int row0, long col) const {
    if (!rows) return;
    for (int i = 0; i < 4; ++i) rows[(row0 + i) * ld + col] = (double)t[i];
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    // HW_ID: cu_id bits 11:8, sh_id bit 12, se_id bits 15:13; XCC_ID bits 3:0
    rows[(row0 + 4) * ld + col] = (double)(((xcc & 0xf) << 8) | (((hw >> 13) & 0x7) << 5) | (((hw >> 12) & 0x1) << 4) | ((hw >> 8) & 0xf));
  }
};
template <class Args>
__device__ __forceinline__ bool role_on(const Args& a, int bit) { return !(a.max_steps & bit); }

}  // namespace hook
}  // namespace lto
