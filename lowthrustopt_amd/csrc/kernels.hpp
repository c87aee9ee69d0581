// kernels.hpp -- argument blocks and launch entry points shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "dynamics.hpp"
#include "sweep_policy.hpp"        // what every indirect form is built for (the indirect_*_available predicates) and which one runs

namespace lto {

// integrator ids (== LTO_* in include/lto.h)
enum Method : int { M_RK4 = 0, M_RKF78_FIXED = 1, M_RKF78_ADAPTIVE = 2, M_DOP853_ADAPTIVE = 3 };

// The launch of a kernel that is built once per integrator, for the flights that know RK4 and DOP853: `lanes` lanes in workgroups
// of 64, k_rk4 for M_RK4, k_dop853 for M_DOP853_ADAPTIVE; any other method: hipErrorInvalidValue.
template <class Args>
static inline hipError_t launch_by_method(int method, void (*k_rk4)(Args), void (*k_dop853)(Args), long lanes, const Args& a,
                                          hipStream_t st) {
  const dim3 grid((unsigned)((lanes + 63) / 64));
  if (method == M_RK4) hipLaunchKernelGGL(k_rk4, grid, dim3(64), 0, st, a);
  else if (method == M_DOP853_ADAPTIVE) hipLaunchKernelGGL(k_dop853, grid, dim3(64), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// Device layout (include/lto.h, "device-resident API"): node j = b*n_nodes + k, segment
// s = b*seg_per_traj + i, component-major with leading dimensions ld*.
struct IndirectArgs {
  const double* X; long ldx;       // [ndim][ldx] nodes (ndim = 12 or 14)
  const double* t; int t_stride;   // t[b*t_stride + k]; t_stride = n_nodes (per-trajectory grids) or 0 (shared)
  const TrajParams* tp; int tp_stride;  // tp[b*tp_stride]; 1 or 0
  int n_nodes, seg_per_traj, S;
  int steps;                       // fixed-step methods
  double rtol, atol; int max_steps;  // adaptive methods
  double* defect; long ldd;        // [12][ldd] or null
  double* errors;                  // [S] or null
  double* Phi; long ldp;           // [144][ldp] (col*12+row) or null
  int* nacc; int* nrej;            // [S] adaptive step counters or null
  const int* order;                // [S] or null: lane -> segment map of adaptive sweeps (lto_indirect_plan_rebalance)
  int xcd_ranges;                  // 1: `order` is the windowed kind (LTO_ORDER_WINDOW below): workgroup b works on unit xcd_unit(b, grid), not b
  int class_filter;                // set by the launchers: 1 = this launch handles only trajectories of the kernel's p-class
  double stm_scale;                // 3^-(steps mod 256): the DPP column lanes of the pipeline kernels carry 3^k Phi (pipe_common.hpp)
  double* h_first;                 // [S] or null: step size of the segment's first ACCEPTED trial step (written by the two-lane adaptive kernels)
  int warm;                        // 1: start every segment from h_first (the previous sweep of this kind) instead of Hairer's rule
  // Record staging of rebalanced sweeps (round 4; kernels_indirect_coop2.hip, kernels_indirect_defect2.hip): with a balanced lane
  // order neighbouring lanes hold unrelated segments, and every element of the struct-of-arrays operands is an 8-byte access to
  // its own cache line (5 - 8 x the algorithmic traffic).  When these are set the kernel reads a node as ONE record
  //   Xa[node * NODE_REC + c], c < 12;  Xa[node * NODE_REC + 12] = the node's time
  // and writes a segment's results as records  Da[s * 12 + c],  Pa[s * 144 + col * 12 + row];  the plan converts between the
  // caller's arrays and the records with coalesced transposes before / after the sweep (lto_indirect_plan.hip).  Null: the arrays above.
  const double* Xa;
  double* Da;
  double* Pa;
};
constexpr int NODE_REC = 16;       // doubles per node record: 12 components, the time, padding to 128 bytes
// operand access of the kernels that support record staging
__device__ __forceinline__ double arg_node(const IndirectArgs& a, const int c, const long node) {
  return a.Xa ? a.Xa[node * NODE_REC + c] : a.X[c * a.ldx + node];
}
__device__ __forceinline__ double arg_span(const IndirectArgs& a, const long node, const long tg) {
  return a.Xa ? a.Xa[(node + 1) * NODE_REC + 12] - a.Xa[node * NODE_REC + 12] : a.t[tg + 1] - a.t[tg];
}
__device__ __forceinline__ void put_defect(const IndirectArgs& a, const int c, const int s, const double v) {
  if (a.Da) a.Da[(long)s * 12 + c] = v; else a.defect[c * a.ldd + s] = v;
}
__device__ __forceinline__ void put_phi(const IndirectArgs& a, const int col, const int row, const int s, const double v) {
  if (a.Pa) a.Pa[(long)s * 144 + col * 12 + row] = v; else a.Phi[(long)(col * 12 + row) * a.ldp + s] = v;
}

struct DirectArgs {
  const double* X; long ldx;       // [nstate][ldx]
  const double* U; long ldu;       // [3][ldu]  thrust, N
  const double* t; int t_stride;
  double MU, kk, isp_g0, TU;       // kk = TU^2/DU/1e3; isp_g0 = Isp * 9.81
  int n_nodes, seg_per_traj, S;
  int half_steps;                  // nsteps - 1 RKF7(8) steps per half segment
  double* defect; long ldd;        // [nstate][ldd] or null
  double* errors;                  // [S] or null
  double* Jac; long ldj;           // [nstate*nvar][ldj] (col*nstate+row) or null
  double* dtf;                     // [nstate][ldd] or null
  double* mid; long ldm;           // [nstate][ldm] or null: forward half-arc end state x(t_i + h_i/2; x_i, u_i)
};

static inline bool single_class(int pm) { return (pm & (pm - 1)) == 0; }   // pm: bit mask of p-classes
static_assert(kThrustLimitedClasses == ((1 << PM_P0) | (1 << PM_P1)) && kOtherClasses == ((1 << PM_P2) | (1 << PM_PGEN)), "sweep_policy.hpp numbers the classes as PMode does");
static_assert(M_RK4 == LTO_RK4 && M_DOP853_ADAPTIVE == LTO_DOP853_ADAPTIVE, "sweep_policy.hpp reads Method ids as LTO_*");

// `pm` = bit mask of the control-law classes present in the batch.  One launch per class of CLASSES that is present: the args are
// copied once and, with more than one class in the batch, every launch filters its own trajectories (class_filter), so no kernel
// ever branches on p.  one(std::integral_constant<int, PM>, args) launches the class's kernel; the first error ends the sequence.
// Forms built for the always-thrust-limited laws only pass <PM_P0, PM_P1>.
// (A recursion, not a fold over the pack: the compiler emits a unit's kernels in the order these calls are instantiated, and a fold
// instantiates the last class first -- same kernels, but every local label of the device assembly renumbered.)
template <int CLASS, int... REST, class One>
static inline hipError_t for_classes_from(int pm, const IndirectArgs& a, One& one) {
  if (pm & (1 << CLASS)) {
    const hipError_t e = one(std::integral_constant<int, CLASS>{}, a);
    if (e != hipSuccess) return e;
  }
  if constexpr (sizeof...(REST) > 0) return for_classes_from<REST...>(pm, a, one);
  else return hipSuccess;
}
template <int... CLASSES, class One>
static inline hipError_t for_classes(int pm, const IndirectArgs& a0, One&& one) {
  IndirectArgs a = a0;
  a.class_filter = single_class(pm) ? 0 : 1;
  return for_classes_from<CLASSES...>(pm, a, one);
}

// Launchers return hipSuccess or the launch error.  `pm` is a bit mask of the PMode classes present in the batch (bit c = class c), `method` a Method.
// One launcher per family; ndim = 12 or 14 (where a family's two dimensions are separate translation units, the switch is in the 12-dim one).
hipError_t launch_indirect_defect(int ndim, int pm, int method, const IndirectArgs& a, hipStream_t st);
// cols_per_lane in {1,2,3}; 0 = choose from S.
hipError_t launch_indirect_stm(int ndim, int pm, int method, int cols_per_lane, const IndirectArgs& a, hipStream_t st);
// dense output: segment s is sampled at td[first[s] .. first[s+1]); Y is SoA [ndim][ldy]
struct DenseArgs {
  const int* first;        // [S+1] prefix offsets into td / columns of Y
  const double* td;        // [n_samples] sample times
  double* Y; long ldy;     // [ND][ldy]
  double* final_state;     // [ND][n_batch] or null: x(t_n) of every trajectory
};
hipError_t launch_indirect_dense(int ndim, int pm, int method, const IndirectArgs& a, const DenseArgs& d, hipStream_t st);
// Switch times, burn arcs and dv (kernels_events.hip).  The per-segment records of k_indirect_events, struct-of-arrays
// over the S segments, and what k_events_compact makes of them per trajectory.
constexpr int kEventsPerSeg = 4;   // crossings a segment keeps
struct EventsArgs {
  double* tev;                     // [kEventsPerSeg][S] crossing times of the segment, in order
  double* q;                       // [S] integral of umag over the segment (NaN: something of the segment is not finite)
  double* ont;                     // [S] time the engine is on inside the segment
  int* nev;                        // [S] crossings located (may exceed kEventsPerSeg: the true count)
  int* on_s; int* on_e;            // [S] on-state at the segment's start / end
  int max_events;
  int* n_events;                   // [B]
  double* t_event; int* kind;      // [B][max_events]
  int* on0;                        // [B]
  double* dv; double* burn;        // [B]
  double* dv_seg;                  // [S] or null
  int* status;                     // [B]
  // the variable-mass form only (null for 12 rows).  Behind everything else: the 12-row kernels read the same offsets.
  double* dm;                      // [S] node mass minus propagated mass (NaN with q)
  double* dm_seg;                  // [S] or null
  double* propellant;              // [B]
};
// 14 rows: one more double per segment (dm)
inline size_t events_record_bytes(long S, int ndim = 12) {
  return ((sizeof(double) * (kEventsPerSeg + 2 + (ndim == 14 ? 1 : 0)) + sizeof(int) * 3) * (size_t)S + 255) & ~(size_t)255;
}
// M_RK4 or M_DOP853_ADAPTIVE, nd = 12 or 14 (X [14][ldx], e.dm and e.propellant set); anything else: hipErrorInvalidValue
hipError_t launch_indirect_events(int nd, int pm, int method, const IndirectArgs& a, const EventsArgs& e, hipStream_t st);
hipError_t launch_events_compact(const IndirectArgs& a, const EventsArgs& e, int n_batch, hipStream_t st);
// Control replay (kernels_replay.hip).  The moment kernel: lamv [n_hist][n_knots][3] as the caller passes it, cp [n_knots]
// the Thomas factors of the (1, 4, 1) system, mom [n_knots][3 n_hist] scratch; vm [n_knots][6][n_hist] = per knot and component the
// value and the moment of the natural spline.
hipError_t launch_replay_moments(const double* lamv, const double* cp, double* mom, double* vm, int n_knots, int n_hist, double h,
                                 hipStream_t st);
// The replay itself: of `a` it reads tp / tp_stride, steps, rtol, atol and max_steps (max_steps per knot interval).
struct ReplayArgs {
  const double* vm; int n_hist;    // as above; n_hist = 1 or n_batch
  int n_knots, n_batch;
  double h;                        // (t1 - t0) / (n_knots - 1)
  const double* x0;                // [nstate][n_batch]
  double* x_final;                 // [nstate][n_batch]
  double* dv;                      // [n_batch]
  int* nacc; int* nrej;            // [n_batch], summed over the intervals
  int* status;                     // [n_batch]: 0 ok, 2 not finite / mass not positive / an interval out of max_steps
  double* samples; long ld_s;      // [nstate][ld_s], trajectory b's sample j in column b n_samples + j; null: none
  int n_samples, sample_every;     // knots k with k % sample_every == 0, and the last one
};
// nstate 6 or 7, method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_control_replay(int nstate, int pm, int method, const IndirectArgs& a, const ReplayArgs& r, hipStream_t st);
// Neighbouring-extremal guidance (kernels_guidance.hip), nx = 6 (12-row solutions) or 7 (14-row, variable mass).
// The backward sweep over the segment STMs of a 2 nx-row sweep: Phi [(2 nx)^2][ldp] (col * 2 nx + row, segment b (n_nodes - 1) + k);
// K [nx^2][(n_nodes - 1) n_batch] = the caller's [nx x nx x (n-1) x B].
struct GainsArgs {
  const double* Phi; long ldp;
  int n_nodes, n_batch;
  double sing_tol;
  double* K;
  double* pivot;                   // [(n_nodes - 1) n_batch] or null
  int* status;                     // [n_batch]: 0 ok, 2 not finite, 3 a pivot ratio below sing_tol
  int nx;                          // 6 or 7; anything else: hipErrorInvalidValue
};
hipError_t launch_guidance_gains(const GainsArgs& g, hipStream_t st);
// The guided flight: of `a` it reads tp / tp_stride, steps, rtol, atol and max_steps (max_steps per node interval).  Everything is
// laid out [row][lanes]: nom row k 2 nx + c, K row k nx^2 + r + nx c and t row k over n_nom = 1 or n_batch columns; x0 row c, nav row
// j nx + c, x_final / lam_final row c and nodes row k nx + c over n_batch columns.
struct GuidedArgs {
  const double* nom; const double* K; const double* t; int n_nom;
  int n_nodes, n_batch;
  int every;                       // update cadence in nodes, 0: never
  const double* x0;
  const double* nav;               // or null
  double* x_final;
  double* lam_final;               // or null
  double* dv;                      // [n_batch]
  double* nodes;                   // or null
  int* nacc; int* nrej;            // [n_batch], summed over the intervals
  int* status;                     // [n_batch]: 0 ok, 2 not finite / an interval out of max_steps / nx = 7: a mass not positive
  int nx;                          // 6 or 7; anything else: hipErrorInvalidValue
};
// method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_guided_flight(int pm, int method, const IndirectArgs& a, const GuidedArgs& g, hipStream_t st);
// Linear covariance of the guided flight (kernels_guidance_cov.hip): the forward pass over the Phi and K that the
// gains sweep left in HBM (their layouts as in GainsArgs).  P0, R [nx^2][n_cases] and every output are the caller's column-major
// arrays as they stand: P_nodes [nx^2][n_nodes][n_cases][n_batch], P_final [nx^2][n_cases][n_batch], status [n_cases][n_batch].
struct CovArgs {
  const double* Phi; long ldp;
  const double* K;
  int n_nodes, n_batch, n_cases;
  const double* P0; const double* R;
  const int* every;                // [n_cases], each >= 0
  double* P_nodes;                 // or null
  double* P_final;
  int* status;                     // 0 ok, 2 not finite
  int nx;                          // 6 or 7; anything else: hipErrorInvalidValue
};
hipError_t launch_guidance_covariance(const CovArgs& a, hipStream_t st);
// the caller's column-major [rows x count] <-> [row][count], any number of rows
hipError_t launch_rows_to_lanes(const double* aos, long rows, long count, double* soa, hipStream_t st);
hipError_t launch_lanes_to_rows(const double* soa, long rows, long count, double* aos, hipStream_t st);
// wave-specialised STM kernel (kernels_indirect_coop.hip): base wave + column waves per 16 segments
hipError_t launch_indirect_stm_coop(int ndim, int pm, int method, const IndirectArgs& a, hipStream_t st);
// the same with every 12-component state split over two lanes (kernels_indirect_coop2.hip), DOP853 adaptive only; the 14-dim form
// (kernels_indirect_coop2_14.hip) splits the states 7 + 7, thirteen columns: the always-thrust-limited laws (p = 0, 1) only
hipError_t launch_indirect_stm_coop2(int ndim, int pm, const IndirectArgs& a, hipStream_t st);
// defect-only sweep with two lanes per segment (kernels_indirect_defect2.hip): 12-dim, DOP853 adaptive only
hipError_t launch_indirect_defect2(int pm, const IndirectArgs& a, hipStream_t st);
// ... with four lanes per segment (same file): while the chip has a SIMD per 16 segments to spare; 14-dim for p = 0 / 1 batches
// (indirect_defect4_available)
hipError_t launch_indirect_defect4(int ndim, int pm, const IndirectArgs& a, hipStream_t st);
// three-role pipeline, fixed-step RK4 only: base wave, coefficient wave and column waves per 16 segments, skewed by one RK4 step.
// Eight-wave form (kernels_indirect_pipe8.hip): one STM column per lane with the coefficients broadcast inside the FMA (v_fmac_f64_dpp
// row_newbcast), two RK4 steps per phase, a fourth of the column work alternates between two SIMDs, base role with paired stages
hipError_t launch_indirect_stm_pipe8(int ndim, int pm, const IndirectArgs& a, hipStream_t st);
// large batches (kernels_indirect_pipe48.hip): 48 segments and 16 waves per workgroup, base lane = segment, DPP column rows
hipError_t launch_indirect_stm_pipe48(int ndim, int pm, const IndirectArgs& a, bool seg44, hipStream_t st);
hipError_t launch_indirect_stm_pipe32(int ndim, int pm, const IndirectArgs& a, hipStream_t st);   // kernels_indirect_pipe32.hip
// one RK4 step, lane = whole segment with all twelve STM columns (kernels_indirect_stream.hip): the HBM-bound corner of the sweep
hipError_t launch_indirect_stm_stream(int ndim, int pm, const IndirectArgs& a, hipStream_t st);
// RK4, any number of steps, lane = whole segment with the full STM (kernels_indirect_lane.hip): batches that fill the chip many times over
hipError_t launch_indirect_stm_lane(int pm, const IndirectArgs& a, hipStream_t st);
hipError_t launch_direct_defect(int nstate, const DirectArgs& a, hipStream_t st);
hipError_t launch_direct_jacobian(int nstate, const DirectArgs& a, hipStream_t st);
// base wave + one wave per sensitivity column for 32 segments, skewed by one RKF7(8) step (one barrier per step)
hipError_t launch_direct_jacobian_pipe(int nstate, const DirectArgs& a, hipStream_t st);

// Errors-driven mesh refinement of the direct transcription (kernels_direct_refine.hip).  All arrays node-major:
// the input as the caller passes it, the working copies with max_nodes (M) nodes of room per trajectory.
constexpr int kRefineLdsNodes = 1024;        // nodes whose estimates and links the removal's workgroup keeps in LDS (16 KB)
enum RefineCtl { RC_N, RC_CUR, RC_ACTIVE, RC_STATUS, RC_NSPLIT, RC_REMOVED, RC_PASSES, RC_ROWS };   // rows of ctl [RC_ROWS][B]
struct DirectRefineArgs {
  const double* X_in;              // [B][n_in][nstate]
  const double* U_in;              // [B][n_in][3]
  const double* t_in; int t_in_stride;   // [n_in] per trajectory (stride 0: one grid for all)
  int n_in, M, B;
  double MU, kk, isp_g0, TU;       // as DirectArgs
  int half_steps;
  double tol_min, tol_max;
  double *X[2], *U[2], *t[2], *E[2];   // working copies [B][M][nstate], [B][M][3], [B][M], [B][M] (E_i: estimate of segment i)
  double* E0;                      // [B][n_in] estimates of the input mesh
  int* ctl;                        // [RC_ROWS][B]: node count, current copy, in the insertion loop, status, splits of this pass, removed, passes
  int* list;                       // [B][M] segments split in this pass, in order
  double* rm_est; int* rm_link;    // removal above kRefineLdsNodes nodes: [B][n_in], [B][2][n_in]; else null
  double *X_out, *U_out, *t_out, *E_out;   // [B][M][nstate], [B][M][3], [B][M], [B][M-1]: NaN beyond the node count
};
// estimates of the input + the whole removal phase + compaction into copy 0
hipError_t launch_direct_refine_begin(int nstate, const DirectRefineArgs& a, hipStream_t st);
// one insertion pass; max_split: upper bound of the splits of one trajectory in this pass (sizes the evaluation's grid)
hipError_t launch_direct_refine_pass(int nstate, const DirectRefineArgs& a, int max_split, hipStream_t st);
hipError_t launch_direct_refine_finish(int nstate, const DirectRefineArgs& a, hipStream_t st);

// QP step of the direct method on the device (kernels_direct_qp.hip): the KKT system as a block-bidiagonal BVP, structured
// orthogonal cyclic reduction.  Operands in the SoA layouts of the direct sweeps; targets [n_batch][19] (lto_direct_targets).
struct DirectQpArgs {
  int n_nodes, n_batch;
  const double* Jac; long ldj;
  const double* defect; long ldd;
  const double* X; long ldx;
  const double* U; long ldu;
  const double* t; int t_stride;
  const double* targets;
  int impulsive;
  double c2;                       // (DU/TU)^2
  double* dX; long ldX;            // [nstate][ldX]
  double* dU; long ldU;            // [3][ldU]
  double* dV;                      // [n_batch][6]: impulse updates at node 0 and node n-1
  double* cost;                    // [n_batch]
  double* singular;                // [n_batch] or null: 1.0 where the trajectory's KKT system is singular
  // free ends only (nr = 3 or 4)
  const double* model;             // [n_batch][14] (lto_direct_end_model): g0[6], gf[6], |c0|, |cf|
  const double* beta;              // [n_batch]
  double* p;                       // [n_batch][2]: the phase updates p1, p2 ([n_batch][3] with p3 = tf_jump: nr = 4)
  // free time of flight only (nr = 4)
  const double* dtf;               // [nstate][ldd]: d defect / d tf
  const double* tfb;               // [n_batch][3]: step, tf_min, tf_max
  const double* tf;                // [n_batch]: current tf
};
// workspace of the step with nr right-hand sides (1, 3 or 4)
size_t direct_qp_workspace_bytes(int nstate, int n_nodes, int n_batch, int nr);
int* direct_qp_status(void* workspace, int n_batch);   // [n_batch] inside the workspace: 1 = singular
// nr right-hand sides: 1 frozen ends; 3 free ends (flagEnd = true): z0 | dz/dp1 | dz/dp2, then the 2 x 2 box QP in p; 4 free ends
// and free tf: z0 | dz/dp1 | dz/dp2 | dz/dp3, then the 3 x 3 box QP in p.  Any other nr: hipErrorInvalidValue.
hipError_t launch_direct_qp(int nstate, int nr, const DirectQpArgs& q, void* workspace, hipStream_t st);
hipError_t launch_direct_qp_update_dv(double* targets, const double* dV, const double* step, int n_batch, hipStream_t st);
// costates from the multipliers of the frozen step last solved in `workspace` (nr = 1): Lambda [nstate][ldl] entry
// b * n_nodes + k, mult [nstate][ldm] entry b * (n_nodes - 1) + i (null: not wanted), kkt_res [n_batch]; XC [12][ldxc] =
// (X; cc Lambda) for nstate 6 (null: not wanted; nstate 7 with XC: hipErrorInvalidValue).  acc: direct_costates_acc_bytes of device
// scratch.
struct DirectCostatesArgs {
  int n_nodes, n_batch;
  const double* Jac; long ldj;
  double* Lambda; long ldl;
  double* mult; long ldm;
  double* kkt_res;
  const double* X; long ldx;
  double* XC; long ldxc;
  double cc;
};
size_t direct_costates_acc_bytes(int n_batch);
hipError_t launch_direct_costates(int nstate, const DirectCostatesArgs& o, void* workspace, void* acc, hipStream_t st);
// the two orbit tables of the free-end model on the device: times [n], states and natural-spline second derivatives [n][6]
struct EndOrbitsDev { int n[2]; const double* t[2]; const double* Y[2]; const double* M[2]; };
// per trajectory b: s[b * s_stride + 0..11] = (s0; sf) at tau[2b], tau[2b+1], model[b][14] = (g0; gf; |c0|; |cf|)
hipError_t launch_end_states(const EndOrbitsDev& o, const double* tau, int n_batch, double* s, int s_stride, double* model,
                             hipStream_t st);
// addTimeFinal on the device (kernels_addtime.hip).  Re-mesh: K trajectories of m dense samples each, Y [rows][ldy]
// with trajectory b's samples in columns b*m .. b*m+m-1 at times td[b*m + j]; the natural spline of every row evaluated at the new
// nodes tn[b*n + k] into G [rows][ldg] (node b*n + k).  cp [m]: the Thomas factors of the (1, 4, 1) moment system; mom [m][rows K]:
// scratch.  rows = 12, or 14 for the variable-mass system.
struct RemeshArgs {
  const double* Y; long ldy;
  const double* td;
  const double* tn;
  const double* cp;
  double* mom;
  double* G; long ldg;
  int m, n, K;
};
hipError_t launch_remesh_spline(int rows, const RemeshArgs& r, hipStream_t st);
// find_tau: node n-1 of each of the K trajectories in G snapped onto the arrival table (o, e = 1); tau [K] = tau*
hipError_t launch_find_tau(const EndOrbitsDev& o, double* G, long ldg, int n, int K, double* tau, hipStream_t st);
// cost [K]: trapezoid over td of umag(|lambda_v|) along the dense outputs Y (layout as RemeshArgs), p / rho / aL of the control law
hipError_t launch_dense_cost(const double* Y, long ldy, const double* td, int m, int K, double aL, double p, double rho, double* cost,
                             hipStream_t st);
// the same along 14-row dense outputs Y [14][ldy]: lambda_v in rows 10..12, aL = cT / (row 6) per sample, cT = thrustLimit / 1e3 TU^2 / DU
hipError_t launch_dense_cost_mass(const double* Y, long ldy, const double* td, int m, int K, double cT, double p, double rho,
                                  double* cost, hipStream_t st);
// Stacked initial guesses (kernels_stack.hip), B starts side by side.  The device keeps everything per start as
// struct-of-arrays over the starts -- element (row, b) of an [R][B] array at row * B + b -- so a wavefront's 64 starts move lines.
constexpr int kStackCand = 1001;             // find_tau's candidates j / 1000
constexpr int kStackCandLd = 1024;           // leading dimension of the candidate table [6][kStackCandLd]
// Candidate table of the arrival orbit, cand [6][kStackCandLd] = s(j / 1000), and the start states y0 [6][B] = the departure
// spline at tau1 [B]
hipError_t launch_stack_prepare(const EndOrbitsDev& o, const double* tau1, int B, double* cand, double* y0, hipStream_t st);
// One ballistic coast per start: from y0 [6][B] at time t_start[b] through the nodes k0[b] <= k < k1[b] of its grid t [n][B], every
// node-to-node advance a fresh start of the integrator, the nodes into X [6 n][B] (row q n + k); then on to t_end[b], the state
// there into xe [6][B].  t_start / t_end null: 0 / the time of the last node.
struct StackArcArgs {
  const double* y0;
  const double* t;
  const int* k0; const int* k1;              // null k0: 0; null k1: n
  const double* t_start; const double* t_end;
  int n, B;
  double MU;
  int steps;                                 // RK4
  double rtol, atol; int max_steps;          // DOP853
  double* X;
  double* xe;
};
hipError_t launch_stack_arc(int method, const StackArcArgs& a, hipStream_t st);
// find_tau of the points x [6][B] over the candidate table: tau [B] = j* / 1000, gap [B] = the smallest distance, snap [6][B] =
// the arrival spline at tau (snap may be null).  With X_out set (the end search) the workgroup of start b also writes the start's
// nodes, X [6 n][B] with node n - 1 replaced by the snap, to X_out [B][n][6] and status[b] = 2 if any of them is not finite, else 0.
struct StackFindArgs {
  EndOrbitsDev o;
  const double* cand;
  const double* x;
  int n, B;
  double* tau; double* gap; double* snap;
  const double* X; double* X_out; int* status;
};
hipError_t launch_stack_find(const StackFindArgs& f, hipStream_t st);
// Periodic orbits with the xz-plane symmetry (kernels_halo.hip): 8 lanes per orbit, 8 orbits per wavefront.  Every
// array is in the caller's layout (orbit b's record contiguous).
// The differential corrector: seed [6][B] (x0, z0 and vy0 are read: rows 0, 2, 4), mode 0 hold z0 / 1 hold x0 / 2 planar.
struct HaloCorrectArgs {
  const double* seed;
  int B, mode, max_iter;
  double MU, tol, t_max, sing_tol;
  int steps;                                 // RK4: steps over t_max
  double rtol, atol; int max_steps;          // DOP853
  double* state;                             // [6][B]
  double* period; double* resid;             // [B]
  double* hist;                              // [max_iter + 1][B]
  int* iters; int* status;                   // [B]
};
// method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_halo_correct(int method, const HaloCorrectArgs& a, hipStream_t st);
// One revolution from state0 [6][B] over period [B], sampled at t_i = i P / (n - 1)
struct HaloTableArgs {
  const double* state0; const double* period;
  int n, B;
  double MU;
  int steps;                                 // RK4: steps per sample interval
  double rtol, atol; int max_steps;          // DOP853: max_steps counts per sample interval
  double* X;                                 // [6][n][B]
  double* M;                                 // [6][6][B]
  double* closure;                           // [B]
  double* jacobi; double* nu;                // [2][B]
  int* status;                               // [B]
};
hipError_t launch_halo_table(int method, const HaloTableArgs& a, hipStream_t st);
// The corrector with a target (kernels_halo_target.hip): the Jacobi constant (what = 0) or the period (what = 1) is
// asked for, (x0, z0, vy0) move -- planar: (x0, vy0) -- and orbit b's T members are corrected one after another in the launch, each
// from the secant through the last two.  Member (k, b) is record T b + k of every output.
struct HaloTargetArgs {
  const double* seed;                        // [6][B]
  const double* target;                      // [T][B]
  int T, B, planar, what, max_iter;
  double MU, tol, t_max, sing_tol;
  int steps;                                 // RK4: steps over t_max
  double rtol, atol; int max_steps;          // DOP853
  double* state;                             // [6][T][B]
  double* period; double* jacobi; double* resid;  // [T][B]
  double* hist;                              // [max_iter + 1][T][B]
  int* iters; int* status;                   // [T][B]
};
hipError_t launch_halo_target(int method, const HaloTargetArgs& a, hipStream_t st);
// Pseudo-arclength continuation of a family of periodic orbits (kernels_halo_arclength.hip): the unknowns (x0, z0, vy0)
// move along the family's tangent, the third equation keeps the iterate on the plane perpendicular to the tangent through the
// predicted point, and orbit b's T members, their step halvings and the growth of ds all run inside the launch.  Member (k, b) is
// record T b + k of every output.
struct HaloArclengthArgs {
  const double* seed;                        // [6][B]
  const double* dir0;                        // [3][B]
  const double* ds0;                         // [B]
  int T, B, planar, dir_is_tangent, max_iter, fast_iter;
  double MU, ds_min, ds_max, grow, cos_min, tol, t_max, sing_tol;
  int steps;                                 // RK4: steps over t_max
  double rtol, atol; int max_steps;          // DOP853
  double* state;                             // [6][T][B]
  double* tangent;                           // [3][T][B]
  double* det; double* ds; double* period; double* jacobi; double* resid;  // [T][B]
  double* hist;                              // [max_iter + 1][T][B]
  int* halvings; int* iters; int* status;    // [T][B]
};
hipError_t launch_halo_arclength(int method, const HaloArclengthArgs& a, hipStream_t st);
// Invariant manifolds of periodic orbits (kernels_manifold.hip).  Every array is in the caller's layout.
// Seeds: the hyperbolic pair of M [6][6][B] (one lane per orbit), the two eigenvectors carried along the orbit to the phases tau [P]
// (one lane per (orbit, phase, kind), kind 0 unstable forward over tau P, kind 1 stable backward over (1 - tau) P), then the starts
// and the statuses (one lane per (orbit, phase)).  Three kernels behind one another on the stream.
struct ManifoldSeedArgs {
  const double* state0; const double* period;  // [6][B], [B]
  const double* M;                             // [6][6][B]
  const double* tau;                           // [P], wrapped into [0, 1) by the host
  int P, B;
  double MU, eps;
  int steps;                                   // RK4: steps per flight
  double rtol, atol; int max_steps;            // DOP853
  double* lambda;                              // [2][B]
  double* vec0;                                // [6][2][B] scratch: (v_u, v_s) at phase 0
  double* eig_flag;                            // [B] scratch: 0 good, 1 no usable hyperbolic pair
  double* fly_flag;                            // [2][P][B] scratch: 0 good, 2 no finite result
  double* X; double* V;                        // [6][2][P][B]
  double* starts;                              // [6][4][P][B]
  int* status;                                 // [B]
};
// method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_manifold_seeds(int method, const ManifoldSeedArgs& a, hipStream_t st);
// Ballistic arcs to a Poincare section, one lane per arc
struct SectionFlightArgs {
  const double* y0; const double* t_max;       // [6][N], [N] signed
  int N, axis, dir, n_cross, n_samples;
  double MU, value, rmin1, rmin2;
  int steps;                                   // RK4: steps per span
  double rtol, atol; int max_steps;            // DOP853: max_steps counts per span
  double* x_end;                               // [6][N]
  double* t_end; double* dC;                   // [N]
  double* X;                                   // [6][n_samples][N], unused with n_samples = 0
  int* count; int* status;                     // [N]
};
hipError_t launch_section_flight(int method, const SectionFlightArgs& a, hipStream_t st);
// The nearest of Bs [6][nB] for each of A [6][nA]; dr / dv may be null
struct StateMatchArgs {
  const double* A; const double* Bs;
  int nA, nB;
  double w;
  int* index;
  double* dist; double* dr; double* dv;
};
hipError_t launch_state_match(const StateMatchArgs& a, hipStream_t st);
// Station-keeping on periodic orbits (kernels_stationkeep.hip).  Every array is in the caller's layout.
// Gains: one lane per (phase, orbit) record g = n_phase b + j of V [6][2][n] (0 unstable, 1 stable).  W and alpha may be null.
struct StationGainsArgs {
  const double* V;                             // [6][2][n]
  long n;                                      // n_phase n_batch
  double sing_tol;
  double* W;                                   // [6][n]
  double* G;                                   // [3][6][n], column-major 3 x 6 blocks
  double* alpha;                               // [n]
  int* status;                                 // [n]
};
hipError_t launch_stationkeep_gains(const StationGainsArgs& a, hipStream_t st);
// Flights with impulsive linear feedback, one lane per run; update u = r n_man + j, n_upd = n_rev n_man.  n_orb = 1: every run reads
// the one orbit's reference, gains and spans; n_orb = B: run b reads orbit b's.  nav, exe, dev, dv_hist, dev_final, n_burn, accepted,
// rejected and lost_at may be null.
struct StationFlightArgs {
  const double* X_ref; const double* dt; const double* G;   // [6][n_man][n_orb], [n_man][n_orb], [3][6][n_man][n_orb]
  const double* x0;                            // [6][B]
  const double* nav; const double* exe;        // [6][n_upd][B], [4][n_upd][B]
  int n_man, n_rev, B, n_orb;
  double MU, dv_min, dv_max, r_lost;
  int steps;                                   // RK4: steps per span
  double rtol, atol; int max_steps;            // DOP853: max_steps counts per span
  double* x_final;                             // [6][B]
  double* dv_total;                            // [B]
  double* dev;                                 // [2][n_upd][B]
  double* dv_hist;                             // [n_upd][B]
  double* dev_final;                           // [2][B]
  int* n_burn; int* accepted; int* rejected; int* status; int* lost_at;   // [B]
};
// method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_stationkeep_flight(int method, const StationFlightArgs& a, hipStream_t st);
// Target-point station-keeping.  Phase-to-phase STMs (kernels_halo_stm.hip): one group of 8 lanes per (phase, orbit)
// record g = P b + j; a coast over tau_j period_b, then the K spans (h_k - h_{k-1}) period_b with Phi carried through from the
// identity at the phase.  Xt, accepted and rejected may be null.
struct HaloStmArgs {
  const double* state0; const double* period;  // [6][B], [B]
  const double* tau;                           // [P], wrapped into [0, 1) by the host
  const double* horizon;                       // [K], in periods, strictly increasing from > 0
  int P, K, B;
  double MU;
  int steps;                                   // RK4: steps per span, the coast counting as one
  double rtol, atol; int max_steps;            // DOP853: max_steps counts per span
  double* X;                                   // [6][P][B]
  double* Phi;                                 // [6][6][K][P][B], column-major blocks
  double* Xt;                                  // [6][K][P][B]
  int* accepted; int* rejected; int* status;   // [P][B]
};
// method M_RK4 or M_DOP853_ADAPTIVE; anything else: hipErrorInvalidValue
hipError_t launch_halo_stm(int method, const HaloStmArgs& a, hipStream_t st);
// Target-point gains (kernels_stationkeep.hip): one lane per record of Phi [6][6][K][n].  pivot may be null.
struct StationTargetGainsArgs {
  const double* Phi;                           // [6][6][K][n]
  const double* r;                             // [K]
  int K; long n;
  double q, sing_tol;
  double* G;                                   // [3][6][n], column-major 3 x 6 blocks
  double* pivot;                               // [n]
  int* status;                                 // [n]
};
hipError_t launch_stationkeep_target_gains(const StationTargetGainsArgs& a, hipStream_t st);
// Mesh equidistribution of the indirect method (kernels_remesh.hip).  Grid: per trajectory b the monitor of old segment
// i is w[b (n-1) + i], or nacc + nrej there when w is null; old grids t[b t_stride + i].
// Out: t_out [n_batch][n_new] and seg_of [n_batch][n_new], the old node each new one is propagated from.
constexpr int kRemeshLdsSegs = 4096;         // segments whose partial sums one workgroup keeps in LDS
constexpr int kRemeshMaxSegs = 64 * 64 * 64; // three radix-64 levels
// doubles of scratch per trajectory above kRemeshLdsSegs segments (C, c_stride)
inline size_t remesh_scratch_doubles(int n) {
  const size_t m = (size_t)n - 1, m1 = (m + 63) / 64;
  return ((m + 63) & ~(size_t)63) + ((m1 + 63) & ~(size_t)63);
}
struct RemeshGridArgs {
  const double* t; int t_stride;
  int n, n_new, n_batch;
  const double* w;
  const int* nacc; const int* nrej;
  double* C; long c_stride;
  double* t_out;
  int* seg_of;
};
hipError_t launch_remesh_grid(const RemeshGridArgs& r, hipStream_t st);
// Nodes: a = the sweep arguments of the OLD trajectories (X, t, tp, the integrator); new node j = b n_new + k -> G [ndim][ldg]
// (ndim = 12, or 14 for the variable-mass system)
struct RemeshNodeArgs {
  const double* tn;
  const int* seg_of;
  double* G; long ldg;
  int n_new, n_batch;
};
hipError_t launch_remesh_nodes(int ndim, int pm, int method, const IndirectArgs& a, const RemeshNodeArgs& r, hipStream_t st);
// Resampling of direct solutions onto one node count (kernels_direct_resample.hip).  The current meshes, node-major
// with `cap` columns per trajectory of which the first n[b] are valid (n null: all of them), and what one pass makes of them.
struct DirectResampleArgs {
  const double* X;                 // [B][cap][nstate]
  const double* U;                 // [B][cap][3]
  const double* t;                 // [B][cap]
  const int* n;                    // [B] or null
  int cap, B, n_new;
  double MU, kk, isp_g0, TU;       // as DirectArgs
  int half_steps;
  double* E;                       // [B][cap-1] estimates of the current meshes, NaN behind the valid part
  int from_E;                      // 1: the weights are made from E; 0: W holds the caller's
  double w_floor;
  double* W;                       // [B][cap-1] weights
  double* C; long c_stride;        // running sums above kRemeshLdsSegs segments (remesh_scratch_doubles(cap) per trajectory), else null
  int* status;                     // [B], sticky: 0, 1 new times not strictly increasing, 2 a NaN estimate
  double* t_new;                   // [B][n_new]
  double *X_new, *U_new;           // [B][n_new][nstate], [B][n_new][3]
};
hipError_t launch_direct_resample_errors(int nstate, const DirectResampleArgs& a, hipStream_t st);   // -> E
hipError_t launch_direct_resample_grid(const DirectResampleArgs& a, hipStream_t st);                 // E or W -> W, t_new, status
hipError_t launch_direct_resample_nodes(int nstate, const DirectResampleArgs& a, hipStream_t st);    // t_new -> X_new, U_new
hipError_t launch_tau_update(double* tau, const double* p, const double* step, int n_batch, hipStream_t st);
// free tf: tau and tf updates from p [n_batch][3]; the grids t [n_batch][n] from tau_grid, t0 [n_batch], tf [n_batch] and their na
// copies per trajectory for the line search, tl [n_batch * na][n]
hipError_t launch_tf_update(double* tau, double* tf, const double* p, const double* step, const double* tfb, int n_batch,
                            hipStream_t st);
hipError_t launch_tf_grid(const double* taug, const double* t0, const double* tf, int n, int n_batch, double* t, double* tl, int na,
                          hipStream_t st);

// Newton step of the indirect method on the device (kernels_bvp.hip): structured orthogonal cyclic reduction, ndim = 12 or 14.
size_t bvp_workspace_doubles(int ndim, int n_nodes, int n_batch);
hipError_t launch_bvp_solve(int ndim, const double* Phi, long ldp, const double* defect, long ldd, int n_nodes, int n_batch,
                            int adjoints_only, double* workspace, double* delta, long ldx, hipStream_t st);
hipError_t launch_axpy(const double* x, const double* d, double alpha, double* y, long count, hipStream_t st);

hipError_t launch_pack_soa(const double* aos, int ndim, long count, double* soa, long ld, hipStream_t st);
hipError_t launch_unpack_soa(const double* soa, long ld, int ndim, long count, double* aos, hipStream_t st);
// two pack / unpack jobs in one launch
hipError_t launch_pack_soa2(const double* aos_a, int ndim_a, long count_a, double* soa_a, long ld_a, const double* aos_b, int ndim_b,
                            long count_b, double* soa_b, long ld_b, hipStream_t st);
hipError_t launch_unpack_soa2(const double* soa_a, long ld_a, int ndim_a, long count_a, double* aos_a, const double* soa_b, long ld_b,
                              int ndim_b, long count_b, double* aos_b, hipStream_t st);
constexpr int LTO_ORDER_BINS = 1024;   // int workspace launch_segment_order needs
// Windowed lane order (round 5): segments are ordered by step count INSIDE windows of LTO_ORDER_WINDOW consecutive segments, the
// windows by their slowest segment, heaviest first, dealt to the eight XCDs in turn (each XCD's windows contiguous in the order).
// With the sweep kernels' workgroups mapped to contiguous ranges per XCD (xcd_unit below), the wavefronts that share a window run
// on ONE XCD at about the same time: its L2 sees every line of the window's nodes, defects and Phi whole, so the sweep reads and
// writes the caller's struct-of-arrays operands directly -- no record passes (kernels.hpp IndirectArgs::Xa / Da / Pa).
constexpr int LTO_ORDER_WINDOW = 1024;       // largest window (one thread per segment in k_order_window)
constexpr int LTO_XCDS = 8;
// Window size for a batch of S segments: as close to 1 024 as gives every XCD the same number of windows -- 8 k windows for
// k = ceil(S / 8 192), a multiple of 16 segments (the interleave unit).  When S is a multiple of 8 192 (or is 4 096) the eight
// lists are equally long and ARE the contiguous eighths of the order the kernels' workgroups are mapped to (xcd_unit below).  At
// any other S the window is rounded up to 16 segments, the lists differ in length, and a few per cent of the positions are worked
// by a neighbouring XCD (DESIGN 4.9 has the figures; results do not depend on it).  S = 65 536, 262 144, 20 x 4 096: 1 024.
inline int order_window_size(long S) {
  const long k = (S + 8191) / 8192 > 0 ? (S + 8191) / 8192 : 1;
  long w = (S + 8 * k - 1) / (8 * k);
  w = (w + 15) / 16 * 16;
  return (int)(w < 16 ? 16 : (w > LTO_ORDER_WINDOW ? LTO_ORDER_WINDOW : w));
}
inline long order_windows(long S) { const long w = order_window_size(S); return (S + w - 1) / w; }
// ints of workspace behind the S entries of an order array: window-local order [S], per window (key, destination, slot) [3 nwin], bins
inline size_t order_workspace_ints(long S) { return (size_t)S + 3 * (size_t)order_windows(S) + LTO_ORDER_BINS + 64; }
inline size_t order_bytes(long S) { return sizeof(int) * ((size_t)S + order_workspace_ints(S)); }
hipError_t launch_segment_order_windowed(const int* nacc, const int* nrej, int S, int weave, int* work, int* order, hipStream_t st);
// Workgroup b of a grid of nb -> the unit it works on, such that the workgroups an XCD receives (round-robin dispatch: b mod 8) own a
// CONTIGUOUS range of units: the nodes two neighbouring units share, and the windows of an ordered sweep, then sit in one L2.
// A bijection of [0, nb) for every nb.
__device__ __forceinline__ int xcd_unit_of(const int b, const int nb) {
  const int x = b % LTO_XCDS, j = b / LTO_XCDS;
  const int chunk = nb / LTO_XCDS, rem = nb % LTO_XCDS;
  return x * chunk + (x < rem ? x : rem) + j;
}
// Only the windowed order wants the ranges: in natural order (slow segments cluster along a trajectory) and in the global order
// (heaviest first) a contiguous eighth per XCD would be an eighth of very different weight.
#define xcd_unit(a, b, nb) ((a).xcd_ranges ? xcd_unit_of((b), (nb)) : (b))
// node records for the staged sweeps: Xa[j][0..11] = X[c][j], Xa[j][12] = the node's time (t[b * t_stride + k], j = b n_nodes + k)
hipError_t launch_node_records(const double* X, long ldx, const double* t, int t_stride, int n_nodes, long J, double* Xa, hipStream_t st);
hipError_t launch_step_stats(const int* nacc, const int* nrej, int S, unsigned long long* acc, long long* host_out, hipStream_t st);
hipError_t launch_segment_order(const int* nacc, const int* nrej, int S, int* bins, int* order, hipStream_t st);
hipError_t launch_trial_points(const double* X, const double* d, long ld, int ndim, int n, int nb, int na, const double* alphas,
                               double* Xt, long ldt, hipStream_t st);
hipError_t launch_axpy_traj(const double* x, const double* d, const double* alpha, double* y, long ld, int ndim, int n, int nb,
                            hipStream_t st);
hipError_t launch_soc_mask(const double* mx, const double* act, double thr, double* step, int nb, hipStream_t st);
hipError_t launch_pick_alpha(const double* ss, const double* alphas, int na, const double* act, const double* search, double* step, int nb,
                             const double* mxt, double* mx, hipStream_t st);
hipError_t launch_take_trial(const double* trial, long ldt, const double* ss, const double* act, const double* search, int na, int seg,
                             int ndim, int nb, double* defect, long ldd, const double* alphas, double* step, const double* mxt, double* mx,
                             hipStream_t st);   // step != nullptr: also k_pick_alpha's outputs (one launch for both)
hipError_t launch_iter_report(const double* a, int na, const double* b, int nb, double* host_dev, long long* seq_dev, long long seq, hipStream_t st);
// pinned end entries (12 or 14 rows): saved[b][nd] = first node rows 0 .. nd/2-1, last node rows 0-5 (and 13 for nd = 14).
// restore = 0 saves them, for nd = 14 after setting the last node's row 13 (lambda_m(tf)) to 0; restore = 1 writes them back.
hipError_t launch_end_pins(double* X, long ld, int n, int nb, int nd, double* saved, int restore, hipStream_t st);
hipError_t launch_defect_norms(const double* defect, long ldd, int ndim, int seg_per_traj, int n_batch, double* sumsq,
                               double* maxabs, hipStream_t st);

}  // namespace lto
