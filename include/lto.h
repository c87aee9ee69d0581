/*
 * lto.h -- C ABI of liblto_hip.so: the MI355X (gfx950) multiple-shooting segment propagator.
 *
 * This is the drop-in boundary for the one data-parallel hot path of
 * travelingspaceman/LowThrustOpt: the `defectCalc` / `jacobianCalc` closures nested inside
 *   multiShoot_CRTBP_indirect  (src/multiShoot_CRTBP_indirect.jl:63-90, :93-146)
 *   multiShoot_CRTBP_direct    (src/multiShoot_CRTBP_direct.jl:66-109, :111-166, tf partial :503-516)
 * The reference has no FFI of its own (pure Julia); these entry points are what a `ccall` from the
 * two Julia drivers binds instead of running the closures' serial `for i = 1:n_nodes-1` loops
 * (INTEGRATION.md shows the Julia side).  Plain C: pointers, ints and doubles only.
 * Beyond the closures the library carries the drivers' loops and what they feed (Newton solves, QP steps, re-meshes, dense
 * output, thrust events) and the replay of a solution's thrust history from dispersed starts (lto_control_replay_batch), and
 * neighbouring-extremal guidance about a solution (lto_guidance_gains_batch, lto_guided_flight_batch, and their _mass forms).
 *
 * Conventions
 *   - All floating point data is binary64.  Host arrays use the reference's Julia layouts
 *     (column-major): XC_all is [ndim x n_nodes], defect is [ndim x (n_nodes-1)], ...
 *   - `n_batch` independent trajectories (line-search trial points, homotopy levels) can be swept by
 *     one call; host arrays then carry a trailing batch dimension.
 *   - Return value: 0 = ok; < 0 = API misuse; > 0 = runtime failure (see LTO_E*).  Non-finite
 *     results are not errors: NaN/Inf propagate into the outputs so the caller's driver reproduces the
 *     reference's status_flag = 2 path (src/multiShoot_CRTBP_indirect.jl:339-341).
 *   - The library never throws across the ABI: it is built without exception support, and what it allocates on the host
 *     inside a call (work arrays, its bookkeeping lists, the threads of a lto_group call) is checked -- running out of
 *     host memory or of threads there returns LTO_ENOMEM, it does not end the caller's process (a Julia session).  It
 *     installs no signal handlers and keeps
 *     no host pointer after a call returns.  One thread per context at a time; distinct contexts are
 *     independent.
 */
#ifndef LTO_H
#define LTO_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTO_VERSION 102 /* 0.1.2: round 6 added lto_comm_rccl_ranks, lto_last_call_order, lto_indirect_auto_kernel, lto_indirect_plan_set_output_layout; LTO_KERNEL_PIPE is now LTO_KERNEL_DIRECT_PIPE (same value), LTO_KERNEL_PIPE6_REMOVED is gone; lto_indirect_plan_set_cols_per_lane: 14 names the whole-segment one-step form of 14-dim plans, 2 is refused for 12-dim plans (0.1.1, round 5: LTO_ENOMEM, LTO_KERNEL_LANE, lto_indirect_plan_staging, lto_comm_set_kernel_payload, lto_kernel_lane_round_us) */

/* error codes */
#define LTO_OK 0
#define LTO_EINVAL (-1)       /* bad dimension / count / enum                                   */
#define LTO_ENULL (-2)        /* required pointer is NULL                                        */
#define LTO_EUNSUPPORTED (-3) /* valid request this build does not implement                     */
#define LTO_EHIP 1            /* HIP runtime error (message in lto_last_error)                   */
#define LTO_EBADP 2           /* reference: error("Invalid value of p!") stateCostate_deriv.jl:52 */
#define LTO_ENODEVICE 3       /* no usable gfx950 device                                         */
#define LTO_ENOMEM 4          /* host memory (or a host thread) could not be had inside a call   */
#define LTO_ESINGULAR 5       /* lto_direct_qp_step: a trajectory's KKT system is singular (its outputs are NaN) */

/* Integrators.  RK4 = GeneralCode/ode.jl:21-73; RKF78_FIXED = ode7_8, ode.jl:773-953 (the direct
 * path's integrator); RKF78_ADAPTIVE = ode78, ode.jl:364-544; DOP853_ADAPTIVE = order-8 adaptive pair
 * standing in for OrdinaryDiffEq's Vern8() at reltol=abstol=1e-13 (multiShoot_CRTBP_indirect.jl:79). */
#define LTO_RK4 0
#define LTO_RKF78_FIXED 1
#define LTO_RKF78_ADAPTIVE 2
#define LTO_DOP853_ADAPTIVE 3

typedef struct lto_ctx lto_ctx;
typedef struct lto_indirect_plan lto_indirect_plan;
typedef struct lto_direct_plan lto_direct_plan;

typedef struct lto_integrator {
  int method;    /* LTO_RK4 ...                                                        */
  int steps;     /* fixed-step methods: number of equal steps per segment              */
  double rtol;   /* adaptive methods (RKF78_ADAPTIVE uses rtol as ode78's `tol`)        */
  double atol;
  int max_steps; /* adaptive methods: per-segment cap on accepted+rejected steps (0 = 100000) */
} lto_integrator;

/* The reference's `params` tuple, src/multiShoot_CRTBP_indirect.jl:260 /
 * src/CRTBP_stateCostate_deriv.jl:13, field for field. */
typedef struct lto_params {
  double MU, DU, TU, thrustLimit, mass, time_direction, p, rho;
} lto_params;

/* Arguments the direct closures forward to ode7_8 / CRTBP_prop_EP_deriv
 * (src/multiShoot_CRTBP_direct.jl:86: MU, DU, TU, Isp). */
typedef struct lto_direct_params {
  double MU, DU, TU, Isp;
} lto_direct_params;

/* ------------------------------------------------------------------------------- context */
/* One context per GPU (one process per GPU under torch.distributed / one Julia task).  device_id
 * is the HIP ordinal.  Owns a stream, grow-only device staging buffers and the plans of the host-pointer
 * API (kept between calls: a Newton iteration calls with the same shapes and parameters every time).
 * Lifetime: plans from lto_*_plan_create keep their context alive -- lto_destroy with such plans
 * outstanding only marks the context, and the last lto_*_plan_destroy frees it (a garbage collector may
 * run the finalizers of a context and of its plans in any order). */
int lto_create(lto_ctx** out, int device_id);
void lto_destroy(lto_ctx* ctx);
/* Page-locked host memory for the arrays of the host-pointer API.  An operand that lies inside a block from here (the
 * whole block or any contiguous part of it) is read / written by the GPU in place: the layout kernels of the call are the
 * transfer and no copy operation is queued (Jacobian call at 4 096 segments: 0.20 ms, of which 0.09 ms are the 4.7 MB of
 * Phi crossing the link).  Other buffers work too: pageable ones are staged by the HIP runtime (0.31 ms for the same call).
 * Julia: unsafe_wrap the pointer as an Array and free it in a finalizer (julia/LowThrustOptHIP.jl: pinned_array). */
int lto_host_alloc(lto_ctx* ctx, size_t bytes, void** out);
/* Lifetime: a block keeps its context alive the way a plan does (lto_destroy only marks a context that still has blocks or
 * plans; whoever releases the last of them -- from any thread, in any order: finalizers -- frees it, exactly once).
 * lto_host_free(NULL, ptr) is allowed: the owner of a block is looked up, so a finalizer need not keep the handle.  Freeing a
 * pointer that is not a live block returns LTO_EINVAL. */
int lto_host_free(lto_ctx* ctx, void* ptr);
const char* lto_last_error(const lto_ctx* ctx);
int lto_version(void);
void* lto_ctx_stream(lto_ctx* ctx); /* the context's own non-blocking hipStream_t */
int lto_ctx_device(const lto_ctx* ctx); /* HIP ordinal the context was created on */
/* When enabled, every sweep brackets its dominant kernel with HIP events on the launch stream;
 * lto_last_kernel_ms blocks on the stop event and returns that kernel's duration. */
int lto_set_timing(lto_ctx* ctx, int enabled);
double lto_last_kernel_ms(lto_ctx* ctx);
/* Wall time [ms] of the last host-pointer call on this context (lto_indirect_defect, lto_indirect_jacobian, lto_direct_*),
 * from entry to return as measured inside the library: what a C or Julia caller waits for, without a binding's overhead. */
double lto_last_call_ms(const lto_ctx* ctx);
/* Lane order the last host-pointer indirect call of this context swept with: 0 = natural, 1 = the global order, 2 = the windowed
 * order (both made from an earlier call's step counts and kept in the context, one slot per kind: defect sweeps take the windowed
 * order, STM sweeps and Newton steps the global one, so a loop that alternates defectCalc and jacobianCalc keeps both). */
int lto_last_call_order(const lto_ctx* ctx);

/* Kernel choice of the RK4 STM sweeps above one round of workgroups (lto_indirect_plan_set_kernel, LTO_KERNEL_AUTO): the family
 * whose rounds are cheapest for the segment count, from a table of microseconds per round at 64 steps -- us_per_round[0]:
 * eight-wave pipeline, rounds of 16 x CUs segments; [1]: large-batch pipeline with 48 segments per workgroup, 48 x CUs; [2]:
 * per-lane kernel with three columns, 64 x CUs; [3]: large-batch pipeline with 44 segments per workgroup, 44 x CUs; [4]:
 * 32-segment / twelve-wave pipeline (LTO_KERNEL_PIPE32), 32 x CUs ([2], [3]: 12-dim only, reported as -1 for 14;
 * LTO_KERNEL_PIPE48 stands for both of its forms and the cheaper one runs).  A new context holds the figures measured on MI355X
 * (profiles/r04z).  lto_calibrate_kernels measures them on the context's own device (about 50 ms: 30 ms of warm-up sweeps, then
 * the median of five launches of one full round per family and dimension) and AUTO uses those from then on;
 * lto_kernel_round_costs reads the table (us_per_round[5]; *calibrated = 1 after a calibration).  Results never depend on the
 * choice. */
int lto_calibrate_kernels(lto_ctx* ctx);
int lto_kernel_round_costs(const lto_ctx* ctx, int ndim, double* us_per_round, int* calibrated);
/* The sixth family AUTO weighs for ndim = 12 (round 5; kept out of the five-entry table so that its callers' arrays stay valid):
 * microseconds per round of 256 x CUs segments at 64 steps of the whole-segment lanes (LTO_KERNEL_LANE) -- 505 on MI355X by
 * default, this device's figure after lto_calibrate_kernels (which then also sweeps one such round: ~5 ms more, and the context's
 * work arena grows to ~110 MB). */
double lto_kernel_lane_round_us(const lto_ctx* ctx);

/* --------------------------------------------------------- host-pointer API (what Julia ccalls)
 * Each call: plan looked up in the context's cache by (shape, integrator, parameter values) -> H2D ->
 * sweep -> D2H -> one stream synchronise.  The caller's buffers are only touched inside the call. */

/* Replaces defectCalc of multiShoot_CRTBP_indirect (src/multiShoot_CRTBP_indirect.jl:63-90).
 *   XC      [ndim x n_nodes x n_batch]   ndim = 12: the reference's state+costate system.
 *                                        ndim = 14: (r, v, m, lambda_r, lambda_v, lambda_m), an EXTENSION with no
 *                                        reference counterpart (BASELINE configs[1]; model after
 *                                        GeneralCode/twoBody_stateCostate_mass_deriv.jl:11-78 in CRTBP units); the
 *                                        `mass` field of lto_params then carries Isp [s] (mass is state[7]).
 *   t       [n_nodes x n_tgrids]         n_tgrids = 1 (shared grid) or n_batch
 *   prm     [n_prm]                      n_prm = 1 or n_batch
 *   defect  [ndim x (n_nodes-1) x n_batch]  = x(t_{i+1}; XC[:,i]) - XC[:,i+1]          (:82)
 *   errors  [(n_nodes-1) x n_batch] or NULL: 0 for RK4 / adaptive (reference: always 0, :85),
 *           RKF7(8) 8th-order estimate for RKF78_FIXED. */
int lto_indirect_defect(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                        int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, double* defect,
                        double* errors);

/* Replaces jacobianCalc of multiShoot_CRTBP_indirect (:93-146), compact form:
 *   Phi     [ndim x ndim x (n_nodes-1) x n_batch], Phi[:,:,i] = d x(t_{i+1}) / d XC[:,i]
 *           (= ForwardDiff.jacobian(f, x0), :121).  The caller forms [Phi_i | -I] (:123), the band
 *           scatter (:128-138) and the fixed-endpoint column mask (:141-142).
 *   defect  as above, or NULL. */
int lto_indirect_jacobian(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                          int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, double* Phi,
                          double* defect);

/* One whole Newton iteration of multiShoot_CRTBP_indirect (indirect.jl:290-296): jacobianCalc (:93-146), the
 * least-squares step of optimizeTraj_OLS (:149-218) incl. the flag_adjointsOnly column mask (:169-178) and the
 * second-order correction (:190-214, applied when norm(xc_update, Inf) < soc_threshold; the reference uses 1e-1).
 * Only XC and t are uploaded and xc_update [ndim x n_nodes x n_batch] and (optionally) the nominal defect are
 * downloaded; Phi stays in HBM.  ndim = 12 or 14 (pinned entries: see lto_indirect_solve); the step reads XC as given (it does
 * not reset lambda_m(tf)) and leaves exact zeros in the pinned entries of xc_update. */
int lto_indirect_newton_step(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                             int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ,
                             int flag_adjointsOnly, double soc_threshold, double* xc_update, double* defect);

/* The whole Newton loop of multiShoot_CRTBP_indirect (src/multiShoot_CRTBP_indirect.jl:254-345) in one call, trajectory
 * resident in HBM: while max|defect| > 1e-10 { jacobianCalc; optimizeTraj_OLS incl. adjoints-only mask and second-order
 * correction (:149-218); after iteration 3 the 20-point lineSearch (:221-246) as ONE batched sweep; XC += alpha *
 * xc_update; end states re-pinned (:324-325); defectCalc }.  Only scalars cross PCIe inside the loop.
 *   ndim = 12: the reference's system; pinned XC[0:6, 0] and XC[0:6, n-1] (the end states).
 *   ndim = 14: the variable-mass system (r, v, m, lambda_r, lambda_v, lambda_m), Isp in prm->mass; pinned XC[0:7, 0] (r0, v0 and
 *              the initial mass m0) and XC[0:6, n-1] (rf, vf) and XC[13, n-1] = lambda_m(tf) = 0, the transversality condition of
 *              the FREE final mass XC[6, n-1].  The loop sets XC[13, n-1] to 0 on entry.  Unknowns 7 + 14(n-2) + 7 = 14(n-1):
 *              the regular step is square; adjoints-only masks the 7 state columns of every node (least squares).
 *   XC_in, XC_out [ndim x n_nodes] (may alias), defect [ndim x (n_nodes-1)] or NULL,
 *   *status_flag: 0 converged, 1 maxIter reached (also after "Not likely to converge", :333-336), 2 NaN (:339-341),
 *   *iterations (or NULL): the reference's iterCount on exit,
 *   history (or NULL): [2 x maxIter] column k = (max|defect|, alpha) after iteration k+1 -- the progress line of :332. */
int lto_indirect_solve(lto_ctx* ctx, int ndim, int n_nodes, const double* XC_in, const double* t, const lto_params* prm,
                       const lto_integrator* integ, int flag_adjointsOnly, int maxIter, double* XC_out, double* defect,
                       int* status_flag, int* iterations, double* history);

/* n_batch independent problems through the same loop, side by side (homotopy / thrust levels, several initial guesses:
 * the concurrent form of the continuation of src/HelperFunctions.jl:105-193).  Every device operation covers the
 * whole batch; a trajectory that has left the reference loop (converged, NaN, iteration limit) is frozen by a zero
 * step length.  Arrays carry a trailing batch dimension: XC [ndim x n_nodes x n_batch], t [n_nodes x n_tgrids],
 * prm [n_prm] (n_tgrids, n_prm = 1 or n_batch), defect [ndim x (n_nodes-1) x n_batch], status_flag / iterations
 * [n_batch], history [2 x maxIter x n_batch]. */
int lto_indirect_solve_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC_in, const double* t,
                             int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ,
                             int flag_adjointsOnly, int maxIter, double* XC_out, double* defect, int* status_flag,
                             int* iterations, double* history);

/* Replaces densify (src/HelperFunctions.jl:51-101) for one trajectory: t_dense = LinRange(t[1], t[end], n_desired),
 * every segment re-propagated from its node and sampled at the t_dense points inside [t_i, t_{i+1}), final propagated
 * state appended.  XC_dense [ndim x n_desired], t_dense [n_desired]. */
int lto_indirect_densify(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                         const lto_integrator* integ, int n_desired, double* XC_dense, double* t_dense);
/* The same for one trajectory of the 14-row variable-mass system: XC [14 x n_nodes], XC_dense [14 x n_desired], Isp in
 * prm->mass as everywhere for 14 rows.  lto_indirect_densify itself keeps answering LTO_EUNSUPPORTED to ndim = 14.  LTO_RK4 or
 * LTO_DOP853_ADAPTIVE; any other method: LTO_EUNSUPPORTED.  LTO_ENULL; LTO_EINVAL (n_nodes < 2, n_desired < 2). */
int lto_indirect_densify_mass(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                              const lto_integrator* integ, int n_desired, double* XC_dense, double* t_dense);

/* Replaces defectCalc of multiShoot_CRTBP_direct (src/multiShoot_CRTBP_direct.jl:66-109).
 *   X [nstate x n_nodes x n_batch] (nstate = 6 or 7), U [3 x n_nodes x n_batch] thrust in N,
 *   nsteps = points of the half-segment grid, i.e. nsteps-1 RKF7(8) steps per half (:84).
 *   defect [nstate x (n_nodes-1) x n_batch], errors [(n_nodes-1) x n_batch] (:104). */
int lto_direct_defect(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                      const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double* defect,
                      double* errors);

/* The propagation inside meshRefine_direct (src/multiShoot_CRTBP_direct.jl:645-656): x_mid[:, i] = state at
 * t_i + (t_{i+1} - t_i)/2 propagated forward from node i with control u_i, for EVERY segment in one sweep (the
 * reference propagates one segment per refinement pass with ode7 = one RKF7(8) step, i.e. nsteps = 2).
 *   x_mid [nstate x (n_nodes-1) x n_batch]; defect, errors as lto_direct_defect on the same grid, or NULL. */
int lto_direct_midpoints(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                         const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double* x_mid,
                         double* defect, double* errors);

/* Replaces meshRefine_direct (src/multiShoot_CRTBP_direct.jl:597-680) for n_batch trajectories in one call, on the device
 * (DESIGN 4.14).  Inputs as lto_direct_defect.  Per trajectory, with the estimates of lto_direct_defect at `nsteps`:
 *   removal    while n > 2 and min(errors) < tol_min: k = the first arg-min (0 becomes 1), node k is deleted;
 *   insertion  while max(errors) > tol_max and n < max_nodes: in index order every segment with errors > tol_max is split, at
 *              most max_nodes - n per pass: time t_i + (t_{i+1} - t_i)/2, state = lto_direct_midpoints' at nsteps = 2 (one
 *              RKF7(8) step, the reference's ode7), control (u_i + u_{i+1})/2.
 * Kept nodes, controls and times are bit copies; the first and the last node stay.  A segment whose propagated states are not
 * numbers has a NaN estimate, which ends both phases for its trajectory.
 *   max_nodes  the insertion's node limit AND the capacity of the outputs per trajectory (>= n_nodes)
 *   X_out [nstate x max_nodes x n_batch], U_out [3 x max_nodes x n_batch] or NULL, t_out [max_nodes x n_batch]: the first
 *              n_out[b] columns of trajectory b, NaN from there on
 *   errors_out [(max_nodes-1) x n_batch] or NULL: the estimates of the final mesh (n_out[b] - 1 of them, then NaN)
 *   n_removed, passes (insertion passes), status [n_batch], each or NULL.  status: 0 refined (min >= tol_min or two nodes
 *              left, and max <= tol_max), 1 stopped at max_nodes with max > tol_max, 2 a NaN estimate.
 * Limits (LTO_EINVAL beyond them): n_batch <= 65535 and max_nodes * n_batch * nstate <= 2^31 - 1.  The call's device scratch is
 * about 37 doubles per node of capacity (max_nodes * n_batch); the whole capacity is filled and copied back, so give
 * max_nodes as a limit near the size expected, not as "unbounded". */
int lto_direct_refine_batch(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                            const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double tol_min,
                            double tol_max, int max_nodes, double* X_out, double* U_out, double* t_out, int* n_out,
                            int* n_removed, int* passes, int* status, double* errors_out);
/* One trajectory (n_batch = 1). */
int lto_direct_refine(lto_ctx* ctx, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                      const lto_direct_params* prm, double tol_min, double tol_max, int max_nodes, double* X_out,
                      double* U_out, double* t_out, int* n_out, int* n_removed, int* passes, int* status,
                      double* errors_out);

/* Direct solutions resampled onto ONE node count n_new, on the device (the reference has no counterpart: its
 * meshRefine_direct bisects and deletes, it never moves a node).  The input may be ragged, as lto_direct_refine_batch writes it:
 *   X [nstate x n_cap x n_batch], U [3 x n_cap x n_batch], t [n_cap x n_batch]; trajectory b is its first n_in[b] columns
 *   (n_in NULL: n_cap everywhere).  Columns from n_in[b] on are never read into a result; they may hold NaN.
 * Per trajectory and pass, with n = its node count (n_in[b], then n_new):
 *   estimates  e_i = the errors of lto_direct_defect at `nsteps` on the valid part, bit for bit; a segment whose propagated
 *              states are not numbers has a NaN estimate;
 *   monitor    r_i = e_i^(1/8) (the estimate is the local error of the 7th-order solution, e ~ C h^8), w_i = max(r_i,
 *              w_floor * max_j r_j); all weights 1 if every r_j is 0.  `weights` [(n_cap-1) x n_batch] (finite, > 0 on every
 *              valid segment; passes must be 1) replace estimates and monitor;
 *   grid       C_0 = 0, C_{i+1} = C_i + w_i; t'_k = t_i + (g_k - C_i)/w_i (t_{i+1} - t_i) at g_k = k C_{n-1}/(n_new - 1), i the
 *              largest index with C_i <= g_k; the end points are the old ones bit for bit;
 *   nodes      i = the largest index with t_i <= t'_k, t_mid = t_i + (t_{i+1} - t_i)/2.  t'_k == t_i, or the last node: a bit
 *              copy of that node's state and control.  t'_k <= t_mid: forward from x_i with u_i over t'_k - t_i.  Otherwise
 *              backward from x_{i+1} (velocity reversed, u_{i+1}) over t_{i+1} - t'_k.  nsteps - 1 equal RKF7(8) steps; at
 *              t'_k == t_mid the span is the sweep's 0.5 (t_{i+1} - t_i), so the state is lto_direct_midpoints' at `nsteps`
 *              bit for bit.  Control u_i + s (u_{i+1} - u_i), s = (t'_k - t_i)/(t_{i+1} - t_i).
 * Each further pass repeats this on the previous pass's output.  The call does not re-solve: the output is a guess in the
 * layout lto_direct_solve_batch takes.
 *   X_out [nstate x n_new x n_batch], U_out [3 x n_new x n_batch], t_out [n_new x n_batch]
 *   errors_before [(n_cap-1) x n_batch] or NULL: the estimates of the input, NaN from n_in[b] - 1 on
 *   errors_after  [(n_new-1) x n_batch] or NULL: the estimates of the output meshes
 *   status [n_batch] or NULL: 0 resampled; 1 the new times of a pass were not strictly increasing (n_new beyond what the grid
 *              resolves); 2 a NaN estimate inside the valid part.  With status != 0 the trajectory's outputs are NaN; the
 *              others are untouched and the call still returns LTO_OK.
 * LTO_ENULL: a NULL X, U, t, prm, X_out, U_out or t_out.  LTO_EINVAL: nstate not 6 or 7; n_cap < 2; n_batch < 1; n_new < 2;
 * passes < 1; nsteps < 2; w_floor outside [0, 1) or not finite; an n_in[b] outside [2, n_cap]; times not finite or not strictly
 * increasing inside a valid part; a weight of a valid segment not finite or <= 0; weights with passes > 1; more than 262 144
 * segments per trajectory (max(n_cap, n_new) - 1); n_batch > 65535; max(n_cap, n_new) * n_batch * nstate > 2^31 - 1. */
int lto_direct_resample_batch(lto_ctx* ctx, int nstate, int n_cap, int n_batch, const double* X, const double* U,
                              const double* t, const int* n_in, int nsteps, const lto_direct_params* prm, int n_new,
                              const double* weights, double w_floor, int passes, double* X_out, double* U_out, double* t_out,
                              double* errors_before, double* errors_after, int* status);
/* One trajectory of n_nodes nodes (n_batch = 1, n_in = NULL). */
int lto_direct_resample(lto_ctx* ctx, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                        const lto_direct_params* prm, int n_new, const double* weights, double w_floor, int passes,
                        double* X_out, double* U_out, double* t_out, double* errors_before, double* errors_after, int* status);

/* Replaces jacobianCalc of multiShoot_CRTBP_direct (:111-143) and the tf partial (:503-516).
 *   Jac_temp    [nstate x nvar x (n_nodes-1) x n_batch], nvar = 2(nstate+3); block i is
 *               d defect_i / d [x_i; x_{i+1}; u_i; u_{i+1}] (variable order of :125), computed from
 *               the variational equations instead of the reference's forward differences.
 *   ddefect_dtf [nstate x (n_nodes-1) x n_batch] or NULL (last column of Jac_full, :516)
 *   defect, errors as lto_direct_defect, or NULL. */
int lto_direct_jacobian(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                        const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double* Jac_temp,
                        double* ddefect_dtf, double* defect, double* errors);

/* ---- Direct multiple shooting: the QP step and the loop of multiShoot_CRTBP_direct (src/multiShoot_CRTBP_direct.jl:477-594)
 * for the reference demo's setting (CRTBP_Multishoot_direct_demo.jl:183-193): flagEnd = false, beta = 0, tf fixed (tf_jump = 0,
 * :292).  optimizeTraj (:248-403) is then a convex QP with equality constraints only,
 *   min  sum_k w_k |u_k + du_k|^2 + (DU/TU)^2 (|dV1 + d1|^2 + |dV2 + d2|^2)      w_k = trapezoid weights of t (:323-326)
 *   s.t. Jac_i [dx_i; dx_{i+1}; du_i; du_{i+1}] = -defect_i                         (:337)
 *        x_0[0:6] + dx_0[0:6] + [0; dV1 + d1] = s0,  x_{n-1}[0:6] + dx_{n-1}[0:6] + [0; dV2 + d2] = sf   (:370-375)
 *        x_0[6] + dx_0[6] = mass (nstate 7, :269-271);  d1 = d2 = 0 unless allow_impulsive (:298-302),
 * solved on the device exactly (its KKT system as a block-bidiagonal BVP, structured orthogonal cyclic reduction).
 * Per-trajectory targets: the interpolated end states (interpEndStates, :434-461), the initial mass and the current impulses. */
typedef struct lto_direct_targets {
  double s0[6], sf[6], mass, dV1[3], dV2[3];
} lto_direct_targets;
/* One Jacobian sweep (lto_direct_jacobian) and one QP step.  Host arrays as lto_direct_jacobian; targets [n_targets] with
 * n_targets = 1 or n_batch.  Outputs: dX [nstate x n_nodes x n_batch], dU [3 x n_nodes x n_batch] (N), dV [6 x n_batch] (the
 * impulse updates d1; d2 -- zero unless allow_impulsive), cost [n_batch] (the QP objective at the step).  A singular KKT system
 * (e.g. too few nodes to reach the terminal state) returns LTO_ESINGULAR with that trajectory's outputs NaN. */
int lto_direct_qp_step(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                       int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets, int n_targets,
                       int allow_impulsive, double* dX, double* dU, double* dV, double* cost);
/* The loop of multiShoot_CRTBP_direct (:477-594) with the trajectories resident in HBM: defect sweep, then while
 * max|defect| > 1e-6 (:491): Jacobian sweep, QP step, line search over LinRange(0.1, 1, 10) after iteration 10 (:557-560, the ten
 * trial points of every trajectory in ONE batched defect sweep), update of X, U, dV1, dV2 (:562-569), t recomputed through tau
 * (:582), defect sweep.  Only scalars cross the link inside the loop; finished trajectories are frozen with a zero step.
 *   X_in/X_out [nstate x n_nodes x n_batch], U_in/U_out [3 x n_nodes x n_batch], t [n_nodes x n_tgrids], targets [n_targets]
 *   (1 or n_batch); dV_out [6 x n_batch] (final dV1; dV2), t_out [n_nodes x n_batch], defect_out [nstate x (n_nodes-1) x n_batch]
 *   (all outputs but X_out and status may be NULL); history [3 x maxIter x n_batch] = (max|defect|, cost, alpha) per iteration.
 *   status [n_batch]: 0 converged, 1 maxIter reached, 2 NaN, 3 singular KKT system.  The reference prints and returns; the flags
 *   extend it with the indirect driver's convention (lto_indirect_solve). */
int lto_direct_solve_batch(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                           const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                           const lto_direct_targets* targets, int n_targets, int allow_impulsive, int maxIter, double* X_out,
                           double* U_out, double* dV_out, double* t_out, double* defect_out, int* status, int* iterations,
                           double* history);
int lto_direct_solve(lto_ctx* ctx, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t, int nsteps,
                     const lto_direct_params* prm, const lto_direct_targets* targets, int allow_impulsive, int maxIter,
                     double* X_out, double* U_out, double* dV_out, double* t_out, double* defect_out, int* status,
                     int* iterations, double* history);

/* ---- Free end points (flagEnd = true, src/multiShoot_CRTBP_direct.jl:278-292, :353-369, :521-569): the optimiser also moves the
 * departure phase tau1 on orbit 1 and the arrival phase tau2 on orbit 2.  With s(.) = interpEndStates (each argument wrapped into
 * [0, 1] on its own) and h = 0.05, the end model at (tau1, tau2) is s0 = s(tau1), g0 = (s(tau1+h) - s(tau1-h)) / 2h,
 * c0 = (s(tau1+h) - 2 s(tau1) + s(tau1-h)) / h^2, and sf, gf, cf the same at tau2 on orbit 2.  A free step solves the frozen step's
 * QP with the end constraints x_0[0:6] + dx_0[0:6] + [0; dV1 + d1] = s0 + g0 p1, x_{n-1}[0:6] + dx_{n-1}[0:6] + [0; dV2 + d2] =
 * sf + gf p2, the bounds |p1|, |p2| <= 0.1 and the cost term beta (|c0|/2 p1^2 + |cf|/2 p2^2); tf stays fixed (:292). */
typedef struct lto_direct_orbits {
  int n0, nf;                        /* samples of the departure and arrival orbit tables (>= 2 each) */
  const double* t0;                  /* [n0] strictly increasing normalised times (host) */
  const double* X0;                  /* [6 x n0] column-major: the state of sample i at X0[6 i .. 6 i + 5] (host) */
  const double* tf;                  /* [nf] */
  const double* Xf;                  /* [6 x nf] */
} lto_direct_orbits;
typedef struct lto_direct_end_model {
  double g0[6], gf[6], c0_norm, cf_norm;     /* g0, gf and the 2-norms of c0, cf */
} lto_direct_end_model;
/* End targets and end model of n_batch trajectories on the device: tau [2 x n_batch] = (tau1; tau2) per trajectory, s_out
 * [12 x n_batch] = (s0; sf), model [n_batch].  The natural-spline moments of the tables are solved on the host once per call. */
int lto_direct_end_states(lto_ctx* ctx, const lto_direct_orbits* orbits, int n_batch, const double* tau, double* s_out,
                          lto_direct_end_model* model);
/* addTimeFinal (src/HelperFunctions.jl:196-250, re-specified): a new time of flight for a converged 12-dim solution XC
 * [12 x n_nodes] on t [n_nodes], for each of n_dt changes dt[k] > 0 (TU) side by side.  Per k: the end costates are zeroed (on a
 * copy) and a ballistic tail node is appended at t_end = t[n-1] + dt[k]; the extended trajectory is densified at
 * LinRange(t[0], t_end, n_desired) (the final propagated state last, as lto_indirect_densify); each component's natural cubic
 * spline through the samples is evaluated at t_out = LinRange(t[0], t_end, n_nodes) (the samples themselves at both ends); the
 * last node's position and velocity are replaced by s(tau*) of the arrival table, tau* the first minimiser of |s(j / 1000) - x|_2
 * over j = 0..1000 (find_tau); then, when XC_out is not NULL, the fixed-end Newton loop of lto_indirect_solve_batch runs on t_out.
 * Only orbits->nf, tf and Xf are read.  Outputs: t_out [n_nodes x n_dt], tau_out [n_dt], XC_guess [12 x n_nodes x n_dt] (the
 * re-meshed guesses; may be NULL), XC_out, defect, status_flag, iterations, history as lto_indirect_solve_batch with n_batch = n_dt
 * (XC_out NULL: guesses only), cost [n_dt] (may be NULL): trapezoid over the n_desired-point dense output of XC_out of the thrust
 * acceleration magnitude umag(|lambda_v|), in DU/TU.  ndim != 12 or an integrator other than LTO_RK4 / LTO_DOP853_ADAPTIVE:
 * LTO_EUNSUPPORTED; a dt <= 0 or not finite, n_desired < 4: LTO_EINVAL. */
int lto_indirect_add_time_batch(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                                const lto_integrator* integ, const lto_direct_orbits* orbits, int n_dt, const double* dt,
                                int n_desired, int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out,
                                double* tau_out, double* defect, int* status_flag, int* iterations, double* history, double* cost);
int lto_indirect_add_time(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                          const lto_integrator* integ, const lto_direct_orbits* orbits, double dt, int n_desired,
                          int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out, double* tau_out,
                          double* defect, int* status_flag, int* iterations, double* history, double* cost);
/* The same for a converged solution of the 14-row variable-mass system y = (r, v, m, lambda_r, lambda_v, lambda_m): XC
 * [14 x n_nodes], prm with Isp in the mass slot; the arguments of lto_indirect_add_time_batch without ndim, its layouts with 14 rows,
 * plus propellant at the end.  Per k: rows 7..13 of the last node are zeroed (on a copy) and the tail node appended at t[n-1] + dt[k].
 * The tail is the 14-row system's own flow from that node, not a second system: with |lambda_v| = 0 the thrust acceleration is
 * exactly zero, so position and velocity coast and rows 7..13 stay exactly 0, while the mass follows mdot = -kappa umag(0, m) m of the
 * same right-hand side -- zero for p > 1 (the mass is constant bit for bit), the full-throttle flow for p = 0, the law's idle flow
 * aL / (1 + e^(1 / rho)) for p = 1.  The mass row of the guess is a starting value only: the re-solve (the 14-row loop of
 * lto_indirect_solve_batch: r, v, m of the first node and r, v of the last fixed, lambda_m of the last node 0) owns the final mass.
 * Dense output, re-mesh (all 14 rows, the mass of the last node being the spline's end sample) and snap (rows 0..5) as above.
 * cost [n_dt] (may be NULL): the trapezoid over the n_desired-point dense output of XC_out of the 14-row law's magnitude with the
 * sample's own mass, aL_j = thrustLimit / 1e3 TU^2 / DU / m_j, in DU/TU; a sample whose magnitude is NaN or whose mass is not
 * positive counts 0 (only a re-solve that did not converge leaves such a sample: read cost where status_flag is 0).  propellant [n_dt] (may be NULL; written when XC_out is set):
 * XC[6, 0] - XC_out[6, n-1, k] in kg.  Codes as lto_indirect_add_time_batch; in addition a node mass that is not finite and
 * positive: LTO_EINVAL. */
int lto_indirect_add_time_mass_batch(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                                     const lto_integrator* integ, const lto_direct_orbits* orbits, int n_dt, const double* dt,
                                     int n_desired, int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out,
                                     double* t_out, double* tau_out, double* defect, int* status_flag, int* iterations,
                                     double* history, double* cost, double* propellant);
int lto_indirect_add_time_mass(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                               const lto_integrator* integ, const lto_direct_orbits* orbits, double dt, int n_desired,
                               int flag_adjointsOnly, int maxIter, double* XC_guess, double* XC_out, double* t_out, double* tau_out,
                               double* defect, int* status_flag, int* iterations, double* history, double* cost, double* propellant);
/* Costates of n_batch direct solutions (host arrays, the layouts of lto_direct_qp_step): one Jacobian sweep, one frozen QP step
 * (flagEnd = false, tf fixed) and the costates kernel at the given point (see lto_direct_costates_dev).  At a converged
 * minimum-energy solution the step is zero and the multipliers are the discrete adjoints of the transcription.  Outputs: Lambda
 * [nstate x n_nodes x n_batch]; mult [nstate x (n_nodes-1) x n_batch] (may be NULL); XC [12 x n_nodes x n_batch] = (X; c^2 Lambda)
 * with c = TU^2 / DU / 1e3 / 1000 (may be NULL), the node vector lto_indirect_solve_batch takes for p = 2: the direct cost is sum
 * w |u|^2 in N^2, the indirect one int |a|^2 dt with a = c u (1000 kg: the mass of the 6-state right-hand side), so lambda = c^2
 * Lambda and lambda_v ~ -2 a; kkt_res [n_batch]; status [n_batch]: 0, or 1 for a singular KKT system (that trajectory's outputs are
 * NaN; the call still returns LTO_OK).  nstate = 7 with XC: LTO_EUNSUPPORTED (the multipliers, the mass row included, are returned
 * without XC; the 14-dim hand-over is not built).  lto_direct_costates: one trajectory. */
int lto_direct_costates_batch(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                              int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                              int n_targets, int allow_impulsive, double* Lambda, double* mult, double* XC, double* kkt_res,
                              int* status);
int lto_direct_costates(lto_ctx* ctx, int nstate, int n_nodes, const double* X, const double* U, const double* t, int nsteps,
                        const lto_direct_params* prm, const lto_direct_targets* targets, int allow_impulsive, double* Lambda,
                        double* mult, double* XC, double* kkt_res, int* status);
/* Trajectory-stacking initial guesses (CRTBP_Multishoot_direct_demo.jl:116-157) for n_batch starts side by side,
 * start b given by tau1[b] (phase on the departure table), tof1[b] and tof2[b] (TU, > 0).  Per start: t_out = LinRange(0, tof1 +
 * tof2, n_nodes); the nodes with t_k < tof1 are the ballistic CRTBP flow (mass ratio MU) of the departure spline at tau1, node 0
 * that state itself; the flow is carried on to tof1, tau2_0 = find_tau of that point on the arrival table (the first minimiser
 * of |s(j / 1000) - x|_2 over j = 0..1000) and the nodes with t_k >= tof1 are the flow of the arrival spline at tau2_0 over
 * t_k - tof1; tau2 = find_tau of node n-1, which is then replaced by the arrival spline at tau2.  The flow goes from node to node,
 * every advance a fresh start of the integrator: LTO_DOP853_ADAPTIVE at integ's rtol / atol / max_steps, or LTO_RK4 with
 * integ->steps steps per advance (any other method: LTO_EUNSUPPORTED).  Outputs: X_out [6 x n_nodes x n_batch], t_out [n_nodes x
 * n_batch], tau_out [3 x n_batch] = (tau1 wrapped into [0, 1]; tau2_0; tau2), gap_out [2 x n_batch] = the two distances find_tau
 * minimised (may be NULL), status [n_batch]: 0, or 2 if a node is not finite (max_steps used up: its nodes are NaN).
 * LTO_EINVAL: n_nodes < 2, n_batch < 1, a tof not finite or <= 0, a tau1 not finite or |tau1| >= 1e6, MU outside (0, 1), a table
 * with fewer than 2 samples, 6 n_nodes n_batch > 2^31 - 1. */
int lto_stack_guess_batch(lto_ctx* ctx, int n_nodes, int n_batch, double MU, const lto_direct_orbits* orbits,
                          const lto_integrator* integ, const double* tau1, const double* tof1, const double* tof2, double* X_out,
                          double* t_out, double* tau_out, double* gap_out, int* status);
/* Periodic orbits of the CRTBP (mass ratio MU) with the xz-plane symmetry -- halo and planar Lyapunov orbits -- for n_batch orbits
 * side by side.  A result does not depend on its batch: orbit b equals its single call bit for bit.
 *
 * lto_halo_correct_batch: the differential corrector.  seeds [6 x n_batch]: rows 0, 2 and 4 are read (x0, z0, vy0); the flight
 * starts at (x0, 0, z0, 0, vy0, 0) and ends at the first return to y = 0, located to adjacent doubles in time.  The residual there
 * is (vx, vz); one Newton step solves the 2 x 2 system of the state-transition matrix, corrected for the moving crossing time, for
 *   LTO_HALO_HOLD_Z0   x0 and vy0          LTO_HALO_HOLD_X0   z0 and vy0
 *   LTO_HALO_PLANAR    vy0 alone, residual vx (z0 must be 0)
 * and the loop ends when max |residual| < tol or after max_iter steps, all inside one kernel.  The flight is LTO_DOP853_ADAPTIVE at
 * integ's rtol / atol / max_steps (the error norm over the state and all 36 variational components) searched up to t_max, or LTO_RK4
 * with integ->steps steps over t_max (the half period is what the call looks for); any other method: LTO_EUNSUPPORTED.
 * Outputs: state_out [6 x n_batch] (the corrected start), period_out [n_batch] = 2 x the crossing time, resid_out [n_batch] (may be
 * NULL), iterations [n_batch] = Newton steps taken (may be NULL), history [(max_iter + 1) x n_batch] = the residual of every flight,
 * NaN past the last (may be NULL), status [n_batch]: 0 converged; 1 max_iter reached (max_iter = 0: the seed is evaluated);
 * 2 unusable seed or flight (not finite, vy0 = 0, z0 != 0 with LTO_HALO_PLANAR, no crossing before t_max, max_steps used up);
 * 3 singular step, |det| <= sing_tol x the product of the Jacobian's row norms.  Status 2 and 3: state, period and residual NaN.
 * LTO_EINVAL: n_batch < 1, max_iter < 0, tol <= 0, t_max not finite or <= 0, sing_tol outside [0, 1), MU outside (0, 1), an unknown
 * mode, LTO_RK4 with steps < 1.
 *
 * lto_halo_table_batch: one revolution from state0 [6 x n_batch] over period [n_batch], the state-transition matrix carried through,
 * stopped at t_i = i P / (n_samples - 1): X_out [6 x n_samples x n_batch] (the last column is the integrated state, not a copy of
 * the first), tau_out [n_samples] = i / (n_samples - 1) (the layout lto_direct_orbits reads), M_out [6 x 6 x n_batch] = Phi(P),
 * closure [n_batch] = max |x(P) - x(0)|, jacobi [2 x n_batch] = (C at the start; the largest |C(t_i) - C(0)|), C = x^2 + y^2 +
 * 2 (1 - MU) / r1 + 2 MU / r2 - v^2, nu [2 x n_batch] = the stability indices -(alpha +- sqrt(alpha^2 - 4 beta + 8)) / 4 with
 * alpha = 2 - tr M, beta = (alpha^2 + 2 - tr M^2) / 2 (NaN where the discriminant is negative), status [n_batch]: 0, or 2 where the
 * flight has no finite result (a period that is not finite and > 0, max_steps used up in a sample interval).  Every output but X_out
 * and status may be NULL.  LTO_DOP853_ADAPTIVE, or LTO_RK4 with integ->steps steps per sample interval; any other method:
 * LTO_EUNSUPPORTED.  LTO_EINVAL: n_samples < 2, n_batch < 1, MU outside (0, 1), 6 n_samples n_batch > 2^31 - 1. */
#define LTO_HALO_HOLD_Z0 0
#define LTO_HALO_HOLD_X0 1
#define LTO_HALO_PLANAR 2
int lto_halo_correct_batch(lto_ctx* ctx, int n_batch, double MU, int mode, const double* seeds, double tol, int max_iter,
                           double t_max, double sing_tol, const lto_integrator* integ, double* state_out, double* period_out,
                           double* resid_out, int* iterations, double* history, int* status);
int lto_halo_table_batch(lto_ctx* ctx, int n_samples, int n_batch, double MU, const double* state0, const double* period,
                         const lto_integrator* integ, double* X_out, double* tau_out, double* M_out, double* closure,
                         double* jacobi, double* nu, int* status);
/* Periodic orbits at a given Jacobi constant or a given period: the corrector of lto_halo_correct_batch with one more
 * unknown and one more equation.  The unknowns are (x0, z0, vy0) -- with planar != 0 (x0, vy0), and z0 must be 0 --, the flight is
 * lto_halo_correct_batch's (from (x0, 0, z0, 0, vy0, 0) to the first return to y = 0, LTO_DOP853_ADAPTIVE with the error norm over
 * the state and the three columns of the state-transition matrix the step reads, or LTO_RK4 with integ->steps steps over t_max), the
 * residual is (vx, vz, q - q*) -- planar: (vx, q - q*) -- with
 *   LTO_HALO_TARGET_JACOBI   q = the Jacobi constant C of the start state (its row of the Jacobian is analytic)
 *   LTO_HALO_TARGET_PERIOD   q = 2 x the crossing time (its row is -2 Phi[1, j] / f[1])
 * and one Newton step solves the 3 x 3 system by LU with partial pivoting; the loop ends when max |residual| < tol or after max_iter
 * steps.  seeds [6 x n_batch] (rows 0, 2 and 4 are read), targets [n_targets x n_batch]: orbit b's members k = 0 .. n_targets - 1 are
 * corrected one after another inside the one launch, member 0 from the seed, member 1 from member 0's state, member k >= 2 from
 *   s_(k-1) + (s_(k-1) - s_(k-2)) w,   w = (q*_k - q*_(k-1)) / (q*_(k-1) - q*_(k-2))
 * (difference, product and sum each rounded once; no predictor where q*_(k-1) = q*_(k-2)).  A result does not depend on its batch:
 * orbit b equals its single call bit for bit, and member k equals a single call seeded with the predictor's point.
 * Outputs, member (k, b) at record n_targets b + k: state_out [6 x n_targets x n_batch], period_out = 2 x the crossing time,
 * jacobi_out = C of state_out (may be NULL), resid_out (may be NULL), iterations = Newton steps taken (may be NULL), history
 * [(max_iter + 1) x n_targets x n_batch] = the residual of every flight, NaN past the last (may be NULL), status: 0 converged;
 * 1 max_iter reached (max_iter = 0: the start is evaluated) -- such a member still serves as a point of the march; 2 unusable (start
 * or target not finite, vy0 = 0, z0 != 0 with planar, a period target <= 0, no crossing before t_max, max_steps used up); 3 singular
 * step, |det| <= sing_tol x the product of the Jacobian's row 2-norms, or det not finite.  Status 2 and 3: state, period, jacobi and
 * resid NaN, and the members after it in the same orbit are NaN with status 2.
 * LTO_EINVAL: n_targets < 1, n_batch < 1, max_iter < 0, tol <= 0, t_max not finite or <= 0, sing_tol outside [0, 1), MU outside
 * (0, 1), an unknown `what`, LTO_RK4 with steps < 1, 6 n_targets n_batch, (max_iter + 1) n_targets n_batch or 8 n_batch > 2^31 - 1.  Any other
 * method than the two: LTO_EUNSUPPORTED. */
#define LTO_HALO_TARGET_JACOBI 0
#define LTO_HALO_TARGET_PERIOD 1
int lto_halo_target_batch(lto_ctx* ctx, int n_targets, int n_batch, double MU, int planar, int what, const double* seeds,
                          const double* targets, double tol, int max_iter, double t_max, double sing_tol,
                          const lto_integrator* integ, double* state_out, double* period_out, double* jacobi_out, double* resid_out,
                          int* iterations, double* history, int* status);
/* Families of periodic orbits by pseudo-arclength continuation.  The unknowns u = (x0, z0, vy0) move along the
 * family's own tangent, so that no coordinate, Jacobi constant or period has to stay monotone along the family.  The flight is
 * lto_halo_target_batch's; F = (vx, vz) at the first return to y = 0 and DF [2 x 3] = Phi[(3,5), j] - f[(3,5)] Phi[1, j] / f[1],
 * j = 0, 2, 4 -- with planar != 0 the z0 row and column of the system are the identity's, and z0 must be 0.
 *   tangent    c = DF_0 x DF_1, n = |c|_2, sigma = the sign of c . t_row, t = sigma c / n, det = sigma n (the signed determinant of
 *              [DF; t]: it changes sign between two members where another family branches off)
 *   a member   from the point u_prev with the row vector t_row and the step ds: u_pred = u_prev + ds t_row (product and sum each
 *              rounded once), then u <- u - [DF; t_row]^-1 (F; t_row . (u - u_pred)) by the 3 x 3 LU of lto_halo_target_batch until
 *              res = max(|vx|, |vz|, |t_row . (u - u_pred)|) < tol (planar: without |vz|), or max_iter steps (status 1)
 *   the step   an attempt fails if its status is not 0 or if t . t_row < cos_min (status 4; cos_min = 0: no such test); then
 *              ds <- ds / 2 and the member is tried again from u_prev; once ds < ds_min the member keeps the last attempt's status
 *              and the rest of the orbit's members are NaN with status 2.  After an accepted member of <= fast_iter Newton steps
 *              ds <- min(ds grow, ds_max).  The next member starts from the accepted u with t_row = its tangent.
 *   the start  dir_is_tangent = 0: member 0 is the seed corrected onto the family perpendicularly to the family -- u_pred = the
 *              seed, t_row = the tangent of the seed's own DF (first flight) with the sign that makes t_row . dir0 > 0, kept for the
 *              member; its ds_out is 0, it is tried once, and ds0 is the step of member 1.  dir_is_tangent = 1: the seed is a point
 *              of the family and dir0 its tangent, used as given (not normalised); member 0 is the step from it by ds0.  With the
 *              seed at a branch point and dir0 = (0, +-1, 0) this leaves a planar family for the one that is born there.
 * seeds [6 x n_batch] (rows 0, 2, 4 are read), dir0 [3 x n_batch], ds0 [n_batch].  A result does not depend on its batch, and member
 * k equals bit for bit (but for `halvings`) the one-member call with dir_is_tangent = 1, grow = 1, seed = member k - 1's state_out,
 * dir0 = its tangent_out and ds0 = member k's ds_out.
 * Outputs, member (k, b) at record n_members b + k: state_out [6 x ..], tangent_out [3 x ..], det_out, ds_out (the step of the last
 * attempt), halvings, period_out = 2 x the crossing time, jacobi_out, resid_out, iterations and history [(max_iter + 1) x ..] of the
 * last attempt (NaN past its last flight), status: 0 converged; 1 max_iter reached (the numbers of the last attempt are kept);
 * 2 unusable (seed or dir0 not finite, dir0 = 0, vy0 = 0, z0 != 0 with planar, with dir_is_tangent = 0 a dir0 perpendicular to the
 * seed's tangent, no crossing before t_max, max_steps used up); 3 singular step (lto_halo_target_batch's test) or no tangent (n or
 * c . t_row zero or not finite); 4 the tangent turned beyond cos_min.  Status 2, 3, 4: the member's numbers are NaN.  Any status but 0
 * ends the orbit's march.  Every output but state_out and status may be NULL.
 * LTO_EINVAL: lto_halo_target_batch's cases (n_members for n_targets), a ds0 not finite or <= 0, ds_min <= 0 or > ds_max, ds_max not
 * finite, grow < 1 or not finite, fast_iter < 0, cos_min outside [0, 1).  Any other method than LTO_RK4 and LTO_DOP853_ADAPTIVE:
 * LTO_EUNSUPPORTED. */
int lto_halo_arclength_batch(lto_ctx* ctx, int n_members, int n_batch, double MU, int planar, int dir_is_tangent, const double* seeds,
                             const double* dir0, const double* ds0, double ds_min, double ds_max, double grow, int fast_iter,
                             double cos_min, double tol, int max_iter, double t_max, double sing_tol, const lto_integrator* integ,
                             double* state_out, double* tangent_out, double* det_out, double* ds_out, int* halvings,
                             double* period_out, double* jacobi_out, double* resid_out, int* iterations, double* history,
                             int* status);
/* Invariant manifolds of periodic orbits: the free ways off an orbit and onto one, from the monodromy matrix
 * lto_halo_table_batch hands back.  A result does not depend on its batch: orbit b, arc b and row b equal their single call bit for
 * bit.  The flights are LTO_DOP853_ADAPTIVE at integ's rtol / atol / max_steps, or LTO_RK4 with integ->steps steps per flight (per
 * span); any other method: LTO_EUNSUPPORTED.
 *
 * lto_halo_manifold_seeds_batch: the eigen-directions at n_phase phases of each orbit and the perturbed starts.  state0 [6 x
 * n_batch], period [n_batch], M [6 x 6 x n_batch] (the layout of lto_halo_table_batch's M_out), tau [n_phase] shared by the batch,
 * each finite and wrapped into [0, 1), eps > 0 the offset in the 6-norm of (DU, DU / TU).
 *   eigen step   lambda_u = the eigenvalue of largest modulus by power iteration on M (Rayleigh quotient of the unit iterate, whose
 *                sign is aligned with the iterate before it, so a negative real lambda_u is accepted), converged when the unit
 *                vector moves by < 1e-15 in max-abs between iterations, at most LTO_MANIFOLD_POWER_CAP iterations; v_s by inverse
 *                iteration on M - I / lambda_u (det M = 1: reciprocal pairs; a 6 x 6 LU with partial pivoting, at most
 *                LTO_MANIFOLD_INVERSE_CAP solves); lambda_s = the Rayleigh quotient of v_s, reported on its own so that lambda_u
 *                lambda_s - 1 measures how symplectic M is.  Both vectors have unit 6-norm and v_x(0) > 0 (v_x(0) = 0 exactly:
 *                the component of largest magnitude positive): "+" is then the exterior branch at L2, for both.  The sign is
 *                fixed at phase 0 only and carried along the orbit by the flow, so a branch is continuous in tau.
 *   transport    the base state and one variational vector, 12 components, the error norm over all of them: the unstable vector
 *                FORWARD from phase 0 over tau P, the stable vector BACKWARD over (1 - tau) P (the time-reversed system over a
 *                positive span; carried forward it would lose two more digits to the unstable direction).  tau = 0 flies nothing.
 *                Both vectors are unit vectors again at the phase.
 * Outputs: lambda_out [2 x n_batch] = (lambda_u, lambda_s); X_out and V_out [6 x 2 x n_phase x n_batch]: the orbit point as each
 * of the two flights reached it (0 the unstable one's, 1 the stable one's) and the vector there; starts_out [6 x 4 x n_phase x
 * n_batch] = X +- eps V in the order (u+, u-, s+, s-), eps V rounded before it is added, the stable starts from the backward
 * flight's point; status [n_batch]: 0; 1 no usable hyperbolic pair (M not finite, the power iteration not converged at its cap --
 * a complex dominant pair, say -- or |lambda_u| <= 1); 2 a flight without a finite result (max_steps used up, a period that is not
 * finite and > 0).  Status 1 and 2 leave NaN in that orbit's outputs.  Every output but starts_out and status may be NULL.
 * LTO_EINVAL: n_phase < 1, n_batch < 1, MU outside (0, 1), eps not finite or <= 0, a tau not finite, 24 n_phase n_batch > 2^31 - 1,
 * LTO_RK4 with steps < 1.
 *
 * lto_section_flight_batch: n_arcs ballistic arcs, one lane each, from y0 [6 x n_arcs] over the SIGNED time t_max [n_arcs] (finite,
 * non-zero; negative: backward in time, the time-reversed system over |t_max|) to the section g(y) = y[sec_axis] - sec_value = 0.
 *   crossing     an accepted step at whose end g has the sign opposite to the arc's current side, the side being the sign of g at
 *                the last point where g != 0 (an arc that starts exactly on the section has not crossed it).  sec_dir = +1 / -1
 *                counts the changes of g from - to + / + to - only, 0 both, IN THE ORDER THE FLIGHT VISITS THE POINTS: for a
 *                backward arc that is the opposite of the physical sense.  Two crossings inside one accepted step are missed, as
 *                by any step-end test.  The n_cross-th counted crossing ends the arc and is located: the step length is bisected
 *                by trial steps of the same formula from the step's start, through the same first slope, until the bracket's ends
 *                are adjacent doubles in time (at most 60 halvings); state and time come from one more trial step to the far end
 *                of the bracket, so a flight started from a returned state looks for the NEXT crossing.  Earlier crossings are
 *                counted and the flight goes on from the accepted step's end.  n_cross = 0: no section, fly to t_max.
 *   r_min [2]    distances from the two primaries (0 disables one): an accepted step that ends closer ends the arc there with
 *                status 3; the event is not located.  A crossing in the same step comes first.
 *   samples      n_samples >= 2: the flight goes sample interval by sample interval, each a fresh start of the integrator
 *                (max_steps counts per interval), and stops exactly at t_k = k dt, dt = |t_max| / (n_samples - 1), t_k = |t_max|
 *                for the last; the crossing count and the side carry across intervals.  X_out [6 x n_samples x n_arcs]
 *                (lto_halo_table_batch's sample layout), sample 0 the start, samples past the arc's end NaN.  n_samples = 0: one
 *                span, X_out unused (may be NULL).  The two forms take different steps, so their ends agree to the tolerance,
 *                not to the bit.
 * Outputs: x_end [6 x n_arcs], t_end [n_arcs] the signed flight time, count [n_arcs] the crossings counted, dC [n_arcs] = |C(end) -
 * C(start)| of the Jacobi constant (may be NULL), status [n_arcs]: 0 ended as asked (the n_cross-th crossing, or t_max with n_cross
 * = 0); 1 t_max reached first (state and time there; count says how far it got); 2 no finite result (the start not finite,
 * max_steps used up): everything NaN; 3 an accepted step ended within r_min of a primary (state and time of that step end).
 * LTO_EINVAL: n_arcs < 1, n_samples = 1 or < 0, n_cross < 0, sec_axis outside 0..5, sec_dir outside {-1, 0, 1}, sec_value not
 * finite, a t_max zero or not finite, r_min negative or not finite, MU outside (0, 1), 6 n_samples n_arcs > 2^31 - 1, LTO_RK4 with
 * steps < 1.
 *
 * lto_state_match_batch: for each state of A [6 x nA] the nearest of Bs [6 x nB] in d = sqrt(|dr|^2 + (w |dv|)^2), w >= 0.  Every
 * product and every sum is rounded on its own (no fused multiply-add), in this order, so the host can reproduce d bit for bit:
 *   q_i = (A_i - Bs_i)^2;  dr2 = (q_0 + q_1) + q_2;  dv2 = (q_3 + q_4) + q_5;  d = sqrt(dr2 + (w w) dv2)
 * with a correctly rounded square root.  The winner is the (distance, index) lexicographic minimum, the same whatever the reduction
 * order: the lowest index on ties, a NaN distance never wins, a row whose distances are all NaN gets index -1 and NaN.  Outputs:
 * index [nA], dist [nA], dr [nA] = sqrt(dr2) and dv [nA] = sqrt(dv2) of the chosen pair (dr and dv may be NULL).  LTO_EINVAL: nA or nB
 * < 1, w negative or not finite. */
#define LTO_MANIFOLD_POWER_CAP 500
#define LTO_MANIFOLD_INVERSE_CAP 8
int lto_halo_manifold_seeds_batch(lto_ctx* ctx, int n_phase, int n_batch, double MU, const double* state0, const double* period,
                                  const double* M, const double* tau, double eps, const lto_integrator* integ, double* lambda_out,
                                  double* X_out, double* V_out, double* starts_out, int* status);
int lto_section_flight_batch(lto_ctx* ctx, int n_arcs, double MU, const double* y0, const double* t_max, int sec_axis,
                             double sec_value, int sec_dir, int n_cross, const double* r_min, int n_samples,
                             const lto_integrator* integ, double* x_end, double* t_end, int* count, double* dC, double* X_out,
                             int* status);
int lto_state_match_batch(lto_ctx* ctx, int nA, int nB, const double* A, const double* Bs, double w, int* index, double* dist,
                          double* dr, double* dv);
/* Station-keeping on periodic orbits: the Floquet-mode feedback gains from the directions
 * lto_halo_manifold_seeds_batch hands back, and batched flights under any impulsive linear feedback.  A result does not depend on
 * its batch: record b and run b equal their single call bit for bit.
 *
 * lto_stationkeep_gains_batch: V [6 x 2 x n_phase x n_batch] in the layout of the seeds call's V_out (0 the unstable unit vector
 * v_u, 1 the stable one v_s), one record per (phase, orbit).  With S = [2 Omega, -I; I, 0], Omega = [0 1 0; -1 0 0; 0 0 0], S v_s is a
 * left eigenvector of the monodromy matrix for lambda_u at every phase.  Every product, sum and quotient is rounded on its own (no
 * fused multiply-add), sums run left to right over the index from the first term, the square roots are correctly rounded, so the
 * host can reproduce the outputs bit for bit:
 *   w = (2 v_s[1] - v_s[3], -2 v_s[0] - v_s[4], -v_s[5], v_s[0], v_s[1], v_s[2])
 *   p = sum_i w_i v_u_i;  ns = sqrt(sum_i w_i w_i);  nu = sqrt(sum_i v_u_i v_u_i)
 *   W_i = w_i / p;  wv2 = (W_3 W_3 + W_4 W_4) + W_5 W_5;  alpha = sqrt(wv2) / sqrt(sum_i W_i W_i)
 *   G[r + 3 c] = (-(W_{3+r} W_c)) / wv2,  r = 0..2, c = 0..5
 * Outputs: W [6 x n_phase x n_batch] (W . v_u = 1), G [3 x 6 x n_phase x n_batch] (column-major 3 x 6 blocks: dv = G dx is the
 * minimum-norm velocity change that zeroes the unstable component W . dx), alpha [n_phase x n_batch] = |w_v| / |W|, how well a
 * velocity change reaches the unstable mode; W and alpha may be NULL.  status [n_phase x n_batch]: 0; 2 a non-finite input; 3 alpha
 * <= sing_tol (or not a number) or |p| <= (sing_tol ns) nu.  Status 2 and 3 leave NaN in that record's outputs and touch no other.
 * LTO_EINVAL: n_phase or n_batch < 1, sing_tol outside [0, 1), 18 n_phase n_batch > 2^31 - 1.
 *
 * lto_stationkeep_flight_batch: n_batch runs, one lane each, about n_orb = 1 (one orbit for every run) or n_batch (run b about orbit
 * b) orbits given by X_ref [6 x n_man x n_orb] the reference points at the burn epochs, dt [n_man x n_orb] the ballistic span after
 * burn j (finite, > 0) and G [3 x 6 x n_man x n_orb] the gains (any finite matrices: the flight knows nothing of their origin).  x0
 * [6 x n_batch] is the state at the first burn epoch; nav [6 x n_upd x n_batch] and exe [4 x n_upd x n_batch], n_upd = n_rev n_man
 * (either may be NULL: no error), are drawn by the caller.  Per run, for u = r n_man + j, r = 0..n_rev-1, j = 0..n_man-1:
 *   1. d = x - X_ref_j;  dev[0, u, b] = |d_r|, dev[1, u, b] = |d_v|
 *   2. r_lost > 0 and |d_r| > r_lost: status 1, lost_at = u, the run ends with the state and the totals it has
 *   3. c = G_j (d + nav[:, u, b]), m = |c|.  m < dv_min: no burn, dv_hist[u, b] = 0.  Otherwise, dv_max > 0 and m > dv_max: c <- c
 *      (dv_max / m); the applied burn a = (1 + exe[0, u, b]) c + exe[1:4, u, b]; v <- v + a, dv_total += |a|, n_burn += 1,
 *      dv_hist[u, b] = |a|
 *   4. x over dt_j as a span of its own: LTO_DOP853_ADAPTIVE at integ's rtol / atol / max_steps (the error norm over the six
 *      components, max_steps counted per span), or LTO_RK4 with integ->steps steps per span; any other method: LTO_EUNSUPPORTED.
 * Outputs: x_final [6 x n_batch] the state after the last span, dv_total [n_batch], n_burn [n_batch], dev [2 x n_upd x n_batch],
 * dv_hist [n_upd x n_batch], dev_final [2 x n_batch] the deviation from X_ref_0 after the last span, accepted / rejected [n_batch]
 * summed over the spans, status [n_batch]: 0; 1 lost; 2 a non-finite start, reference, gain, error draw, burn or state, or a span
 * that used up max_steps: x_final, dv_total and dev_final are NaN; lost_at [n_batch] (-1: not lost).  A lost run keeps dev[:, lost_at]
 * and reports it as dev_final; its dv_hist from lost_at on and its dev past lost_at are NaN.  A failed run's dev and dv_hist are
 * NaN from the update that failed on.  dev, dv_hist, dev_final, n_burn, accepted, rejected and lost_at may be NULL.
 * LTO_EINVAL: n_man, n_rev or n_batch < 1, n_orb neither 1 nor n_batch, a dt not finite or <= 0, dv_min, dv_max or r_lost negative
 * or not finite, MU outside (0, 1), LTO_RK4 with steps < 1, 6 n_upd n_batch > 2^31 - 1. */
int lto_stationkeep_gains_batch(lto_ctx* ctx, int n_phase, int n_batch, const double* V, double sing_tol, double* W, double* G,
                                double* alpha, int* status);
int lto_stationkeep_flight_batch(lto_ctx* ctx, int n_man, int n_rev, int n_batch, double MU, const double* X_ref, const double* dt,
                                 const double* G, int n_orb, const double* x0, const double* nav, const double* exe, double dv_min,
                                 double dv_max, double r_lost, const lto_integrator* integ, double* x_final, double* dv_total,
                                 int* n_burn, double* dev, double* dv_hist, double* dev_final, int* accepted, int* rejected,
                                 int* status, int* lost_at);
/* Target-point station-keeping: the state-transition matrices between phases of a periodic orbit, and the law of
 * Howell & Pernicka built from them.  A record does not depend on its batch: it equals its single call bit for bit.
 *
 * lto_halo_stm_batch: one record per (phase, orbit), record g = n_phase b + j.  state0 [6 x n_batch] and period [n_batch] as
 * lto_halo_table_batch takes them, tau [n_phase] the phases, shared by the batch, each finite and wrapped into [0, 1), horizon
 * [n_tgt] the targets in periods, finite, > 0 and strictly increasing.  Per record, with t_j = tau_j P:
 *   coast     the six-component ballistic state from state0 over tau_j P (tau = 0 flies nothing): X_out [6 x n_phase x n_batch]
 *   spans     from X_out and Phi = I, the base state with all six columns of the variational equations (42 components in the
 *             error norm, the lanes of lto_halo_table_batch) over (h_k - h_{k-1}) P, h_0 = 0, k = 1..n_tgt, each a span of its
 *             own: Phi_out [6 x 6 x n_tgt x n_phase x n_batch] (column-major 6 x 6 blocks) = Phi(t_j + h_k P, t_j), X_tgt [6 x
 *             n_tgt x n_phase x n_batch] the orbit point there (may be NULL)
 * LTO_DOP853_ADAPTIVE at integ's rtol / atol / max_steps, max_steps counted per span (the coast is one), or LTO_RK4 with
 * integ->steps steps per span, the coast counting as one span; any other method: LTO_EUNSUPPORTED.  accepted / rejected [n_phase x
 * n_batch] (may be NULL) are summed over the coast and the spans.  status [n_phase x n_batch]: 0; 2 no finite result (a state or
 * period that is not finite, period <= 0, a span that used up max_steps, a result that is not finite): NaN in every output of that
 * record and in no other.
 * LTO_EINVAL: n_phase, n_tgt or n_batch < 1, MU outside (0, 1), a horizon not finite, <= 0 or not above the one before it, a tau not
 * finite, LTO_RK4 with steps < 1, 36 n_tgt n_phase n_batch > 2^31 - 1.
 *
 * lto_stationkeep_target_gains_batch: Phi [6 x 6 x n_tgt x n_rec] in the layout of Phi_out, one record per 6 x 6 x n_tgt block.
 * With Phi_k = [A_k B_k; C_k D_k] (3 x 3 blocks) a burn dv at the record's epoch leaves the position deviation m_k = A_k p + B_k (e
 * + dv) at target k for the measured deviation dx = (p, e).  dv = G dx minimises q |dv|^2 + sum_k r_k |m_k|^2:
 *   H = q I + sum_k r_k B_k^T B_k,  N = sum_k r_k B_k^T [A_k | B_k],  G = -H^-1 N.
 * q >= 0, r [n_tgt] each >= 0 and not all zero.  Every product, sum, difference and quotient is rounded on its own (no fused
 * multiply-add), the square roots are correctly rounded, in this order, so the host can reproduce G bit for bit.  T_k [3 x 6] =
 * rows 0..2 of Phi_k (T_k[m, c] = Phi[m + 6 c + 36 k]), B_k = its columns 3..5:
 *   s_k[i, c] = (T_k[0, 3+i] T_k[0, c] + T_k[1, 3+i] T_k[1, c]) + T_k[2, 3+i] T_k[2, c]       i = 0..2, c = 0..5
 *   n[i, c]   = r_0 s_0[i, c], then n[i, c] + r_k s_k[i, c] for k = 1, 2, ...
 *   h[i, j]   = the same sum with c = 3 + j, for j <= i;  H[i, i] = q + h[i, i],  H[i, j] = h[i, j] (j < i)
 *   hmax = max(max(H00, H11), H22)
 *   d0 = H00, L00 = sqrt(d0), L10 = H10 / L00, L20 = H20 / L00
 *   d1 = H11 - L10 L10, L11 = sqrt(d1), L21 = (H21 - L20 L10) / L11
 *   d2 = (H22 - L20 L20) - L21 L21, L22 = sqrt(d2)
 *   per column c:  z0 = n[0, c] / L00,  z1 = (n[1, c] - L10 z0) / L11,  z2 = ((n[2, c] - L20 z0) - L21 z1) / L22
 *                  x2 = z2 / L22,  x1 = (z1 - L21 x2) / L11,  x0 = ((z0 - L10 x1) - L20 x2) / L00
 *                  G[r + 3 c] = -x_r
 * Outputs: G [3 x 6 x n_rec], the layout lto_stationkeep_flight_batch reads; pivot [n_rec] (may be NULL) = min(min(d0, d1), d2) /
 * hmax, the smallest squared Cholesky pivot over the largest diagonal entry of H; status [n_rec]: 0; 2 an entry of the record's
 * Phi that is not finite; 3 a d_i that is not > sing_tol hmax.  Status 2 and 3 leave NaN in that record's G and pivot and touch no
 * other.
 * LTO_EINVAL: n_tgt or n_rec < 1, q negative or not finite, an r negative or not finite, every r zero, sing_tol outside [0, 1), 36
 * n_tgt n_rec > 2^31 - 1. */
int lto_halo_stm_batch(lto_ctx* ctx, int n_phase, int n_tgt, int n_batch, double MU, const double* state0, const double* period,
                       const double* tau, const double* horizon, const lto_integrator* integ, double* X_out, double* Phi_out,
                       double* X_tgt, int* accepted, int* rejected, int* status);
int lto_stationkeep_target_gains_batch(lto_ctx* ctx, int n_tgt, int n_rec, const double* Phi, double q, const double* r,
                                       double sing_tol, double* G, double* pivot, int* status);
/* Mesh re-distribution of converged 12-dim solutions (the indirect method's counterpart of meshRefine_direct): the
 * nodes of XC [12 x n_nodes x n_batch] on t [n_nodes x n_tgrids] (n_tgrids = 1 or n_batch) are moved, and their number changed to
 * n_new, so that every new segment carries the same share of a per-segment monitor w_i > 0.  Per trajectory:
 *   monitor   weights [(n_nodes-1) x n_batch] if not NULL (passes must be 1), otherwise the trial-step counts (accepted + rejected)
 *             of one defect sweep of the input on its own grid (adaptive integrators only);
 *   grid      C_0 = 0, C_{i+1} = C_i + w_i, W = C_{n-1}; for 0 < k < n_new - 1: g_k = k W / (n_new - 1), i the largest index with
 *             C_i <= g_k, t_out_k = t_i + (g_k - C_i) / w_i (t_{i+1} - t_i); the first and last time are the input's, bit for bit.
 *             (The C_i are summed in a fixed radix-64 order; integer counts are exact in any order.)
 *   nodes     new node k = the input's own piecewise trajectory at t_out_k: old node i (the largest i with t_i <= t_out_k)
 *             propagated over t_out_k - t_i with integ (RK4: integ.steps steps over that span).  A zero span, the first and the
 *             last node are copies, bit for bit.  These are XC_guess [12 x n_new x n_batch].
 *   passes    > 1 (counts only): monitor, grid and nodes again on the result, `passes` times in all.
 *   re-solve  XC_out not NULL: the Newton loop of lto_indirect_solve_batch on t_out [n_new x n_batch] started from the guess
 *             (XC_out, defect [12 x (n_new-1) x n_batch], status_flag, iterations, history as there); NULL: grid and guess only.
 * steps_before [(n_nodes-1) x n_batch] / steps_after [(n_new-1) x n_batch] (may be NULL): the trial steps of a one-lane-per-segment
 * defect sweep of the input / of the result (of the guess without a re-solve); a fixed-step integrator reports integ.steps.
 * Every output but t_out may be NULL.  ndim != 12 or an integrator other than LTO_RK4 / LTO_DOP853_ADAPTIVE: LTO_EUNSUPPORTED;
 * weights == NULL with a fixed-step integrator, passes < 1, passes > 1 with weights, n_new < 2, a weight that is not finite and
 * positive, a grid (the input's, or a pass's result) that is not strictly increasing, more than 262 144 segments: LTO_EINVAL. */
int lto_indirect_remesh_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                              const lto_params* prm, int n_prm, const lto_integrator* integ, int n_new, const double* weights,
                              int passes, int flag_adjointsOnly, int maxIter, double* t_out, double* XC_guess, double* XC_out,
                              double* defect, int* status_flag, int* iterations, double* history, int* steps_before,
                              int* steps_after);
int lto_indirect_remesh(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                        const lto_integrator* integ, int n_new, const double* weights, int passes, int flag_adjointsOnly,
                        int maxIter, double* t_out, double* XC_guess, double* XC_out, double* defect, int* status_flag,
                        int* iterations, double* history, int* steps_before, int* steps_after);
/* The same for converged solutions of the 14-row variable-mass system, y = (r, v, m, lambda_r, lambda_v, lambda_m):
 * XC [14 x n_nodes x n_batch], XC_guess / XC_out [14 x n_new x n_batch], defect [14 x (n_new-1) x n_batch], lto_params.mass carrying
 * Isp as everywhere for 14 rows.  The monitor, the grid rule and its summation order, `passes`, the bit-copy rules (a zero span, the
 * first and the last node), the limits and the error codes are those of lto_indirect_remesh_batch above; the nodes are propagated
 * with the 14-row system, so the mass row of a new node is the propagated mass.  The re-solve is the 14-row loop of
 * lto_indirect_solve_batch: it pins XC[0:7, 0] (position, velocity and m0) and XC[0:6, n_new-1], sets XC[13, n_new-1] = 0 and leaves
 * the final mass free.  The guess's first and last nodes being copies, m0 and a converged input's lambda_m(tf) = 0 arrive there
 * unchanged.  An integrator other than LTO_RK4 / LTO_DOP853_ADAPTIVE: LTO_EUNSUPPORTED. */
int lto_indirect_remesh_mass_batch(lto_ctx* ctx, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                   const lto_params* prm, int n_prm, const lto_integrator* integ, int n_new, const double* weights,
                                   int passes, int flag_adjointsOnly, int maxIter, double* t_out, double* XC_guess, double* XC_out,
                                   double* defect, int* status_flag, int* iterations, double* history, int* steps_before,
                                   int* steps_after);
int lto_indirect_remesh_mass(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                             const lto_integrator* integ, int n_new, const double* weights, int passes, int flag_adjointsOnly,
                             int maxIter, double* t_out, double* XC_guess, double* XC_out, double* defect, int* status_flag,
                             int* iterations, double* history, int* steps_before, int* steps_after);

/* One Jacobian sweep and one free-end QP step (arguments as lto_direct_qp_step); targets, model and beta [n_targets] (1 or
 * n_batch).  p_out [2 x n_batch] = (p1; p2); cost includes the beta term.  The 2 x 2 bound-constrained problem in p is solved
 * exactly on the device: smallest reduced cost over the interior point, the clamped edge minimisers and the corners;
 * exact ties go to the smaller max|p|, then to that order. */
int lto_direct_qp_step_free(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                            int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                            const lto_direct_end_model* model, const double* beta, int n_targets, int allow_impulsive, double* dX,
                            double* dU, double* dV, double* p_out, double* cost);
/* The loop of lto_direct_solve_batch with the end points taken from the orbit tables at tau: tau_in [2 x n_batch], beta
 * [n_targets].  The mass and the impulses dV1, dV2 come from targets; its s0 and sf are ignored and recomputed from tau at the
 * start and after every tau update.  flag_end = 1: odd iterations are free-end steps and tau += alpha p afterwards (not wrapped);
 * even iterations are frozen-end steps at the current tau (:521-526).  flag_end = 0: every step is frozen.  tau_out [2 x n_batch]
 * (may be NULL); history [5 x maxIter x n_batch] = (max|defect|, cost, alpha, tau1, tau2) after each iteration.  Other arguments and
 * status codes as lto_direct_solve_batch. */
int lto_direct_solve_free_batch(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                                const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                                const lto_direct_orbits* orbits, const lto_direct_targets* targets, int n_targets,
                                const double* tau_in, const double* beta, int flag_end, int allow_impulsive, int maxIter,
                                double* X_out, double* U_out, double* dV_out, double* t_out, double* defect_out, double* tau_out,
                                int* status, int* iterations, double* history);
int lto_direct_solve_free(lto_ctx* ctx, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t, int nsteps,
                          const lto_direct_params* prm, const lto_direct_orbits* orbits, const lto_direct_targets* targets,
                          const double* tau_in, double beta, int flag_end, int allow_impulsive, int maxIter, double* X_out,
                          double* U_out, double* dV_out, double* t_out, double* defect_out, double* tau_out, int* status,
                          int* iterations, double* history);

/* ---- Free time of flight with free end points (src/multiShoot_CRTBP_direct.jl:286-295, :503-516, :567, :582): on a
 * free iteration the subproblem gains p3 = tf_jump, the defect constraints read Jac_i [dx_i; dx_{i+1}; du_i; du_{i+1}] + dtf_i p3 =
 * -defect_i with dtf_i = d defect_i / d tf (the Jacobian sweep's tf column), and p3 is bounded by lo = max(-step, tf_min - tf),
 * hi = min(step, tf_max - tf).  The 3 x 3 box QP in (p1, p2, p3) is solved exactly on the device.  Times in TU. */
typedef struct lto_direct_tf_bounds {
  double step;                       /* bound of |tf_jump| per free iteration (the reference: 1 day) */
  double tf_min, tf_max;             /* absolute bounds of tf; tf_min > t0 keeps the grid from collapsing */
} lto_direct_tf_bounds;
/* One Jacobian sweep (with the tf column) and one free-end, free-tf QP step: arguments as lto_direct_qp_step_free, tfb [n_targets];
 * tf = the last entry of each trajectory's grid.  p_out [3 x n_batch] = (p1; p2; p3).  Ties of the box QP go to the smaller
 * max(|p1|/0.1, |p2|/0.1, |p3|/step), then to the earlier candidate (interior point, then the faces p1 = lo, hi, p2 = lo, hi,
 * p3 = lo, hi); a coordinate on a bound is the bound value itself.  LTO_EINVAL for step < 0, tf outside [tf_min, tf_max] or
 * tf_min <= t0. */
int lto_direct_qp_step_free_tf(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X, const double* U, const double* t,
                               int n_tgrids, int nsteps, const lto_direct_params* prm, const lto_direct_targets* targets,
                               const lto_direct_end_model* model, const double* beta, const lto_direct_tf_bounds* tfb, int n_targets,
                               int allow_impulsive, double* dX, double* dU, double* dV, double* p_out, double* cost);
/* The loop of lto_direct_solve_free_batch with tf a variable of the free iterations (flag_end = 1, odd iterations): after the line
 * search tau += alpha (p1, p2), tf += alpha p3 (kept in [tf_min, tf_max]), and every trajectory's grid is rebuilt from the entry
 * grid, t = t0 + (tau_grid + 1) / 2 (tf - t0).  As in the reference (:560) the line search evaluates its trial points on the
 * current grid, not at tf + alpha p3.  tfb [n_targets]; t_out [n_nodes x n_batch] is each trajectory's final grid; history
 * [6 x maxIter x n_batch] = (max|defect|, cost, alpha, tau1, tau2, tf).  flag_end = 0, or step = 0 for every trajectory, runs
 * lto_direct_solve_free_batch (same outputs byte for byte, history row 5 the constant tf).  Argument codes as
 * lto_direct_qp_step_free_tf. */
int lto_direct_solve_free_tf_batch(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, const double* X_in, const double* U_in,
                                   const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm,
                                   const lto_direct_orbits* orbits, const lto_direct_targets* targets, int n_targets,
                                   const double* tau_in, const double* beta, const lto_direct_tf_bounds* tfb, int flag_end,
                                   int allow_impulsive, int maxIter, double* X_out, double* U_out, double* dV_out, double* t_out,
                                   double* defect_out, double* tau_out, int* status, int* iterations, double* history);
int lto_direct_solve_free_tf(lto_ctx* ctx, int nstate, int n_nodes, const double* X_in, const double* U_in, const double* t,
                             int nsteps, const lto_direct_params* prm, const lto_direct_orbits* orbits,
                             const lto_direct_targets* targets, const double* tau_in, double beta, const lto_direct_tf_bounds* tfb,
                             int flag_end, int allow_impulsive, int maxIter, double* X_out, double* U_out, double* dV_out,
                             double* t_out, double* defect_out, double* tau_out, int* status, int* iterations, double* history);

/* ------------------------------------------------- device-resident API (operands already in HBM)
 * Struct-of-arrays, segment/node index fastest, so that a wavefront's 64 lanes read 512
 * contiguous bytes per component.  With J = n_nodes*n_batch nodes and S = (n_nodes-1)*n_batch
 * segments (node j = b*n_nodes + k, segment s = b*(n_nodes-1) + i):
 *   X[c*ldx + j]  t[g*n_nodes + k]  defect[c*ldd + s]  Phi[(col*ndim+row)*ldp + s]  errors[s]
 *   U[c*ldu + j]  Jac[(col*nstate+row)*ldj + s]  dtf[c*ldd + s]
 * Launches are asynchronous on `stream`, a hipStream_t taken literally (NULL = HIP's default stream,
 * which is also PyTorch's default current stream); lto_ctx_stream() returns the context's own stream.
 * One exception to "asynchronous": lto_indirect_defect_dev on an ndim = 12 DOP853_ADAPTIVE plan under LTO_KERNEL_AUTO with at
 * least 64 x CUs segments may WAIT ON THE HOST for an event recorded behind an EARLIER defect sweep of the same plan (the trial-step
 * statistics its lanes-per-segment choice reads: after the plan's first two sweeps, then every sixteenth) -- i.e. for work the
 * caller enqueued before, never for the sweep being enqueued; lto_indirect_plan_set_defect_lanes(plan, 1 | 2 | 4) fixes the
 * choice and removes the wait, and inside a stream capture nothing is waited for. */
int lto_indirect_plan_create(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const lto_params* prm, int n_prm,
                             const lto_integrator* integ, lto_indirect_plan** out);
void lto_indirect_plan_destroy(lto_indirect_plan* plan);
int lto_indirect_defect_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t,
                            int n_tgrids, double* defect, long ldd, double* errors);
int lto_indirect_jacobian_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t,
                              int n_tgrids, double* Phi, long ldp, double* defect, long ldd);
/* Per-segment accepted / rejected step counts of the last adaptive sweep (device pointers owned by the
 * plan, S ints each; NULL for fixed-step plans). */
const int* lto_indirect_plan_steps_accepted(const lto_indirect_plan* plan);
const int* lto_indirect_plan_steps_rejected(const lto_indirect_plan* plan);
/* Copies the counters of the last adaptive sweep launched on `stream` to host arrays of S ints (either may be NULL). */
int lto_indirect_plan_copy_steps(lto_indirect_plan* plan, void* stream, int* accepted, int* rejected);
/* Load balancing of adaptive sweeps.  Segments that need many steps (long or sharply switching arcs) hold their
 * whole wavefront / workgroup until they finish.  lto_indirect_plan_rebalance orders the lanes of all SUBSEQUENT sweeps
 * of this plan by the step counts of the LAST sweep, heaviest first, so that neighbouring lanes do similar work
 * (counting sort on the device, asynchronous on `stream`).  Results do not change: every segment still takes its own
 * step sequence and is stored at its own index.  Call it again when the trajectory has moved enough to change the
 * step counts; lto_indirect_plan_reset_order returns to the natural order.  Fixed-step plans, and plans that have not
 * swept yet: LTO_EINVAL.
 * Two kinds of order (round 5), chosen by what the plan has run so far.  A plan that has run an STM sweep gets the GLOBAL order
 * (heaviest segment first over the whole batch) and, for ndim = 12 DOP853 plans, record staging: nodes in and results out travel
 * as per-segment records with coalesced transposes either side of the sweep (lto_indirect_plan_staging) -- the shortest sweep,
 * 2.7-2.9 x the algorithmic HBM bytes.  A plan that has only run defect sweeps gets the WINDOWED order: segments ordered inside
 * windows of 1 024 consecutive segments, the windows ranked by their slowest segment, dealt to the XCDs in turn and interleaved
 * there 16 segments at a time, the sweep's workgroups mapped to contiguous ranges per XCD -- the wavefronts that share a window's
 * cache lines then share an L2, the sweep gathers from and scatters to the caller's arrays directly (no records, no extra
 * passes): the same sweep time and ~1.0 x the algorithmic bytes (65 536 segments of BASELINE configs[4]: 0.29 ms and 17.7 MB
 * against 0.30 ms and 54 MB). */
int lto_indirect_plan_rebalance(lto_indirect_plan* plan, void* stream);
int lto_indirect_plan_reset_order(lto_indirect_plan* plan);
/* Read-only: the lane order the plan's NEXT adaptive sweep would use.  *kind_out = 0: the natural order (fixed-step plans, plans
 * that were never rebalanced, after lto_indirect_plan_reset_order) -- order_host is not touched and may be NULL; 1: the global
 * order; 2: the windowed order -- order_host[0 .. S) receives the lane -> segment map (S = (n_nodes - 1) * n_batch ints), copied
 * behind everything queued on `stream`, which is synchronised before the call returns.  plan or kind_out NULL, or order_host NULL
 * with an order in use: LTO_ENULL, nothing written. */
int lto_indirect_plan_copy_order(lto_indirect_plan* plan, void* stream, int* order_host, int* kind_out);
/* Warm start of the adaptive step-size controller (ndim = 12, DOP853_ADAPTIVE -- the reference's integrator setting, whose
 * sweeps last as long as their slowest segment; other plans: LTO_EINVAL).  When on, every STM sweep / defect-only sweep of
 * this plan that runs the two-lane kernels starts each segment from the step size that segment's first accepted step had in
 * the plan's PREVIOUS sweep of the same kind, instead of Hairer's start rule (an extra right-hand-side evaluation and a start a
 * decade or two low).  Consecutive Newton iterations and line-search trials sweep nearly the same trajectory, and any positive
 * start is valid: the controller corrects it.  Results then depend on the plan's history at the level of the tolerance
 * (1e-13), which is why it is off by default: with it off, equal inputs give equal bits.  Turning it off forgets the stored sizes. */
int lto_indirect_plan_set_warm_start(lto_indirect_plan* plan, int on);

/* Tuning knobs for the STM sweep.  Kernel: LTO_KERNEL_AUTO picks
 *   - fixed-step RK4 with >= 6 steps per segment: the three-role pipeline kernels -- the eight-wave form (LTO_KERNEL_PIPE8) while
 *     the batch is one round of it (16 segments per CU: 4 096 on MI355X); above that the family whose rounds are cheapest for the
 *     segment count, by the context's cost table (lto_kernel_round_costs / lto_calibrate_kernels above): eight-wave form in
 *     rounds of 16 x CUs segments, 32-segment form (LTO_KERNEL_PIPE32, where it is built) in rounds of 32 x CUs, large-batch form
 *     (LTO_KERNEL_PIPE48) in rounds of 48 x CUs -- 12-dim also 44 x CUs --, and for ndim = 12 the whole-segment lanes
 *     (LTO_KERNEL_LANE) in rounds of 256 x CUs (lto_indirect_auto_kernel below is this rule as a pure function).  On
 *     MI355X (256 CUs, default table): 4 097 ... 8 192 segments -> PIPE32, 8 193 ... 12 288 -> PIPE48, 65 536 and 262 144 -> LANE
 *     (12-dim) / PIPE32 (14-dim);
 *   - RK4 with fewer steps: the per-lane kernel (each lane re-integrates the base state with 1-3 columns); for ndim = 12 on a
 *     full chip the whole-segment forms instead: ONE step per segment and >= 65 536 segments the one-step sweep
 *     (lto_indirect_plan_set_cols_per_lane, 12), 2 ... 5 steps LTO_KERNEL_LANE when its rounds are the cheaper ones;
 *   - the 13-stage integrators: the wave-specialised kernel (LTO_KERNEL_COOP: base wave + column waves per 16 segments,
 *     coefficients handed over through LDS at every RK stage) -- for ndim = 12 with DOP853_ADAPTIVE, the reference's setting, its
 *     form with two lanes per state (LTO_KERNEL_COOP2).
 * Results never depend on the choice beyond round-off; lto_indirect_plan_last_kernel reports what ran.
 * Round 6 removed three dominated forms; their selectors stay valid and resolve to the family that took over: LTO_KERNEL_PER_LANE on
 * a 13-stage plan selects the one-lane DEFECT sweep only (its STM sweep runs the cooperative kernels -- the one-column-per-lane form
 * with memory-resident slopes is gone), LTO_KERNEL_COOP on an RK4 plan runs the pipeline AUTO would take, LTO_KERNEL_COOP on a
 * 12-dim DOP853 plan runs LTO_KERNEL_COOP2. */
#define LTO_KERNEL_AUTO 0
#define LTO_KERNEL_PER_LANE 1
#define LTO_KERNEL_COOP 2
/* Direct plans only (lto_direct_plan_set_kernel): the pipelined Jacobian kernel (base wave + one wave per sensitivity column per 32
 * segments, skewed by one RKF7(8) step); AUTO takes it from 3 072 segments.  On an indirect plan: LTO_EINVAL. */
#define LTO_KERNEL_DIRECT_PIPE 3
/* RK4 plans only (other integrators: LTO_EINVAL): base wave, coefficient wave and column waves per 16 segments run as a software
 * pipeline skewed by one RK4 step.  Four column waves, one STM column per lane, a DPP row = one segment and the
 * coefficients broadcast inside the FMA (v_fmac_f64_dpp row_newbcast), TWO RK4 steps per phase and eight waves -- a fourth of
 * the column work alternates between two SIMDs so that all four SIMDs of a CU carry the same load -- and a base wave that
 * evaluates RK4 stages 1|2 and then 3|4 side by side in neighbouring lanes (one workgroup per CU: 91 KB of LDS). */
#define LTO_KERNEL_PIPE8 5
/* ndim = 12, DOP853_ADAPTIVE plans only: the cooperative kernel with every 12-component state split over two lanes (top /
 * bottom halves of a column in different waves, the two halves of the base state in neighbouring DPP banks): six components
 * per lane keep all slopes of the 13-stage method in addressable registers (round 3: the base state takes a DPP quad, three
 * components per lane).  Other plans: LTO_EINVAL.  The defect-only sweep of such a plan comes with one, two or four lanes per
 * segment (see lto_indirect_plan_set_defect_lanes for what AUTO takes): LTO_KERNEL_PER_LANE and LTO_KERNEL_COOP2 select the
 * first two, lto_indirect_plan_set_defect_lanes any of them. */
#define LTO_KERNEL_COOP2 6
/* RK4 plans only: the pipeline for large batches -- 48 segments and 16 wavefronts per workgroup, the base wave's lanes are 48
 * different segments, twelve column waves with one segment per DPP row; 12-dim also with 44 segments and eleven column waves (the
 * cheaper of the two forms for the segment count runs). */
#define LTO_KERNEL_PIPE48 7
/* 32 segments and twelve wavefronts per workgroup: the eight-wave form's roles (paired-stage base role, four lanes per segment) with one
 * barrier per step.  For batches between one round of LTO_KERNEL_PIPE8 and a few (4 097 ... 8 192 segments on MI355X: one round
 * instead of two).  RK4; 12-dim, and 14-dim with p = 0 or p = 1; anything else: LTO_EINVAL from lto_indirect_plan_set_kernel
 * (AUTO does not consider it there).  Results equal LTO_KERNEL_PIPE8's bit for bit. */
#define LTO_KERNEL_PIPE32 8
/* RK4, ndim = 12 plans only (others: LTO_EINVAL): a lane owns a whole segment -- its base trajectory, the four stage matrices of
 * every step and all twelve STM columns, which it sends through those matrices one after the other (eight columns parked in
 * accumulation registers, four in LDS).  No DPP row with idle lanes, no barrier, no hand-over: ~61 wave-instructions per segment
 * and RK4 step against ~118 of LTO_KERNEL_PIPE48 -- but one wavefront of 64 segments per SIMD, so it only pays once the batch
 * fills the chip: AUTO compares its rounds of 256 x CUs segments (505 us at 64 steps on MI355X) with the pipelines' rounds and
 * takes it from 36 865 segments on MI355X (not for the sizes just above a multiple of a pipeline's smaller round: 65 537 ...
 * 78 848).  The defect equals the pipeline kernels' bit for bit; Phi agrees with theirs to round-off (~1e-15 of max |Phi|: since
 * round 6 the stage matrices come from the base evaluations' by-products, not from a second evaluation of the control law). */
#define LTO_KERNEL_LANE 9
int lto_indirect_plan_set_kernel(lto_indirect_plan* plan, int kernel);
/* What LTO_KERNEL_AUTO resolves to for the STM sweep of a plan of this shape on a device with `n_cus` compute units, by the MI355X
 * cost table (a context's own table after lto_calibrate_kernels may differ): ndim 12 | 14, method LTO_RK4 ..., steps per segment,
 * p the control-law exponent (0, 1, 2 or > 1), n_segments = (n_nodes - 1) x n_batch, ordered = the plan sweeps with a lane order.
 * A pure function: no context, no device -- callable on a host without a GPU (sizing an N-GPU run, tests).  Returns LTO_KERNEL_* or
 * LTO_EINVAL. */
int lto_indirect_auto_kernel(int ndim, int method, int steps, double p, long n_segments, int n_cus, int ordered);
/* Lanes per segment of the DEFECT-ONLY sweep of an ndim = 12 DOP853_ADAPTIVE plan (the reference's setting, indirect.jl:63-90):
 * 1, 2 or 4 (a DPP quad per segment: r, v, lambda_v, lambda_r), or 0 = choose (default).  The choice: by size -- four lanes up to
 * eight wavefronts of 16 segments per SIMD, i.e. 512 x CUs segments (131 072 on MI355X), two lanes up to 262 144 segments, one
 * beyond -- and, from 64 x CUs segments, by the trial-step statistics of an EARLIER defect sweep of the same plan once they are
 * in (taken after the plan's first two sweeps, then every sixteenth): if no segment took more than three times the mean number
 * of trial steps (a line search's trial trajectories) there is no tail worth shortening and fewer lanes issue fewer
 * instructions -- two lanes up to 160 x CUs segments, one above.  The statistics are consumed behind an event, so the choice is
 * a function of the plan's call sequence, not of timing (inside a graph capture the last verdict stands).  All forms take the
 * same step controller (rk.hpp dp8_decide) but sum the error norm in different orders: results agree to round-off of the
 * converged flow (~1e-15), and bit for bit only between sweeps with the same number of lanes.  Two and four lanes on other
 * plans: LTO_EINVAL. */
int lto_indirect_plan_set_defect_lanes(lto_indirect_plan* plan, int lanes);
/* Record staging of a plan's ordered (rebalanced) sweeps, a bit mask: 1 = node and defect records are in place, 2 = Phi records
 * too (only plans that run STM sweeps get them), 4 = an allocation for them failed and staging is off for this plan -- the sweeps
 * then read and write the caller's arrays directly (same results, 3-8 x the HBM traffic); lto_last_error() holds the note. */
int lto_indirect_plan_staging(const lto_indirect_plan* plan);
/* Output layout of a plan's sweeps (round 6).  LTO_LAYOUT_SOA (default): defect [ndim][ldd], Phi [(col*ndim+row)][ldp] -- struct of
 * arrays, segment index fastest.  LTO_LAYOUT_BLOCKS: one block per segment, defect [S][ndim] and Phi [S][ndim*ndim] with the block
 * column-major -- i.e. exactly the reference's (Julia's, column-major) defect[ndim x S] and the Phi_i blocks of jacobianCalc
 * (indirect.jl:121-123), what the host-pointer entry points return; ldd / ldp are then ignored.  Built for ndim = 12
 * DOP853_ADAPTIVE plans (the reference's integrator setting; others: LTO_EUNSUPPORTED): their kernels write a segment's results
 * as one record, so with a lane order (lto_indirect_plan_rebalance) the sweep needs no record arrays of its own and no transposes
 * behind it -- C5 + STM (65 536 segments): 104 instead of 280 MB of HBM traffic per sweep (algorithmic 95), same bits.  The
 * defect-only sweep of such a plan runs with two or four lanes per segment (the one-lane kernel writes struct-of-arrays only);
 * lto_indirect_newton_solve_dev reads struct-of-arrays and refuses such a plan. */
#define LTO_LAYOUT_SOA 0
#define LTO_LAYOUT_BLOCKS 1
int lto_indirect_plan_set_output_layout(lto_indirect_plan* plan, int layout);
/* LTO_KERNEL_* family the last STM sweep of this plan ran (what AUTO resolved to); LTO_KERNEL_AUTO before any sweep. */
int lto_indirect_plan_last_kernel(const lto_indirect_plan* plan);
/* Per-lane kernel only: STM columns integrated per lane (12-dim: 1 or 3, 14-dim: 1 or 2 -- LTO_EUNSUPPORTED for the other
 * grouping; every lane re-integrates the base state with its columns); 0 = choose from S.  cols = the plan's dimension (12 or 14) = the
 * whole STM in the segment's own lane (kernels_indirect_stream.hip): built for RK4 plans with ONE step per segment (LTO_EINVAL
 * otherwise, and for the other dimension's value) -- the HBM-bound corner of the sweep, where the lane of a segment runs the four
 * stage evaluations once and sends the columns through the four stage matrices; 0 chooses it for such plans from 65 536 segments.
 * One kernel per dimension whatever the batch's control laws (the law is chosen per trajectory at run time; round 6). */
int lto_indirect_plan_set_cols_per_lane(lto_indirect_plan* plan, int cols);

/* QP step of the direct method on the device (see lto_direct_qp_step), operands in the SoA layouts above: Jac / defect as
 * lto_direct_jacobian_dev leaves them, X, U, t the point they were taken at, targets a DEVICE array of n_batch
 * lto_direct_targets.  dX [nstate][ldx], dU [3][ldu] (node-indexed), dV [n_batch][6], cost [n_batch] (device).  The workspace
 * (rows and records of the reduction, ~1.5 KB per segment and level-0 row) is allocated by the plan at its first step and kept.
 * lto_direct_plan_qp_status: device int [n_batch] of the plan's last step, 1 = singular KKT system (outputs NaN), else 0. */
int lto_direct_qp_step_dev(lto_direct_plan* plan, void* stream, const double* Jac, long ldj, const double* defect, long ldd,
                           const double* X, long ldx, const double* U, long ldu, const double* t, int n_tgrids,
                           const lto_direct_targets* targets, int allow_impulsive, double* dX, double* dU, double* dV,
                           double* cost);
const int* lto_direct_plan_qp_status(const lto_direct_plan* plan);
/* Costates of the direct transcription from the multipliers of the plan's last frozen step (covector mapping).  Valid
 * after lto_direct_qp_step_dev on this plan, on the same stream, with the Jac that step read (LTO_EINVAL before any step, or when
 * the plan's last step was another variant).  With l_i the multiplier of defect i and E_i = d defect_i / d x_i, F_i = d defect_i /
 * d x_{i+1}:  Lambda_k = E_k^T l_k for k < n_nodes - 1 and Lambda_{n-1} = -F_{n-2}^T l_{n-2}; at an interior node the two agree up
 * to the solve's rounding (the QP's stationarity in dx_k).  Device outputs: Lambda [nstate][ldl], entry b * n_nodes + k; mult
 * [nstate][ldm], entry b * (n_nodes - 1) + i, the raw multipliers l_i (may be NULL); kkt_res [n_batch], per trajectory the largest
 * |E_k^T l_k + F_{k-1}^T l_{k-1}| over the interior nodes and components divided by its largest |Lambda| (0 with n_nodes = 2).  A
 * trajectory whose step was singular (lto_direct_plan_qp_status) gets NaN in all three.  Units: the cost is sum w |u|^2 with u in N
 * and w in TU; lto_direct_costates_batch gives the scaling to the indirect method's costates.
 * LTO_ENULL: plan, Jac, Lambda or kkt_res NULL.  LTO_EINVAL: ldj < (n_nodes-1) n_batch, ldl < n_nodes n_batch, mult with ldm <
 * (n_nodes-1) n_batch. */
int lto_direct_costates_dev(lto_direct_plan* plan, void* stream, const double* Jac, long ldj, double* Lambda, long ldl, double* mult,
                            long ldm, double* kkt_res);

/* Newton step of the indirect method solved on the device: delta = -Jac_full \ defect for the block-bidiagonal
 * [Phi_i | -I] system with both end states fixed (src/multiShoot_CRTBP_indirect.jl:123-142, :181-182), by structured
 * orthogonal cyclic reduction.  adjoints_only = 0: the square system of the regular iterations.  adjoints_only = 1:
 * the state columns of every node are masked out (:169-178) and the over-determined system is solved in the
 * least-squares sense, as `\` does.  Phi != NULL factors and solves; Phi == NULL re-uses the stored factorisation
 * of the same variant for a new right-hand side (the second-order-correction re-solve, :190-214).
 * delta is SoA [ndim][ldx], node-indexed.  ndim = 14 plans: the pinned columns are those of lto_indirect_solve (first node
 * 0-6, last node 0-5 and 13), and delta is exactly 0 there; LTO_LAYOUT_BLOCKS plans are refused for either ndim. */
int lto_indirect_newton_solve_dev(lto_indirect_plan* plan, void* stream, const double* Phi, long ldp,
                                  const double* defect, long ldd, int adjoints_only, double* delta, long ldx);
/* y[i] = x[i] + alpha d[i], i < count (trial points X + alpha dX, update accumulation) */
int lto_axpy_dev(lto_ctx* ctx, void* stream, const double* x, const double* d, double alpha, double* y, long count);
/* The n_alpha trial trajectories of lineSearch (src/multiShoot_CRTBP_indirect.jl:227-233) of every trajectory of a batch, one
 * launch: Xt[c*ldt + (b*n_alpha + a)*n_nodes + k] = X[c*ld + b*n_nodes + k] + alphas[a] * delta[c*ld + b*n_nodes + k] for
 * c < ndim, b < n_batch, a < n_alpha, k < n_nodes (SoA, node-indexed; alphas is a DEVICE array).  Together with a plan of
 * n_batch*n_alpha trajectories and lto_defect_norms_dev this is the batched line search for callers that keep their
 * own loop around the device-resident entry points. */
int lto_trial_points_dev(lto_ctx* ctx, void* stream, const double* X, const double* delta, long ld, int ndim, int n_nodes,
                         int n_batch, int n_alpha, const double* alphas, double* Xt, long ldt);
/* The per-iteration read-back of a Newton loop kept around the device-resident entry points: out[0..na) = a[..], out[na..na+nb) =
 * b[..] (device arrays; b may be NULL with nb = 0), returning when the values have arrived.  One small kernel writes them into a
 * page-locked block of the context behind everything queued on `stream`, and the host polls a sequence word -- no copy-engine
 * operation and no stream synchronisation; falls back to copies + synchronisation when the block cannot be mapped.  Not
 * thread-safe per context; `stream` must not be capturing. */
int lto_read_scalars_dev(lto_ctx* ctx, void* stream, const double* a, int na, const double* b, int nb, double* out);
/* lineSearch's decision (indirect.jl:244-245) and the defect check that follows the update (:328-331), without another sweep.  For
 * every trajectory b < n_batch: a* = first minimiser of sumsq[b*n_alpha .. ) (NaN trials never win), step[b] = alphas[a*];
 * maxabs_out[b] = maxabs[b*n_alpha + a*]; defect[c*ldd + b*seg + i] = trial_defect[c*ldt + (b*n_alpha + a*)*seg + i].  The updated
 * trajectory XC_all + xc_update*alpha with its end states pinned (:304, :324-325) is the chosen trial point bit for bit (one fma
 * each, the update's end-state rows are zero), so `defectCalc` at it is the part of the line search's own sweep that integrated it.
 * sumsq / maxabs as lto_defect_norms_dev leaves them for the n_batch*n_alpha trial trajectories; alphas is a DEVICE array.
 * maxabs with maxabs_out and trial_defect with defect may be NULL in pairs. */
int lto_line_search_pick_dev(lto_ctx* ctx, void* stream, const double* sumsq, const double* maxabs, const double* alphas, int n_alpha,
                             const double* trial_defect, long ldt, int ndim, int seg_per_traj, int n_batch, double* step,
                             double* maxabs_out, double* defect, long ldd);
/* Read-only entries to the load balancing of the adaptive sweeps, for step counts of the caller's choosing: the same
 * launches lto_indirect_plan_rebalance and the defect sweeps run, without a plan.  The environment switches LTO_ORDER_MODE and
 * LTO_ORDER_WEAVE play no part.  Both synchronise `stream` before they return; not thread-safe per context.
 * lto_segment_order_dev: order_dev[0 .. n_segments) (device ints) <- the lane order for the step counts accepted_dev[s] +
 * rejected_dev[s] (device ints), kind 1 = global (heaviest first over the whole batch), kind 2 = windowed with `weave` windows of
 * an XCD's list interleaved (1 .. 255; 0 = the kernel's choice; ignored by kind 1 but checked).  Workspace comes from the context.
 * kind not 1 or 2, weave outside 0 .. 255, n_segments < 1: LTO_EINVAL; a NULL pointer: LTO_ENULL; order_dev is then untouched. */
int lto_segment_order_dev(lto_ctx* ctx, int kind, int weave, int n_segments, const int* accepted_dev, const int* rejected_dev,
                          int* order_dev, void* stream);
/* lto_step_stats_dev: out_host[0 .. 3) <- [sum, max, n_segments] of accepted_dev[s] + rejected_dev[s] over s < n_segments: the
 * trial-step statistics a defect sweep leaves for the next one's choice of lanes per segment.  The maximum is taken from 0 up (step
 * counts are not negative).  The call also checks that the kernel left its device scratch zeroed for the next launch (LTO_EHIP if
 * not).  n_segments < 1: LTO_EINVAL; a NULL pointer: LTO_ENULL; out_host is then untouched. */
int lto_step_stats_dev(lto_ctx* ctx, int n_segments, const int* accepted_dev, const int* rejected_dev, long long* out_host,
                       void* stream);

/* Dense output (device): segment s is sampled at t_samples[first[s] .. first[s+1]) (sorted, inside the segment);
 * Y[c*ldy + j] = x_c(t_samples[j]); final_state[c*n_batch + b] (or NULL) = x(t_n) of trajectory b.  Built for what densify
 * (src/HelperFunctions.jl:51-101) needs -- ndim = 12 with LTO_DOP853_ADAPTIVE (for its Vern8) -- and for LTO_RK4; other plans:
 * LTO_EUNSUPPORTED (round 6 removed the 14-dim and RKF7(8) instantiations, which nothing ran). */
int lto_indirect_dense_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t,
                           int n_tgrids, const int* first, const double* t_samples, double* Y, long ldy,
                           double* final_state);
/* Dense output of the 14-row variable-mass system: the contract of lto_indirect_dense_dev on a 14-row plan, X [14][ldx],
 * Y [14][ldy], final_state [14 x n_batch]; every sample is reached by stepping the 14-row system onto it, so row 6 of Y is the
 * propagated mass.  LTO_RK4 and LTO_DOP853_ADAPTIVE; a plan that is not 14-row, or any other method: LTO_EUNSUPPORTED, before
 * anything is launched. */
int lto_indirect_dense_mass_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t,
                                int n_tgrids, const int* first, const double* t_samples, double* Y, long ldy,
                                double* final_state);

/* Switch times, burn arcs and dv of indirect solutions.  For a trajectory with parameters (thrustLimit, mass, p, rho):
 * n = |lambda_v|, aL = thrustLimit / mass / 1e3 * TU^2 / DU, umag(n) the control law of stateCostate_deriv.jl:36-53.  The engine is
 * ON iff g > 0 with   p = 0: always on (no event);   p = 1: g = n - 1 (more than half thrust);   p > 1: g = n - p aL^(p-1) (clamped
 * at the limit).  The trajectory is the piecewise multiple-shooting one: segment i is the flow from node i over [t_i, t_{i+1}], as
 * the defect sweep integrates it.  Every segment integrates (y, q), q' = umag(n), q(t_i) = 0, with the integrator of the call --
 * LTO_RK4 (`steps` steps) or LTO_DOP853_ADAPTIVE (all 13 components in the error norm, so the controller resolves the switch);
 * any other method, or ndim != 12: LTO_EUNSUPPORTED.  After every accepted step the on-state at the step's two ends is compared;
 * where it differs the crossing is bracketed by trial steps of the same formula from the step's start state, until the bracket's
 * ends are adjacent doubles in absolute time (at most 60 halvings), and t_event is the bracket's upper end: the first time on the
 * new side.  Integration continues from the accepted step unchanged.  TWO CROSSINGS INSIDE ONE ACCEPTED STEP ARE NOT SEEN.  A
 * segment keeps at most 4 events.  Where the on-state at the end of segment i differs from the one at the start of segment i+1
 * (the node's discontinuity straddles g = 0) an event at t_{i+1} is emitted, so that every list strictly alternates and its first
 * kind is +1 iff the trajectory starts off.
 * Outputs (column-major, trajectory b):  n_events[b];  t_event[max_events x B] ascending, NaN beyond the listed events;  kind[max_events x B]
 * +1 off->on, -1 on->off, 0 unused;  on0[b] the on-state at t[0];  dv[b] (DU/TU) the sum of the segments' q;  burn_time[b] (TU);
 * dv_seg[(n_nodes-1) x B] the segments' q (may be NULL);  status[b]: 0 ok;  1 more than max_events events, or more than 4 in one
 * segment: the lists are truncated in time order, n_events is the count of all events located, dv and burn_time are complete;
 * 2 non-finite trajectory: every output of it is NaN or 0.
 * n_tgrids and n_prm are 1 or n_batch.  LTO_ENULL; LTO_EINVAL (max_events < 1, n_nodes < 2, t not strictly increasing).
 * _dev: X [12][ldx], t and the outputs are device arrays in the layouts above; asynchronous on `stream`. */
int lto_indirect_events_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                              const lto_params* prm, int n_prm, const lto_integrator* integ, int max_events, int* n_events,
                              double* t_event, int* kind, int* on0, double* dv, double* burn_time, double* dv_seg, int* status);
int lto_indirect_events(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                        const lto_integrator* integ, int max_events, int* n_events, double* t_event, int* kind, int* on0,
                        double* dv, double* burn_time, double* dv_seg, int* status);
int lto_indirect_events_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                            int max_events, int* n_events, double* t_event, int* kind, int* on0, double* dv, double* burn_time,
                            double* dv_seg, int* status);

/* The same for the variable-mass system, y = (r, v, m, lambda_r, lambda_v, lambda_m), 14 rows.  Parameters
 * (thrustLimit, Isp, p, rho), lto_params.mass carrying Isp as everywhere for 14 rows.  n = |lambda_v| (rows 10..12), m = y[6],
 * cT = thrustLimit / 1e3 * TU^2 / DU, aL = cT / m, kappa = time_direction * 1e3 * DU / (TU * Isp * 9.81), umag(n, m) the law of the
 * 14-row system (the 12-row law with aL = cT / m).  The engine is ON iff g > 0 (g == 0 and NaN are off) with   p = 0: always on (no
 * event);   p = 1: g = n - 1;   p > 1: g = n - p (cT / m)^(p-1) with the CURRENT mass: the threshold moves as the engine burns.
 * Every segment integrates (y[14], q), q' = umag, q(t_i) = 0, with LTO_RK4 (`steps` steps) or LTO_DOP853_ADAPTIVE (all 15
 * components in the error norm); any other method, or a plan that is not 14-row: LTO_EUNSUPPORTED.  The crossing search (on-state
 * compared at the two ends of every accepted step, bisection in theta by trial steps of the same formula from the step's start
 * state to adjacent doubles, at most 60 halvings, t_event the bracket's upper end), the limit of 4 events per segment, the join
 * events, the truncation rules and the status codes are exactly those of lto_indirect_events_batch above; TWO CROSSINGS INSIDE ONE
 * ACCEPTED STEP ARE NOT SEEN here either.
 * Mass budget:  dm_seg[(n_nodes-1) x B] (kg, may be NULL) = m_i - m(t_{i+1}), the node's mass minus the propagated one.  The lane
 * carries the mass as m_i plus its change, so dm_seg keeps the digits that m_i + change would round away; where m_i + change == m_i
 * as doubles the propagated mass is the node's mass and dm_seg is exactly 0 (Isp -> infinity: the constant-mass system).
 * propellant[b] (kg, required) the sum of the trajectory's dm_seg in the order dv sums the q.
 * A node mass that is not finite and positive makes its trajectory status 2 (outputs NaN or 0 as for a non-finite trajectory); no
 * other trajectory is affected.  Errors as above.  _dev: X [14][ldx] on a 14-row plan. */
int lto_indirect_events_mass_batch(lto_ctx* ctx, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                   const lto_params* prm, int n_prm, const lto_integrator* integ, int max_events, int* n_events,
                                   double* t_event, int* kind, int* on0, double* dv, double* burn_time, double* dv_seg,
                                   double* propellant, double* dm_seg, int* status);
int lto_indirect_events_mass(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                             const lto_integrator* integ, int max_events, int* n_events, double* t_event, int* kind, int* on0,
                             double* dv, double* burn_time, double* dv_seg, double* propellant, double* dm_seg, int* status);
int lto_indirect_events_mass_dev(lto_indirect_plan* plan, void* stream, const double* X, long ldx, const double* t, int n_tgrids,
                                 int max_events, int* n_events, double* t_event, int* kind, int* on0, double* dv, double* burn_time,
                                 double* dv_seg, double* propellant, double* dm_seg, int* status);

/* Control replay: fly a given history of lambda_v from n_batch starts.  x = (r, v) for nstate = 6, (r, v, m) for
 * nstate = 7; the right-hand side is rows 0..5 of the 12-row system, or rows 0..6 of the 14-row system, with lambda_v replaced by
 * the spline value L(t) and every other costate unused:  n = |L|;  aL = thrustLimit / mass / 1e3 * TU^2 / DU (nstate 6, the
 * constant lto_params.mass) or cT / m with the current mass (nstate 7, lto_params.mass carrying Isp as everywhere for 14 rows);
 * umag(n) the control law for p = 0, p = 1, p > 1;  thrust acceleration -umag L / n (0 where n is 0);  mdot = -kappa umag m,
 * kappa = time_direction * 1e3 * DU / (TU * Isp * 9.81);  q' = umag.  This is the reference's CRTBP_prop_EP_NNControl_deriv!
 * (src/CRTBP_prop_EP_deriv.jl:128-215) with its two defects resolved: the `mass` undefined at :142 is the one above, and the flow
 * rate of :195, which feeds an acceleration into a formula in newtons, is the 14-row system's.
 * Control history: knots LinRange(t0, t1, n_knots), values lamv [3 x n_knots x n_hist] column-major, n_hist = 1 (one history for
 * every start) or n_batch (each start its own); L is the natural cubic spline (second derivative 0 at both ends) per component.
 * The integration runs knot interval by knot interval -- no step spans a knot -- each interval a span of its own with
 * LTO_DOP853_ADAPTIVE (x and q in the error norm; max_steps counts per interval) or LTO_RK4 (`steps` steps per interval); any
 * other method, or nstate not 6 or 7: LTO_EUNSUPPORTED.
 * x0 [nstate x B];  n_prm is 1 or B.  Out: x_final [nstate x B];  dv [B] (DU/TU) = q(t1);  accepted / rejected [B] summed over the
 * intervals (either may be NULL);  X_samples [nstate x n_samples x B]: the state at the knots k with k % sample_every == 0, and at
 * the last knot if that rule does not list it (sample_every = 0: none, X_samples may be NULL); the sample at knot 0 is x0 and the
 * last sample x_final, bit for bit.  status[b]: 0 ok;  2 a non-finite input or state, a start mass that is not finite and positive
 * (nstate 7), or an interval out of max_steps: x_final, dv and the samples from that interval on are NaN, no other trajectory is
 * affected.  LTO_ENULL; LTO_EINVAL (n_knots < 4, t1 <= t0 or not finite, n_hist or n_prm not 1 or B, sample_every < 0,
 * n_batch < 1). */
int lto_control_replay_batch(lto_ctx* ctx, int nstate, int n_knots, int n_batch, double t0, double t1, const double* lamv,
                             int n_hist, const double* x0, const lto_params* prm, int n_prm, const lto_integrator* integ,
                             int sample_every, double* x_final, double* X_samples, double* dv, int* accepted, int* rejected,
                             int* status);
int lto_control_replay(lto_ctx* ctx, int nstate, int n_knots, double t0, double t1, const double* lamv, const double* x0,
                       const lto_params* prm, const lto_integrator* integ, int sample_every, double* x_final, double* X_samples,
                       double* dv, int* accepted, int* rejected, int* status);

/* Neighbouring-extremal guidance: the first-order optimal feedback about a converged 12-row solution with a fixed
 * arrival state.  ndim must be 12: 14-row input (the variable-mass system) is refused with LTO_EUNSUPPORTED -- it goes to
 * lto_guidance_gains_mass_batch and lto_guided_flight_mass_batch below -- and so is every method but LTO_RK4 and LTO_DOP853_ADAPTIVE.
 * Gains.  XC [12 x n_nodes x n_batch], t [n_nodes x n_tgrids], prm and integ as in lto_indirect_events_batch.  The call runs the STM
 * sweep of lto_indirect_jacobian on a plan of its own (the kernel LTO_KERNEL_AUTO picks) and, with Phi_k = d y(t_{k+1}) / d y(t_k)
 * cut into 6 x 6 blocks A = Phi[0:6,0:6], B = Phi[0:6,6:12], C = Phi[6:12,0:6], D = Phi[6:12,6:12], the backward sweep
 *   K_{n-2} = -B^-1 A,   K_k = (D - K_{k+1} B)^-1 (K_{k+1} A - C),  k = n-3 .. 0,
 * every solve an LU with partial (row) pivoting and six right-hand sides: d lambda_k = K_k d x_k keeps the linearised arrival state
 * where it is.  Outputs: K [6 x 6 x (n_nodes-1) x n_batch] column-major blocks;  pivot [(n_nodes-1) x n_batch] (may be NULL) = the
 * smallest |u_ii| over the largest |entry| of the matrix solved at that node;  status[b]: 0 ok;  2 a non-finite Phi or gain;  3 a
 * node's pivot ratio is below sing_tol -- a state of the problem, not an error: for p = 0 the costate's scale is a null direction of
 * B, and so it is for p = 1 with a sharp switch while the law is saturated over the last segment (fully on or off: the thrust
 * magnitude no longer answers to the costate, so the arrival state is not controllable to first order).  On status 2 and 3
 * the gains of the failing node and of every earlier node are NaN, the later ones are valid (pivot: the failing node's ratio -- NaN
 * where the block itself is not finite -- and NaN before it); no other trajectory is affected, and a trajectory's gains are bit for
 * bit those of its single call.  LTO_ENULL; LTO_EINVAL (n_nodes < 2, n_batch < 1, t not strictly increasing, n_tgrids or n_prm not 1
 * or n_batch, sing_tol not in (0, 1)). */
int lto_guidance_gains_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                             const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, double* K,
                             double* pivot, int* status);
int lto_guidance_gains(lto_ctx* ctx, int ndim, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                       const lto_integrator* integ, double sing_tol, double* K, double* pivot, int* status);
/* Guided flight.  The nominal XC_nom [12 x n_nodes x n_nom] with its node times t [n_nodes x n_nom] and gains K [6 x 6 x
 * (n_nodes-1) x n_nom], n_nom = 1 (one nominal for every start) or n_batch;  x0 [6 x n_batch] the starts;  nav [6 x n_upd x
 * n_batch] or NULL, n_upd = (n_nodes-2) / update_every + 1: the navigation error added to the measured state at update j.  A start
 * carries y = (x, lambda, q), q' = umag (the 13 components of the thrust-event sweep), lambda(t_0) = lambda_nom,0.  For
 * k = 0 .. n_nodes-2:  if update_every > 0 and k % update_every == 0, lambda <- lambda_nom,k + K_k (x - x_nom,k + e_j),
 * j = k / update_every, otherwise lambda runs on by its own equation;  then y is integrated over [t_k, t_{k+1}] as a span of its own
 * with LTO_DOP853_ADAPTIVE (all 13 components in the error norm; max_steps counts per span) or LTO_RK4 (`steps` steps per span).
 * update_every = 0 never updates: the plain 12-row flow from (x0, lambda_nom,0).
 * Out: x_final [6 x B];  lam_final [6 x B] (may be NULL);  dv [B] (DU/TU) the sum of the spans' q;  X_nodes [6 x n_nodes x B] (may
 * be NULL): node 0 is x0 and the last node x_final, bit for bit;  accepted / rejected [B] summed over the spans (either may be
 * NULL);  status[b]: 0 ok;  2 a non-finite input, state or applied gain, or a span out of max_steps: x_final, lam_final, dv and the
 * nodes behind the failing span's start are NaN, no other start is affected.  n_prm is 1 or n_batch.  LTO_ENULL; LTO_EINVAL
 * (n_nodes < 2, n_batch < 1, n_nom or n_prm not 1 or n_batch, update_every < 0, t not strictly increasing). */
int lto_guided_flight_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC_nom, const double* t, const double* K,
                            int n_nom, const double* x0, int update_every, const double* nav, const lto_params* prm, int n_prm,
                            const lto_integrator* integ, double* x_final, double* lam_final, double* dv, double* X_nodes,
                            int* accepted, int* rejected, int* status);
int lto_guided_flight(lto_ctx* ctx, int ndim, int n_nodes, const double* XC_nom, const double* t, const double* K, const double* x0,
                      int update_every, const double* nav, const lto_params* prm, const lto_integrator* integ, double* x_final,
                      double* lam_final, double* dv, double* X_nodes, int* accepted, int* rejected, int* status);
/* The same for solutions of the 14-row variable-mass system: y = (x, lambda), x = (r, v, m), lambda = (lambda_r,
 * lambda_v, lambda_m), prm.mass carries Isp [s] as everywhere for 14 rows.  The solve pins r_f, v_f and lambda_m(t_f) = 0 and leaves
 * m_f free, so the gains keep d r_f = d v_f = 0 and d lambda_m(t_f) = 0: with Phi_k cut into 7 x 7 blocks A = Phi[0:7,0:7],
 * B = Phi[0:7,7:14], C = Phi[7:14,0:7], D = Phi[7:14,7:14],
 *   K_{n-2} = -M^-1 N,  M = rows 0..5 of B over row 6 of D,  N = rows 0..5 of A over row 6 of C,
 *   K_k = (D - K_{k+1} B)^-1 (K_{k+1} A - C),  k = n-3 .. 0,
 * every node one 7 x 7 system with seven right-hand sides, the matrix as it stands (no scaling).  XC [14 x n_nodes x n_batch];
 * K [7 x 7 x (n_nodes-1) x n_batch];  pivot, status, sing_tol and the LTO_ENULL / LTO_EINVAL rules as lto_guidance_gains_batch.
 * p = 0 and a law saturated over the whole last segment are singular (status 3) as in 12 rows.  Every method but LTO_RK4 and
 * LTO_DOP853_ADAPTIVE: LTO_EUNSUPPORTED. */
int lto_guidance_gains_mass_batch(lto_ctx* ctx, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                  const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, double* K,
                                  double* pivot, int* status);
int lto_guidance_gains_mass(lto_ctx* ctx, int n_nodes, const double* XC, const double* t, const lto_params* prm,
                            const lto_integrator* integ, double sing_tol, double* K, double* pivot, int* status);
/* Guided flight of the 14-row system.  XC_nom [14 x n_nodes x n_nom], t [n_nodes x n_nom], K [7 x 7 x (n_nodes-1) x n_nom];
 * x0 [7 x n_batch] (r, v, m);  nav [7 x n_upd x n_batch] or NULL.  A start carries (x[7], lambda[7], q), q' = umag, the 15 components
 * of lto_indirect_events_mass_batch, all in LTO_DOP853_ADAPTIVE's error norm; the update resets all seven costates,
 * lambda <- lambda_nom,k + K_k (x - x_nom,k + e_j), the measured mass included.  Spans, update_every, accepted / rejected and the
 * LTO_ENULL / LTO_EINVAL rules as lto_guided_flight_batch; update_every = 0 is the plain 14-row flow from (x0, lambda_nom,0).
 * Out: x_final [7 x B] (row 6 the final mass: the propellant is x0[6] - x_final[6]);  lam_final [7 x B] (may be NULL);  dv [B];
 * X_nodes [7 x n_nodes x B] (may be NULL): node 0 is x0 and the last node x_final, bit for bit;  status[b]: 0 ok;  2 a non-finite
 * input, state or applied gain, a span out of max_steps, or a mass that is not finite and positive at a span's start (the start
 * mass first of all): NaN from the failing span on, no other start is affected. */
int lto_guided_flight_mass_batch(lto_ctx* ctx, int n_nodes, int n_batch, const double* XC_nom, const double* t, const double* K,
                                 int n_nom, const double* x0, int update_every, const double* nav, const lto_params* prm, int n_prm,
                                 const lto_integrator* integ, double* x_final, double* lam_final, double* dv, double* X_nodes,
                                 int* accepted, int* rejected, int* status);
int lto_guided_flight_mass(lto_ctx* ctx, int n_nodes, const double* XC_nom, const double* t, const double* K, const double* x0,
                           int update_every, const double* nav, const lto_params* prm, const lto_integrator* integ, double* x_final,
                           double* lam_final, double* dv, double* X_nodes, int* accepted, int* rejected, int* status);
/* Linear covariance of the guided flight: what a start covariance P0 and a navigation covariance R leave of the state
 * covariance at every node, to first order -- exactly the linearisation of the guided flight above, nothing more (no process noise,
 * no execution error, no dv statistics).  ndim is 12 or 14 (NX = ndim / 2, ND = ndim; with 14 rows the gains are those of
 * lto_guidance_gains_mass_batch and prm.mass carries Isp).  The call runs the gains call as it stands (the same STM sweep, backward
 * sweep and split of mixed 14-row DOP853 batches: K, pivot and gain_status are bit for bit its outputs) and then, with Phi_k and
 * K_k still on the device, one forward pass per (trajectory, case).  A case i is (P0[:, :, i], R[:, :, i], update_every[i]); the
 * cases are shared by all trajectories.  Per pair the pass carries the ND x ND covariance Z of z = (dx, dlambda):
 *   P0 and R are symmetrised on load, a[r][c] <- 0.5 * (a[r][c] + a[c][r]);  Z = 0 but Z_xx = P0;  for k = 0 .. n_nodes-2:
 *   1. if update_every > 0 and k % update_every == 0, with P = Z_xx:  S = P + R (element by element, first);  U = K_k P;
 *      V = K_k S;  Z_lx = U;  Z_xl = U^T (copied, not recomputed);  Z_ll = V K_k^T;  Z_xx is left alone;
 *   2. T = Phi_k Z;  Z' = T Phi_k^T;  Z[r][c] = 0.5 * (Z'[r][c] + Z'[c][r]);
 *   3. P_{k+1} = Z_xx.
 * The arithmetic is fixed so that a host reproduces it bit for bit: binary64, every product and every sum rounded on its own (no
 * fused multiply-add), every dot product accumulated from its first product over j = 0, 1, ..:
 *   U[r][c] = sum_j K[r][j] P[j][c];  V[r][c] = sum_j K[r][j] S[j][c];  Z_ll[r][c] = sum_j V[r][j] K[c][j];
 *   T[r][c] = sum_j Phi[r][j] Z[j][c];  Z'[r][c] = sum_j T[r][j] Phi[c][j].
 * update_every = 0 never reads a gain; a gain at a node that is not an update node is never looked at.
 * In: n_cases >= 1;  P0, R [NX x NX x n_cases];  update_every [n_cases], each >= 0.  Out: K [NX x NX x (n_nodes-1) x n_batch], pivot
 * [(n_nodes-1) x n_batch], Phi [ND x ND x (n_nodes-1) x n_batch] (the STMs the call used, laid out as lto_indirect_jacobian's) and
 * P_nodes [NX x NX x n_nodes x n_cases x n_batch] may each be NULL;  gain_status [n_batch];  P_final [NX x NX x n_cases x n_batch];
 * cov_status [n_cases x n_batch].  Node 0 of P_nodes is the symmetrised P0 as it is, its last node equals P_final bit for bit.
 * cov_status: 0 ok;  2 a non-finite P0 or R (found at node 0, whether R is used or not), a non-finite Phi_k, or a non-finite gain
 * at an update node k -- the NaN gains of a gain_status 2 or 3 trajectory end up here: P is NaN from node k + 1 on and P_final is NaN;
 * no other case and no other trajectory is affected.  A (trajectory, case) pair's outputs are bit for bit those of the call with
 * that trajectory and that case alone.  LTO_ENULL and LTO_EINVAL as lto_guidance_gains_batch, and LTO_EINVAL for n_cases < 1
 * (or above 262140) or an update_every[i] < 0;  LTO_EUNSUPPORTED for ndim not 12 or 14 and for every method but LTO_RK4 and
 * LTO_DOP853_ADAPTIVE. */
int lto_guidance_covariance_batch(lto_ctx* ctx, int ndim, int n_nodes, int n_batch, const double* XC, const double* t, int n_tgrids,
                                  const lto_params* prm, int n_prm, const lto_integrator* integ, double sing_tol, int n_cases,
                                  const double* P0, const double* R, const int* update_every, double* K, double* pivot,
                                  int* gain_status, double* Phi, double* P_nodes, double* P_final, int* cov_status);

int lto_direct_plan_create(lto_ctx* ctx, int nstate, int n_nodes, int n_batch, int nsteps,
                           const lto_direct_params* prm, lto_direct_plan** out);
void lto_direct_plan_destroy(lto_direct_plan* plan);
/* Jacobian kernel: LTO_KERNEL_PER_LANE (each lane re-integrates the half-arc with one sensitivity column) or
 * LTO_KERNEL_PIPE (base wave + one wave per sensitivity column for 32 segments, skewed by one RKF7(8) step: one barrier
 * per step).  AUTO = PIPE from 3 072 segments, PER_LANE below.  LTO_KERNEL_COOP (the wave-specialised form of rounds 1-2,
 * one barrier per RK stage, never the fastest) was removed in round 3: LTO_EINVAL. */
int lto_direct_plan_set_kernel(lto_direct_plan* plan, int kernel);
int lto_direct_defect_dev(lto_direct_plan* plan, void* stream, const double* X, long ldx, const double* U, long ldu,
                          const double* t, int n_tgrids, double* defect, long ldd, double* errors);
/* x_mid[c*ldm + s] = forward half-arc end state of segment s (see lto_direct_midpoints); defect/errors optional. */
int lto_direct_midpoints_dev(lto_direct_plan* plan, void* stream, const double* X, long ldx, const double* U, long ldu,
                             const double* t, int n_tgrids, double* x_mid, long ldm, double* defect, long ldd,
                             double* errors);
int lto_direct_jacobian_dev(lto_direct_plan* plan, void* stream, const double* X, long ldx, const double* U,
                            long ldu, const double* t, int n_tgrids, double* Jac, long ldj, double* dtf,
                            double* defect, long ldd, double* errors);

/* Layout kernels: Julia column-major [ndim x count] (node-contiguous) <-> SoA [ndim][ld]. */
int lto_pack_soa_dev(lto_ctx* ctx, void* stream, const double* aos, int ndim, long count, double* soa, long ld);
int lto_unpack_soa_dev(lto_ctx* ctx, void* stream, const double* soa, long ld, int ndim, long count, double* aos);

/* Per-trajectory reductions the drivers take of a defect array (line search cost sum(defect.^2),
 * src/multiShoot_CRTBP_indirect.jl:240; convergence test norm(defect[:], Inf), :331):
 *   sumsq[b], maxabs[b] for b < n_batch over the ndim x seg_per_traj block of trajectory b. */
int lto_defect_norms_dev(lto_ctx* ctx, void* stream, const double* defect, long ldd, int ndim, int seg_per_traj,
                         int n_batch, double* sumsq, double* maxabs);

/* ------------------------------------------------- several GPUs behind one host process
 * For a single-process host (the Julia drivers) that owns more than one GPU.  A group holds one context per entry of
 * device_ids (ids may repeat).  Each call is split into contiguous shards -- whole trajectories when n_batch > 1,
 * otherwise segment blocks of the one trajectory with a one-node halo (segment i reads nodes i and i+1 only:
 * multiShoot_CRTBP_indirect.jl:71-86, multiShoot_CRTBP_direct.jl:77-105) -- and every shard runs the single-device entry
 * point of the same name on its own host thread.  Arguments, layouts, results and error codes are those of
 * lto_indirect_defect / lto_indirect_jacobian / lto_direct_defect / lto_direct_jacobian; each shard writes its own
 * contiguous slab of the caller's column-major outputs, so there is no collective.  (Multi-process hosts shard the
 * same way with one lto_ctx per process: bench.py, lowthrustopt_amd/sharding.py.) */
typedef struct lto_group lto_group;
int lto_group_create(int n_devices, const int* device_ids, lto_group** out);
void lto_group_destroy(lto_group* group);
const char* lto_group_last_error(const lto_group* group);
int lto_group_size(const lto_group* group);
lto_ctx* lto_group_ctx(lto_group* group, int k); /* member k's context (owned by the group): device-resident plans and sweeps per GPU */
int lto_group_indirect_defect(lto_group* group, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                              int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, double* defect,
                              double* errors);
int lto_group_indirect_jacobian(lto_group* group, int ndim, int n_nodes, int n_batch, const double* XC, const double* t,
                                int n_tgrids, const lto_params* prm, int n_prm, const lto_integrator* integ, double* Phi,
                                double* defect);
int lto_group_direct_defect(lto_group* group, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                            const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double* defect,
                            double* errors);
int lto_group_direct_jacobian(lto_group* group, int nstate, int n_nodes, int n_batch, const double* X, const double* U,
                              const double* t, int n_tgrids, int nsteps, const lto_direct_params* prm, double* Jac_temp,
                              double* ddefect_dtf, double* defect, double* errors);

/* ------------------------------------------------------------------------------- collectives (RCCL over xGMI)
 * The one exchange step of the path.  A sweep shards with no data-path collective (segment i needs nodes i, i+1 only:
 * multiShoot_CRTBP_indirect.jl:71-86); what every rank needs afterwards is the full defect vector or its norms for the
 * convergence test and the line-search decision (indirect.jl:240 sum(defect.^2), :331 norm(defect, Inf)).  These entry
 * points do that device to device -- nothing returns to the host between sweep and decision:
 *   sweep (lto_*_dev) -> lto_defect_norms_dev on the local slab -> lto_comm_allreduce_dev(SUM / MAX), or
 *   sweep -> lto_comm_allgather_dev of the slabs -> lto_defect_norms_dev on the gathered vector.
 * RCCL is bound at run time (dlopen): without it these calls return LTO_EUNSUPPORTED and everything else works. */
#define LTO_COMM_ID_BYTES 128
#define LTO_COMM_SUM 0
#define LTO_COMM_MAX 1
typedef struct lto_comm lto_comm;
int lto_comm_available(void);
/* One process per GPU: one rank calls lto_comm_unique_id, the launcher (torch.distributed, MPI, a file) hands the 128
 * bytes to every rank, every rank calls lto_comm_create (collective: ncclCommInitRank on the context's device). */
int lto_comm_unique_id(void* id128);
int lto_comm_create(lto_ctx* ctx, int world, int rank, const void* id128, lto_comm** out);
void lto_comm_destroy(lto_comm* comm);
const char* lto_comm_last_error(const lto_comm* comm);
int lto_comm_size(const lto_comm* comm);
int lto_comm_rank(const lto_comm* comm);
/* Number of ranks RCCL itself reports for this communicator (ncclCommCount): world for an lto_comm_create communicator, 0 for a
 * window communicator (no RCCL behind it), LTO_ENULL / LTO_EUNSUPPORTED (< 0) when it cannot be asked.  What a scaling run quotes as "RCCL saw N ranks". */
int lto_comm_rccl_ranks(const lto_comm* comm);
/* recv [world][count] <- send [count] of every rank (equal counts); asynchronous on `stream` (hipStream_t). */
int lto_comm_allgather_dev(lto_comm* comm, void* stream, const double* send, double* recv, long count);
/* buf [count] <- LTO_COMM_SUM / LTO_COMM_MAX over ranks, in place; asynchronous on `stream`.  Both propagate NaN (the max
 * carries a NaN indicator per element), so a NaN on one rank reaches every rank: norm(defect, Inf) of indirect.jl:330. */
int lto_comm_allreduce_dev(lto_comm* comm, void* stream, double* buf, long count, int op);
/* Second transport for the same two collectives, without RCCL and without compute units for the payload ("windows"): every
 * rank owns a receive window in device memory, its peers map it through HIP IPC, a rank pushes its slab into every window
 * with device copies and raises a sequence flag there; the consumer's stream waits on the flags with a one-wavefront kernel
 * (bounded: a rank that never arrives turns the result into NaN instead of hanging the stream).  It is also the transport for
 * two ranks that share one device, which RCCL refuses.  Set-up, every rank:
 *   lto_comm_window_export(ctx, world, rank, max_count, handle, &comm)   handle: LTO_COMM_WINDOW_BYTES bytes
 *   the launcher gathers the world handles in rank order (torch.distributed all_gather, MPI_Allgather, a file)
 *   lto_comm_window_open(comm, all_handles)
 * then lto_comm_allgather_dev / lto_comm_allreduce_dev with count <= max_count, lto_comm_destroy at the end (after a
 * barrier of the launcher: a peer may still be pushing).  One process per rank.
 * ONE STREAM: the collectives of a window communicator must all be enqueued on the same stream (the first one it is used on; a
 * different one returns LTO_EINVAL) -- the reuse of a window half, the push counters and the sequence numbers are ordered by it.
 * A driver that gathers on a side stream and reduces norms on its main stream uses two communicators.
 * FAILURE: a wait that runs out (lto_comm_set_wait_limit polls of ~1.5 us each, default 4e6) or a peer found two or more
 * collectives ahead (the ranks have lost step) sets the communicator's fail word: that collective and every later one of this
 * rank return NaN -- never a slab of another iteration -- and lto_comm_status reports it to the host. */
#define LTO_COMM_WINDOW_BYTES 128
int lto_comm_status(lto_comm* comm, void* stream, int* failed);
int lto_comm_set_wait_limit(lto_comm* comm, long polls);
/* Window transport: payloads of up to `bytes` per rank travel by the push / collect KERNELS (default 4 MiB: a kernel after a
 * kernel costs ~2 us of queue hand-over, a copy-engine operation between kernels ~10 us), larger ones by the copy engines with a
 * one-wavefront wait kernel; 0 = always the copy engines.  Every block of the collect kernel polls for its peers' flags, which is
 * free when each rank owns its GPU (the deployment) and starves the peers' push kernels when several ranks SHARE one device
 * and the payload needs thousands of blocks: rehearsals on a shared device lower this (bench.py, LTO_BENCH_SHARE_DEVICE). */
int lto_comm_set_kernel_payload(lto_comm* comm, long bytes);
int lto_comm_window_export(lto_ctx* ctx, int world, int rank, long max_count, void* handle_out, lto_comm** out);
int lto_comm_window_open(lto_comm* comm, const void* all_handles);
int lto_comm_uses_windows(const lto_comm* comm);
/* One host process, several GPUs: the communicators of an lto_group (ncclCommInitAll over its devices).  send[k] /
 * recv[k] / buf[k] live on member k's device; the work is enqueued on member k's context stream (lto_ctx_stream), after
 * the sweep that produced send[k] there.  A group that repeats one device (1-GPU boxes) uses device copies instead. */
typedef struct lto_group_comm lto_group_comm;
/* all-gather payloads up to this many bytes per member go by peer copies ordered by events (copy engines over xGMI, no
 * compute unit taken from the sweeps) even when the group has an RCCL clique; larger ones through RCCL */
#define LTO_GROUP_PEER_COPY_BYTES (1 << 20)
int lto_group_comm_create(lto_group* group, lto_group_comm** out);
void lto_group_comm_destroy(lto_group_comm* comm);
const char* lto_group_comm_last_error(const lto_group_comm* comm);
int lto_group_comm_uses_rccl(const lto_group_comm* comm);
int lto_group_comm_allgather_dev(lto_group_comm* comm, const double* const* send, double* const* recv, long count);
int lto_group_comm_allreduce_dev(lto_group_comm* comm, double* const* buf, long count, int op);

#ifdef __cplusplus
}
#endif
#endif /* LTO_H */
