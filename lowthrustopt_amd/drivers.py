"""Host-side mirror of the reference's indirect shooting drivers, calling the HIP hot path.

  multiShoot_CRTBP_indirect   src/multiShoot_CRTBP_indirect.jl:58-61, :254-345   (Newton loop, status flags)
  optimizeTraj_OLS            :149-218   (least-squares step, adjoints-only mask, second-order correction)
  lineSearch                  :221-246   (20 alphas; here ONE batched device launch instead of 20 sweeps -- SURVEY N2)
  reduceFuel_indirect         src/HelperFunctions.jl:105-193   (rho continuation -- SURVEY N3)
  meshRefine_direct           src/multiShoot_CRTBP_direct.jl:597-680   (errors-driven mesh refinement -- SURVEY N4)
  lineSearch_direct           src/multiShoot_CRTBP_direct.jl:405-430   (10 alphas in ONE batched launch -- SURVEY N2)
  homotopy_solve              concurrent form of the rho continuation (HelperFunctions.jl:105-193): every level of the
                              ladder is a trajectory of ONE batched device Newton loop (lto_indirect_solve_batch)
  multiShoot_CRTBP_indirect_mass / optimizeTraj_OLS_mass / reduceFuel_indirect_mass / lift_to_mass
                              the same loop on the 14-dim variable-mass system (free final mass, lambda_m(tf) = 0):
                              what the reference's `nstate == 7` branches (:158-161, :195-199) were meant to solve.
                              Both systems run one loop (_solve_indirect) and one least-squares step (_ols_step); they
                              differ only in which entries of XC_all[:, node] are pinned (_PINS, keyed by the row count)
  fly_control / dispersion    src/CRTBP_prop_EP_deriv.jl:128-215 re-specified (CRTBP_prop_EP_NNControl_deriv!): a
                              solution's lambda_v(t) as a spline, flown open loop from dispersed starts in ONE device call
  controlLaw_cart             src/multiShoot_CRTBP_indirect.jl:389-440 (costates -> thrust vectors in N: the u_all format
                                                                        of the direct transcription; host post-processing)

Same signatures, return tuples and status flags as the Julia functions (the reference is Julia; this mirror exists
because no `julia` binary is available to run julia/LowThrustOptHIP.jl -- see INTEGRATION.md).  The propagation
(defects, STM blocks) always runs on the GPU through the C ABI; only the small sparse least-squares solve is on the
host, as in the reference (`-Jac_sparse \\ defect_vec`, :182).

  multiShoot_CRTBP_direct     src/multiShoot_CRTBP_direct.jl:58-594 for flagEnd = false (the reference demo's setting): the
                              JuMP/Ipopt subproblem optimizeTraj (:248-403) is then an equality-constrained convex QP, solved
                              exactly -- on the device by lto_direct_solve (ops=None), on the host by a dense KKT solve
                              (direct_qp_dense) when `ops` is injected.  flagEnd = true (box-bounded tau updates, beta
                              penalty) stays out of scope.
  interpEndStates             :434-461 (natural cubic spline of the end-orbit tables)

`ops` lets the CPU unit tests inject a different propagation back end; the product default is the HIP library.
"""
import collections

import numpy as np

from . import hotpath
from .constants import day


class HipOps:
    """Hot-path operators backed by liblto_hip.so (the product path)."""

    def __init__(self, ctx=None, integ=None):
        self.ctx = ctx or hotpath.default_context()
        self.integ = integ or hotpath.integrator()     # adaptive order 8 @ 1e-13 = the reference's Vern8 setting

    def defect(self, XC, t, params):
        d, _ = hotpath.indirect_defectCalc(XC, t, params, self.integ, ctx=self.ctx)
        return d

    def stm(self, XC, t, params):
        return hotpath.indirect_stm(XC, t, params, self.integ, ctx=self.ctx)

    def newton_step(self, XC, t, params, flag_adjointsOnly=False):
        """jacobianCalc + least-squares step (incl. the adjoints-only mask) + second-order correction in one
        device-resident call (indirect.jl:290-296): Phi never leaves HBM."""
        upd, _ = hotpath.indirect_newton_step(XC, t, params, self.integ, ctx=self.ctx, flag_adjointsOnly=flag_adjointsOnly)
        return upd

    def defect_batch_sumsq(self, XC_batch, t, params):
        """sum(defect.^2) per trial trajectory: one batched launch (+ on-device reduction when torch is present)."""
        d, _ = hotpath.indirect_defectCalc(XC_batch, t, params, self.integ, ctx=self.ctx)
        return np.sum(d * d, axis=(0, 1))


def _solve_ls(J, rhs):
    """x = -J \\ rhs (least squares).  The systems here are square or over-determined once the fixed-end-state
    columns are dropped, so the solution is unique and independent of the factorisation used."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    if sp.issparse(J):
        keep = np.flatnonzero(np.diff(J.tocsc().indptr) > 0)
        Jk = J.tocsc()[:, keep]
        x = np.zeros(J.shape[1])
        if Jk.shape[0] == Jk.shape[1]:
            try:
                x[keep] = spl.spsolve(Jk, -rhs)
                if np.all(np.isfinite(x)):
                    return x
            except Exception:
                pass
        sol = spl.lsmr(Jk, -rhs, atol=1e-15, btol=1e-15, conlim=1e14, maxiter=20 * Jk.shape[1])[0]
        x[keep] = sol
        return x
    return np.linalg.lstsq(J, -rhs, rcond=None)[0]


# Entries of XC_all[:, node] pinned in every Newton iteration, by row count: (rows at the first node, rows at the last node, rows
# of the last node held at 0).  12 rows: r, v at both ends (indirect.jl:270-271, :324-325).  14 rows: also m0 at the first node,
# and lambda_m(tf) = 0 at the last -- the transversality condition of the free final mass.
_PINS = {12: ([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], []),
         14: ([0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 13], [13])}


def _pinned(nd, n_nodes):
    """[nd x n_nodes] mask of the pinned entries."""
    first, last, _ = _PINS[nd]
    m = np.zeros((nd, n_nodes), dtype=bool)
    m[first, 0] = True
    m[last, -1] = True
    return m


def _ols_step(XC_all, t_TU, defect, Phi, n_nodes, params, flag_adjointsOnly, ops):
    """optimizeTraj_OLS of 12 or 14 rows (indirect.jl:149-218): x = -J \\ defect over the free columns of Jac_full -- all but the
    pinned ones, adjoints-only also without every node's state columns (:169-178) -- then the second-order correction with the
    same Jacobian.  The pinned entries of the update are exactly 0."""
    Phi = np.asarray(Phi)
    nd = Phi.shape[0]
    J = hotpath.indirect_scatter(Phi, sparse=True) if nd == 12 else hotpath.indirect_scatter_mass(Phi, sparse=True)
    free = ~_pinned(nd, n_nodes)
    if flag_adjointsOnly:
        free[:nd // 2] = False
    free = free.reshape(-1, order="F")
    Jm = J[:, np.flatnonzero(free)]
    upd = np.zeros(nd * n_nodes)
    upd[free] = _solve_ls(Jm, np.asarray(defect).reshape(-1, order="F"))     # :182
    xc_update = upd.reshape(nd, n_nodes, order="F")
    if np.abs(xc_update).max() < 1e-1:                      # :190  SOC: same Jacobian, defect at the trial point
        d_soc = ops.defect(XC_all + xc_update, t_TU, params)
        upd2 = np.zeros(nd * n_nodes)
        upd2[free] = _solve_ls(Jm, np.asarray(d_soc).reshape(-1, order="F"))
        xc_update = xc_update + upd2.reshape(nd, n_nodes, order="F")
    return xc_update


def optimizeTraj_OLS(XC_all, t_TU, defect, Phi, nstate, n_nodes, params, flag_adjointsOnly, ops):
    """Least-squares Newton step with second-order correction (indirect.jl:149-218), 12 rows."""
    return _ols_step(XC_all, t_TU, defect, Phi, n_nodes, params, flag_adjointsOnly, ops)


def lineSearch(XC_all, xc_update, t_TU, params, ops):
    """alpha in LinRange(0.1, 1, 20) minimising sum(defect.^2) (indirect.jl:221-246), all 20 trial trajectories in
    one batched sweep."""
    alpha_all = np.linspace(0.1, 1.0, 20)
    trial = XC_all[:, :, None] + xc_update[:, :, None] * alpha_all[None, None, :]
    er = ops.defect_batch_sumsq(np.asfortranarray(trial), t_TU, params)
    return float(alpha_all[int(np.argmin(er))])             # first minimiser, as `alpha[er .== minimum(er)][1]`


def _solve_indirect(XC_all, t_TU, n_nodes, params, flag_adjointsOnly, maxIter, ops, verbose):
    """The Newton loop of multiShoot_CRTBP_indirect (indirect.jl:254-345) for 12 or 14 rows: with ops=None one lto_indirect_solve
    call, the trajectory resident on the device; with an injected `ops` the Python mirror below.  Returns (XC_all, defect,
    status_flag)."""
    if ops is None:
        XC_out, defect, status_flag, iterCount, hist = hotpath.indirect_solve(XC_all, t_TU, params, None, flag_adjointsOnly, maxIter)
        if verbose:
            for k, (er, alpha) in enumerate(hist):
                print("Iter %d. Max defect = %.2e. alpha = %.3f." % (k + 1, er, alpha))
                if not (er <= 1e3):
                    print("Not likely to converge. Aborting.")
            if status_flag == 1:
                print("Reached max iteration count at %d iterations" % iterCount)
        return XC_out, defect, status_flag
    nd = XC_all.shape[0]
    t_TU = np.array(t_TU, dtype=np.float64)
    XC_all[_PINS[nd][2], -1] = 0.0                           # 14 rows: lambda_m(tf) = 0 on entry
    pinned = _pinned(nd, XC_all.shape[1])
    pins = XC_all[pinned]                                    # :270-271
    # the 12-row mirror takes an injected device step where there is one; the 14-row mirror always takes the host step
    device_step = nd == 12 and hasattr(ops, "newton_step") and getattr(ops, "device_newton", True)
    status_flag = 0
    defect = ops.defect(XC_all, t_TU, params)                # :274
    iterCount = 0
    er = 1.0
    while er > 1e-10:                                        # :280
        iterCount += 1
        if iterCount > maxIter:
            if verbose:
                print("Reached max iteration count at %d iterations" % iterCount)
            status_flag = 1
            break
        if device_step:
            xc_update = ops.newton_step(XC_all, t_TU, params, flag_adjointsOnly)   # :290-296 on the device
        else:
            Phi, _ = ops.stm(XC_all, t_TU, params)           # jacobianCalc, :290
            xc_update = _ols_step(XC_all, t_TU, defect, Phi, n_nodes, params, flag_adjointsOnly, ops)
        alpha = 1.0
        if iterCount > 3:                                    # :300
            alpha = lineSearch(XC_all, xc_update, t_TU, params, ops)
        XC_all = XC_all + xc_update * alpha
        XC_all[pinned] = pins                                # :324-325
        defect = ops.defect(XC_all, t_TU, params)            # :328
        er = float(np.max(np.abs(defect))) if np.all(np.isfinite(defect)) else float("nan")
        if verbose:
            print("Iter %d. Max defect = %.2e. alpha = %.3f." % (iterCount, er, alpha))
        if not (er <= 1e3):                                  # :333-336 (also leaves the loop on NaN)
            if verbose:
                print("Not likely to converge. Aborting.")
            iterCount += 100
            if er != er:
                break
    if np.isnan(XC_all[0, 0]) or not np.all(np.isfinite(defect)):
        status_flag = 2                                      # :339-341
    return XC_all, defect, status_flag


def multiShoot_CRTBP_indirect(XC_all, t_TU, MU, DU, TU, n_nodes, mass0, thrustLimit, plot_yn, flag_adjointsOnly,
                              maxIter, p, rho, ops=None, verbose=True):
    """Indirect multiple shooting with fixed end states (indirect.jl:58-61, :254-345).
    Returns (XC_all, defect, status_flag): 0 converged, 1 maxIter reached, 2 NaN.
    The driver is the reference's: 12 rows (state + costate, constant mass `mass0`).  The 14-dim extension (mass and mass
    costate as states, Isp in the parameter tuple's mass slot) is solved by multiShoot_CRTBP_indirect_mass -- the reference's
    loop pins XC_all[1:6] and solves 12x12 blocks (indirect.jl:324-325).  ops=None: one lto_indirect_solve call; an injected
    `ops` runs the Python mirror of the loop, with `ops.newton_step` when it has one (and `device_newton` is not False), else
    `ops.stm` and the host step optimizeTraj_OLS."""
    if np.asarray(XC_all).shape[0] != 12:
        raise ValueError("multiShoot_CRTBP_indirect drives the reference's 12-row state+costate system; got %d rows "
                         "(the 14-row variable-mass system is solved by multiShoot_CRTBP_indirect_mass)" % np.asarray(XC_all).shape[0])
    params = hotpath.make_params(MU, DU, TU, thrustLimit, mass0, 1.0, p, rho)   # :258-260
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    return _solve_indirect(XC_all, t_TU, n_nodes, params, flag_adjointsOnly, maxIter, ops, verbose)


def reduceFuel_indirect(XC_all, t_TU, MU, DU, TU, n_nodes, mass, thrustLimit, rho_current, rho_target, ops=None,
                        verbose=True, rng=None):
    """rho continuation (HelperFunctions.jl:105-193): halve rho on success, back off on failure.
    status_flag 3 = continuation exhausted (:161)."""
    def run(X, rho):
        return multiShoot_CRTBP_indirect(X, t_TU, MU, DU, TU, n_nodes, mass, thrustLimit, False, False, 10, 1.0, rho,
                                         ops=ops, verbose=verbose)
    return _rho_continuation(run, XC_all, rho_current, rho_target, rng)


def _rho_continuation(run, XC_all, rho_current, rho_target, rng=None):
    """The continuation loop of reduceFuel_indirect (HelperFunctions.jl:105-193); run(X, rho) -> (XC, defect, status)."""
    rng = rng or np.random.default_rng(0)
    if rho_target > rho_current:
        rho_target = rho_current
    rho_temp = rho_current

    XC_new, defect, status = run(XC_all, rho_temp)
    if status == 0 and rho_current == rho_target:
        return XC_new, defect, status
    while status != 0 and rho_temp < 1:                      # :133-143
        rho_temp = min(rho_temp * 5, 1.0)
        XC_new, defect, status = run(XC_all, rho_temp)
    if rho_temp == 1 and status != 0:
        return XC_new, defect, status
    if status == 0:
        XC_all = XC_new.copy()
    count = 0
    while rho_temp > rho_target or status != 0:              # :158-188
        count += 1
        if count > 100:
            return XC_new, defect, 3
        if status == 0:
            XC_all = XC_new.copy()
            rho_temp = max(rho_temp / 2, rho_target)
        else:
            rho_temp *= 3 * (1 + rng.random())
        XC_new, defect, status = run(XC_all, rho_temp)
    return XC_new, defect, status


def lift_to_mass(XC12, mass0):
    """12 rows (r, v, lambda_r, lambda_v) -> the 14 rows of the variable-mass system (r, v, m, lambda_r, lambda_v, lambda_m)
    with m = mass0 and lambda_m = 0 at every node.  [12 x n] or [12 x n x B]."""
    X = np.asarray(XC12, dtype=np.float64)
    if X.shape[0] != 12:
        raise ValueError("lift_to_mass takes 12 rows; got %d" % X.shape[0])
    out = np.zeros((14,) + X.shape[1:], order="F")
    out[0:6] = X[0:6]
    out[6] = mass0
    out[7:13] = X[6:12]
    return out


def optimizeTraj_OLS_mass(XC_all, t_TU, defect, Phi, n_nodes, params, flag_adjointsOnly, ops):
    """The least-squares Newton step of the 14-dim variable-mass system: optimizeTraj_OLS on Jac_full from indirect_scatter_mass.
    Square for the regular step, least squares for adjoints-only."""
    return _ols_step(XC_all, t_TU, defect, Phi, n_nodes, params, flag_adjointsOnly, ops)


def multiShoot_CRTBP_indirect_mass(XC_all, t_TU, MU, DU, TU, n_nodes, Isp, thrustLimit, plot_yn, flag_adjointsOnly,
                                   maxIter, p, rho, ops=None, verbose=True):
    """Indirect multiple shooting of the 14-dim variable-mass system y = (r, v, m, lambda_r, lambda_v, lambda_m), free final
    mass.  Pinned in every iteration: XC_all[0:7, 0] (r0, v0, m0 = XC_all[6, 0]) and XC_all[0:6, -1] (rf, vf); on entry
    XC_all[13, -1] = lambda_m(tf) is set to 0, the transversality condition of the free final mass.  Otherwise the reference
    loop of multiShoot_CRTBP_indirect: stop at max|defect| <= 1e-10, second-order correction, the 20-point line search from
    iteration 4, status flags 0 / 1 / 2.  ops=None: one lto_indirect_solve call (ndim = 14, Isp in the parameter tuple's mass
    slot); an injected `ops` runs the Python mirror with `ops.stm` and the host step optimizeTraj_OLS_mass.
    Returns (XC_all, defect, status_flag)."""
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    if XC_all.ndim != 2 or XC_all.shape[0] != 14:
        raise ValueError("multiShoot_CRTBP_indirect_mass takes the 14-row variable-mass system; got shape %s "
                         "(lift_to_mass(XC12, mass0) builds it from 12 rows)" % (XC_all.shape,))
    if not (Isp > 0):
        raise ValueError("Isp must be positive; got %r" % (Isp,))
    if not (XC_all[6, 0] > 0):
        raise ValueError("the initial mass XC_all[6, 0] must be positive; got %r" % (XC_all[6, 0],))
    params = hotpath.make_params(MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)   # mass slot = Isp for 14 rows
    return _solve_indirect(XC_all, t_TU, n_nodes, params, flag_adjointsOnly, maxIter, ops, verbose)


def reduceFuel_indirect_mass(XC_all, t_TU, MU, DU, TU, n_nodes, Isp, thrustLimit, rho_current, rho_target, ops=None,
                             verbose=True, rng=None):
    """The rho continuation of reduceFuel_indirect (HelperFunctions.jl:105-193) on the 14-dim variable-mass system: p = 1,
    10 iterations per level, halve rho on success, back off on failure; status_flag 3 = continuation exhausted."""
    def run(X, rho):
        return multiShoot_CRTBP_indirect_mass(X, t_TU, MU, DU, TU, n_nodes, Isp, thrustLimit, False, False, 10, 1.0, rho,
                                              ops=ops, verbose=verbose)
    return _rho_continuation(run, XC_all, rho_current, rho_target, rng)


def homotopy_defect_sweep(XC_levels, t_TU, MU, DU, TU, mass, thrustLimit, rhos, ops=None):
    """All continuation levels evaluated concurrently (BASELINE configs[3]): level l has its own node array
    XC_levels[:, :, l] and smoothing rho_l; ONE launch returns max|defect| and sum(defect^2) per level."""
    ops = ops or HipOps()
    prms = [hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, 1.0, r) for r in rhos]
    d, _ = hotpath.indirect_defectCalc(np.asfortranarray(XC_levels), t_TU, prms, ops.integ, ctx=ops.ctx)
    return np.max(np.abs(d), axis=(0, 1)), np.sum(d * d, axis=(0, 1)), d


class HipDirectOps:
    """Direct-method hot-path operators backed by liblto_hip.so."""

    def __init__(self, MU, DU, TU, Isp, ctx=None):
        self.ctx = ctx or hotpath.default_context()
        self.MU, self.DU, self.TU, self.Isp = MU, DU, TU, Isp

    def defect(self, X, U, t, nsteps):
        return hotpath.direct_defectCalc(X, U, t, nsteps, self.MU, self.DU, self.TU, self.Isp, ctx=self.ctx)

    def midpoints(self, X, U, t):
        """x(t_i + h_i/2) from node i with u_i, one RKF7(8) step (`ode7` over [t_i, t_new], direct.jl:651-656)."""
        return hotpath.direct_midpoints(X, U, t, 2, self.MU, self.DU, self.TU, self.Isp, ctx=self.ctx)[0]

    def defect_batch_sumsq(self, X_batch, U_batch, t, nsteps):
        """sum(defect.^2) of every trial trajectory X_batch[:, :, b], U_batch[:, :, b]: one batched launch."""
        d, _ = hotpath.direct_defectCalc(X_batch, U_batch, t, nsteps, self.MU, self.DU, self.TU, self.Isp, ctx=self.ctx)
        return np.sum(d * d, axis=(0, 1))


    def jacobian(self, X, U, t, nsteps):
        """(Jac_temp [nstate x nvar x (n-1)], defect): the blocks d defect_i / d [x_i; x_{i+1}; u_i; u_{i+1}] (:111-143)."""
        Jt, _, d, _ = hotpath.direct_jacobian_blocks(X, U, t, nsteps, self.MU, self.DU, self.TU, self.Isp, ctx=self.ctx)
        return Jt, d

    def jacobian_tf(self, X, U, t, nsteps):
        """(Jac_temp, dtf, defect): the blocks and the tf column d defect_i / d tf (:503-516, exact on the device)."""
        Jt, dtf, d, _ = hotpath.direct_jacobian_blocks(X, U, t, nsteps, self.MU, self.DU, self.TU, self.Isp, ctx=self.ctx)
        return Jt, dtf, d


def _natural_spline(x, Y, xq):
    """Natural cubic spline through (x, Y[:, j]) (second derivative 0 at both ends), evaluated at xq: one column per row of Y."""
    x = np.asarray(x, dtype=np.float64)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    n = x.size
    h = np.diff(x)
    # second derivatives M: M_0 = M_{n-1} = 0, h_{i-1} M_{i-1} + 2 (h_{i-1} + h_i) M_i + h_i M_{i+1} = 6 (slope_i - slope_{i-1})
    A = np.zeros((n, n))
    R = np.zeros((n, Y.shape[0]))
    A[0, 0] = A[-1, -1] = 1.0
    slope = np.diff(Y, axis=1) / h
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
        R[i] = 6.0 * (slope[:, i] - slope[:, i - 1])
    M = np.linalg.solve(A, R)
    i = int(np.clip(np.searchsorted(x, xq, side="right") - 1, 0, n - 2))
    a, b = x[i + 1] - xq, xq - x[i]
    return (M[i] * a ** 3 + M[i + 1] * b ** 3) / (6.0 * h[i]) + (Y[:, i] - M[i] * h[i] ** 2 / 6.0) * a / h[i] + \
        (Y[:, i + 1] - M[i + 1] * h[i] ** 2 / 6.0) * b / h[i]


def interpEndStates(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states, MU=None):
    """Interpolated initial and final states (direct.jl:434-461): τ1 and τ2 are wrapped into [0, 1] as the reference does (`while
    τ > 1: τ -= 1`, `while τ < 0: τ += 1`), then each of the six components is interpolated in its orbit table by
    `BSpline(Cubic(Natural()))` on grid.  In Interpolations.jl `Natural` is the `Line` boundary condition: the second derivative
    of the interpolant vanishes at the first and last grid point, i.e. the classical natural cubic spline through the samples
    (the one scipy.interpolate.CubicSpline(bc_type="natural") builds).  Returns (state_0[6], state_f[6])."""
    def wrap(tau):
        tau = float(tau)
        while tau > 1:
            tau -= 1
        while tau < 0:
            tau += 1
        return tau
    s0 = _natural_spline(X0_times, np.asarray(X0_states)[:6], wrap(τ1))
    sf = _natural_spline(Xf_times, np.asarray(Xf_states)[:6], wrap(τ2))
    return s0, sf


def _direct_qp_kkt(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, mass, dV1, dV2, DU, TU, allowImpulsive):
    """The dense KKT solve of direct_qp_dense.  Returns (z, w, c2, (ns, n, nz, iu, iv)): z = (dx node-major, du, the two impulse
    updates, then the multipliers in the order of the constraints: the S linearised defects first)."""
    Jt = np.asarray(Jac_temp, dtype=np.float64)
    d = np.asarray(defect, dtype=np.float64)
    X = np.asarray(X_all, dtype=np.float64)
    U = np.asarray(u_all, dtype=np.float64)
    t = np.asarray(t_TU, dtype=np.float64)
    ns, _, S = Jt.shape
    n = S + 1
    c2 = (DU / TU) ** 2
    nz = ns * n + 3 * n + 6                               # dx (node-major), du, dV1_jump, dV2_jump
    iu, iv = ns * n, ns * n + 3 * n
    dt = np.diff(t)
    w = np.concatenate([dt / 2, [dt[-1] / 2]]) + np.concatenate([[0.0], dt[:-1] / 2, [0.0]])   # :324-326
    Q = np.zeros(nz)
    q = np.zeros(nz)                                      # cost = z'Qz + 2q'z + const
    for k in range(n):
        Q[iu + 3 * k:iu + 3 * k + 3] = w[k]
        q[iu + 3 * k:iu + 3 * k + 3] = w[k] * U[:, k]
    Q[iv:iv + 6] = c2
    q[iv:iv + 3] = c2 * np.asarray(dV1, dtype=np.float64)
    q[iv + 3:iv + 6] = c2 * np.asarray(dV2, dtype=np.float64)
    rows, rhs = [], []
    for i in range(S):                                    # -Jac_full * [X_jump; u_jump] = defect   (:337)
        A = np.zeros((ns, nz))
        A[:, ns * i:ns * i + 2 * ns] = Jt[:, :2 * ns, i]
        A[:, iu + 3 * i:iu + 3 * i + 6] = Jt[:, 2 * ns:, i]
        rows.append(A)
        rhs.append(-d[:, i])
    for k, s, dv, o in ((0, state_0, dV1, 0), (n - 1, state_f, dV2, 3)):    # hard-fixed end points (:370-375)
        A = np.zeros((6, nz))
        A[:, ns * k:ns * k + 6] = np.eye(6)
        A[3:, iv + o:iv + o + 3] = np.eye(3)
        rows.append(A)
        rhs.append(np.asarray(s, dtype=np.float64) - X[:6, k] - np.r_[0.0, 0.0, 0.0, np.asarray(dv, dtype=np.float64)])
    if ns == 7:                                           # initial mass (:269-271)
        A = np.zeros((1, nz))
        A[0, 6] = 1.0
        rows.append(A)
        rhs.append(np.array([mass - X[6, 0]]))
    if not allowImpulsive:                                # dV1_jump = dV2_jump = 0 (:298-302)
        A = np.zeros((6, nz))
        A[:, iv:iv + 6] = np.eye(6)
        rows.append(A)
        rhs.append(np.zeros(6))
    A = np.vstack(rows)
    b = np.concatenate(rhs)
    m = A.shape[0]
    K = np.zeros((nz + m, nz + m))
    K[:nz, :nz] = np.diag(2.0 * Q)
    K[:nz, nz:] = A.T
    K[nz:, :nz] = A
    r = np.concatenate([-2.0 * q, b])
    D = np.ones(nz + m)
    for _ in range(20):                                   # rows mix nondimensional states with controls in N
        Ks = K * D[:, None] * D[None, :]
        D = D / np.sqrt(np.maximum(np.abs(Ks).max(axis=1), 1e-300))
    z = np.linalg.solve(K * D[:, None] * D[None, :], r * D) * D
    return z, w, c2, (ns, n, nz, iu, iv)


def direct_qp_dense(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, mass, dV1, dV2, DU, TU, allowImpulsive=False):
    """optimizeTraj (direct.jl:248-403) for flagEnd = false, beta = 0, tf fixed -- the host restatement of the device QP step: the
    equality-constrained QP's KKT system, assembled densely and solved by LU after symmetric (Ruiz) equilibration.
    Returns (x_update, u_update, dV1_update, dV2_update, cost)."""
    z, w, c2, (ns, n, nz, iu, iv) = _direct_qp_kkt(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, mass, dV1, dV2, DU, TU,
                                                    allowImpulsive)
    U = np.asarray(u_all, dtype=np.float64)
    x_update = z[:ns * n].reshape(n, ns).T
    u_update = z[iu:iv].reshape(n, 3).T
    dV1_u, dV2_u = (z[iv:iv + 3], z[iv + 3:iv + 6]) if allowImpulsive else (np.zeros(3), np.zeros(3))   # exact zeros when pinned
    cost = float(np.sum(w[None, :] * (U + u_update) ** 2) + c2 * (np.sum((dV1 + dV1_u) ** 2) + np.sum((dV2 + dV2_u) ** 2)))
    return x_update, u_update, dV1_u, dV2_u, cost


def costates_from_multipliers(Jac_temp, mult):
    """The node costates of the transcription from the multipliers l_i of its defects, with E_i = d defect_i / d x_i
    and F_i = d defect_i / d x_{i+1}: Lambda_k = E_k' l_k for k < n - 1, Lambda_{n-1} = -F_{n-2}' l_{n-2}.  Returns (Lambda [ns x n],
    kkt_res): the largest |E_k' l_k + F_{k-1}' l_{k-1}| over the interior nodes (the QP's stationarity in dx_k) divided by the
    largest |Lambda|, 0 without an interior node."""
    Jt = np.asarray(Jac_temp, dtype=np.float64)
    l = np.asarray(mult, dtype=np.float64)
    ns, _, S = Jt.shape
    El = np.einsum("rci,ri->ci", Jt[:, :ns, :], l)
    Fl = np.einsum("rci,ri->ci", Jt[:, ns:2 * ns, :], l)
    Lam = np.concatenate([El, -Fl[:, -1:]], axis=1)
    res = float(np.abs(El[:, 1:] + Fl[:, :-1]).max()) if S > 1 else 0.0
    return Lam, (res / float(np.abs(Lam).max()) if res > 0.0 else 0.0)


def direct_costates_dense(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, mass, dV1, dV2, DU, TU, allowImpulsive=False):
    """The host mirror of lto_direct_costates: the multipliers of the defect constraints read out of direct_qp_dense's KKT solve
    (grad cost + A' l = 0, the sign of kernels_direct_qp.hip) and the costates from them.  Returns (Lambda [ns x n], mult [ns x
    (n-1)], kkt_res)."""
    z, _, _, (ns, n, nz, _, _) = _direct_qp_kkt(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, mass, dV1, dV2, DU, TU,
                                                allowImpulsive)
    mult = z[nz:nz + ns * (n - 1)].reshape(n - 1, ns).T
    Lam, res = costates_from_multipliers(Jac_temp, mult)
    return Lam, mult, res


def costates_from_direct(X_all, u_all, t_TU, nsteps, mass, Isp, MU, DU, TU, state_0=None, state_f=None, dV1=None, dV2=None,
                         allowImpulsive=False, ops=None, ctx=None):
    """XC_all [12 x n (x B)] = (X; c^2 Lambda), the indirect method's node vector for p = 2 from direct solutions X_all [6 x n (x
    B)], u_all (N), t_TU [n] or [n x B]: the costates are the multipliers of a frozen QP step at the given point, c =
    hotpath.costate_scale(DU, TU).  The end targets default to the solutions' own end states (a converged frozen-end
    solution sits on them; plus the impulses, which default to zero).  ops=None: lto_direct_costates_batch on the device; an injected `ops`
    (`jacobian`, e.g. HipDirectOps or a CPU back end) runs the host mirror direct_costates_dense trajectory by trajectory.  The
    record of the call is kept in `costates_from_direct.last` = {"Lambda", "mult", "kkt_res", "status"}."""
    X = np.asarray(X_all, dtype=np.float64)
    U = np.asarray(u_all, dtype=np.float64)
    if X.shape[0] != 6:
        raise NotImplementedError("costates_from_direct hands over to the 12-row system; the 14-row hand-over is not built")
    batched = X.ndim == 3
    X3, U3 = (X, U) if batched else (X[..., None], U[..., None])
    B = X3.shape[2]
    T = np.asarray(t_TU, dtype=np.float64)
    per = lambda v, k: np.zeros((k, B)) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(k, -1), (k, B))  # noqa: E731
    d1, d2 = per(dV1, 3).T, per(dV2, 3).T
    s0 = [X3[:6, 0, b] + np.r_[0.0, 0.0, 0.0, d1[b]] for b in range(B)] if state_0 is None else per(state_0, 6).T
    sf = [X3[:6, -1, b] + np.r_[0.0, 0.0, 0.0, d2[b]] for b in range(B)] if state_f is None else per(state_f, 6).T
    if ops is None:
        tg = [hotpath.direct_targets(s0[b], sf[b], mass, d1[b], d2[b]) for b in range(B)]
        Lam, mult, XC, res, status = hotpath.direct_costates(X3, U3, T, nsteps, MU, DU, TU, Isp, tg, allowImpulsive, True, ctx=ctx)
    else:
        c = hotpath.costate_scale(DU, TU)
        Lam, mult = np.zeros_like(X3), np.zeros((6, X3.shape[1] - 1, B))
        res, status = np.zeros(B), np.zeros(B, dtype=np.int32)
        for b in range(B):
            t = T if T.ndim == 1 else T[:, b]
            Jt, d = ops.jacobian(X3[..., b], U3[..., b], t, nsteps)
            try:
                Lam[..., b], mult[..., b], res[b] = direct_costates_dense(Jt, d, X3[..., b], U3[..., b], t, s0[b], sf[b], mass, d1[b],
                                                                          d2[b], DU, TU, allowImpulsive)
            except np.linalg.LinAlgError:
                Lam[..., b], mult[..., b], res[b], status[b] = np.nan, np.nan, np.nan, 1
        XC = np.concatenate([X3, (c * c) * Lam], axis=0)
    costates_from_direct.last = {"Lambda": Lam if batched else Lam[..., 0], "mult": mult if batched else mult[..., 0],
                                 "kkt_res": res if batched else float(res[0]), "status": status if batched else int(status[0])}
    return np.asfortranarray(XC if batched else XC[..., 0])


def direct_to_indirect(X_all, u_all, t_TU, nsteps, mass, Isp, MU, DU, TU, thrustLimit=10.0, maxIter=50, state_0=None, state_f=None,
                       dV1=None, dV2=None, allowImpulsive=False, integ=None, ctx=None):
    """The hand-over of the reference's workflow ("converge the direct method, then the indirect one") for a batch of converged
    minimum-energy direct solutions X_all [6 x n x B] (or one, [6 x n]): the costate seed from the QP multipliers
    (costates_from_direct), then lto_indirect_solve_batch with p = 2, full Newton from the first iteration -- no random costates
    and no adjoints-only phase.  Returns a dict of per-trajectory results: XC [12 x n x B], defect, max_defect [B], status [B]
    (0 converged to 1e-10, 1 maxIter, 2 NaN; 3 = no seed: the costates' KKT system was singular), iterations [B], seed [12 x n x B],
    kkt_res [B]."""
    X = np.asarray(X_all, dtype=np.float64)
    batched = X.ndim == 3
    X3 = X if batched else X[..., None]
    U3 = np.asarray(u_all, dtype=np.float64).reshape(3, X3.shape[1], -1)
    seed = costates_from_direct(X3, U3, t_TU, nsteps, mass, Isp, MU, DU, TU, state_0, state_f, dV1, dV2, allowImpulsive, ctx=ctx)
    rec = costates_from_direct.last
    B = X3.shape[2]
    ok = np.flatnonzero(np.asarray(rec["status"]) == 0)
    out = {"XC": np.full(seed.shape, np.nan, order="F"), "defect": np.full((12, X3.shape[1] - 1, B), np.nan, order="F"),
           "max_defect": np.full(B, np.nan), "status": np.full(B, 3, dtype=np.int32), "iterations": np.zeros(B, dtype=np.int32),
           "seed": seed, "kkt_res": np.asarray(rec["kkt_res"])}
    if ok.size:
        T = np.asarray(t_TU, dtype=np.float64)
        prm = hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, 2.0, 1.0)
        XC, d, status, iters, _ = hotpath.indirect_solve_batch(seed[..., ok], T if T.ndim == 1 else T[:, ok], prm, integ, False, maxIter,
                                                               ctx=ctx)
        out["XC"][..., ok], out["defect"][..., ok] = XC, d
        out["max_defect"][ok] = np.abs(d).max(axis=(0, 1))
        out["status"][ok], out["iterations"][ok] = status, iters
    return out


END_PERT = 0.05          # pert of the end model's finite differences (direct.jl:340)
P_BOUND = 0.1            # |p1|, |p2| <= 0.1 with flagEnd (direct.jl:280-284)


def end_model(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states):
    """The free-end model of optimizeTraj (direct.jl:339-349) at (τ1, τ2): interpEndStates at τ and τ ± 0.05 (each argument
    wrapped on its own), g = central first difference, c = second difference.  Returns (s0, sf, g0, gf, |c0|, |cf|)."""
    h = END_PERT
    s0, sf = interpEndStates(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states)
    s0p, sfp = interpEndStates(τ1 + h, τ2 + h, X0_times, X0_states, Xf_times, Xf_states)
    s0m, sfm = interpEndStates(τ1 - h, τ2 - h, X0_times, X0_states, Xf_times, Xf_states)
    g0, gf = (s0p - s0m) / (2 * h), (sfp - sfm) / (2 * h)
    c0, cf = (s0p - 2 * s0 + s0m) / h ** 2, (sfp - 2 * sf + sfm) / h ** 2
    return s0, sf, g0, gf, float(np.linalg.norm(c0)), float(np.linalg.norm(cf))


def direct_qp_dense_free(Jac_temp, defect, X_all, u_all, t_TU, state_0, state_f, g0, gf, c0_norm, cf_norm, β, mass, dV1, dV2, DU, TU,
                         allowImpulsive=False):
    """optimizeTraj with flagEnd = true (direct.jl:278-292, :353-369): the host reference of the device's free-end step, by a
    different route.  The phase updates p1, p2 are two more variables of one dense KKT system, the end constraints are
    x_0 + dx_0 + [0; dV1 + d1] = s0 + g0 p1 and x_{n-1} + dx_{n-1} + [0; dV2 + d2] = sf + gf p2, the cost gains
    β (|c0|/2 p1² + |cf|/2 p2²), and the bounds |p| <= 0.1 are handled by enumerating the nine active sets (each p free, at -0.1
    or at +0.1).  An active set is accepted when its free p lie in the box and the multipliers of its active bounds have the right
    sign; the accepted point of smallest cost is returned (ties: smaller max|p|).  Returns (x_update, u_update, dV1_update,
    dV2_update, p1, p2, cost)."""
    Jt = np.asarray(Jac_temp, dtype=np.float64)
    d = np.asarray(defect, dtype=np.float64)
    X = np.asarray(X_all, dtype=np.float64)
    U = np.asarray(u_all, dtype=np.float64)
    t = np.asarray(t_TU, dtype=np.float64)
    dV1 = np.asarray(dV1, dtype=np.float64)
    dV2 = np.asarray(dV2, dtype=np.float64)
    ns, _, S = Jt.shape
    n = S + 1
    c2 = (DU / TU) ** 2
    nz = ns * n + 3 * n + 6 + 2                           # dx (node-major), du, dV1_jump, dV2_jump, p1, p2
    iu, iv, ip = ns * n, ns * n + 3 * n, ns * n + 3 * n + 6
    dt = np.diff(t)
    w = np.concatenate([dt / 2, [dt[-1] / 2]]) + np.concatenate([[0.0], dt[:-1] / 2, [0.0]])
    Q = np.zeros(nz)
    q = np.zeros(nz)                                      # cost = z'Qz + 2q'z + const
    for k in range(n):
        Q[iu + 3 * k:iu + 3 * k + 3] = w[k]
        q[iu + 3 * k:iu + 3 * k + 3] = w[k] * U[:, k]
    Q[iv:iv + 6] = c2
    q[iv:iv + 3] = c2 * dV1
    q[iv + 3:iv + 6] = c2 * dV2
    Q[ip], Q[ip + 1] = β * c0_norm / 2, β * cf_norm / 2
    rows, rhs = [], []
    for i in range(S):
        A = np.zeros((ns, nz))
        A[:, ns * i:ns * i + 2 * ns] = Jt[:, :2 * ns, i]
        A[:, iu + 3 * i:iu + 3 * i + 6] = Jt[:, 2 * ns:, i]
        rows.append(A)
        rhs.append(-d[:, i])
    for k, s, g, dv, o in ((0, state_0, g0, dV1, 0), (n - 1, state_f, gf, dV2, 1)):   # linear end model (:356-357)
        A = np.zeros((6, nz))
        A[:, ns * k:ns * k + 6] = np.eye(6)
        A[3:, iv + 3 * o:iv + 3 * o + 3] = np.eye(3)
        A[:, ip + o] = -np.asarray(g, dtype=np.float64)
        rows.append(A)
        rhs.append(np.asarray(s, dtype=np.float64) - X[:6, k] - np.r_[0.0, 0.0, 0.0, dv])
    if ns == 7:
        A = np.zeros((1, nz))
        A[0, 6] = 1.0
        rows.append(A)
        rhs.append(np.array([mass - X[6, 0]]))
    if not allowImpulsive:
        A = np.zeros((6, nz))
        A[:, iv:iv + 6] = np.eye(6)
        rows.append(A)
        rhs.append(np.zeros(6))
    A0 = np.vstack(rows)
    b0 = np.concatenate(rhs)
    best = None
    for pat in [(a1, a2) for a1 in (0, -1, 1) for a2 in (0, -1, 1)]:      # 0 free, -1 at -0.1, +1 at +0.1
        act = [(j, sgn) for j, sgn in enumerate(pat) if sgn]
        A = A0
        b = b0
        if act:
            Ab = np.zeros((len(act), nz))
            for r, (j, sgn) in enumerate(act):
                Ab[r, ip + j] = 1.0
            A = np.vstack([A0, Ab])
            b = np.concatenate([b0, [sgn * P_BOUND for _, sgn in act]])
        m = A.shape[0]
        K = np.zeros((nz + m, nz + m))
        K[:nz, :nz] = np.diag(2.0 * Q)
        K[:nz, nz:] = A.T
        K[nz:, :nz] = A
        r = np.concatenate([-2.0 * q, b])
        D = np.ones(nz + m)
        with np.errstate(all="ignore"):
            for _ in range(20):
                Ks = K * D[:, None] * D[None, :]
                D = D / np.sqrt(np.maximum(np.abs(Ks).max(axis=1), 1e-300))
        try:
            sol = np.linalg.solve(K * D[:, None] * D[None, :], r * D) * D
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(sol)):                  # singular for this active set (e.g. beta = 0 and g = 0: p undetermined)
            continue
        z, lam = sol[:nz], sol[nz:]
        p = z[ip:ip + 2]
        if any(sgn == 0 and abs(p[j]) > P_BOUND * (1 + 1e-12) for j, sgn in enumerate(pat)):
            continue                                      # a free p outside the box
        lam_b = lam[A0.shape[0]:]                         # row p_j = ±0.1: grad f + lam e_j = 0, lam >= 0 at +0.1, <= 0 at -0.1
        scale = 1e-9 * max(1.0, float(np.abs(2.0 * Q * z + 2.0 * q).max()))
        if any(sgn * lb < -scale for (j, sgn), lb in zip(act, lam_b)):
            continue
        p = np.array([sgn * P_BOUND if sgn else p[j] for j, sgn in enumerate(pat)])   # exact bounds
        dx = z[:ns * n].reshape(n, ns).T
        du = z[iu:iv].reshape(n, 3).T
        d1, d2 = (z[iv:iv + 3], z[iv + 3:iv + 6]) if allowImpulsive else (np.zeros(3), np.zeros(3))
        cost = float(np.sum(w[None, :] * (U + du) ** 2) + c2 * (np.sum((dV1 + d1) ** 2) + np.sum((dV2 + d2) ** 2)) +
                     β * (c0_norm / 2 * p[0] ** 2 + cf_norm / 2 * p[1] ** 2))
        key = (cost, float(np.abs(p).max()))
        if best is None or key < best[0]:
            best = (key, (dx, du, d1, d2, float(p[0]), float(p[1]), cost))
    if best is None:
        raise np.linalg.LinAlgError("direct_qp_dense_free: no active set satisfies the optimality conditions")
    return best[1]


TF_STEP_DAYS = 1.0       # |tf_jump| <= 1 day per free iteration (direct.jl:288)
TF_MAX_DAYS = 40.0       # tf <= 40 days (direct.jl:294)


def tf_bounds_default(t0, TU, step_days=TF_STEP_DAYS):
    """(step, tf_min, tf_max) in TU: the reference's 1-day step and 40-day ceiling (direct.jl:288-295); its floor tf >= 0 would let
    the grid collapse onto t0, so tf_min is one day past t0."""
    return (step_days * day / TU, t0 + day / TU, TF_MAX_DAYS * day / TU)


def direct_qp_dense_free_tf(Jac_temp, dtf, defect, X_all, u_all, t_TU, state_0, state_f, g0, gf, c0_norm, cf_norm, β, mass, dV1, dV2,
                            DU, TU, tf, tf_bounds, allowImpulsive=False):
    """optimizeTraj with flagEnd = true and a free time of flight (direct.jl:278-295, :337, :353-369): the host reference of the
    device's free-tf step, by a different route.  p1, p2 and p3 = tf_jump are three more variables of one dense KKT system; the
    defect rows read Jac_i [dx_i; dx_{i+1}; du_i; du_{i+1}] + dtf_i p3 = -defect_i; tf_bounds = (step, tf_min, tf_max) bound p3 to
    [max(-step, tf_min - tf), min(step, tf_max - tf)] and |p1|, |p2| <= 0.1.  The 27 active sets (each p free, at its lower or at
    its upper bound) are enumerated; a set is accepted when its free p lie in their bounds and the multipliers of its active bounds
    have the right sign, and the accepted point of smallest cost is returned (ties: the smaller max(|p1|/0.1, |p2|/0.1, |p3|/step)).
    Returns (x_update, u_update, dV1_update, dV2_update, p1, p2, p3, cost)."""
    Jt = np.asarray(Jac_temp, dtype=np.float64)
    dtf = np.asarray(dtf, dtype=np.float64)
    d = np.asarray(defect, dtype=np.float64)
    X = np.asarray(X_all, dtype=np.float64)
    U = np.asarray(u_all, dtype=np.float64)
    t = np.asarray(t_TU, dtype=np.float64)
    dV1 = np.asarray(dV1, dtype=np.float64)
    dV2 = np.asarray(dV2, dtype=np.float64)
    step, tf_min, tf_max = (float(v) for v in tf_bounds)
    lo = np.array([-P_BOUND, -P_BOUND, max(-step, tf_min - tf)])
    hi = np.array([P_BOUND, P_BOUND, min(step, tf_max - tf)])
    ns, _, S = Jt.shape
    n = S + 1
    c2 = (DU / TU) ** 2
    nz = ns * n + 3 * n + 6 + 3                           # dx (node-major), du, dV1_jump, dV2_jump, p1, p2, p3
    iu, iv, ip = ns * n, ns * n + 3 * n, ns * n + 3 * n + 6
    dt = np.diff(t)
    w = np.concatenate([dt / 2, [dt[-1] / 2]]) + np.concatenate([[0.0], dt[:-1] / 2, [0.0]])
    Q = np.zeros(nz)
    q = np.zeros(nz)                                      # cost = z'Qz + 2q'z + const
    for k in range(n):
        Q[iu + 3 * k:iu + 3 * k + 3] = w[k]
        q[iu + 3 * k:iu + 3 * k + 3] = w[k] * U[:, k]
    Q[iv:iv + 6] = c2
    q[iv:iv + 3] = c2 * dV1
    q[iv + 3:iv + 6] = c2 * dV2
    Q[ip], Q[ip + 1] = β * c0_norm / 2, β * cf_norm / 2
    rows, rhs = [], []
    for i in range(S):                                    # -Jac_full * [X_jump; u_jump; tf_jump] = defect (:337, :516)
        A = np.zeros((ns, nz))
        A[:, ns * i:ns * i + 2 * ns] = Jt[:, :2 * ns, i]
        A[:, iu + 3 * i:iu + 3 * i + 6] = Jt[:, 2 * ns:, i]
        A[:, ip + 2] = dtf[:, i]
        rows.append(A)
        rhs.append(-d[:, i])
    for k, s, g, dv, o in ((0, state_0, g0, dV1, 0), (n - 1, state_f, gf, dV2, 1)):
        A = np.zeros((6, nz))
        A[:, ns * k:ns * k + 6] = np.eye(6)
        A[3:, iv + 3 * o:iv + 3 * o + 3] = np.eye(3)
        A[:, ip + o] = -np.asarray(g, dtype=np.float64)
        rows.append(A)
        rhs.append(np.asarray(s, dtype=np.float64) - X[:6, k] - np.r_[0.0, 0.0, 0.0, dv])
    if ns == 7:
        A = np.zeros((1, nz))
        A[0, 6] = 1.0
        rows.append(A)
        rhs.append(np.array([mass - X[6, 0]]))
    if not allowImpulsive:
        A = np.zeros((6, nz))
        A[:, iv:iv + 6] = np.eye(6)
        rows.append(A)
        rhs.append(np.zeros(6))
    A0 = np.vstack(rows)
    b0 = np.concatenate(rhs)
    scale_p = np.array([1 / P_BOUND, 1 / P_BOUND, 1 / step if step > 0 else 0.0])
    best = None
    for pat in [(a1, a2, a3) for a1 in (0, -1, 1) for a2 in (0, -1, 1) for a3 in (0, -1, 1)]:   # 0 free, -1 at lo, +1 at hi
        act = [(j, sgn) for j, sgn in enumerate(pat) if sgn]
        A, b = A0, b0
        if act:
            Ab = np.zeros((len(act), nz))
            for r, (j, sgn) in enumerate(act):
                Ab[r, ip + j] = 1.0
            A = np.vstack([A0, Ab])
            b = np.concatenate([b0, [lo[j] if sgn < 0 else hi[j] for j, sgn in act]])
        m = A.shape[0]
        K = np.zeros((nz + m, nz + m))
        K[:nz, :nz] = np.diag(2.0 * Q)
        K[:nz, nz:] = A.T
        K[nz:, :nz] = A
        r = np.concatenate([-2.0 * q, b])
        D = np.ones(nz + m)
        with np.errstate(all="ignore"):
            for _ in range(20):
                Ks = K * D[:, None] * D[None, :]
                D = D / np.sqrt(np.maximum(np.abs(Ks).max(axis=1), 1e-300))
        try:
            sol = np.linalg.solve(K * D[:, None] * D[None, :], r * D) * D
        except np.linalg.LinAlgError:
            continue
        if not np.all(np.isfinite(sol)):                  # singular for this active set (p undetermined)
            continue
        z, lam = sol[:nz], sol[nz:]
        p = z[ip:ip + 3]
        tol = 1e-12 * np.maximum(hi - lo, 1e-300)
        if any(sgn == 0 and (p[j] < lo[j] - tol[j] or p[j] > hi[j] + tol[j]) for j, sgn in enumerate(pat)):
            continue                                      # a free p outside its bounds
        lam_b = lam[A0.shape[0]:]                         # row p_j = bound: lam >= 0 at the upper bound, <= 0 at the lower one
        scale = 1e-9 * max(1.0, float(np.abs(2.0 * Q * z + 2.0 * q).max()))
        if any(sgn * lb < -scale for (j, sgn), lb in zip(act, lam_b)):
            continue
        p = np.array([(lo[j] if sgn < 0 else hi[j]) if sgn else min(max(p[j], lo[j]), hi[j]) for j, sgn in enumerate(pat)])
        dx = z[:ns * n].reshape(n, ns).T
        du = z[iu:iv].reshape(n, 3).T
        d1, d2 = (z[iv:iv + 3], z[iv + 3:iv + 6]) if allowImpulsive else (np.zeros(3), np.zeros(3))
        cost = float(np.sum(w[None, :] * (U + du) ** 2) + c2 * (np.sum((dV1 + d1) ** 2) + np.sum((dV2 + d2) ** 2)) +
                     β * (c0_norm / 2 * p[0] ** 2 + cf_norm / 2 * p[1] ** 2))
        key = (cost, float(np.max(np.abs(p) * scale_p)))
        if best is None or key < best[0]:
            best = (key, (dx, du, d1, d2, float(p[0]), float(p[1]), float(p[2]), cost))
    if best is None:
        raise np.linalg.LinAlgError("direct_qp_dense_free_tf: no active set satisfies the optimality conditions")
    return best[1]


def multiShoot_CRTBP_direct(X_all, u_all, τ1, τ2, t_TU, dV1, dV2, MU, DU, TU, n_nodes, nsteps, mass, Isp, X0_times, X0_states,
                            Xf_times, Xf_states, plot_yn, flagEnd, β, allowImpulsive, maxIter, ops=None, verbose=True, *, tf_step=0.0,
                            tf_bounds=None):
    """Direct multiple shooting with frozen end points (direct.jl:58-594).  Returns the reference's tuple
    (X_all, u_all, τ1, τ2, t_TU, dV1, dV2, defect).

    ops=None: the whole loop is ONE library call (lto_direct_solve: Jacobian sweep, QP step, batched line search and update on
    the device); with flagEnd = true it is lto_direct_solve_free (free end points on odd iterations, τ1 and τ2 updated and
    returned).  An injected `ops` (defect / jacobian / defect_batch_sumsq, e.g. HipDirectOps or a CPU back end) runs this
    Python mirror of the loop (direct_loop_host) with the QP solved on the host (direct_qp_dense).  The status of the last call
    is kept in `multiShoot_CRTBP_direct.last` = {"status", "iterations", "history"} (0 converged, 1 maxIter, 2 NaN, 3 singular
    KKT system; history rows: max|defect|, cost, alpha (, τ1, τ2 with flagEnd)) -- the reference prints its progress and returns
    no flag.  flagEnd = true with an injected `ops` raises NotImplementedError: only the device path covers it (the mirror loop
    with free ends is direct_loop_host).

    tf_step (TU, keyword): 0 pins tf, as the reference does (`d = 0.`, :292).  With flagEnd and tf_step > 0 the time of flight is a
    variable of the free iterations too (lto_direct_solve_free_tf): |tf_jump| <= tf_step per iteration, tf in tf_bounds = (tf_min,
    tf_max) (default: one day past t0, 40 days), and the returned t_TU is the final grid; the history gains the row tf."""
    if flagEnd and ops is not None:
        raise NotImplementedError("multiShoot_CRTBP_direct: flagEnd = true runs on the device only (ops=None); the host mirror of "
                                  "the free-end loop is drivers.direct_loop_host")
    del plot_yn                                           # no plotting
    X = np.array(X_all, dtype=np.float64, order="F")
    U = np.array(u_all, dtype=np.float64, order="F")
    t = np.array(t_TU, dtype=np.float64)
    dV1 = np.array(dV1, dtype=np.float64).reshape(3)
    dV2 = np.array(dV2, dtype=np.float64).reshape(3)
    assert X.shape[1] == n_nodes
    state_0, state_f = interpEndStates(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states, MU)
    maxIter = int(maxIter)
    if ops is None:
        tg = hotpath.direct_targets(state_0, state_f, mass, dV1, dV2)
        orbits = hotpath.DirectOrbits(X0_times, X0_states, Xf_times, Xf_states)
        if flagEnd and tf_step > 0:
            _, tf_min, tf_max = tf_bounds_default(t[0], TU)
            if tf_bounds is not None:
                tf_min, tf_max = tf_bounds
            tb = hotpath.direct_tf_bounds(tf_step, tf_min, tf_max)
            X, U, dV, t, defect, tau, status, iters, hist = hotpath.direct_solve_free_tf(
                X, U, t, nsteps, MU, DU, TU, Isp, orbits, tg, [τ1, τ2], β, tb, True, allowImpulsive, maxIter)
            line = lambda k: "Iter %d. Max defect = %.2e. Cost = %.5f. tf = %.2f days. alpha = %.3f." % (
                k + 1, hist[0, k], hist[1, k], hist[5, k] * TU / day, hist[2, k])
        elif flagEnd:
            X, U, dV, t, defect, tau, status, iters, hist = hotpath.direct_solve_free(
                X, U, t, nsteps, MU, DU, TU, Isp, orbits, tg, [τ1, τ2], β, True, allowImpulsive, maxIter)
            line = lambda k: "Iter %d. Max defect = %.2e. Cost = %.5f. alpha = %.3f. tau1 = %.6f, tau2 = %.6f." % (k + 1, *hist[:, k])
        else:
            X, U, dV, t, defect, status, iters, hist = hotpath.direct_solve(X, U, t, nsteps, MU, DU, TU, Isp, tg, allowImpulsive, maxIter)
            line = lambda k: "Iter %d. Max defect = %.2e. Cost = %.5f. alpha = %.3f." % (k + 1, hist[0, k], hist[1, k], hist[2, k])
        if verbose:
            for k in range(iters):
                print(line(k))
        multiShoot_CRTBP_direct.last = {"status": status, "iterations": iters, "history": hist}
        τ1, τ2 = (float(tau[0]), float(tau[1])) if flagEnd else (τ1, τ2)
        return X, U, τ1, τ2, t, dV[:3].copy(), dV[3:].copy(), defect
    out, last = direct_loop_host(X, U, τ1, τ2, t, dV1, dV2, MU, DU, TU, n_nodes, nsteps, mass, Isp, X0_times, X0_states, Xf_times,
                                 Xf_states, False, β, allowImpulsive, maxIter, ops, verbose)
    last["history"] = last["history"][:3]
    multiShoot_CRTBP_direct.last = last
    return out


def stacked_guess(n_nodes, tof1, tof2, τ1, X0_times, X0_states, Xf_times, Xf_states, MU, ctx=None):
    """The trajectory-stacking initial guess of the reference demos (CRTBP_Multishoot_direct_demo.jl:116-157) as one function and
    one library call (lto_stack_guess_batch): tof1 TU ballistically on the departure orbit from phase τ1, the closest
    point of the arrival orbit, tof2 TU ballistically from there, n_nodes samples over LinRange(0, tof1 + tof2, n_nodes), the last
    one snapped onto the arrival orbit.  Returns (X_all [6 x n_nodes], t_TU, τ1 (wrapped into [0, 1]), τ2 (the phase of the last
    node)).  The full record of the call is kept in `stacked_guess.last` (hotpath.StackGuess)."""
    g = hotpath.stack_guess(float(τ1), float(tof1), float(tof2), n_nodes, (X0_times, X0_states, Xf_times, Xf_states), MU=MU, ctx=ctx)
    stacked_guess.last = g
    return g.X, g.t, g.tau1, g.tau2


def multiStart_direct(τ1s, tof1s, tof2s, n_nodes, nsteps, mass, Isp, X0_times, X0_states, Xf_times, Xf_states, MU, DU, TU,
                      flagEnd=False, β=0.0, allowImpulsive=False, maxIter=100, ctx=None, then_indirect=False, thrustLimit=10.0,
                      maxIter_indirect=50, remesh_nodes=None, remesh_tol_max=1e-16, remesh_w_floor=None):
    """A multi-start search of the direct method in three library calls: the stacked guesses of all starts (τ1s, tof1s, tof2s:
    scalars or arrays, broadcast to B starts; hotpath.stack_guess), their end targets at (τ1, τ2) (hotpath.direct_end_states) and
    the loop of multiShoot_CRTBP_direct for all of them side by side on their own grids, zero thrust as the guess
    (hotpath.direct_solve_free).  Returns a dict of per-start arrays: status [B], iterations [B], max_defect [B], cost [B] (of the
    last iteration; NaN where none ran), tau [2 x B] (final τ1; τ2), tau_guess [3 x B] (τ1; τ2 at the junction; τ2 at the end),
    gap [2 x B], guess_status [B], X [6 x n x B], U [3 x n x B], t [n x B], dV [6 x B], defect, history [5 x maxIter x B], and
    order: the indices of the status-0 starts by increasing cost.
    then_indirect: the converged starts are handed to the indirect method (direct_to_indirect: costates from the QP multipliers,
    p = 2 at thrustLimit N, at most maxIter_indirect iterations); the dict gains "indirect" = direct_to_indirect's dict for those
    starts, in the order of "indirect_starts" (their indices, increasing).
    remesh_nodes (None: nothing of this runs): the converged starts are refined side by side (hotpath.direct_refine: nodes removed
    below remesh_tol_max / 1000, segments bisected above remesh_tol_max, at most 4 n_nodes nodes), resampled onto remesh_nodes nodes
    each (meshEquidistribute_direct, two passes, remesh_w_floor or its default) and solved again with fixed ends at their final
    phases by one hotpath.direct_solve batch.  The dict gains "remesh_starts" (their indices) and "remesh" = a dict of X, U, t,
    dV, status, iterations, max_defect, nodes_refined, resample_status and errors [(remesh_nodes-1) x starts] (the estimates of the
    re-solved meshes), or None without a converged start; then_indirect then starts from the re-solved starts of status 0."""
    orbits = hotpath.DirectOrbits(X0_times, X0_states, Xf_times, Xf_states)
    τ1s, tof1s, tof2s = (np.ascontiguousarray(v) for v in np.broadcast_arrays(
        *(np.asarray(v, dtype=np.float64).reshape(-1) for v in (τ1s, tof1s, tof2s))))
    g = hotpath.stack_guess(τ1s, tof1s, tof2s, n_nodes, orbits, MU=MU, ctx=ctx)
    B = g.status.size
    tau = np.asfortranarray(np.vstack([g.tau1, g.tau2]))
    s0, sf, _, _, _, _ = hotpath.direct_end_states(tau, orbits, ctx=ctx)
    targets = [hotpath.direct_targets(s0[:, b], sf[:, b], mass, np.zeros(3), np.zeros(3)) for b in range(B)]
    U0 = np.zeros((3, int(n_nodes), B), order="F")
    X, U, dV, t, defect, tau_out, status, iters, hist = hotpath.direct_solve_free(
        g.X, U0, g.t, nsteps, MU, DU, TU, Isp, orbits, targets, tau, β, flagEnd, allowImpulsive, maxIter, ctx=ctx)
    last = np.minimum(iters, hist.shape[1])               # a start that reached maxIter reports a count past it
    cost = np.array([hist[1, last[b] - 1, b] if last[b] > 0 else np.nan for b in range(B)])
    ok = np.flatnonzero(status == 0)
    order = ok[np.argsort(cost[ok], kind="stable")]
    out = {"status": status, "iterations": iters, "max_defect": np.abs(defect).max(axis=(0, 1)), "cost": cost, "tau": tau_out,
           "tau_guess": np.vstack([g.tau1, g.tau2_0, g.tau2]), "gap": g.gap, "guess_status": g.status, "X": X, "U": U, "t": t,
           "dV": dV, "defect": defect, "history": hist, "order": order}
    if remesh_nodes is not None:
        out["remesh_starts"] = ok
        out["remesh"] = None
        if ok.size:
            parts = hotpath.direct_refine(X[..., ok], U[..., ok], t[:, ok], nsteps, MU, DU, TU, Isp, remesh_tol_max / 1000.0,
                                          remesh_tol_max, 4 * int(n_nodes), ctx=ctx)
            kw = {} if remesh_w_floor is None else {"w_floor": remesh_w_floor}
            Xr, Ur, tr, rs = meshEquidistribute_direct(parts, None, None, 6, None, nsteps, Isp, MU, DU, TU, int(remesh_nodes), ctx=ctx, **kw)
            s0, sf, _, _, _, _ = hotpath.direct_end_states(np.asfortranarray(tau_out[:, ok]), orbits, ctx=ctx)
            targets = [hotpath.direct_targets(s0[:, j], sf[:, j], mass, dV[:3, b], dV[3:, b]) for j, b in enumerate(ok)]
            X2, U2, dV2, t2, d2, st2, it2, _ = hotpath.direct_solve(Xr, Ur, tr, nsteps, MU, DU, TU, Isp, targets, allowImpulsive,
                                                                    maxIter, ctx=ctx)
            _, e2 = hotpath.direct_defectCalc(X2, U2, t2, nsteps, MU, DU, TU, Isp, ctx=ctx)
            out["remesh"] = {"X": X2, "U": U2, "t": t2, "dV": dV2, "status": st2, "iterations": it2,
                             "max_defect": np.abs(d2).max(axis=(0, 1)), "nodes_refined": np.array([p.n for p in parts]),
                             "resample_status": rs, "errors": e2}
            keep = np.flatnonzero(st2 == 0)
            ok, X, U, t, dV = ok[keep], X2[..., keep], U2[..., keep], t2[:, keep], dV2[:, keep]
    if then_indirect:
        out["indirect_starts"] = ok
        out["indirect"] = None
        if ok.size:
            # the end targets of the frozen step are the states the direct loop ended on (with flagEnd: at the final phases)
            sel = ok if remesh_nodes is None else slice(None)     # (after a re-mesh X, U, t, dV hold the re-solved starts alone)
            out["indirect"] = direct_to_indirect(X[..., sel], U[..., sel], t[:, sel], nsteps, mass, Isp, MU, DU, TU, thrustLimit,
                                                 maxIter_indirect, dV1=dV[:3, sel], dV2=dV[3:, sel], allowImpulsive=allowImpulsive,
                                                 ctx=ctx)
    return out


W_FLOOR_DIRECT = 0.1      # meshEquidistribute_direct's default floor of the monitor


def meshEquidistribute_direct(X, U, t, nstate, n_in, nsteps, Isp, MU, DU, TU, n_new, passes=2, w_floor=W_FLOOR_DIRECT, ctx=None):
    """Direct solutions moved onto n_new nodes each whose RKF7(8) estimates are equidistributed (hotpath.direct_resample, one
    library call; the reference's meshRefine_direct only bisects and deletes).  One trajectory X [nstate x n], U
    [3 x n], t [n] or a batch with a trailing axis; n_in = the valid columns per trajectory as lto_direct_refine_batch leaves them
    (None: all).  X may be what hotpath.direct_refine returned (then U, t and n_in are None).  No new segment is longer than
    1 / w_floor times the finest in monitor measure.  The result is a guess for the solve calls, not a solution.  Returns (X, U, t,
    status); the full record of the call is kept in `meshEquidistribute_direct.last` (hotpath.DirectResample)."""
    first = X[0] if isinstance(X, (list, tuple)) and len(X) and isinstance(X[0], hotpath.DirectRefine) else X
    rows = np.shape(first.X if isinstance(first, hotpath.DirectRefine) else first)[0]
    if rows != nstate:
        raise ValueError("meshEquidistribute_direct: X has %d rows, nstate is %d" % (rows, nstate))
    r = hotpath.direct_resample(X, U, t, nsteps, MU, DU, TU, Isp, n_new, n_in=n_in, w_floor=w_floor, passes=passes, ctx=ctx)
    meshEquidistribute_direct.last = r
    return r.X, r.U, r.t, r.status


def direct_loop_host(X_all, u_all, τ1, τ2, t_TU, dV1, dV2, MU, DU, TU, n_nodes, nsteps, mass, Isp, X0_times, X0_states, Xf_times,
                     Xf_states, flagEnd, β, allowImpulsive, maxIter, ops, verbose=True, *, tf_bounds=None):
    """The Python mirror of the multiShoot_CRTBP_direct loop (direct.jl:477-594) on an injected `ops` back end, the QP solved on
    the host: direct_qp_dense, or with flagEnd on odd iterations direct_qp_dense_free at the end model of the current τ
    (:521-526), followed by τ += alpha p (:564-565).  Returns ((X_all, u_all, τ1, τ2, t_TU, dV1, dV2, defect),
    {"status", "iterations", "history"}) with history rows max|defect|, cost, alpha, τ1, τ2.

    tf_bounds = (step, tf_min, tf_max) (TU, keyword): None keeps tf pinned, as above.  Otherwise the history gains the row tf, and
    with flagEnd and step > 0 the odd iterations also move tf: `ops.jacobian_tf(X, U, t, nsteps) -> (Jac_temp, dtf, defect)` gives
    the tf column, direct_qp_dense_free_tf the step, and after the line search (on the current grid, :560) τ += alpha (p1, p2),
    tf += alpha p3 (kept in [tf_min, tf_max]) and t = t0 + (τ_grid + 1) / 2 (tf - t0) (:567, :582)."""
    X = np.array(X_all, dtype=np.float64, order="F")
    U = np.array(u_all, dtype=np.float64, order="F")
    t = np.array(t_TU, dtype=np.float64)
    dV1 = np.array(dV1, dtype=np.float64).reshape(3)
    dV2 = np.array(dV2, dtype=np.float64).reshape(3)
    nstate = X.shape[0]
    assert X.shape[1] == n_nodes
    maxIter = int(maxIter)
    t0, tf = t[0], t[-1]
    tau = (t - t0) / (tf - t0) * 2 - 1                   # :480
    t_fixed = t0 + (tau + 1) / 2 * (tf - t0)              # t_TU_fixed (:321) = t after the first update (:582)
    move_tf = tf_bounds is not None and flagEnd and float(tf_bounds[0]) > 0
    defect, _ = ops.defect(X, U, t, nsteps)               # :485
    hist = np.full((5 if tf_bounds is None else 6, max(maxIter, 1)), np.nan)
    it, er, status = 0, 1.0, 0                            # er = 1.0: at least one step (:488)
    while er > 1e-6:                                      # :491 (NaN leaves the loop)
        it += 1
        if it > maxIter:
            it, status = maxIter, 1
            break
        p1 = p2 = p3 = 0.0
        if move_tf and it % 2 == 1:                       # free ends and free tf (:503-516, :523-526)
            Jt, dtf, _ = ops.jacobian_tf(X, U, t, nsteps)
            s0, sf, g0, gf, c0n, cfn = end_model(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states)
            x_up, u_up, dV1_up, dV2_up, p1, p2, p3, cost = direct_qp_dense_free_tf(
                Jt, dtf, defect, X, U, t_fixed, s0, sf, g0, gf, c0n, cfn, β, mass, dV1, dV2, DU, TU, tf, tf_bounds, allowImpulsive)
        elif flagEnd and it % 2 == 1:                     # free ends on odd iterations (:523-526)
            Jt, _ = ops.jacobian(X, U, t, nsteps)
            s0, sf, g0, gf, c0n, cfn = end_model(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states)
            x_up, u_up, dV1_up, dV2_up, p1, p2, cost = direct_qp_dense_free(Jt, defect, X, U, t_fixed, s0, sf, g0, gf, c0n, cfn, β,
                                                                            mass, dV1, dV2, DU, TU, allowImpulsive)
        else:
            Jt, _ = ops.jacobian(X, U, t, nsteps)
            state_0, state_f = interpEndStates(τ1, τ2, X0_times, X0_states, Xf_times, Xf_states, MU)
            x_up, u_up, dV1_up, dV2_up, cost = direct_qp_dense(Jt, defect, X, U, t_fixed, state_0, state_f, mass, dV1, dV2, DU, TU,
                                                               allowImpulsive)
        if not np.isfinite(cost):
            status = 3
            break
        alpha = 1.0
        if it > 10:                                       # :557-560
            alpha = lineSearch_direct(X, x_up, U, u_up, t_fixed, nstate, n_nodes, nsteps, Isp, MU, DU, TU, ops=ops)
        X = X + x_up * alpha
        U = U + u_up * alpha
        dV1 = dV1 + dV1_up * alpha
        dV2 = dV2 + dV2_up * alpha
        if flagEnd and it % 2 == 1:
            τ1 = τ1 + p1 * alpha                          # :564-565, not wrapped
            τ2 = τ2 + p2 * alpha
        if move_tf and it % 2 == 1:                       # :567, :582
            tf = min(max(tf + p3 * alpha, float(tf_bounds[1])), float(tf_bounds[2]))
            t_fixed = t0 + (tau + 1) / 2 * (tf - t0)
        t = t_fixed
        defect, _ = ops.defect(X, U, t, nsteps)           # :585
        er = float(np.abs(defect).max())
        hist[:, it - 1] = (er, cost, alpha, τ1, τ2) if tf_bounds is None else (er, cost, alpha, τ1, τ2, tf)
        if verbose:
            print("Iter %d. Max defect = %.2e. Cost = %.5f. alpha = %.3f." % (it, er, cost, alpha))
    if status == 0 and not np.isfinite(er):
        status = 2
    return (X, U, τ1, τ2, t, dV1, dV2, defect), {"status": status, "iterations": it, "history": hist[:, :maxIter]}


def lineSearch_direct(X_all, x_update, u_all, u_update, t_TU, nstate, n_nodes, nsteps, Isp, MU, DU, TU, ops=None):
    """alpha in LinRange(0.1, 1, 10) minimising sum(defect.^2) of the direct transcription (direct.jl:405-430); the ten
    trial trajectories are one batched sweep instead of ten."""
    ops = ops or HipDirectOps(MU, DU, TU, Isp)
    alpha_all = np.linspace(0.1, 1.0, 10)
    X_all = np.asarray(X_all, dtype=np.float64); x_update = np.asarray(x_update, dtype=np.float64)
    u_all = np.asarray(u_all, dtype=np.float64); u_update = np.asarray(u_update, dtype=np.float64)
    Xt = X_all[:, :, None] + x_update[:, :, None] * alpha_all[None, None, :]
    Ut = u_all[:, :, None] + u_update[:, :, None] * alpha_all[None, None, :]
    er = ops.defect_batch_sumsq(np.asfortranarray(Xt), np.asfortranarray(Ut), t_TU, nsteps)
    return float(alpha_all[int(np.argmin(er))])             # first minimiser, as `alpha[1]` (:428-429)


def addTimeFinal(XC_all, t_TU, Δt, MU, DU, TU, n_nodes, mass, thrustLimit, p, rho, Xf_times, Xf_states, maxIter=10,
                 n_desired=200, flag_adjointsOnly=False, integ=None, ctx=None, verbose=True):
    """addTimeFinal (HelperFunctions.jl:196-250), re-specified where the reference cannot run: a converged 12-row
    solution on t_TU gets a ballistic tail of Δt TU (end costates zeroed -- on a copy, the caller's array is not changed), is
    densified at n_desired points (the reference's 200, :208), re-meshed onto LinRange(t[0], t[end] + Δt, n_nodes), its end
    snapped onto the arrival orbit table (find_τ, :38-48) and re-solved by the fixed-end indirect loop.  Every phase runs in one
    library call (lto_indirect_add_time_batch).  Returns (XC_new, t_new) on status 0, otherwise the original (XC_all, t_TU)
    unchanged (:239-249)."""
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    t_TU = np.array(t_TU, dtype=np.float64)
    if XC_all.shape != (12, int(n_nodes)):
        raise ValueError("addTimeFinal takes the 12-row solution [12 x n_nodes]; got shape %s" % (XC_all.shape,))
    params = hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, p, rho)
    r = hotpath.indirect_add_time(XC_all, t_TU, params, Xf_times, Xf_states, [float(Δt)], n_desired=n_desired, integ=integ,
                                  flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    if verbose:
        print("addTimeFinal: Δt = %.6g TU, τ* = %.3f, status %d after %d iterations" % (Δt, r.tau[0], r.status[0], r.iterations[0]))
    if r.status[0] == 0:
        return r.XC_out[:, :, 0].copy(), r.t_out[:, 0].copy()
    return XC_all, t_TU


def tf_sweep(XC_all, t_TU, Δts, MU, DU, TU, mass, thrustLimit, p, rho, Xf_times, Xf_states, maxIter=10, n_desired=200,
             flag_adjointsOnly=False, integ=None, ctx=None):
    """addTimeFinal for many Δt at once: the cost-versus-time-of-flight curve of a converged transfer in one library call.
    Returns a dict of per-Δt arrays: dt [K], tof [K] (TU), XC [12 x n x K], t [n x K], tau [K], status [K], iterations [K],
    max_defect [K] and cost [K] (Δv of the control law, DU/TU)."""
    params = hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, p, rho)
    dts = np.asarray(Δts, dtype=np.float64).reshape(-1)
    r = hotpath.indirect_add_time(XC_all, t_TU, params, Xf_times, Xf_states, dts, n_desired=n_desired, integ=integ,
                                  flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    return {"dt": dts, "tof": r.t_out[-1] - r.t_out[0], "XC": r.XC_out, "t": r.t_out, "tau": r.tau, "status": r.status,
            "iterations": r.iterations, "max_defect": np.abs(r.defect).max(axis=(0, 1)), "cost": r.cost}


def addTimeFinal_mass(XC_all, t_TU, Δt, MU, DU, TU, n_nodes, Isp, thrustLimit, p, rho, Xf_times, Xf_states, maxIter=10,
                      n_desired=200, flag_adjointsOnly=False, integ=None, ctx=None, verbose=True):
    """addTimeFinal for a converged solution of the 14-row variable-mass system (one library call,
    lto_indirect_add_time_mass_batch): rows 7..13 of the last node are zeroed on a copy (the caller's array is not changed), the
    tail of Δt TU is the 14-row system's own flow with zero costates -- the orbit coasts, the mass follows the law's flow at
    |λ_v| = 0: constant for p > 1, full throttle for p = 0, the idle flow aL / (1 + e^(1/ρ)) for p = 1 -- and the 14-row loop
    re-solves on LinRange(t[0], t[end] + Δt, n_nodes) with r0, v0, m0 and rf, vf fixed and the final mass free: the guess's mass
    row is a starting value only.  Returns (XC_new, t_new) on status 0, otherwise the original (XC_all, t_TU) unchanged."""
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    t_TU = np.array(t_TU, dtype=np.float64)
    if XC_all.shape != (14, int(n_nodes)):
        raise ValueError("addTimeFinal_mass takes the 14-row solution [14 x n_nodes]; got shape %s" % (XC_all.shape,))
    if not (Isp > 0):
        raise ValueError("Isp must be positive; got %r" % (Isp,))
    params = hotpath.make_params(MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)
    r = hotpath.indirect_add_time_mass(XC_all, t_TU, params, Xf_times, Xf_states, [float(Δt)], n_desired=n_desired, integ=integ,
                                       flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    if verbose:
        print("addTimeFinal_mass: Δt = %.6g TU, τ* = %.3f, status %d after %d iterations, propellant %.6f kg"
              % (Δt, r.tau[0], r.status[0], r.iterations[0], r.propellant[0]))
    if r.status[0] == 0:
        return r.XC_out[:, :, 0].copy(), r.t_out[:, 0].copy()
    return XC_all, t_TU


def tf_sweep_mass(XC_all, t_TU, Δts, MU, DU, TU, Isp, thrustLimit, p, rho, Xf_times, Xf_states, maxIter=10, n_desired=200,
                  flag_adjointsOnly=False, integ=None, ctx=None):
    """addTimeFinal_mass for many Δt at once: the propellant-versus-time-of-flight curve of a converged variable-mass transfer in
    one library call.  Returns the dict of tf_sweep (XC [14 x n x K]; cost with every sample's own mass) plus propellant_kg [K] =
    XC_all[6, 0] - XC[6, -1, k] and mass_final_kg [K] = XC[6, -1, k]."""
    XC_all = np.asarray(XC_all, dtype=np.float64)
    if XC_all.ndim != 2 or XC_all.shape[0] != 14:
        raise ValueError("tf_sweep_mass takes the 14-row solution [14 x n_nodes]; got shape %s" % (XC_all.shape,))
    if not (Isp > 0):
        raise ValueError("Isp must be positive; got %r" % (Isp,))
    params = hotpath.make_params(MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)
    dts = np.asarray(Δts, dtype=np.float64).reshape(-1)
    r = hotpath.indirect_add_time_mass(XC_all, t_TU, params, Xf_times, Xf_states, dts, n_desired=n_desired, integ=integ,
                                       flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    return {"dt": dts, "tof": r.t_out[-1] - r.t_out[0], "XC": r.XC_out, "t": r.t_out, "tau": r.tau, "status": r.status,
            "iterations": r.iterations, "max_defect": np.abs(r.defect).max(axis=(0, 1)), "cost": r.cost,
            "propellant_kg": r.propellant, "mass_final_kg": r.XC_out[6, -1, :].copy()}


def meshRefine_indirect(XC_all, t_TU, MU, DU, TU, n_nodes, mass, thrustLimit, p, rho, n_new=None, passes=2, weights=None, maxIter=10,
                        flag_adjointsOnly=False, integ=None, ctx=None, verbose=True):
    """Mesh re-distribution of a converged 12-row indirect solution, the counterpart of meshRefine_direct: the nodes
    are moved -- and their number changed to n_new (default: n_nodes) -- so that every segment takes the same share of the
    integrator's trial steps (or of the caller's per-segment weights), the new nodes are taken from the solution's own piecewise
    trajectory, and the fixed-end indirect loop re-solves on the new grid.  One library call (lto_indirect_remesh_batch).
    Returns (XC_new, t_new, n_new) on status 0, otherwise the original (XC_all, t_TU, n_nodes) unchanged -- the convention of
    addTimeFinal."""
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    t_TU = np.array(t_TU, dtype=np.float64)
    if XC_all.shape != (12, int(n_nodes)):
        raise ValueError("meshRefine_indirect takes the 12-row solution [12 x n_nodes]; got shape %s" % (XC_all.shape,))
    if t_TU.shape != (int(n_nodes),):
        raise ValueError("meshRefine_indirect takes one time per node; got shape %s" % (t_TU.shape,))
    n_new = int(n_nodes) if n_new is None else int(n_new)
    params = hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, p, rho)
    r = hotpath.indirect_remesh(XC_all, t_TU, params, n_new=n_new, weights=weights, passes=passes, integ=integ,
                                flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    if verbose:
        print("meshRefine_indirect: %d -> %d nodes, max trial steps %d -> %d (mean %.2f -> %.2f), status %d after %d iterations"
              % (n_nodes, n_new, r.steps_before.max(), r.steps_after.max(), r.steps_before.mean(), r.steps_after.mean(), r.status,
                 r.iterations))
    if r.status == 0:
        return r.XC_out.copy(), r.t_out.copy(), n_new
    return XC_all, t_TU, int(n_nodes)


def meshRefine_indirect_mass(XC_all, t_TU, MU, DU, TU, n_nodes, Isp, thrustLimit, p, rho, n_new=None, passes=2, weights=None,
                             maxIter=10, flag_adjointsOnly=False, integ=None, ctx=None, verbose=True):
    """meshRefine_indirect for a converged solution of the 14-row variable-mass system: the nodes are moved onto the
    equidistributed grid along the solution's own piecewise trajectory, mass included, and the 14-row loop of
    multiShoot_CRTBP_indirect_mass re-solves there (r0, v0, m0 and rf, vf fixed, final mass free).  One library call
    (lto_indirect_remesh_mass_batch).  Returns (XC_new, t_new, n_new) on status 0, otherwise the original (XC_all, t_TU, n_nodes)
    unchanged."""
    XC_all = np.array(XC_all, dtype=np.float64, order="F")
    t_TU = np.array(t_TU, dtype=np.float64)
    if XC_all.shape != (14, int(n_nodes)):
        raise ValueError("meshRefine_indirect_mass takes the 14-row solution [14 x n_nodes]; got shape %s" % (XC_all.shape,))
    if t_TU.shape != (int(n_nodes),):
        raise ValueError("meshRefine_indirect_mass takes one time per node; got shape %s" % (t_TU.shape,))
    if not (Isp > 0):
        raise ValueError("Isp must be positive; got %r" % (Isp,))
    n_new = int(n_nodes) if n_new is None else int(n_new)
    params = hotpath.make_params(MU, DU, TU, thrustLimit, Isp, 1.0, p, rho)
    r = hotpath.indirect_remesh_mass(XC_all, t_TU, params, n_new=n_new, weights=weights, passes=passes, integ=integ,
                                     flag_adjointsOnly=flag_adjointsOnly, maxIter=maxIter, ctx=ctx)
    if verbose:
        print("meshRefine_indirect_mass: %d -> %d nodes, max trial steps %d -> %d (mean %.2f -> %.2f), status %d after %d iterations"
              % (n_nodes, n_new, r.steps_before.max(), r.steps_after.max(), r.steps_before.mean(), r.steps_after.mean(), r.status,
                 r.iterations))
    if r.status == 0:
        return r.XC_out.copy(), r.t_out.copy(), n_new
    return XC_all, t_TU, int(n_nodes)


def meshRefine_direct(X_all, u_all, t_TU, nstate, n_nodes, nsteps, Isp, MU, DU, TU, tol_min=1e-20, tol_max=1e-18,
                      max_nodes=1 << 20, batched=True, ops=None, verbose=True, device=False):
    """Errors-driven mesh refinement of the direct transcription (direct.jl:597-680): nodes are removed while the
    smallest RKF7(8) error estimate of a segment is below tol_min, then segments are bisected while the largest is above
    tol_max (new state = forward propagation to the segment's middle, new control = mean of its two controls).
    Returns (X_all, u_all, t_TU, n_nodes).

    Re-specified where the reference cannot run as written: `find(errors .== minimum(errors))[1]` (removed from Julia
    1.x) is the first arg-min / arg-max; MU, DU, TU are arguments instead of globals; the removal phase stops at two
    nodes and the addition phase at max_nodes (the reference loops forever if the estimate never reaches tol_max).

    batched=True bisects EVERY segment above tol_max in one pass: one error sweep + one mid-point sweep on the GPU per
    pass instead of one full sweep per inserted node.  The result is identical to the reference's one-node-per-pass
    loop, because a segment's error estimate depends only on its own two nodes, controls and times (direct.jl:77-105),
    so splitting one segment never changes the decision for another; batched=False runs the literal loop.

    device=True (with ops=None) runs both phases in ONE library call with the trajectory resident on the GPU
    (lto_direct_refine) instead of one or two round trips per removed node / insertion pass; same result and the
    same 4-tuple.  The call allocates, fills and returns its whole capacity, so the driver does not hand it max_nodes as it
    stands: it starts with room for max(8 n_nodes, 1 024) nodes and, only if the refinement stops at that room while
    max_nodes allows more, repeats the call from the input with eight times the room.  A call that does not reach its
    capacity gives the mesh of any larger capacity, so the result is that of max_nodes itself."""
    if device and ops is None:
        limit = max(int(max_nodes), int(n_nodes))
        room = min(limit, max(8 * int(n_nodes), 1024))
        while True:
            r = hotpath.direct_refine(X_all, u_all, t_TU, nsteps, MU, DU, TU, Isp, tol_min, tol_max, room)
            if r.status != 1 or room >= limit:
                break
            room = min(limit, 8 * room)
        if verbose:
            print("Starting with %d nodes." % n_nodes)
            print("Removed %d nodes, added %d in %d passes (status %d). Now have %d nodes."
                  % (r.n_removed, r.n - (int(n_nodes) - r.n_removed), r.passes, r.status, r.n))
        return r.X, r.U, r.t, r.n
    ops = ops or HipDirectOps(MU, DU, TU, Isp)
    X = np.array(X_all, dtype=np.float64, order="F")
    U = np.array(u_all, dtype=np.float64, order="F")
    t = np.array(t_TU, dtype=np.float64)
    n_nodes = int(n_nodes)
    n_start = n_nodes
    if verbose:
        print("Starting with %d nodes." % n_nodes)
    _, errors = ops.defect(X, U, t, nsteps)
    # ---- remove nodes that only make things messy (:611-628); inherently sequential: a removal merges two segments
    while n_nodes > 2 and np.min(errors) < tol_min:
        k = int(np.argmin(errors))
        if k == 0:
            k = 1                                            # never remove the first node (:616-618)
        X = np.delete(X, k, axis=1)
        U = np.delete(U, k, axis=1)
        t = np.delete(t, k)
        n_nodes -= 1
        _, errors = ops.defect(X, U, t, nsteps)
    if verbose and n_nodes != n_start:
        print("Removed nodes, now n_nodes = %d" % n_nodes)
    n_mid = n_nodes
    # ---- add nodes where the estimate is too large (:635-668)
    while np.max(errors) > tol_max and n_nodes < max_nodes:
        if batched:
            split = np.flatnonzero(errors > tol_max)[: max_nodes - n_nodes]
        else:
            split = np.array([int(np.argmax(errors))])
        x_mid = ops.midpoints(X, U, t)                       # every segment's mid-point state in one sweep
        t_new = t[split] + (t[split + 1] - t[split]) / 2     # :644
        u_new = (U[:, split] + U[:, split + 1]) / 2          # :659
        X = np.insert(X, split + 1, x_mid[:, split], axis=1)
        U = np.insert(U, split + 1, u_new, axis=1)
        t = np.insert(t, split + 1, t_new)
        n_nodes += len(split)
        _, errors = ops.defect(X, U, t, nsteps)
    if verbose:
        if n_nodes != n_mid:
            print("Added nodes, now n_nodes = %d" % n_nodes)
        if n_nodes == n_start:
            print("Did not need to add or remove nodes.")
        else:
            print("Refined the mesh. Now have %d nodes." % n_nodes)
    return np.asfortranarray(X), np.asfortranarray(U), t, n_nodes


def controlLaw_cart(lambda_v, thrustLimit, p, rho, mass, DU=None, TU=None):
    """Thrust vector(s) in N from the velocity costate(s) (indirect.jl:389-440): lambda_v [3] or [3 x n] ->
    control of the same shape.  Same law as the propagated dynamics (stateCostate_deriv.jl:33-64); like the reference,
    a zero primer vector yields NaN (0/0 in `lambda_v ./ norm(lambda_v)`, :439) and an invalid p raises."""
    from .constants import DU as _DU, TU as _TU
    DU = _DU if DU is None else DU
    TU = _TU if TU is None else TU
    lam = np.asarray(lambda_v, dtype=np.float64)
    n = np.sqrt(np.sum(lam * lam, axis=0))
    accelLimit = thrustLimit / mass / 1e3 * TU ** 2 / DU            # N -> DU/TU^2 (:412)
    if p == 0:
        umag = np.full_like(n, accelLimit)
    elif p == 1:
        umag = 0.5 * (1.0 + np.tanh((n - 1.0) / (2.0 * rho))) * accelLimit
    elif p > 1:
        umag = np.minimum((n / p) ** (1.0 / (p - 1.0)), accelLimit)
    else:
        raise ValueError("Invalid value of p!")
    umag = np.where(np.isnan(umag), 0.0, umag)                      # :431-433
    with np.errstate(invalid="ignore", divide="ignore"):
        return -umag * lam / n * mass * DU * 1e3 / TU ** 2          # DU/TU^2 -> N (:439)


def thrust_arcs(XC_all, t_TU, MU, DU, TU, mass, thrustLimit, p, rho, Isp=None, max_events=64, integ=None, ctx=None):
    """Burn arcs and dv of indirect solutions, read off the integration itself (hotpath.indirect_events) instead of
    a plot of controlLaw_cart along densify (indirect.jl:348-440).  XC_all [12 x n] or [12 x n x B], t_TU [n] or [n x B]; mass,
    thrustLimit, p and rho scalars or one per trajectory.  Per trajectory a dict: arcs = [(t_on, t_off)] in TU clipped to
    [t0, tf], dv (DU/TU), dv_ms (m/s), burn_time (TU), burn_days, n_events, status, and with Isp the rocket-equation propellant
    mass (1 - exp(-dv_ms / (Isp 9.81))) in kg.  A list of dicts for a batch, one dict otherwise."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim not in (2, 3) or XC.shape[0] != 12:
        raise ValueError("XC_all must be [12 x n] or [12 x n x B]")
    batched = XC.ndim == 3
    B = XC.shape[2] if batched else 1
    t = np.asarray(t_TU, dtype=np.float64)
    if t.shape not in ((XC.shape[1],), (XC.shape[1], B)):
        raise ValueError("t_TU must be [n] or [n x B]")
    per = [np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)) for v in (mass, thrustLimit, p, rho)]
    prms = [hotpath.make_params(MU, DU, TU, per[1][b], per[0][b], 1.0, per[2][b], per[3][b]) for b in range(B)]
    ev = hotpath.indirect_events(XC if batched else XC[:, :, None], t if t.ndim == 1 else t, prms, max_events, integ, ctx)
    out = []
    for b in range(B):
        tb = t if t.ndim == 1 else t[:, b]
        t0, tf = float(tb[0]), float(tb[-1])
        k = min(int(ev.n_events[b]), int(max_events))
        times = ev.t_event[:k, b]
        times = times[np.isfinite(times)]
        on, mark, arcs = bool(ev.on0[b]), t0, []
        for te in times:
            if on:
                arcs.append((mark, float(te)))
            else:
                mark = float(te)
            on = not on
        if on and ev.status[b] == 0:
            arcs.append((mark, tf))
        dv = float(ev.dv[b])
        dv_ms = dv * DU / TU * 1e3
        r = dict(arcs=arcs, dv=dv, dv_ms=dv_ms, burn_time=float(ev.burn_time[b]), burn_days=float(ev.burn_time[b]) * TU / 86400.0,
                 n_events=int(ev.n_events[b]), status=int(ev.status[b]))
        if Isp is not None:
            r["propellant"] = float(per[0][b] * (1.0 - np.exp(-dv_ms / (Isp * 9.81))))
        out.append(r)
    return out if batched else out[0]


def _arcs_of(ev, b, t0, tf, max_events):
    """[(t_on, t_off)] of trajectory b of a batched ThrustEvents, clipped to [t0, tf]."""
    k = min(int(ev.n_events[b]), int(max_events))
    times = ev.t_event[:k, b]
    times = times[np.isfinite(times)]
    on, mark, arcs = bool(ev.on0[b]), t0, []
    for te in times:
        if on:
            arcs.append((mark, float(te)))
        else:
            mark = float(te)
        on = not on
    if on and ev.status[b] == 0:
        arcs.append((mark, tf))
    return arcs


def _mass_budget(ev, m0, Isp, DU, TU, t, max_events):
    """The per-trajectory dicts of thrust_arcs_mass from a batched ThrustEvents of the 14-row system: m0 [B] the masses of the
    first nodes, Isp [B], t [n] or [n x B]."""
    out = []
    for b in range(len(m0)):
        tb = t if t.ndim == 1 else t[:, b]
        dv = float(ev.dv[b])
        dv_ms = dv * DU / TU * 1e3
        prop = float(ev.propellant[b])
        m_f = float(m0[b]) - prop
        with np.errstate(invalid="ignore", divide="ignore"):
            dv_rocket = float(Isp[b] * 9.81 * np.log(m0[b] / m_f))
        out.append(dict(arcs=_arcs_of(ev, b, float(tb[0]), float(tb[-1]), max_events), dv=dv, dv_ms=dv_ms,
                        burn_time=float(ev.burn_time[b]), burn_days=float(ev.burn_time[b]) * TU / 86400.0,
                        n_events=int(ev.n_events[b]), status=int(ev.status[b]), propellant_kg=prop, mass_final_kg=m_f,
                        dv_rocket_ms=dv_rocket))
    return out


def thrust_arcs_mass(XC_all, t_TU, MU, DU, TU, Isp, thrustLimit, p, rho, max_events=64, integ=None, ctx=None):
    """thrust_arcs for solutions of the 14-row variable-mass system (hotpath.indirect_events_mass): XC_all [14 x n] or
    [14 x n x B]; Isp, thrustLimit, p and rho scalars or one per trajectory.  The propellant is a state of the integration and is
    read off it, not estimated from the rocket equation.  Per trajectory the dict of thrust_arcs plus propellant_kg (the sum of
    the segments' mass drops), mass_final_kg = XC_all[6, 0] - propellant_kg and dv_rocket_ms = Isp 9.81 ln(m0 / mass_final): the
    ideal velocity increment of that mass ratio, which dv_ms equals on a continuous trajectory."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim not in (2, 3) or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n] or [14 x n x B]")
    batched = XC.ndim == 3
    B = XC.shape[2] if batched else 1
    t = np.asarray(t_TU, dtype=np.float64)
    if t.shape not in ((XC.shape[1],), (XC.shape[1], B)):
        raise ValueError("t_TU must be [n] or [n x B]")
    per = [np.broadcast_to(np.asarray(v, dtype=np.float64), (B,)) for v in (Isp, thrustLimit, p, rho)]
    if not np.all(per[0] > 0.0):
        raise ValueError("Isp must be positive")
    prms = [hotpath.make_params(MU, DU, TU, per[1][b], per[0][b], 1.0, per[2][b], per[3][b]) for b in range(B)]
    X3 = XC if batched else XC[:, :, None]
    ev = hotpath.indirect_events_mass(X3, t, prms, max_events, integ, ctx)
    out = _mass_budget(ev, X3[6, 0, :], per[0], DU, TU, t, max_events)
    return out if batched else out[0]


def replay_misses(x_final, x_target, DU, TU):
    """Misses of replayed end states x_final [nstate x B] against x_target [nstate]: dict of miss_r_km and miss_v_ms [B] (the
    2-norms of the position and velocity differences) and, for 7 states, miss_m_kg (final mass minus the target's)."""
    xf = np.asarray(x_final, dtype=np.float64)
    d = xf - np.asarray(x_target, dtype=np.float64)[:, None]
    out = dict(miss_r_km=np.linalg.norm(d[0:3], axis=0) * DU, miss_v_ms=np.linalg.norm(d[3:6], axis=0) * DU / TU * 1e3)
    if xf.shape[0] == 7:
        out["miss_m_kg"] = d[6].copy()
    return out


def dispersion_starts(x_nominal, n_samples, sigma_r_km, sigma_v_ms, seed, DU, TU):
    """x0 [nstate x n_samples]: the nominal start with Gaussian position errors of sigma_r_km per axis and velocity errors of
    sigma_v_ms per axis from numpy.random.default_rng(seed); sample 0 is the nominal start itself, a mass row is left alone."""
    x = np.asarray(x_nominal, dtype=np.float64)
    n = int(n_samples)
    if n < 1:
        raise ValueError("n_samples must be >= 1")
    rng = np.random.default_rng(seed)
    err = rng.standard_normal((6, n))
    err[0:3] *= float(sigma_r_km) / DU
    err[3:6] *= float(sigma_v_ms) / 1e3 * TU / DU
    err[:, 0] = 0.0
    x0 = np.array(np.repeat(x[:, None], n, axis=1), order="F")
    x0[0:6] += err
    x0[:, 0] = x
    return x0


def fly_control(ctx, XC_all, t_TU, prm, x0=None, lamv=None, n_knots=257, integ=None, sample_every=0):
    """Fly the thrust history of an indirect solution from given starts (hotpath.control_replay).  XC_all [12 x n] or
    [14 x n] with its grid t_TU and its parameters prm (LtoParams or the 8-tuple; 14 rows: Isp in the mass slot).  The solution
    is sampled at n_knots even times with hotpath.densify / densify_mass, lambda_v (rows 9..11, or 10..12) at those knots is the
    control history -- or lamv [3 x n_knots] / [3 x n_knots x B], a corrector's -- and the 6- or 7-state is replayed from x0
    [nstate x B] (default: the solution's own first node).  Returns a dict: x_final, miss_r_km, miss_v_ms (and miss_m_kg for 14
    rows) against the solution's last node, dv (DU/TU), dv_ms, status, accepted, rejected, samples, sample_knots, lamv, t_knots."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] not in (12, 14):
        raise ValueError("XC_all must be [12 x n] or [14 x n]")
    nd = XC.shape[0]
    ns = 6 if nd == 12 else 7
    t = np.asarray(t_TU, dtype=np.float64)
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    if lamv is None:
        dense, t_knots = (hotpath.densify if nd == 12 else hotpath.densify_mass)(XC, t, p, int(n_knots), integ, ctx)
        lamv = np.array(dense[9:12] if nd == 12 else dense[10:13], order="F")
    else:
        lamv = np.asarray(lamv, dtype=np.float64)
        t_knots = np.linspace(t[0], t[-1], lamv.shape[1])
    x0 = XC[:ns, :1].copy() if x0 is None else np.asarray(x0, dtype=np.float64).reshape(ns, -1)
    r = hotpath.control_replay(x0, lamv, float(t[0]), float(t[-1]), p, integ, sample_every, ctx)
    out = dict(x_final=r.x_final, dv=r.dv, dv_ms=r.dv * p.DU / p.TU * 1e3, status=r.status, accepted=r.accepted,
               rejected=r.rejected, samples=r.samples, sample_knots=r.sample_knots, lamv=lamv, t_knots=t_knots)
    out.update(replay_misses(r.x_final, XC[:ns, -1], p.DU, p.TU))
    return out


def dispersion(ctx, XC_all, t_TU, prm, n_samples, sigma_r_km, sigma_v_ms, seed, n_knots=257, integ=None, lamv=None):
    """Monte-Carlo dispersion of an indirect solution's open-loop thrust history: n_samples starts drawn by dispersion_starts
    around the solution's first node (sample 0 undisturbed), all flown by fly_control in one call.  Returns fly_control's dict
    plus x0 and, over the samples of status 0, percentiles = {"miss_r_km": {50: .., 95: .., 99: ..}, "miss_v_ms": {..}}."""
    XC = np.asarray(XC_all, dtype=np.float64)
    ns = 6 if XC.shape[0] == 12 else 7
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    x0 = dispersion_starts(XC[:ns, 0], n_samples, sigma_r_km, sigma_v_ms, seed, p.DU, p.TU)
    out = fly_control(ctx, XC, t_TU, p, x0, lamv, n_knots, integ)
    ok = np.asarray(out["status"]) == 0
    out["x0"] = x0
    out["percentiles"] = {k: {q: (float(np.percentile(out[k][ok], q)) if ok.any() else float("nan")) for q in (50, 95, 99)}
                          for k in ("miss_r_km", "miss_v_ms")}
    return out


def neighbouring_gains(ctx, XC_all, t_TU, prm, integ=None, sing_tol=1e-10):
    """Neighbouring-extremal feedback gains of 12-row solutions (hotpath.guidance_gains): XC_all [12 x n] or
    [12 x n x B] with its grid and parameters.  Returns a dict: K [6 x 6 x (n-1) (x B)], pivot, status, and ok = status == 0."""
    g = hotpath.guidance_gains(XC_all, t_TU, prm, integ, sing_tol, ctx)
    return dict(K=g.K, pivot=g.pivot, status=g.status, ok=np.asarray(g.status) == 0)


def guided_nav(n_updates, n_samples, nav_sigma_r_km, nav_sigma_v_ms, seed, DU, TU):
    """nav [6 x n_updates x n_samples]: Gaussian navigation errors of nav_sigma_r_km per position axis and nav_sigma_v_ms per
    velocity axis from numpy.random.default_rng(seed); sample 0 navigates without error."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((6, int(n_updates), int(n_samples)))
    e[0:3] *= float(nav_sigma_r_km) / DU
    e[3:6] *= float(nav_sigma_v_ms) / 1e3 * TU / DU
    e[:, :, 0] = 0.0
    return np.asfortranarray(e)


def fly_guided(ctx, XC_all, t_TU, prm, x0=None, n_guid=None, update_every=1, nav=None, integ=None):
    """Fly a 12-row indirect solution with neighbouring-extremal feedback from given starts (hotpath.guidance_gains and
    hotpath.guided_flight).  XC_all [12 x n] with its grid t_TU and its parameters prm (LtoParams or the 8-tuple).
    n_guid resamples the solution onto that many even nodes with hotpath.densify first -- an extremal sampled more finely is still
    an extremal, and that is how more frequent updates are had.  The costate is updated at every update_every-th node (0: never,
    the open-loop flow of the start's state under the nominal's first costate); nav [6 x n_upd (x B)] is added to the measured state
    at the updates.  x0 [6 x B] (default: the solution's own first node).  Returns a dict: x_final, lam_final, miss_r_km and
    miss_v_ms against the solution's last node, dv (DU/TU), dv_ms, dv_nominal_ms (the guided flight of the nominal start without
    navigation error), dv_excess_ms = dv_ms - dv_nominal_ms, status, accepted, rejected, K, pivot, gain_status, XC_guid, t_guid."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] != 12:
        raise ValueError("XC_all must be [12 x n]: guidance is built for 12-row solutions")
    t = np.asarray(t_TU, dtype=np.float64)
    if t.shape != (XC.shape[1],):
        raise ValueError("t_TU must hold one time per node")
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    if n_guid is not None:
        if int(n_guid) < 2:
            raise ValueError("n_guid must be >= 2")
        XC, t = hotpath.densify(XC, t, p, int(n_guid), integ, ctx)
    n = XC.shape[1]
    n_upd = hotpath.guided_updates(n, update_every)
    x0 = XC[:6, :1].copy() if x0 is None else np.asarray(x0, dtype=np.float64).reshape(6, -1)
    B = x0.shape[1]
    if nav is not None:
        nav = np.asarray(nav, dtype=np.float64)
        if nav.shape not in ((6, n_upd), (6, n_upd, B)):
            raise ValueError("nav must be [6 x %d] or [6 x %d x %d]" % (n_upd, n_upd, B))
        if nav.ndim == 2:
            nav = np.repeat(nav[:, :, None], B, axis=2)
    g = hotpath.guidance_gains(XC, t, p, integ, ctx=ctx)
    if int(update_every) > 0 and g.status != 0:
        raise ValueError("the solution has no finite gains (status %d, smallest pivot ratio %.3g): fly it with update_every = 0"
                         % (g.status, np.nanmin(g.pivot)))
    K = g.K if g.status == 0 else np.zeros_like(g.K)
    x_all = np.concatenate([XC[:6, :1], x0], axis=1)         # column 0: the nominal start, the reference of the dv excess
    nav_all = None if nav is None else np.concatenate([np.zeros((6, n_upd, 1)), nav], axis=2)
    r = hotpath.guided_flight(XC, t, K, x_all, p, update_every, nav_all, integ, ctx=ctx)
    dv_ms = r.dv * p.DU / p.TU * 1e3
    out = dict(x_final=r.x_final[:, 1:], lam_final=r.lam_final[:, 1:], dv=r.dv[1:], dv_ms=dv_ms[1:], dv_nominal_ms=float(dv_ms[0]),
               dv_excess_ms=dv_ms[1:] - dv_ms[0], status=r.status[1:], accepted=r.accepted[1:], rejected=r.rejected[1:], K=g.K,
               pivot=g.pivot, gain_status=g.status, XC_guid=XC, t_guid=t)
    out.update(replay_misses(out["x_final"], XC[:6, -1], p.DU, p.TU))
    return out


def dispersion_guided(ctx, XC_all, t_TU, prm, n_samples, sigma_r_km, sigma_v_ms, seed, n_guid=None, update_every=1, integ=None,
                      nav_sigma_r_km=None, nav_sigma_v_ms=None, nav_seed=None):
    """Monte-Carlo dispersion of a 12-row indirect solution flown with neighbouring-extremal feedback: the starts of `dispersion`
    (the same dispersion_starts draws, sample 0 undisturbed), all flown by fly_guided in one call, so the two runs compare sample
    by sample.  nav_sigma_r_km / nav_sigma_v_ms (both or neither) add Gaussian navigation errors from
    numpy.random.default_rng(nav_seed) at every update (guided_nav).  Returns fly_guided's dict plus x0, nav and, over the samples
    of status 0, percentiles = {"miss_r_km": {50: .., 95: .., 99: ..}, "miss_v_ms": {..}, "dv_excess_ms": {..}}."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] != 12:
        raise ValueError("XC_all must be [12 x n]: guidance is built for 12-row solutions")
    if (nav_sigma_r_km is None) != (nav_sigma_v_ms is None):
        raise ValueError("nav_sigma_r_km and nav_sigma_v_ms are given together")
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    x0 = dispersion_starts(XC[:6, 0], n_samples, sigma_r_km, sigma_v_ms, seed, p.DU, p.TU)
    nav = None
    if nav_sigma_r_km is not None:
        n_upd = hotpath.guided_updates(XC.shape[1] if n_guid is None else int(n_guid), update_every)
        nav = guided_nav(n_upd, n_samples, nav_sigma_r_km, nav_sigma_v_ms, nav_seed, p.DU, p.TU)
    out = fly_guided(ctx, XC, t_TU, p, x0, n_guid, update_every, nav, integ)
    ok = np.asarray(out["status"]) == 0
    out["x0"] = x0
    out["nav"] = nav
    out["percentiles"] = {k: {q: (float(np.percentile(out[k][ok], q)) if ok.any() else float("nan")) for q in (50, 95, 99)}
                          for k in ("miss_r_km", "miss_v_ms", "dv_excess_ms")}
    return out


def neighbouring_gains_mass(ctx, XC_all, t_TU, prm, integ=None, sing_tol=1e-10):
    """neighbouring_gains for solutions of the 14-row variable-mass system (hotpath.guidance_gains_mass): XC_all
    [14 x n] or [14 x n x B], Isp in the mass slot of prm.  Returns a dict: K [7 x 7 x (n-1) (x B)], pivot, status, ok."""
    g = hotpath.guidance_gains_mass(XC_all, t_TU, prm, integ, sing_tol, ctx)
    return dict(K=g.K, pivot=g.pivot, status=g.status, ok=np.asarray(g.status) == 0)


def fly_guided_mass(ctx, XC_all, t_TU, prm, x0=None, n_guid=None, update_every=1, nav=None, integ=None):
    """fly_guided for a solution of the 14-row variable-mass system (hotpath.guidance_gains_mass and hotpath.guided_flight_mass,
    DESIGN 4.24).  XC_all [14 x n] with its grid t_TU and its parameters prm (Isp in the mass slot); n_guid resamples through
    hotpath.densify_mass; x0 [7 x B] (r, v, m; default: the solution's own first node); nav [7 x n_upd (x B)] is added to the
    measured state, the mass included, at the updates.  Returns fly_guided's dict with x_final and lam_final [7 x B], K
    [7 x 7 x (n-1)], and besides miss_m_kg (final mass minus the solution's last node's), propellant_kg = x0[6] - x_final[6] per
    start, propellant_nominal_kg (the guided flight of the nominal start, which rides in the same call) and propellant_excess_kg
    = propellant_kg - propellant_nominal_kg."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n]")
    t = np.asarray(t_TU, dtype=np.float64)
    if t.shape != (XC.shape[1],):
        raise ValueError("t_TU must hold one time per node")
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    if n_guid is not None:
        if int(n_guid) < 2:
            raise ValueError("n_guid must be >= 2")
        XC, t = hotpath.densify_mass(XC, t, p, int(n_guid), integ, ctx)
    n = XC.shape[1]
    n_upd = hotpath.guided_updates(n, update_every)
    x0 = XC[:7, :1].copy() if x0 is None else np.asarray(x0, dtype=np.float64).reshape(7, -1)
    B = x0.shape[1]
    if nav is not None:
        nav = np.asarray(nav, dtype=np.float64)
        if nav.shape not in ((7, n_upd), (7, n_upd, B)):
            raise ValueError("nav must be [7 x %d] or [7 x %d x %d]" % (n_upd, n_upd, B))
        if nav.ndim == 2:
            nav = np.repeat(nav[:, :, None], B, axis=2)
    g = hotpath.guidance_gains_mass(XC, t, p, integ, ctx=ctx)
    if int(update_every) > 0 and g.status != 0:
        raise ValueError("the solution has no finite gains (status %d, smallest pivot ratio %.3g): fly it with update_every = 0"
                         % (g.status, np.nanmin(g.pivot)))
    K = g.K if g.status == 0 else np.zeros_like(g.K)
    x_all = np.concatenate([XC[:7, :1], x0], axis=1)         # column 0: the nominal start, the reference of the excesses
    nav_all = None if nav is None else np.concatenate([np.zeros((7, n_upd, 1)), nav], axis=2)
    r = hotpath.guided_flight_mass(XC, t, K, x_all, p, update_every, nav_all, integ, ctx=ctx)
    dv_ms = r.dv * p.DU / p.TU * 1e3
    prop = x_all[6] - r.x_final[6]
    out = dict(x_final=r.x_final[:, 1:], lam_final=r.lam_final[:, 1:], dv=r.dv[1:], dv_ms=dv_ms[1:], dv_nominal_ms=float(dv_ms[0]),
               dv_excess_ms=dv_ms[1:] - dv_ms[0], propellant_kg=prop[1:], propellant_nominal_kg=float(prop[0]),
               propellant_excess_kg=prop[1:] - prop[0], status=r.status[1:], accepted=r.accepted[1:], rejected=r.rejected[1:],
               K=g.K, pivot=g.pivot, gain_status=g.status, XC_guid=XC, t_guid=t)
    out.update(replay_misses(out["x_final"], XC[:7, -1], p.DU, p.TU))
    return out


def guided_nav_mass(n_updates, n_samples, nav_sigma_m_kg, seed):
    """nav_m [n_updates x n_samples]: Gaussian errors of nav_sigma_m_kg on the measured mass from numpy.random.default_rng(seed);
    sample 0 navigates without error."""
    e = np.random.default_rng(seed).standard_normal((int(n_updates), int(n_samples))) * float(nav_sigma_m_kg)
    e[:, 0] = 0.0
    return e


def dispersion_guided_mass(ctx, XC_all, t_TU, prm, n_samples, sigma_r_km, sigma_v_ms, seed, n_guid=None, update_every=1, integ=None,
                           nav_sigma_r_km=None, nav_sigma_v_ms=None, nav_seed=None, sigma_m_kg=None, m_seed=None,
                           nav_sigma_m_kg=None, nav_m_seed=None):
    """dispersion_guided for a solution of the 14-row variable-mass system: the starts `dispersion` makes for that solution (the
    same dispersion_starts draws, sample 0 undisturbed, the mass row left alone), all flown by fly_guided_mass in one call.
    sigma_m_kg adds a Gaussian error to the start mass of every sample but 0 from numpy.random.default_rng(m_seed);
    nav_sigma_r_km / nav_sigma_v_ms (both or neither; guided_nav, nav_seed) and nav_sigma_m_kg (guided_nav_mass, nav_m_seed) add
    navigation errors at every update.  Returns fly_guided_mass's dict plus x0, nav and, over the samples of status 0, percentiles
    = {"miss_r_km": {50: .., 95: .., 99: ..}, "miss_v_ms": {..}, "dv_excess_ms": {..}, "propellant_excess_kg": {..}}."""
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] != 14:
        raise ValueError("XC_all must be [14 x n]")
    if (nav_sigma_r_km is None) != (nav_sigma_v_ms is None):
        raise ValueError("nav_sigma_r_km and nav_sigma_v_ms are given together")
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    n_samples = int(n_samples)
    x0 = dispersion_starts(XC[:7, 0], n_samples, sigma_r_km, sigma_v_ms, seed, p.DU, p.TU)
    if sigma_m_kg is not None:
        em = np.random.default_rng(m_seed).standard_normal(n_samples) * float(sigma_m_kg)
        em[0] = 0.0
        x0[6] += em
    nav = None
    if nav_sigma_r_km is not None or nav_sigma_m_kg is not None:
        n_upd = hotpath.guided_updates(XC.shape[1] if n_guid is None else int(n_guid), update_every)
        nav = np.zeros((7, n_upd, n_samples), order="F")
        if nav_sigma_r_km is not None:
            nav[0:6] = guided_nav(n_upd, n_samples, nav_sigma_r_km, nav_sigma_v_ms, nav_seed, p.DU, p.TU)
        if nav_sigma_m_kg is not None:
            nav[6] = guided_nav_mass(n_upd, n_samples, nav_sigma_m_kg, nav_m_seed)
    out = fly_guided_mass(ctx, XC, t_TU, p, x0, n_guid, update_every, nav, integ)
    ok = np.asarray(out["status"]) == 0
    out["x0"] = x0
    out["nav"] = nav
    out["percentiles"] = {k: {q: (float(np.percentile(out[k][ok], q)) if ok.any() else float("nan")) for q in (50, 95, 99)}
                          for k in ("miss_r_km", "miss_v_ms", "dv_excess_ms", "propellant_excess_kg")}
    return out


def covariance_diag(nx, sigma_r_km, sigma_v_ms, sigma_m_kg, DU, TU):
    """The diagonal covariance [nx x nx] of per-axis position, velocity and (nx = 7) mass sigmas in the units of dispersion_starts
    and guided_nav: km -> DU, m/s -> DU/TU, the mass row in kg as it is.  None counts as zero."""
    d = np.zeros(nx)
    d[0:3] = (0.0 if sigma_r_km is None else float(sigma_r_km)) / DU
    d[3:6] = (0.0 if sigma_v_ms is None else float(sigma_v_ms)) / 1e3 * TU / DU
    if nx == 7:
        d[6] = 0.0 if sigma_m_kg is None else float(sigma_m_kg)
    return np.diag(d * d)


def covariance_sigmas(P, DU, TU):
    """What covariance_guided reports of covariances P [nx x nx x ...] (nx = 6 or 7, DU and DU/TU units, the mass in kg): a dict of
    sigma_r_km and sigma_v_ms (the trace RSS of the position and velocity blocks), sigma_r_max_km (the largest principal position
    sigma) and, for nx = 7, sigma_m_kg, each of P's trailing shape; every root is sqrt(max(0, .)), NaN stays NaN."""
    P = np.asarray(P, dtype=np.float64)
    nx = P.shape[0]
    if P.ndim < 2 or P.shape[1] != nx or nx not in (6, 7):
        raise ValueError("P must be [6 x 6 x ...] or [7 x 7 x ...]")

    def root(v):
        return np.sqrt(np.where(np.isnan(v), np.nan, np.maximum(0.0, v)))
    tr_r = P[0, 0] + P[1, 1] + P[2, 2]
    tr_v = P[3, 3] + P[4, 4] + P[5, 5]
    Prr = np.moveaxis(P[0:3, 0:3], (0, 1), (-2, -1))
    Prr = 0.5 * (Prr + np.swapaxes(Prr, -1, -2))
    ok = np.all(np.isfinite(Prr), axis=(-2, -1))
    lam = np.full(Prr.shape[:-2], np.nan)
    if np.any(ok):
        lam[ok] = np.linalg.eigvalsh(Prr[ok])[..., -1]
    out = dict(sigma_r_km=root(tr_r) * DU, sigma_v_ms=root(tr_v) * DU / TU * 1e3, sigma_r_max_km=root(lam) * DU)
    if nx == 7:
        out["sigma_m_kg"] = root(P[6, 6])
    return out


def _covariance_guided(nx, ctx, XC_all, t_TU, prm, sigma_r_km, sigma_v_ms, sigma_m_kg, n_guid, update_every, integ, nav_sigma_r_km,
                       nav_sigma_v_ms, nav_sigma_m_kg, sing_tol):
    XC = np.asarray(XC_all, dtype=np.float64)
    if XC.ndim != 2 or XC.shape[0] != 2 * nx:
        raise ValueError("XC_all must be [%d x n]" % (2 * nx))
    t = np.asarray(t_TU, dtype=np.float64)
    if t.shape != (XC.shape[1],):
        raise ValueError("t_TU must hold one time per node")
    p = prm if isinstance(prm, hotpath.LtoParams) else hotpath.make_params(*prm)
    navs = [np.asarray(0.0 if v is None else v, dtype=np.float64) for v in (nav_sigma_r_km, nav_sigma_v_ms, nav_sigma_m_kg)]
    ev = np.asarray(update_every)
    if not np.issubdtype(ev.dtype, np.integer) or np.any(ev < 0):
        raise ValueError("update_every must hold integers >= 0")
    shape = np.broadcast_shapes(ev.shape, *[v.shape for v in navs])           # the case list: the settings broadcast together
    ev_c = np.broadcast_to(ev, shape).reshape(-1)
    nav_c = [np.broadcast_to(v, shape).reshape(-1) for v in navs]
    nc = ev_c.shape[0]
    P0 = np.repeat(covariance_diag(nx, sigma_r_km, sigma_v_ms, sigma_m_kg, p.DU, p.TU)[:, :, None], nc, axis=2)
    R = np.stack([covariance_diag(nx, nav_c[0][i], nav_c[1][i], nav_c[2][i], p.DU, p.TU) for i in range(nc)], axis=2)
    if n_guid is not None:
        if int(n_guid) < 2:
            raise ValueError("n_guid must be >= 2")
        XC, t = (hotpath.densify if nx == 6 else hotpath.densify_mass)(XC, t, p, int(n_guid), integ, ctx)
    c = hotpath.guidance_covariance(XC, t, p, P0, R, ev_c, integ, sing_tol, with_nodes=True, ctx=ctx)
    n = XC.shape[1]
    nodes = covariance_sigmas(c.P_nodes, p.DU, p.TU)                           # [n x n_cases]
    out = dict(P_final=c.P_final.reshape((nx, nx) + shape), P_nodes=c.P_nodes.reshape((nx, nx, n) + shape),
               cov_status=c.cov_status.reshape(shape), gain_status=c.gain_status, K=c.K, pivot=c.pivot, XC_guid=XC, t_guid=t,
               update_every=np.broadcast_to(ev, shape).copy(), sigma_r_km=nodes["sigma_r_km"].reshape((n,) + shape),
               sigma_v_ms=nodes["sigma_v_ms"].reshape((n,) + shape))
    out["miss_r_km_rss"] = out["sigma_r_km"][-1]
    out["miss_v_ms_rss"] = out["sigma_v_ms"][-1]
    out["miss_r_km_max"] = nodes["sigma_r_max_km"].reshape((n,) + shape)[-1]
    if nx == 7:
        out["sigma_m_kg"] = nodes["sigma_m_kg"].reshape((n,) + shape)
        out["sigma_mf_kg"] = out["sigma_m_kg"][-1]
    return out


def covariance_guided(ctx, XC_all, t_TU, prm, sigma_r_km, sigma_v_ms, n_guid=None, update_every=1, integ=None, nav_sigma_r_km=None,
                      nav_sigma_v_ms=None, sing_tol=1e-10):
    """Linear covariance of a 12-row solution flown with neighbouring-extremal feedback (hotpath.guidance_covariance):
    the deterministic twin of dispersion_guided.  The start covariance is diagonal with sigma_r_km per position axis and sigma_v_ms
    per velocity axis (the units of dispersion_starts), the navigation covariance likewise from nav_sigma_r_km / nav_sigma_v_ms
    (guided_nav; None: no navigation error).  nav_sigma_* and update_every may be arrays that broadcast together into the case
    list -- a whole table of settings costs one call.  n_guid resamples the solution as fly_guided does.  Returns a dict, every entry
    with the broadcast shape of the cases behind its own axes: sigma_r_km and sigma_v_ms [n x ...] (the trace RSS at every node),
    miss_r_km_rss and miss_v_ms_rss (the arrival node's), miss_r_km_max (the largest principal position sigma at arrival), P_final
    [6 x 6 x ...], P_nodes [6 x 6 x n x ...], cov_status (0 ok, 2 not finite: the case has no finite gains or inputs), gain_status,
    K, pivot, XC_guid, t_guid, update_every."""
    return _covariance_guided(6, ctx, XC_all, t_TU, prm, sigma_r_km, sigma_v_ms, None, n_guid, update_every, integ, nav_sigma_r_km,
                              nav_sigma_v_ms, None, sing_tol)


def covariance_guided_mass(ctx, XC_all, t_TU, prm, sigma_r_km, sigma_v_ms, n_guid=None, update_every=1, integ=None,
                           nav_sigma_r_km=None, nav_sigma_v_ms=None, sigma_m_kg=None, nav_sigma_m_kg=None, sing_tol=1e-10):
    """covariance_guided for a solution of the 14-row variable-mass system, the twin of dispersion_guided_mass: sigma_m_kg is the
    start mass's sigma and nav_sigma_m_kg the measured mass's (it broadcasts with the other case settings).  The dict gains
    sigma_m_kg [n x ...] and sigma_mf_kg (the final mass's sigma); P_final is [7 x 7 x ...]."""
    return _covariance_guided(7, ctx, XC_all, t_TU, prm, sigma_r_km, sigma_v_ms, sigma_m_kg, n_guid, update_every, integ,
                              nav_sigma_r_km, nav_sigma_v_ms, nav_sigma_m_kg, sing_tol)


def homotopy_solve(XC_all, t_TU, MU, DU, TU, mass, thrustLimit, rhos, p=1.0, maxIter=10, max_waves=12, ctx=None, verbose=True,
                   arcs=False):
    """Solve the whole smoothing ladder rho_0 > rho_1 > ... concurrently.  reduceFuel_indirect walks the
    ladder one level at a time, halving rho after each success (HelperFunctions.jl:158-188); here every unsolved level is
    one trajectory of a batched device Newton loop.  Wave 1 starts all levels from XC_all (a solution at or above
    rho_0); each later wave restarts the levels that failed from the converged solution of the nearest level with a
    larger rho.  Stops when every level has converged, a wave makes no progress, or after max_waves.

    Returns (XC_levels [12 x n x L], defect [12 x (n-1) x L], status [L] (0 converged, else the last status_flag of the
    level, 3 = never converged: HelperFunctions.jl:161), waves).  arcs=True: one more batched call (thrust_arcs) over the
    converged levels, returned as a fifth element -- a list with one dict per level, None where the level did not converge."""
    rhos = np.asarray(rhos, dtype=np.float64)
    order = np.argsort(-rhos)                                 # descending: neighbours in the list are neighbours in rho
    L = len(rhos)
    XC0 = np.array(XC_all, dtype=np.float64, order="F")
    n = XC0.shape[1]
    X = np.repeat(XC0[:, :, None], L, axis=2)
    D = np.full((12, n - 1, L), np.nan)
    status = np.full(L, 3, dtype=np.int32)
    solved = np.zeros(L, dtype=bool)
    waves = 0
    while not solved.all() and waves < max_waves:
        waves += 1
        todo = [k for k in order if not solved[k]]
        guess = np.empty((12, n, len(todo)), order="F")
        for j, k in enumerate(todo):                          # nearest converged level with a larger rho, else the input
            better = [q for q in order if solved[q] and rhos[q] > rhos[k]]
            guess[:, :, j] = X[:, :, better[-1]] if better else XC0
        prms = [hotpath.make_params(MU, DU, TU, thrustLimit, mass, 1.0, p, float(rhos[k])) for k in todo]
        Xo, Do, st, it, _ = hotpath.indirect_solve_batch(guess, t_TU, prms, None, False, maxIter, ctx=ctx)
        progress = 0
        for j, k in enumerate(todo):
            if st[j] == 0:
                X[:, :, k], D[:, :, k], status[k], solved[k] = Xo[:, :, j], Do[:, :, j], 0, True
                progress += 1
            elif status[k] == 3:
                D[:, :, k] = Do[:, :, j]
        if verbose:
            print("wave %d: %d of %d levels converged (%d remaining)" % (waves, progress, len(todo), int((~solved).sum())))
        if progress == 0:
            break
    if arcs:
        ok = [k for k in range(L) if solved[k]]
        level_arcs = [None] * L
        if ok:
            found = thrust_arcs(np.asfortranarray(X[:, :, ok]), t_TU, MU, DU, TU, mass, thrustLimit, p, rhos[ok], ctx=ctx)
            for k, a in zip(ok, found):
                level_arcs[k] = a
        return np.asfortranarray(X), np.asfortranarray(D), status, waves, level_arcs
    return np.asfortranarray(X), np.asfortranarray(D), status, waves


# ------------------------------------------------------------------------------------ periodic orbits
def libration_point(which, MU):
    """x of the collinear libration point L1 (which = 1 or 'L1') or L2 (2 or 'L2') of the CRTBP with mass ratio MU: the root of
    x - (1 - MU) (x + MU) / |x + MU|^3 - MU (x - 1 + MU) / |x - 1 + MU|^3 by Newton's method from the Hill-sphere estimate."""
    which = {1: 1, 2: 2, "L1": 1, "L2": 2}.get(which)
    if which is None:
        raise ValueError("which must be 1, 2, 'L1' or 'L2'")
    rh = (MU / 3.0) ** (1.0 / 3.0)
    x = 1.0 - MU - rh if which == 1 else 1.0 - MU + rh
    for _ in range(50):
        a, b = x + MU, x - 1.0 + MU
        f = x - (1.0 - MU) * a / abs(a) ** 3 - MU * b / abs(b) ** 3
        df = 1.0 + 2.0 * (1.0 - MU) / abs(a) ** 3 + 2.0 * MU / abs(b) ** 3
        dx = f / df
        x -= dx
        if abs(dx) < 1e-16:
            break
    return float(x)


def lyapunov_seed(which, Ax, MU):
    """The linear planar Lyapunov seed of x-amplitude Ax about L1 or L2: x0 = x_L - Ax, vy0 = k lam Ax with
    lam^2 = (2 - c2 + sqrt(9 c2^2 - 8 c2)) / 2, k = (lam^2 + 1 + 2 c2) / (2 lam), c2 = (1 - MU) / |x_L + MU|^3 + MU / |x_L - 1 + MU|^3.
    Returns (seed [6], the linear period 2 pi / lam)."""
    xL = libration_point(which, MU)
    c2 = (1.0 - MU) / abs(xL + MU) ** 3 + MU / abs(xL - 1.0 + MU) ** 3
    lam = np.sqrt((2.0 - c2 + np.sqrt(9.0 * c2 * c2 - 8.0 * c2)) / 2.0)
    k = (lam * lam + 1.0 + 2.0 * c2) / (2.0 * lam)
    return np.array([xL - Ax, 0.0, 0.0, 0.0, k * lam * Ax, 0.0]), float(2.0 * np.pi / lam)


HaloOrbit = collections.namedtuple("HaloOrbit", "times states state0 period jacobi nu M closure resid iterations status")
# tangent, det and ds are filled by the pseudo-arclength march (halo_family_arclength) and None otherwise
HaloFamily = collections.namedtuple("HaloFamily", "states period resid iterations status tangent det ds", defaults=(None, None, None))


def halo_orbit(seed, mode, n_samples=100, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """A periodic orbit from a rough symmetric seed [6], both steps on the device: correct it (hotpath.halo_correct; mode 'z0',
    'x0' or 'planar'), then sample one revolution (hotpath.halo_table).  Returns HaloOrbit: (times [n], states [6 x n]) ready for
    DirectOrbits, the corrected start, the period, the Jacobi constant (C, its largest drift over the samples), the stability
    indices, the monodromy matrix, the closure max |x(P) - x(0)|, the corrector's last residual and step count, and status: the
    corrector's (0 converged, 1 max_iter, 2 unusable, 3 singular) or, if that is 0, the table's (0 or 2).  The table of an orbit
    the corrector gave up on (status 2 or 3) is NaN."""
    MU = hotpath.MU if MU is None else MU
    c = hotpath.halo_correct(np.asarray(seed, dtype=np.float64).reshape(6), mode, tol=tol, max_iter=max_iter, t_max=t_max, MU=MU,
                             integ=integ, ctx=ctx)
    tb = hotpath.halo_table(c.state, c.period, n_samples, MU=MU, integ=integ, ctx=ctx)
    return HaloOrbit(tb.times, tb.X, c.state, c.period, tb.jacobi, tb.nu, tb.M, tb.closure, c.resid, c.iterations,
                     c.status if c.status else tb.status)


def halo_family(seed, values, hold="x0", tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """Natural-parameter continuation of a family of periodic orbits in the held coordinate (hold = 'x0' or 'z0'): member k has
    that coordinate = values[k]; its seed is the secant through the last two points of the march (the caller's seed counts as the
    first point, and the first member starts from the seed itself with the coordinate set), corrected on the device.  seed [6]
    with values [K], or seed [6 x F] with values [K] or [K x F]: the F families advance side by side, one device call per member
    index.  Returns HaloFamily(states [6 x K (x F)], period, resid, iterations, status [K (x F)]).  A member the corrector gives up
    on (status 2 or 3) is NaN and so is the rest of its family."""
    if hold not in ("x0", "z0"):
        raise ValueError("hold must be 'x0' or 'z0'")
    MU = hotpath.MU if MU is None else MU
    ip = 0 if hold == "x0" else 2
    S = np.asarray(seed, dtype=np.float64)
    batched = S.ndim == 2
    S = S.reshape(6, -1).copy()
    F = S.shape[1]
    V = np.asarray(values, dtype=np.float64)
    V = np.broadcast_to(V.reshape(V.shape[0], -1), (V.shape[0], F))
    K = V.shape[0]
    states = np.zeros((6, K, F))
    period, resid = np.zeros((K, F)), np.zeros((K, F))
    its, status = np.zeros((K, F), dtype=np.int32), np.zeros((K, F), dtype=np.int32)
    prev, cur = None, S
    for k in range(K):
        guess = cur.copy()
        if prev is not None:
            d = cur[ip] - prev[ip]
            ok = d != 0.0
            guess[:, ok] = cur[:, ok] + (cur[:, ok] - prev[:, ok]) * ((V[k, ok] - cur[ip, ok]) / d[ok])
        guess[ip] = V[k]
        c = hotpath.halo_correct(guess, hold, tol=tol, max_iter=max_iter, t_max=t_max, MU=MU, integ=integ, ctx=ctx)
        states[:, k], period[k], resid[k], its[k], status[k] = c.state, c.period, c.resid, c.iterations, c.status
        prev, cur = cur, np.array(c.state)
    if not batched:
        return HaloFamily(states[:, :, 0], period[:, 0], resid[:, 0], its[:, 0], status[:, 0])
    return HaloFamily(states, period, resid, its, status)


def halo_family_fill(members, k, hold="x0", tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """k new members between each neighbouring pair of members [6 x K] of a family: the seeds are the pair's linear interpolants
    at j / (k + 1), j = 1..k, and all (K - 1) k of them are corrected in ONE device call with the interpolated coordinate `hold`
    kept.  Returns hotpath.HaloCorrect over the new members in the order of the family."""
    if hold not in ("x0", "z0"):
        raise ValueError("hold must be 'x0' or 'z0'")
    Mb = np.asarray(members, dtype=np.float64)
    if Mb.ndim != 2 or Mb.shape[0] != 6 or Mb.shape[1] < 2 or int(k) < 1:
        raise ValueError("members must be [6 x K] with K >= 2, and k >= 1")
    k = int(k)
    w = np.arange(1, k + 1) / (k + 1.0)
    seeds = np.concatenate([Mb[:, [i]] * (1.0 - w) + Mb[:, [i + 1]] * w for i in range(Mb.shape[1] - 1)], axis=1)
    return hotpath.halo_correct(seeds, hold, tol=tol, max_iter=max_iter, t_max=t_max, MU=hotpath.MU if MU is None else MU, integ=integ,
                                ctx=ctx)


ManifoldArcs = collections.namedtuple("ManifoldArcs", "branch tau start x_end t_end count dC status lam seeds")
ManifoldConnection = collections.namedtuple(
    "ManifoldConnection", "dist dr_km dv_ms tau1 tau2 branch1 branch2 t1 t2 x1 x2 start1 start2 MU")
_MANIFOLD_BRANCHES = ("u+", "u-", "s+", "s-")


def _orbit_parts(orbit):
    """(state0 [6], period, M [6 x 6]) of what halo_orbit returns, or of such a tuple."""
    if isinstance(orbit, HaloOrbit):
        return np.asarray(orbit.state0, dtype=np.float64), float(orbit.period), np.asarray(orbit.M, dtype=np.float64)
    try:
        state0, period, M = orbit
    except (TypeError, ValueError):
        raise ValueError("orbit must be what halo_orbit returns, or (state0, period, M)")
    state0, M = np.asarray(state0, dtype=np.float64), np.asarray(M, dtype=np.float64)
    if state0.shape != (6,) or M.shape != (6, 6):
        raise ValueError("orbit must be what halo_orbit returns, or (state0 [6], period, M [6 x 6])")
    return state0, float(period), M


def _branch_list(branches):
    if not isinstance(branches, str) or len(branches) % 2 or not branches:
        raise ValueError("branches must be a string made of 'u+', 'u-', 's+', 's-'")
    out = [branches[i:i + 2] for i in range(0, len(branches), 2)]
    if any(b not in _MANIFOLD_BRANCHES for b in out) or len(set(out)) != len(out):
        raise ValueError("branches must be a string made of 'u+', 'u-', 's+', 's-', each at most once")
    return out


def halo_manifold(orbit, n_phase, eps=1e-6, branches="u+u-s+s-", section=None, n_cross=1, t_max=12.0, r_min=(0.0, 0.0), MU=None,
                  integ=None, ctx=None):
    """The invariant-manifold tubes of a periodic orbit flown to a Poincare section, in two library calls: the
    eigen-directions and perturbed starts at the phases j / n_phase (hotpath.manifold_seeds), then one flight call for all selected
    arcs (hotpath.section_flight) -- unstable arcs forward over t_max TU, stable arcs backward.  orbit: what halo_orbit returns, or
    (state0, period, M); branches: which of 'u+', 'u-', 's+', 's-' fly ('+': the side with v_x(0) > 0, the exterior one at L2);
    section = (axis, value), default x = 1 - MU.  Returns ManifoldArcs of N = n_phase x len(branches) arcs, phase by phase: branch
    [N], tau [N], start [6 x N], x_end [6 x N], t_end [N] (signed), count [N], dC [N], status [N] (section_flight's), lam =
    (lambda_u, lambda_s) and seeds, the hotpath.ManifoldSeeds record.  A seed status other than 0 raises ValueError."""
    MU = hotpath.MU if MU is None else MU
    state0, period, M = _orbit_parts(orbit)
    names = _branch_list(branches)
    n_phase = int(n_phase)
    if n_phase < 1:
        raise ValueError("n_phase must be >= 1")
    section = ("x", 1.0 - MU) if section is None else section
    tau = np.arange(n_phase) / float(n_phase)
    seeds = hotpath.manifold_seeds(state0, period, M, tau, eps=eps, MU=MU, integ=integ, ctx=ctx)
    if seeds.status != 0:
        raise ValueError("the orbit has no usable hyperbolic pair (status %d of manifold_seeds)" % seeds.status)
    which = [_MANIFOLD_BRANCHES.index(b) for b in names]
    start = np.asfortranarray(seeds.starts[:, which, :].transpose(0, 2, 1).reshape(6, -1, order="C"))      # arc = phase * nb + branch
    branch = np.array(names * n_phase)
    T = np.where(np.char.startswith(branch, "u"), abs(float(t_max)), -abs(float(t_max)))
    fl = hotpath.section_flight(start, T, section=section, sec_dir=0, n_cross=n_cross, r_min=r_min, MU=MU, integ=integ, ctx=ctx)
    return ManifoldArcs(branch, np.repeat(tau, len(names)), start, fl.x_end, fl.t_end, fl.count, fl.dC, fl.status, seeds.lam, seeds)


def manifold_connections(dep, arr, section=None, n_phase=64, eps=1e-6, n_cross=1, t_max=12.0, r_min=(0.0, 0.0), w=1.0, k=10, MU=None,
                         DU=None, TU=None, integ=None, ctx=None):
    """Where the unstable manifold of `dep` and the stable manifold of `arr` come close on a section: both tubes by halo_manifold
    (n_phase phases each, both branches), every departure arc that reached the section matched to its nearest arrival arc by one
    hotpath.state_match call in d = sqrt(|dr|^2 + (w |dv|)^2), and the k best pairs by increasing distance.  Returns a list of
    ManifoldConnection(dist, dr_km, dv_ms, tau1, tau2 (the phases on the two orbits), branch1, branch2, t1 > 0, t2 < 0 (the flight
    times to the section, TU), x1, x2 (the two states on the section), start1, start2 (the arcs' starts), MU)."""
    from .constants import DU as DU0, TU as TU0
    MU = hotpath.MU if MU is None else MU
    DU, TU = DU0 if DU is None else DU, TU0 if TU is None else TU
    a = halo_manifold(dep, n_phase, eps=eps, branches="u+u-", section=section, n_cross=n_cross, t_max=t_max, r_min=r_min, MU=MU,
                      integ=integ, ctx=ctx)
    b = halo_manifold(arr, n_phase, eps=eps, branches="s+s-", section=section, n_cross=n_cross, t_max=t_max, r_min=r_min, MU=MU,
                      integ=integ, ctx=ctx)
    A = np.where(a.status == 0, a.x_end, np.nan)
    Bs = np.where(b.status == 0, b.x_end, np.nan)
    m = hotpath.state_match(A, Bs, w=w, ctx=ctx)
    order = [i for i in np.argsort(m.dist, kind="stable") if m.index[i] >= 0][:int(k)]
    out = []
    for i in order:
        j = int(m.index[i])
        out.append(ManifoldConnection(float(m.dist[i]), float(m.dr[i]) * DU, float(m.dv[i]) * DU / TU * 1e3, float(a.tau[i]),
                                      float(b.tau[j]), str(a.branch[i]), str(b.branch[j]), float(a.t_end[i]), float(b.t_end[j]),
                                      a.x_end[:, i].copy(), b.x_end[:, j].copy(), a.start[:, i].copy(), b.start[:, j].copy(), MU))
    return out


def manifold_guess(connection, n_nodes, integ=None, ctx=None):
    """A connection of manifold_connections as an initial guess: both arcs flown again with samples (hotpath.section_flight with
    n_cross = 0 and t_max = their crossing times) and stitched in flight order -- departure point, section, arrival point; the nodes
    are shared out in proportion to the two flight times and the section is represented by the departure arc's end alone.  Returns
    (X [6 x n_nodes], t_TU, tau1, tau2), the tuple stacked_guess returns."""
    c = connection
    n_nodes = int(n_nodes)
    if n_nodes < 4:
        raise ValueError("n_nodes must be >= 4")
    t1, t2 = float(c.t1), abs(float(c.t2))
    n1 = min(max(int(round(n_nodes * t1 / (t1 + t2))), 2), n_nodes - 2)
    n2 = n_nodes - n1
    f1 = hotpath.section_flight(c.start1, t1, n_cross=0, n_samples=n1, MU=c.MU, integ=integ, ctx=ctx)
    f2 = hotpath.section_flight(c.start2, -t2, n_cross=0, n_samples=n2 + 1, MU=c.MU, integ=integ, ctx=ctx)
    X = np.asfortranarray(np.concatenate([f1.X, f2.X[:, ::-1][:, 1:]], axis=1))
    s2 = np.arange(n2 + 1) * (t2 / n2)
    s2[-1] = t2
    t = np.concatenate([np.arange(n1) * (t1 / (n1 - 1)), t1 + (t2 - s2[::-1][1:])])
    t[n1 - 1] = t1
    return X, t, c.tau1, c.tau2


# ------------------------------------------------------------------------------------ orbits at a given C or period
def _one_target(jacobi, period):
    """('jacobi' | 'period', value): exactly one of the two must be given."""
    if (jacobi is None) == (period is None):
        raise ValueError("give exactly one of jacobi and period")
    return ("jacobi", float(jacobi)) if period is None else ("period", float(period))


def _jacobi_of(state, MU):
    """The Jacobi constant of states [6 (x F)] in numpy."""
    x, y, z, vx, vy, vz = np.asarray(state, dtype=np.float64)
    r1 = np.sqrt((x + MU) ** 2 + y * y + z * z)
    r2 = np.sqrt((x + MU - 1.0) ** 2 + y * y + z * z)
    return x * x + y * y + 2.0 * (1.0 - MU) / r1 + 2.0 * MU / r2 - (vx * vx + vy * vy + vz * vz)


def _step_table(start, end, n_steps):
    """[n_steps x F]: row k = start + (end - start) (k + 1) / n_steps, the last row `end` itself."""
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError("n_steps must be >= 1")
    start = np.asarray(start, dtype=np.float64).reshape(-1)
    end = np.broadcast_to(np.asarray(end, dtype=np.float64).reshape(-1), start.shape)
    tab = start[None, :] + (end - start)[None, :] * (np.arange(1, n_steps + 1) / float(n_steps))[:, None]
    tab[-1] = end
    return tab


def halo_orbit_at(seed, jacobi=None, period=None, planar=False, n_samples=100, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None,
                  ctx=None):
    """A periodic orbit of a prescribed Jacobi constant or a prescribed period from a symmetric seed [6], both steps on the device:
    the targeted corrector (hotpath.halo_target), then one revolution sampled (hotpath.halo_table).  Exactly one of jacobi and period
    must be given.  Returns HaloOrbit as halo_orbit does."""
    what, q = _one_target(jacobi, period)
    MU = hotpath.MU if MU is None else MU
    c = hotpath.halo_target(np.asarray(seed, dtype=np.float64).reshape(6), q, what=what, planar=planar, tol=tol, max_iter=max_iter,
                            t_max=t_max, MU=MU, integ=integ, ctx=ctx)
    tb = hotpath.halo_table(c.state, c.period, n_samples, MU=MU, integ=integ, ctx=ctx)
    return HaloOrbit(tb.times, tb.X, c.state, c.period, tb.jacobi, tb.nu, tb.M, tb.closure, c.resid, c.iterations,
                     c.status if c.status else tb.status)


def halo_family_by(seed, values, what, planar=False, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """A family of periodic orbits parametrised by the Jacobi constant (what = 'jacobi') or the period ('period'): member k has that
    quantity = values[k], its start the secant through the last two members in the value -- the whole march in ONE device call
    (hotpath.halo_target).  seed [6] with values [K], or seed [6 x F] with values [K] or [K x F]: the F families advance side by
    side.  Returns HaloFamily(states [6 x K (x F)], period, resid, iterations, status [K (x F)]).  A member the corrector gives up on
    (status 2 or 3) is NaN and so is the rest of its family."""
    V = np.asarray(values, dtype=np.float64)
    if V.ndim < 1:
        raise ValueError("values must be [K] or [K x F]")
    c = hotpath.halo_target(seed, V, what=what, planar=planar, tol=tol, max_iter=max_iter, t_max=t_max,
                            MU=hotpath.MU if MU is None else MU, integ=integ, ctx=ctx)
    return HaloFamily(c.state, c.period, c.resid, c.iterations, c.status)


def matched_orbits(seeds, jacobi, n_steps=8, planar=False, n_samples=100, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None,
                   ctx=None):
    """Several periodic orbits brought to ONE Jacobi constant in one device call: orbit f of seeds [6 x F] (corrected orbits, as
    halo_correct returns them) marches from its own C to `jacobi` in n_steps equal steps (hotpath.halo_target), then all F are
    sampled in one hotpath.halo_table call.  Returns a list of F HaloOrbit; `iterations` counts the last member's Newton steps and
    `status` is that member's, or the table's."""
    MU = hotpath.MU if MU is None else MU
    S = np.asarray(seeds, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != 6 or S.shape[1] < 1:
        raise ValueError("seeds must be [6 x F]")
    if not np.isfinite(float(jacobi)):
        raise ValueError("jacobi must be finite")
    steps = _step_table(_jacobi_of(S, MU), float(jacobi), n_steps)
    c = hotpath.halo_target(S, steps, what="jacobi", planar=planar, tol=tol, max_iter=max_iter, t_max=t_max, MU=MU, integ=integ, ctx=ctx)
    state, period = np.asfortranarray(c.state[:, -1, :]), np.ascontiguousarray(c.period[-1])
    tb = hotpath.halo_table(state, period, n_samples, MU=MU, integ=integ, ctx=ctx)
    return [HaloOrbit(tb.times, tb.X[:, :, f], state[:, f], float(period[f]), tb.jacobi[:, f], tb.nu[:, f], tb.M[:, :, f],
                      float(tb.closure[f]), float(c.resid[-1, f]), int(c.iterations[-1, f]),
                      int(c.status[-1, f]) if c.status[-1, f] else int(tb.status[f])) for f in range(S.shape[1])]


def _refine_phases(centre, half_width, n_phase):
    """The n_phase phases of one refinement level: equally spaced over centre -+ half_width, both ends included."""
    return centre + half_width * np.linspace(-1.0, 1.0, int(n_phase))


def _refine_shrink(half_width, n_phase):
    """The next level's half width: the window shrinks by n_phase / 2."""
    return half_width / (0.5 * int(n_phase))


def manifold_connection_refine(dep, arr, connection, levels=4, n_phase=16, spacing=1.0 / 64.0, eps=1e-6, section=None, n_cross=1,
                               t_max=12.0, r_min=(0.0, 0.0), w=1.0, MU=None, DU=None, TU=None, integ=None, ctx=None):
    """Zoom in on a pair manifold_connections found.  `spacing` is the phase spacing of the search that found it (1 / its n_phase).
    Each level takes n_phase phases within -+ one previous spacing of (tau1, tau2) on the pair's two branches only -- one
    hotpath.manifold_seeds call for both orbits with the explicit phases, one section_flight call for the 2 n_phase arcs, one
    state_match call -- the best pair becomes the next centre and the window shrinks by n_phase / 2.  A level that finds nothing
    closer keeps its centre, so the distance never grows.  Returns the list of ManifoldConnection, one per level."""
    from .constants import DU as DU0, TU as TU0
    c = connection
    MU = c.MU if MU is None else MU
    DU, TU = DU0 if DU is None else DU, TU0 if TU is None else TU
    levels, n_phase = int(levels), int(n_phase)
    if levels < 1 or n_phase < 3:
        raise ValueError("need levels >= 1 and n_phase >= 3")
    if c.branch1 not in ("u+", "u-") or c.branch2 not in ("s+", "s-"):
        raise ValueError("connection must pair an unstable branch of dep with a stable branch of arr")
    parts = [_orbit_parts(dep), _orbit_parts(arr)]
    state0 = np.asfortranarray(np.array([p[0] for p in parts]).T)
    period = np.array([p[1] for p in parts])
    M = np.asfortranarray(np.stack([p[2] for p in parts], axis=2))
    section = ("x", 1.0 - MU) if section is None else section
    i1, i2 = _MANIFOLD_BRANCHES.index(c.branch1), _MANIFOLD_BRANCHES.index(c.branch2)
    T = np.concatenate([np.full(n_phase, abs(float(t_max))), np.full(n_phase, -abs(float(t_max)))])
    best, tau1, tau2, h = c, float(c.tau1), float(c.tau2), float(spacing)
    out = []
    for _ in range(levels):
        p1, p2 = _refine_phases(tau1, h, n_phase), _refine_phases(tau2, h, n_phase)
        seeds = hotpath.manifold_seeds(state0, period, M, np.concatenate([p1, p2]), eps=eps, MU=MU, integ=integ, ctx=ctx)
        if np.any(seeds.status != 0):
            raise ValueError("an orbit has no usable hyperbolic pair (status %s of manifold_seeds)" % list(seeds.status))
        start = np.asfortranarray(np.concatenate([seeds.starts[:, i1, :n_phase, 0], seeds.starts[:, i2, n_phase:, 1]], axis=1))
        fl = hotpath.section_flight(start, T, section=section, sec_dir=0, n_cross=n_cross, r_min=r_min, MU=MU, integ=integ, ctx=ctx)
        ends = np.where(fl.status == 0, fl.x_end, np.nan)
        m = hotpath.state_match(ends[:, :n_phase], ends[:, n_phase:], w=w, ctx=ctx)
        ok = [i for i in range(n_phase) if m.index[i] >= 0]
        if ok:
            i = min(ok, key=lambda q: m.dist[q])
            j = int(m.index[i])
            if m.dist[i] < best.dist:
                best = ManifoldConnection(float(m.dist[i]), float(m.dr[i]) * DU, float(m.dv[i]) * DU / TU * 1e3, float(seeds.tau[i]),
                                          float(seeds.tau[n_phase + j]), c.branch1, c.branch2, float(fl.t_end[i]),
                                          float(fl.t_end[n_phase + j]), fl.x_end[:, i].copy(), fl.x_end[:, n_phase + j].copy(),
                                          start[:, i].copy(), start[:, n_phase + j].copy(), MU)
                tau1, tau2 = float(p1[i]), float(p2[j])
        out.append(best)
        h = _refine_shrink(h, n_phase)
    return out


# ------------------------------------------------------------------------------------ families by pseudo-arclength
HaloBranchPoint = collections.namedtuple("HaloBranchPoint", "state tangent det period jacobi s trials status")
HaloBranch = collections.namedtuple("HaloBranch", "family branch_point lyapunov table")


def halo_family_arclength(seed, n_members, ds, direction, planar=False, tangent=None, ds_min=None, ds_max=None, grow=1.0, fast_iter=3,
                          cos_min=0.0, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """A family of periodic orbits followed along its own tangent in (x0, z0, vy0), the whole march with its step control in ONE
    device call (hotpath.halo_arclength): it passes the folds of x0, z0, vy0, C and P that stop halo_family and halo_family_by.
    seed [6] or [6 x F] (the F families advance side by side).  Without `tangent` member 0 is the seed corrected onto the family and
    the march leaves it towards `direction` [3] or [3 x F]; with `tangent` [3] or [3 x F] the seed is a point of the family, member
    0 the step of ds from it along that tangent, and `direction` is not read (pass None).  Returns HaloFamily(states
    [6 x K (x F)], period, resid, iterations, status, tangent [3 x K (x F)], det, ds [K (x F)])."""
    mode1 = tangent is not None
    if not mode1 and direction is None:
        raise ValueError("give a direction [3] to leave the seed along, or the seed's tangent")
    c = hotpath.halo_arclength(seed, n_members, ds, tangent if mode1 else direction, planar=planar, dir_is_tangent=mode1, ds_min=ds_min,
                               ds_max=ds_max, grow=grow, fast_iter=fast_iter, cos_min=cos_min, tol=tol, max_iter=max_iter, t_max=t_max,
                               MU=hotpath.MU if MU is None else MU, integ=integ, ctx=ctx)
    return HaloFamily(c.state, c.period, c.resid, c.iterations, c.status, c.tangent, c.det, c.ds)


def _sign_changes(v):
    """The indices k >= 1 with v[k] v[k - 1] < 0 (a NaN on either side is no change)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return [int(k) for k in np.nonzero(v[1:] * v[:-1] < 0.0)[0] + 1]


def family_bifurcations(fam):
    """The members k of one family (HaloFamily of halo_family_arclength, no family axis) with det_k det_(k-1) < 0: between members
    k - 1 and k another family branches off."""
    if fam.det is None or np.ndim(fam.det) != 1:
        raise ValueError("fam must be one family marched by halo_family_arclength")
    return _sign_changes(fam.det)


def family_folds(fam):
    """Per unknown, the members k of one family where that component of the tangent changes sign: {'x0': [...], 'z0': [...],
    'vy0': [...]} -- the coordinate has an extremum between members k - 1 and k."""
    if fam.tangent is None or np.ndim(fam.tangent) != 2:
        raise ValueError("fam must be one family marched by halo_family_arclength")
    return {name: _sign_changes(fam.tangent[j]) for j, name in enumerate(("x0", "z0", "vy0"))}


def _secant_next(s0, d0, s1, d1):
    """The zero of the line through (s0, d0) and (s1, d1)."""
    return s1 - d1 * (s1 - s0) / (d1 - d0)


def halo_branch_point(fam, k, planar=False, max_trials=8, rel=1e-9, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """The point between members k - 1 and k of one family (k from family_bifurcations) where det = 0: a secant in the arclength s
    from member k - 1 on det(s), every trial a one-member call from member k - 1 along its tangent; it stops at |det| < rel
    |det_(k-1)| or after max_trials.  Returns HaloBranchPoint(state, tangent, det, period, jacobi, s, trials [(s, det)], status of
    the last trial)."""
    k = int(k)
    if fam.det is None or np.ndim(fam.det) != 1 or not 1 <= k < fam.det.shape[0]:
        raise ValueError("fam must be one family marched by halo_family_arclength and 1 <= k < its length")
    if not fam.det[k] * fam.det[k - 1] < 0.0:
        raise ValueError("det does not change sign between members k - 1 and k")
    MU = hotpath.MU if MU is None else MU
    s0, d0, s1, d1 = 0.0, float(fam.det[k - 1]), float(fam.ds[k]), float(fam.det[k])
    trials, m, s = [], None, s1
    for _ in range(int(max_trials)):
        s = _secant_next(s0, d0, s1, d1)
        if not (np.isfinite(s) and s > 0.0):
            break
        m = hotpath.halo_arclength(fam.states[:, k - 1], 1, s, fam.tangent[:, k - 1], planar=planar, dir_is_tangent=True, ds_min=s, ds_max=s,
                                   tol=tol, max_iter=max_iter, t_max=t_max, MU=MU, integ=integ, ctx=ctx)
        if m.status[0] != 0:
            break
        trials.append((s, float(m.det[0])))
        if abs(m.det[0]) < rel * abs(fam.det[k - 1]):
            break
        s0, d0, s1, d1 = s1, d1, s, float(m.det[0])
    if m is None:
        raise ValueError("the secant left the interval at its first trial")
    return HaloBranchPoint(m.state[:, 0], m.tangent[:, 0], float(m.det[0]), float(m.period[0]), float(m.jacobi[0]), float(s), trials,
                           int(m.status[0]))


def halo_from_lyapunov(which, n_members, ds, north=True, Ax=1e-2, ds_switch=1e-2, ds_lyapunov=1e-2, block=16, max_blocks=16, n_samples=0,
                       grow=1.0, tol=1e-12, max_iter=15, t_max=10.0, MU=None, integ=None, ctx=None):
    """A halo family from the mass ratio alone: the linear Lyapunov seed of x-amplitude Ax about L1 or L2 (lyapunov_seed), the planar
    corrector, the planar family in the 3-unknown form (z0 = 0) towards larger orbits in blocks of `block` members of step
    ds_lyapunov until det changes sign, the branch point (halo_branch_point), one step of ds_switch off the plane along (0, +1, 0)
    (north) or (0, -1, 0), and n_members members of step ds up the halo family (a step the kernel had to halve grows back by `grow`
    up to ds).  n_samples > 0: one hotpath.halo_table call for all members.  Returns HaloBranch(family: HaloFamily whose member 0 is
    the step off the plane, branch_point: HaloBranchPoint, lyapunov: the planar family's last block as HaloFamily, table: HaloTable
    or None)."""
    MU = hotpath.MU if MU is None else MU
    kw = dict(tol=tol, max_iter=max_iter, t_max=t_max, MU=MU, integ=integ, ctx=ctx)
    seed, _ = lyapunov_seed(which, Ax, MU)
    c = hotpath.halo_correct(seed, "planar", **kw)
    if c.status != 0:
        raise ValueError("the planar corrector gave up on the Lyapunov seed (status %d)" % c.status)
    fam = halo_family_arclength(c.state, block, ds_lyapunov, [0.0, 0.0, 1.0 if c.state[4] > 0.0 else -1.0], **kw)
    for _ in range(int(max_blocks)):
        if np.any(fam.status != 0):
            raise ValueError("the planar family ended before a bifurcation (statuses %s)" % list(fam.status))
        flips = family_bifurcations(fam)
        if flips:
            break
        nxt = halo_family_arclength(fam.states[:, -1], block, float(fam.ds[-1]) if fam.ds[-1] > 0.0 else ds_lyapunov, None,
                                    tangent=fam.tangent[:, -1], **kw)
        # the last member of the block before leads the new one, so that a sign change across the seam is seen
        fam = HaloFamily(*[np.concatenate([np.asarray(a)[..., -1:], np.asarray(b)], axis=-1) for a, b in zip(fam, nxt)])
    else:
        raise ValueError("no bifurcation within %d blocks of %d members" % (int(max_blocks), int(block)))
    bp = halo_branch_point(fam, flips[0], **kw)
    if bp.status != 0:
        raise ValueError("the branch point's last trial has status %d" % bp.status)
    sw = halo_family_arclength(bp.state, 1, ds_switch, None, tangent=[0.0, 1.0 if north else -1.0, 0.0], **kw)
    if sw.status[0] != 0:
        raise ValueError("the step off the plane has status %d" % sw.status[0])
    up = halo_family_arclength(sw.states[:, 0], n_members, ds, None, tangent=sw.tangent[:, 0], grow=grow, ds_max=ds, **kw)
    family = HaloFamily(*[np.concatenate([np.asarray(a), np.asarray(b)], axis=-1) for a, b in zip(sw, up)])
    table = None
    if int(n_samples) > 0:
        table = hotpath.halo_table(np.asfortranarray(family.states), np.ascontiguousarray(family.period), int(n_samples), MU=MU,
                                   integ=integ, ctx=ctx)
    return HaloBranch(family, bp, fam, table)


# ------------------------------------------------------------------------------------------- station-keeping
StationGains = collections.namedtuple("StationGains", "tau X_ref dt G W alpha lam")
YEAR_DAYS = 365.25


def stationkeep_spans(tau, period):
    """dt [n_man]: the ballistic span after the burn at phase tau_j, ((tau_{j+1} - tau_j) mod 1) P, the wrap-round span from the
    last phase to the first one of the next revolution last.  tau [n_man] in [0, 1), strictly increasing; one phase: dt = P."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    if tau.size < 1 or not np.all(np.isfinite(tau)) or np.any(tau < 0.0) or np.any(tau >= 1.0) or np.any(np.diff(tau) <= 0.0):
        raise ValueError("the burn phases must lie in [0, 1) and increase strictly")
    d = np.mod(np.roll(tau, -1) - tau, 1.0)
    if tau.size == 1:
        d[0] = 1.0
    return d * float(period)


def stationkeeping_gains(orbit, taus=None, n_man=4, sing_tol=1e-8, MU=None, integ=None, ctx=None):
    """The Floquet-mode station-keeping law of a periodic orbit in two library calls: the hyperbolic directions at
    the burn phases (hotpath.manifold_seeds), then the gains (hotpath.stationkeep_gains).  orbit: what halo_orbit returns, or
    (state0, period, M); taus [n_man] the burn phases (any finite values, wrapped into [0, 1), increasing after the wrap), default j
    / n_man.  Returns StationGains(tau [n_man] as wrapped, X_ref [6 x n_man] the orbit point at each phase as the stable vector's
    flight reached it, dt [n_man] the span after each burn (stationkeep_spans), G [3 x 6 x n_man], W [6 x n_man], alpha [n_man],
    lam = (lambda_u, lambda_s)).  A seeds or gains status other than 0 raises ValueError."""
    MU = hotpath.MU if MU is None else MU
    state0, period, M = _orbit_parts(orbit)
    if taus is None:
        n_man = int(n_man)
        if n_man < 1:
            raise ValueError("n_man must be >= 1")
        taus = np.arange(n_man) / float(n_man)
    seeds = hotpath.manifold_seeds(state0, period, M, taus, MU=MU, integ=integ, ctx=ctx)
    if seeds.status != 0:
        raise ValueError("the orbit has no usable hyperbolic pair (status %d of manifold_seeds)" % seeds.status)
    dt = stationkeep_spans(seeds.tau, period)
    g = hotpath.stationkeep_gains(seeds.V, sing_tol, ctx=ctx)
    if np.any(g.status != 0):
        raise ValueError("no usable gain at phase(s) %s (statuses %s of stationkeep_gains)"
                         % (list(seeds.tau[g.status != 0]), list(g.status[g.status != 0])))
    return StationGains(seeds.tau, np.asfortranarray(seeds.X[:, 1, :]), dt, g.G, g.W, g.alpha, seeds.lam)


def target_point_gains(orbit, taus=None, n_man=4, horizons=(0.5, 1.0), q=1e-2, weights=None, sing_tol=1e-12, MU=None, integ=None,
                       ctx=None):
    """The target-point station-keeping law of a periodic orbit in two library calls: the state-transition matrices
    from every burn phase to its targets (hotpath.halo_stm), then the gains (hotpath.stationkeep_target_gains).  The law needs no
    hyperbolic pair, so it also serves orbits manifold_seeds refuses.  orbit: what halo_orbit returns, or (state0, period, M) (M is not read);
    taus [n_man] the burn phases (any finite values, wrapped into [0, 1), increasing after the wrap), default j / n_man; horizons
    [K] the targets in periods after each burn; q the weight of |dv|^2 and weights [K] those of the position deviation at each
    target (default ones), in DU and DU/TU.  Returns StationGains(tau [n_man] as wrapped, X_ref [6 x n_man] the orbit point at each
    phase, dt [n_man] the span after each burn (stationkeep_spans), G [3 x 6 x n_man], W = alpha = lam = None), which
    stationkeep(..., gains=...) flies as it is.  An STM or gains status other than 0 raises ValueError."""
    MU = hotpath.MU if MU is None else MU
    state0, period = _orbit_parts(orbit)[:2]
    if taus is None:
        n_man = int(n_man)
        if n_man < 1:
            raise ValueError("n_man must be >= 1")
        taus = np.arange(n_man) / float(n_man)
    stm = hotpath.halo_stm(state0, period, taus, horizons, MU=MU, integ=integ, ctx=ctx)
    if np.any(stm.status != 0):
        raise ValueError("no state-transition matrix at phase(s) %s (status 2 of halo_stm)" % list(stm.tau[stm.status != 0]))
    dt = stationkeep_spans(stm.tau, period)
    g = hotpath.stationkeep_target_gains(stm.Phi, q, weights, sing_tol, ctx=ctx)
    if np.any(g.status != 0):
        raise ValueError("no usable gain at phase(s) %s (statuses %s of stationkeep_target_gains)"
                         % (list(stm.tau[g.status != 0]), list(g.status[g.status != 0])))
    return StationGains(stm.tau, np.asfortranarray(stm.X), dt, g.G, None, None, None)


def stationkeep_draws(n_runs, n_upd, inj_sigma_r_km, inj_sigma_v_ms, nav_sigma_r_km, nav_sigma_v_ms, exe_sigma_frac, exe_sigma_ms,
                      seed, DU, TU):
    """The error draws of a station-keeping Monte Carlo from numpy.random.default_rng(seed), always in the order injection,
    navigation, execution, so that a stream does not move when another sigma changes: inj [6 x n_runs] (Gaussian, sigma per
    position axis in km and per velocity axis in m/s), nav [6 x n_upd x n_runs] (the same units, added to the measured deviation
    at every update), exe [4 x n_upd x n_runs] (row 0 the relative magnitude error of sigma exe_sigma_frac, rows 1:4 a bias of
    exe_sigma_ms m/s per axis).  Every run is disturbed: there is no nominal run 0 as in dispersion_starts, a run on the orbit
    itself says nothing about keeping it.  nav is None when both its sigmas are None, exe likewise; a single None counts as 0."""
    n, m = int(n_runs), int(n_upd)
    if n < 1 or m < 1:
        raise ValueError("n_runs and n_upd must be >= 1")
    pos, vel = 1.0 / DU, 1e-3 * TU / DU
    rng = np.random.default_rng(seed)
    inj = rng.standard_normal((6, n))
    nav = rng.standard_normal((6, m, n))
    exe = rng.standard_normal((4, m, n))
    inj[0:3] *= float(inj_sigma_r_km) * pos
    inj[3:6] *= float(inj_sigma_v_ms) * vel
    if nav_sigma_r_km is None and nav_sigma_v_ms is None:
        nav = None
    else:
        nav[0:3] *= float(nav_sigma_r_km or 0.0) * pos
        nav[3:6] *= float(nav_sigma_v_ms or 0.0) * vel
        nav = np.asfortranarray(nav)
    if exe_sigma_frac is None and exe_sigma_ms is None:
        exe = None
    else:
        exe[0] *= float(exe_sigma_frac or 0.0)
        exe[1:4] *= float(exe_sigma_ms or 0.0) * vel
        exe = np.asfortranarray(exe)
    return np.asfortranarray(inj), nav, exe


def stationkeep(orbit, n_rev, n_runs, inj_sigma_r_km=1.0, inj_sigma_v_ms=0.01, nav_sigma_r_km=None, nav_sigma_v_ms=None,
                exe_sigma_frac=None, exe_sigma_ms=None, n_man=4, taus=None, dv_min_ms=0.0, dv_max_ms=0.0, r_lost_km=0.0, seed=0,
                DU=None, TU=None, MU=None, integ=None, gains=None, ctx=None):
    """Monte-Carlo station-keeping cost of a periodic orbit: n_runs runs injected at the first burn phase with
    Gaussian errors (stationkeep_draws), flown for n_rev revolutions of n_man burns each under the Floquet-mode
    law of stationkeeping_gains -- or under `gains`, any StationGains (one with G = 0 flies uncontrolled) -- in ONE flight call
    (hotpath.stationkeep_flight).  dv_min_ms the dead band, dv_max_ms the largest burn (0: none), r_lost_km the position deviation
    that ends a run as lost (0: never).  Returns a dict: dv_ms [n_runs] the summed |dv|, t_days [n_runs] the time flown (to the
    loss for a lost run), dv_per_year_ms = dv_ms per 365.25 days of t_days, n_burn, dev_r_km and dev_v_ms [n_upd x n_runs] the
    deviation at every update, dv_hist_ms [n_upd x n_runs], dev_final_r_km, dev_final_v_ms, x_final, status, lost_at, lost_share,
    gains, x0, nav, exe and, over the runs of status 0, percentiles = {"dv_ms": {50: .., 95: .., 99: ..}, "dv_per_year_ms": {..},
    "dev_r_km": {..}, "dev_v_ms": {..}} (the last two of each run's largest deviation)."""
    from .constants import DU as DU0, TU as TU0
    DU, TU = DU0 if DU is None else float(DU), TU0 if TU is None else float(TU)
    MU = hotpath.MU if MU is None else MU
    n_rev, n_runs = int(n_rev), int(n_runs)
    if n_rev < 1 or n_runs < 1:
        raise ValueError("n_rev and n_runs must be >= 1")
    g = stationkeeping_gains(orbit, taus, n_man, MU=MU, integ=integ, ctx=ctx) if gains is None else gains
    X_ref = np.asarray(g.X_ref, dtype=np.float64)
    dt = np.asarray(g.dt, dtype=np.float64).reshape(-1)
    if X_ref.ndim != 2 or X_ref.shape != (6, dt.size):
        raise ValueError("gains must be a StationGains of one orbit: X_ref [6 x n_man], dt [n_man], G [3 x 6 x n_man]")
    n_upd = n_rev * dt.size
    inj, nav, exe = stationkeep_draws(n_runs, n_upd, inj_sigma_r_km, inj_sigma_v_ms, nav_sigma_r_km, nav_sigma_v_ms, exe_sigma_frac,
                                      exe_sigma_ms, seed, DU, TU)
    x0 = np.asfortranarray(X_ref[:, :1] + inj)
    km, ms = DU, DU / TU * 1e3
    r = hotpath.stationkeep_flight(X_ref, dt, g.G, x0, n_rev, nav, exe, float(dv_min_ms) / ms, float(dv_max_ms) / ms,
                                   float(r_lost_km) / km, MU=MU, integ=integ, ctx=ctx)
    status, lost_at = np.asarray(r.status), np.asarray(r.lost_at)
    t_upd = np.concatenate([[0.0], np.cumsum(np.tile(dt, n_rev))])            # the time of update u; [n_upd]: the end
    t_days = t_upd[np.where(status == 1, lost_at, n_upd)] * TU / day
    dv_ms = np.asarray(r.dv_total) * ms
    with np.errstate(divide="ignore", invalid="ignore"):
        per_year = np.where(t_days > 0.0, dv_ms / (t_days / YEAR_DAYS), np.nan)
    out = dict(dv_ms=dv_ms, t_days=t_days, dv_per_year_ms=per_year, n_burn=r.n_burn, dev_r_km=r.dev[0] * km, dev_v_ms=r.dev[1] * ms,
               dv_hist_ms=r.dv_hist * ms, dev_final_r_km=r.dev_final[0] * km, dev_final_v_ms=r.dev_final[1] * ms, x_final=r.x_final,
               status=status, lost_at=lost_at, lost_share=float(np.mean(status == 1)), gains=g, x0=x0, nav=nav, exe=exe)
    ok = status == 0
    per_run = dict(dv_ms=dv_ms, dv_per_year_ms=per_year, dev_r_km=np.max(out["dev_r_km"], axis=0, initial=0.0),
                   dev_v_ms=np.max(out["dev_v_ms"], axis=0, initial=0.0))
    out["percentiles"] = {k: {q: (float(np.percentile(v[ok], q)) if ok.any() else float("nan")) for q in (50, 95, 99)}
                          for k, v in per_run.items()}
    return out
