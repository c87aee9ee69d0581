"""One iteration of the direct multiple-shooting loop (direct_solve_impl in lto_direct_solve.hip, behind lto_direct_solve_batch,
lto_direct_solve_free_batch and lto_direct_solve_free_tf_batch), replayed from a given state.

replay_iteration(state_k, it, variant, back_end) returns everything iteration it = k + 1 must produce from
state_k = (X, U, dV1, dV2, tau1, tau2, tf, t): which step is taken (frozen / free / free tf), the step, the ten sums of squares of the
line search with the pick and its margin, alpha, the updated X, U, dV, tau and tf (clamped), the new grid, the defect, max|defect| and
the history row.  All arrays carry a trailing batch axis: X [nstate x n x B], U [3 x n x B], dV1 / dV2 [3 x B], tau1 / tau2 / tf [B],
t [n x B].  Nothing accumulates: every call starts from the state it is given.

Two back ends:

  OracleBackEnd  independent, CPU only.  Sweeps from direct_helpers.OracleDirectOps, the step from drivers.direct_qp_dense / _free /
                 _free_tf, updates in numpy exactly as drivers.direct_loop_host writes them (so a chain of replays reproduces the
                 mirror loop's history bit for bit), and the mirror's per-trajectory rule for a free tf (step > 0 of that trajectory).

  DeviceStepBackEnd  the library's one-step entries lto_direct_qp_step / _free / _free_tf at the loop's shape (n, B), the end states
                 of lto_direct_end_states, trial and final defects through DirectPlan.defect on plans of shape (n, B) and (n, 10 B);
                 every decision in between on the host in exact arithmetic, following the C loop: the free / frozen parity and the
                 free-tf switch are batch-wide (`tfm`: some trajectory of the batch has step > 0, so a step-0 neighbour takes the
                 free-tf step in a zero-width box), X, U and dV move by one fma (k_axpy_traj, k_qp_update_dv), the sums of squares
                 are exact rationals and the pick is their first minimiser.
                 tau and tf: the library is built without -ffp-contract, and hipcc's default contracts `tau[i] + p[i] * a` and
                 `tf[b] + p[3 b + 2] * a`: the gfx950 code object of k_tau_update and k_tf_update holds one v_fmac_f64 for each of
                 them (followed for tf by v_max_f64 / v_min_f64 with the two bounds).  So tau and tf are fma(a, p, x) here too.
                 k_tf_grid is compiled with `fp contract(off)`: the grid is t0 + (tau_grid + 1) / 2 * (tf - t0) as written."""
import collections
import math

import numpy as np

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers

import direct_helpers as DH
import newton_loop_reference as NR

NA = 10
SEARCH_AFTER = 10                 # line search from iteration 11 (direct.jl:557)
TOL = 1e-6                        # `while er > 1e-6` (direct.jl:491)
# NewtonBatch (lto_host.hpp): alphas[a] = 0.1 + (1.0 - 0.1) / (n_alpha - 1) * a, the last one exactly 1.0
ALPHAS = np.array([0.1 + (1.0 - 0.1) / (NA - 1) * a for a in range(NA)])
ALPHAS[NA - 1] = 1.0
ALPHAS_MIRROR = np.linspace(0.1, 1.0, NA)      # drivers.lineSearch_direct

State = collections.namedtuple("State", "X U dV1 dV2 tau1 tau2 tf t")


def fixed_grid(t):
    """t recomputed through tau with tf unchanged (direct.jl:478-480, :582), as the loop and the mirror both write it."""
    t = np.asarray(t, dtype=np.float64)
    t0, tf = t[0], t[-1]
    tau = (t - t0) / (tf - t0) * 2 - 1
    return t0 + (tau + 1) / 2 * (tf - t0)


class Variant:
    """A batch of problems of one entry point.  kind: "frozen" (lto_direct_solve_batch, the targets fixed at tau), "free"
    (lto_direct_solve_free_batch, flagEnd) or "free_tf" (lto_direct_solve_free_tf_batch, flagEnd, tf_bounds one (step, tf_min,
    tf_max) per trajectory).  t_entry [n] is the caller's grid, shared by the batch; tau [2 x B] the starting phases."""

    def __init__(self, kind, X, U, t_entry, tau, tabs, mass=1000.0, nsteps=10, Isp=DH.ISP, beta=0.0, allow_impulsive=False,
                 tf_bounds=None, max_iter=100, dV=None):
        assert kind in ("frozen", "free", "free_tf")
        self.kind = kind
        self.X = np.array(X, dtype=np.float64, order="F")
        self.U = np.array(U, dtype=np.float64, order="F")
        self.nstate, self.n, self.B = self.X.shape
        self.t_entry = np.array(t_entry, dtype=np.float64)
        self.tau = np.array(tau, dtype=np.float64, order="F").reshape(2, self.B)
        self.tabs = tabs
        self.mass, self.nsteps, self.Isp, self.beta, self.allow_impulsive = float(mass), int(nsteps), float(Isp), float(beta), bool(allow_impulsive)
        self.tf_bounds = None if tf_bounds is None else [tuple(float(v) for v in q) for q in tf_bounds]
        assert (kind == "free_tf") == (self.tf_bounds is not None)
        self.max_iter = int(max_iter)
        self.dV = np.zeros((6, self.B), order="F") if dV is None else np.array(dV, dtype=np.float64, order="F")
        self.t0 = self.t_entry[0]
        self.tau_grid = (self.t_entry - self.t0) / (self.t_entry[-1] - self.t0) * 2 - 1
        self.t_fixed = fixed_grid(self.t_entry)
        self.flag_end = kind != "frozen"
        # the C loop's `tfm`: free tf for the whole batch as soon as one trajectory has a positive step
        self.tfm = bool(self.tf_bounds) and any(q[0] > 0.0 for q in self.tf_bounds)

    def step_of(self, b):
        return self.tf_bounds[b][0] if self.tf_bounds else 0.0

    def entry_state(self):
        B = self.B
        return State(self.X.copy(order="F"), self.U.copy(order="F"), self.dV[:3].copy(), self.dV[3:].copy(), self.tau[0].copy(),
                     self.tau[1].copy(), np.full(B, self.t_entry[-1]), np.asfortranarray(np.repeat(self.t_entry[:, None], B, axis=1)))

    def single(self, b):
        """Trajectory b as a batch of one."""
        return Variant(self.kind, self.X[:, :, b:b + 1], self.U[:, :, b:b + 1], self.t_entry, self.tau[:, b:b + 1], self.tabs, self.mass,
                       self.nsteps, self.Isp, self.beta, self.allow_impulsive, None if self.tf_bounds is None else [self.tf_bounds[b]],
                       self.max_iter, self.dV[:, b:b + 1])

    def mirror(self, b, ops, max_iter=None):
        """drivers.direct_loop_host on trajectory b: (outputs, {"status", "iterations", "history"})."""
        return drivers.direct_loop_host(self.X[:, :, b], self.U[:, :, b], self.tau[0, b], self.tau[1, b], self.t_entry, self.dV[:3, b],
                                        self.dV[3:, b], lto.MU, lto.DU, lto.TU, self.n, self.nsteps, self.mass, self.Isp, *self.tabs,
                                        self.flag_end, self.beta, self.allow_impulsive, self.max_iter if max_iter is None else max_iter,
                                        ops, verbose=False, tf_bounds=None if self.tf_bounds is None else self.tf_bounds[b])


def still_active(er):
    """`while er > 1e-6`: a NaN leaves the loop."""
    return bool(er > TOL)


def loop_counters(er, max_iter):
    """(status before the NaN / singular rules, iterations) of one trajectory as NewtonBatch::next and the cap at the loop's end
    produce them, from er[j - 1] = max|defect| after iteration j."""
    it, h_er = 0, 1.0
    while True:
        if not (h_er > TOL):
            return 0, it
        it += 1
        if it > max_iter:
            return 1, max_iter
        h_er = er[it - 1]


def margin_of(ss):
    """second smallest / smallest - 1 over the ten sums (inf where the smallest is 0 or fewer than two are comparable)."""
    v = sorted(s for s in ss if s == s)
    if len(v) < 2 or not v[0] > 0:
        return math.inf
    return float(v[1] / v[0] - 1) if v[1] != math.inf else math.inf


class Replay:
    """What replay_iteration found.  Per trajectory b: kind[b] the step taken ("frozen" / "free" / "free_tf", None for one that has
    left), searched[b], ss[b] the ten sums (None unless searched), pick[b] the index into the ten alphas (None unless searched),
    margin[b], alpha[b] (0 for one that has left).  dX, dU, dV_up [6 x B], p [3 x B] and cost [B] are the step; state the State after
    the iteration, defect [nstate x (n-1) x B] and er [B] its defect block and max|defect|, row [6 x B] the history row
    (max|defect|, cost, alpha, tau1, tau2, tf)."""


def replay_iteration(state_k, it, variant, back_end, active=None, alpha=None):
    """Iteration `it` (1-based) from state_k, the loop's state after it - 1 iterations.  active [B]: which trajectories are still
    in their loop (default: all).  alpha [B]: step lengths to apply instead of the replay's own picks (the picks, sums and margins are
    reported all the same); 0 entries of trajectories that have left are ignored."""
    v, s = variant, state_k
    B, n = v.B, v.n
    active = [True] * B if active is None else [bool(a) for a in active]
    r = Replay()
    r.kind = [back_end.kind_of(v, b, it) if active[b] else None for b in range(B)]
    r.dX, r.dU, r.dV_up, r.p, r.cost = back_end.steps(v, s, it, active)
    r.searched = [bool(active[b] and it > SEARCH_AFTER) for b in range(B)]
    r.ss = back_end.trial_sums(v, s, r.dX, r.dU, r.searched)
    r.pick, r.margin, r.alpha = [None] * B, [math.nan] * B, [0.0] * B
    for b in range(B):
        if r.searched[b]:
            r.pick[b] = NR.first_minimiser(r.ss[b])
            r.margin[b] = margin_of(r.ss[b])
            r.alpha[b] = float(back_end.alphas[r.pick[b]])
        elif active[b]:
            r.alpha[b] = 1.0
    r.alpha_own = list(r.alpha)
    if alpha is not None:
        r.alpha = [float(alpha[b]) if active[b] else 0.0 for b in range(B)]
    X, U = s.X.copy(order="F"), s.U.copy(order="F")
    dV = np.vstack([s.dV1, s.dV2])
    tau = np.vstack([s.tau1, s.tau2])
    tf = np.array(s.tf, dtype=np.float64)
    for b in range(B):
        a = r.alpha[b]
        if a == 0.0:                                       # a trajectory that has left keeps its values whatever the step holds
            continue
        X[:, :, b] = back_end.axpy(a, r.dX[:, :, b], s.X[:, :, b])
        U[:, :, b] = back_end.axpy(a, r.dU[:, :, b], s.U[:, :, b])
        dV[:, b] = back_end.axpy(a, r.dV_up[:, b], dV[:, b])
        if r.kind[b] in ("free", "free_tf"):               # direct.jl:564-565, not wrapped
            tau[:, b] = back_end.axpy_scalar(a, r.p[:2, b], tau[:, b])
        if r.kind[b] == "free_tf":                         # direct.jl:567, kept in [tf_min, tf_max]
            _, lo, hi = v.tf_bounds[b]
            tf[b] = min(max(float(back_end.axpy_scalar(a, r.p[2, b], tf[b])), lo), hi)
    t = back_end.grid(v, s, it, tf, active)
    r.state = State(X, U, dV[:3].copy(), dV[3:].copy(), tau[0].copy(), tau[1].copy(), tf, t)
    r.defect = back_end.defect(v, X, U, t)
    r.er = [NR.maxabs(r.defect[:, :, b]) for b in range(B)]
    r.row = np.array([[r.er[b], r.cost[b], r.alpha[b], tau[0, b], tau[1, b], tf[b]] for b in range(B)]).T
    return r


# ------------------------------------------------------------------------------------------------ independent back end (CPU)
class OracleBackEnd:
    """Sweeps from the CPU oracle, the step from the dense host QPs, updates in numpy as drivers.direct_loop_host writes them."""
    name = "independent"
    alphas = ALPHAS_MIRROR

    def __init__(self, Isp=DH.ISP):
        self.ops = DH.OracleDirectOps(Isp)

    @staticmethod
    def kind_of(v, b, it):
        if v.flag_end and it % 2 == 1:
            return "free_tf" if v.step_of(b) > 0.0 else "free"
        return "frozen"

    def steps(self, v, s, it, active):
        ns, n, B = v.nstate, v.n, v.B
        dX, dU = np.zeros((ns, n, B), order="F"), np.zeros((3, n, B), order="F")
        dV, p, cost = np.zeros((6, B), order="F"), np.zeros((3, B), order="F"), np.full(B, math.nan)
        for b in range(B):
            if not active[b]:
                continue
            X, U, t = s.X[:, :, b], s.U[:, :, b], s.t[:, b]
            kind = self.kind_of(v, b, it)
            defect, _ = self.ops.defect(X, U, t, v.nsteps)
            # the grid of the QP's weights is t through tau at the current tf (t_TU_fixed, direct.jl:321)
            t_w = v.t0 + (v.tau_grid + 1) / 2 * (s.tf[b] - v.t0)
            if kind == "free_tf":
                Jt, dtf, _ = self.ops.jacobian_tf(X, U, t, v.nsteps)
                s0, sf, g0, gf, c0, cf = drivers.end_model(s.tau1[b], s.tau2[b], *v.tabs)
                out = drivers.direct_qp_dense_free_tf(Jt, dtf, defect, X, U, t_w, s0, sf, g0, gf, c0, cf, v.beta, v.mass, s.dV1[:, b],
                                                      s.dV2[:, b], lto.DU, lto.TU, s.tf[b], v.tf_bounds[b], v.allow_impulsive)
                dX[:, :, b], dU[:, :, b], dV[:3, b], dV[3:, b], p[0, b], p[1, b], p[2, b], cost[b] = out
            elif kind == "free":
                Jt, _ = self.ops.jacobian(X, U, t, v.nsteps)
                s0, sf, g0, gf, c0, cf = drivers.end_model(s.tau1[b], s.tau2[b], *v.tabs)
                out = drivers.direct_qp_dense_free(Jt, defect, X, U, t_w, s0, sf, g0, gf, c0, cf, v.beta, v.mass, s.dV1[:, b], s.dV2[:, b],
                                                   lto.DU, lto.TU, v.allow_impulsive)
                dX[:, :, b], dU[:, :, b], dV[:3, b], dV[3:, b], p[0, b], p[1, b], cost[b] = out
            else:
                Jt, _ = self.ops.jacobian(X, U, t, v.nsteps)
                s0, sf = drivers.interpEndStates(s.tau1[b], s.tau2[b], *v.tabs)
                out = drivers.direct_qp_dense(Jt, defect, X, U, t_w, s0, sf, v.mass, s.dV1[:, b], s.dV2[:, b], lto.DU, lto.TU,
                                              v.allow_impulsive)
                dX[:, :, b], dU[:, :, b], dV[:3, b], dV[3:, b], cost[b] = out
        return dX, dU, dV, p, cost

    def trial_sums(self, v, s, dX, dU, searched):
        out = [None] * v.B
        for b in range(v.B):
            if not searched[b]:
                continue
            al = self.alphas
            Xt = s.X[:, :, b, None] + dX[:, :, b, None] * al[None, None, :]
            Ut = s.U[:, :, b, None] + dU[:, :, b, None] * al[None, None, :]
            out[b] = [float(e) for e in self.ops.defect_batch_sumsq(np.asfortranarray(Xt), np.asfortranarray(Ut), s.t[:, b], v.nsteps)]
        return out

    @staticmethod
    def axpy(a, d, x):
        return x + d * a

    axpy_scalar = axpy

    @staticmethod
    def grid(v, s, it, tf, active):
        t = np.array(s.t, order="F")
        for b in range(v.B):
            if active[b]:
                t[:, b] = v.t0 + (v.tau_grid + 1) / 2 * (tf[b] - v.t0)
        return t

    def defect(self, v, X, U, t):
        return np.asfortranarray(np.stack([self.ops.defect(X[:, :, b], U[:, :, b], t[:, b], v.nsteps)[0] for b in range(v.B)], axis=2))


# ------------------------------------------------------------------------------------------------ device-step back end
class DeviceStepBackEnd:
    """The library's one-step entries and DirectPlan.defect at the loop's own shapes; the C loop's decisions on the host."""
    name = "device step"
    alphas = ALPHAS

    def __init__(self, ctx, variant):
        import torch
        self.torch, self.ctx = torch, ctx
        v = variant
        self.orbits = lto.DirectOrbits(*v.tabs)
        self.plan = lto.DirectPlan(ctx, v.nstate, v.n, v.B, v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp)
        self.plan_trials = lto.DirectPlan(ctx, v.nstate, v.n, v.B * NA, v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp)

    def close(self):
        self.plan.close()
        self.plan_trials.close()

    @staticmethod
    def kind_of(v, b, it):
        if v.flag_end and it % 2 == 1:                     # the active trajectories share the iteration count
            return "free_tf" if v.tfm else "free"
        return "frozen"

    def end_states(self, v, s):
        """(s0 [6 x B], sf, g0, gf, c0 [B], cf): k_end_states at the state's tau; the fixed targets of the frozen variant."""
        if v.kind == "frozen":
            ends = [drivers.interpEndStates(s.tau1[b], s.tau2[b], *v.tabs) for b in range(v.B)]
            return np.stack([e[0] for e in ends], axis=1), np.stack([e[1] for e in ends], axis=1), None, None, None, None
        return lto.direct_end_states(np.vstack([s.tau1, s.tau2]), self.orbits, ctx=self.ctx)

    def steps(self, v, s, it, active):
        B = v.B
        kind = self.kind_of(v, 0, it)
        s0, sf, g0, gf, c0, cf = self.end_states(v, s)
        tg = [lto.direct_targets(s0[:, b], sf[:, b], v.mass, s.dV1[:, b], s.dV2[:, b]) for b in range(B)]
        args = (s.X, s.U, s.t, v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp, tg)
        p = np.zeros((3, B), order="F")
        if kind == "frozen":
            dX, dU, dV, cost = lto.direct_qp_step(*args, allowImpulsive=v.allow_impulsive, ctx=self.ctx)
        else:
            em = [lto.direct_end_model(g0[:, b], gf[:, b], c0[b], cf[b]) for b in range(B)]
            betas = np.full(B, v.beta)
            if kind == "free":
                dX, dU, dV, p2, cost = lto.direct_qp_step_free(*args, em, betas, allowImpulsive=v.allow_impulsive, ctx=self.ctx)
                p[:2] = p2
            else:
                tb = [lto.direct_tf_bounds(*q) for q in v.tf_bounds]
                dX, dU, dV, p, cost = lto.direct_qp_step_free_tf(*args, em, betas, tb, allowImpulsive=v.allow_impulsive, ctx=self.ctx)
        return dX, dU, dV, p, cost

    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def trial_defects(self, v, s, dX, dU):
        """[nstate x (n-1) x NA x B]: the defect blocks of the ten trial trajectories of every trajectory, one sweep on the plan of
        shape (n, 10 B), each trial on its trajectory's current grid (d_tl)."""
        ns, n, B = v.nstate, v.n, v.B
        J, S = n * B * NA, (n - 1) * B * NA
        Xt = NR.trial_points(s.X, dX, ALPHAS)
        Ut = NR.trial_points(s.U, dU, ALPHAS)
        tl = np.ascontiguousarray(np.repeat(s.t.T[:, None, :], NA, axis=1).reshape(-1))          # [(b*NA + a)*n + k]
        d = self.torch.zeros(ns, S, dtype=self.torch.float64, device="cuda")
        self.plan_trials.defect(self._dev(NR.trials_to_soa(Xt)), J, self._dev(NR.trials_to_soa(Ut)), J, self._dev(tl), B * NA, d, S)
        self.torch.cuda.synchronize()
        return NR.trials_from_soa(d.cpu().numpy(), n - 1, NA, B)

    def trial_sums(self, v, s, dX, dU, searched):
        out = [None] * v.B
        if any(searched):
            dt = self.trial_defects(v, s, dX, dU)
            for b in range(v.B):
                if searched[b]:
                    out[b] = [NR.sumsq_rational(dt[:, :, a, b]) for a in range(NA)]
        return out

    @staticmethod
    def axpy(a, d, x):
        return NR.fma_exact(a, d, x)

    axpy_scalar = axpy                                     # contracted on the device: see the module's docstring

    @staticmethod
    def grid(v, s, it, tf, active):
        if v.tfm and v.flag_end and it % 2 == 1:           # k_tf_grid: every trajectory of the batch, from its own tf
            return np.asfortranarray(np.stack([v.t0 + (v.tau_grid + 1) / 2 * (tf[b] - v.t0) for b in range(v.B)], axis=1))
        if v.tfm:
            return np.array(s.t, order="F")
        return np.asfortranarray(np.repeat(v.t_fixed[:, None], v.B, axis=1))

    def defect(self, v, X, U, t):
        ns, n, B = v.nstate, v.n, v.B
        J, S = n * B, (n - 1) * B
        d = self.torch.zeros(ns, S, dtype=self.torch.float64, device="cuda")
        self.plan.defect(self._dev(NR.to_soa(X)), J, self._dev(NR.to_soa(U)), J, self._dev(np.ascontiguousarray(t.T).reshape(-1)), B, d, S)
        self.torch.cuda.synchronize()
        return NR.from_soa(d.cpu().numpy(), n - 1, B)

    def jacobian_defect(self, v, X, U, t):
        """The defect block k_direct_jacobian emits, through the host entry the step entries' sweep goes through."""
        return lto.direct_jacobian_blocks(X, U, t, v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp, ctx=self.ctx)[2]


# ------------------------------------------------------------------------------------------------ the problem sets
DAY = lto.day / lto.TU
TAU2 = 0.02                       # the demos' offset of tau2 from its stacked value


def demo_on_fixed_grid():
    """The 30-node halo demo with its grid replaced by t1(t), the recomputation through tau, which is a fixed point of itself
    (asserted where it is used): the loop's first sweep and its QP weights then see one grid."""
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    return X, U, fixed_grid(t), tau1, tau2, tabs


def problem_sets():
    """The sets of the tests, all from the halo demo (30 nodes, nsteps 10, mass 1000, Isp 2000, beta 0, U = 0; no impulses in A to E)."""
    X, U, t, tau1, tau2, tabs = demo_on_fixed_grid()
    n = X.shape[1]

    def rep(A, B):
        return np.asfortranarray(np.repeat(np.asarray(A)[:, :, None], B, axis=2))

    rng = np.random.default_rng(3)
    Xp = X.copy()
    Xp[:, 1:-1] += 0.1 * rng.standard_normal((6, n - 2)) * np.maximum(1e-3, np.abs(X[:, 1:-1]))
    X7 = np.vstack([X, np.full((1, n), 1000.0)])
    tfb = drivers.tf_bounds_default(t[0], lto.TU)
    tfb0 = (0.0,) + tuple(tfb[1:])
    sets = collections.OrderedDict()
    sets["A"] = Variant("frozen", rep(X, 3), rep(U, 3), t, [[tau1] * 3, [tau2 + 0.2, tau2 + 0.02, tau2 + 0.1]], tabs)
    sets["B"] = Variant("free", np.asfortranarray(np.stack([Xp, X, X], axis=2)), rep(U, 3), t,
                        [[tau1] * 3, [tau2 + 0.02, tau2 + 0.05, tau2 + 0.02]], tabs)
    sets["C"] = Variant("free", rep(X7, 1), rep(U, 1), t, [[tau1], [tau2 + TAU2]], tabs)
    sets["D"] = Variant("free_tf", rep(X, 2), rep(U, 2), t, [[tau1] * 2, [tau2 + TAU2] * 2], tabs, tf_bounds=[tfb, tfb0])
    sets["E"] = Variant("free_tf", rep(X7, 1), rep(U, 1), t, [[tau1], [tau2 + TAU2]], tabs, tf_bounds=[tfb], max_iter=16)
    # impulses allowed and 1e-3 at the start: the only set whose dV moves, so the only one that sees k_qp_update_dv's alpha
    sets["F"] = Variant("frozen", rep(X, 1), rep(U, 1), t, [[tau1], [tau2 + 0.25]], tabs, allow_impulsive=True, dV=np.full((6, 1), 1e-3),
                        max_iter=14)
    return sets
