"""Host references for the dense-output kernel (k_indirect_dense) and the addTimeFinal kernels that consume it (k_remesh_spline,
k_dense_cost): the library's sample assignment stated in numpy, the expected state at every sample from the CPU oracle (from the
owning node, and hop by hop), the natural cubic spline on general knots with its moments and its evaluation in long double, the
cost trapezoid accumulated in long double, and the table of shapes the GPU sweep runs.  Plain numpy; nothing here touches a GPU.
tests/test_dense_reference_host.py checks it on the CPU, tests/test_dense_shapes_gpu.py and tests/test_add_time_shapes_gpu.py
compare the device against it."""
import collections

import numpy as np

import addtime_reference as R
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

RK4, DOP853 = 0, 3                                  # the oracle's and the library's method numbers (they agree)
METHODS = {"dop853": (DOP853, 0), "rk4x8": (RK4, 8), "rk4x64": (RK4, 64)}
TOL = {"dop853": 1e-11, "rk4x8": 1e-10, "rk4x64": 1e-10}      # the bars of test_densify_vs_oracle (test_gpu_parity.py)
FROM_NODE = ("dop853", "rk4x64")                    # RK4 x 8 shows its own truncation against an adaptive reference: hop by hop only
MASS = 1000.0


# ---- the sample assignment

def segment_ranges(t, td, last_takes_end):
    """first[S + 1] of the library's sample assignment (segment_samples, lto_host_sweeps.hip): segment i of the grid t owns the
    samples td[first[i] : first[i + 1]], those in [t_i, t_{i+1}).  last_takes_end = False leaves the last sample (the last grid
    point) to final_state, the lto_indirect_densify form; True gives it to the last segment, the add-time form."""
    t = np.asarray(t, dtype=np.float64)
    td = np.asarray(td, dtype=np.float64)
    S = t.size - 1
    count = td.size if last_takes_end else td.size - 1
    seg = np.clip(np.searchsorted(t, td[:count], side="right") - 1, 0, S - 1)
    first = np.searchsorted(seg, np.arange(S + 1), side="left").astype(np.int32)
    first[S] = count
    return first


# ---- the expected states

def rel(a, ref):
    """|a - ref|_inf relative to max(1, |ref|_inf): the measure of test_densify_vs_oracle."""
    return float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))


def dense_expected(oracle, XC, t, prm_l, td, first, method, steps, Y=None, base=0):
    """The expected state at every sample of one trajectory, for both comparisons: (node_ref, hop_ref), each [12 x len(td)], NaN in
    the columns no segment owns.  first[S + 1] are the trajectory's ranges, `base` what they are offset by (a global first[]).
    node_ref[:, j] is the oracle's DOP853 flow of the owning node XC[:, i] over td[j] - t[i].  hop_ref[:, j] is the oracle's flow
    by (method, steps) over td[j] - td[j-1] of the sample before it -- column j-1 of Y, the states to be checked, or of hop_ref
    itself when Y is None (the oracle chained alone) -- and of the node over td[j] - t[i] for the first sample of a segment.  A
    span of zero is no flow: the start itself, bit for bit."""
    XC = np.asarray(XC, dtype=np.float64)
    td = np.asarray(td, dtype=np.float64)
    node_ref = np.full((12, td.size), np.nan)
    hop_ref = np.full((12, td.size), np.nan)
    for i in range(len(first) - 1):
        prev, tprev = XC[:, i], t[i]
        for j in range(first[i] - base, first[i + 1] - base):
            if td[j] == t[i]:
                node_ref[:, j] = XC[:, i]
            else:
                node_ref[:, j], rc, _, _ = oracle.flow_state_costate(XC[:, i], prm_l, td[j] - t[i], oracle.DOP853_ADAPTIVE)
                assert rc == 0
            if td[j] == tprev:
                hop_ref[:, j] = prev
            else:
                hop_ref[:, j], rc, _, _ = oracle.flow_state_costate(prev, prm_l, td[j] - tprev, method, steps)
                assert rc == 0
            prev, tprev = (hop_ref if Y is None else Y)[:, j], td[j]
    return node_ref, hop_ref


def final_expected(oracle, XC, t, prm_l, td, first, method, steps, Y=None, base=0):
    """What final_state holds for the trajectory, as dense_expected's pair: the flow of the last node's segment to t[-1], from the
    node and from the segment's last sample."""
    i = len(first) - 2
    node_ref, rc, _, _ = oracle.flow_state_costate(XC[:, i], prm_l, t[i + 1] - t[i], oracle.DOP853_ADAPTIVE)
    assert rc == 0
    prev, tprev = XC[:, i], t[i]
    if first[i + 1] > first[i]:
        j = first[i + 1] - base - 1
        src = Y if Y is not None else dense_expected(oracle, XC, t, prm_l, td, first, method, steps, None, base)[1]
        prev, tprev = src[:, j], td[j]
    if t[i + 1] == tprev:
        return node_ref, np.array(prev)
    hop_ref, rc, _, _ = oracle.flow_state_costate(prev, prm_l, t[i + 1] - tprev, method, steps)
    assert rc == 0
    return node_ref, hop_ref


def worst_errors(Y, node_ref, hop_ref, cols):
    """(largest from-the-node, largest hop-by-hop) relative difference over the columns `cols`."""
    en = max([rel(Y[:, j], node_ref[:, j]) for j in cols], default=0.0)
    eh = max([rel(Y[:, j], hop_ref[:, j]) for j in cols], default=0.0)
    return en, eh


# ---- the natural cubic spline in long double

def natural_spline_ld(x, Y, xq):
    """The natural cubic spline through (x, Y[r, :]) on general knots at the points xq, [rows x len(xq)]: the moments by a Thomas
    sweep in long double, the evaluation in long double, rounded to float64 once at the end.  At a knot the sample itself
    (addtime_reference.natural_spline_eval's rule)."""
    ld = np.longdouble
    x64 = np.asarray(x, dtype=np.float64)
    Y64 = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    xq = np.atleast_1d(np.asarray(xq, dtype=np.float64))
    x, Yl = x64.astype(ld), Y64.astype(ld)
    n = x.size
    h = np.diff(x)
    M = np.zeros(Yl.shape, dtype=ld)
    if n >= 3:
        slope = np.diff(Yl, axis=1) / h
        cp = np.zeros(n, dtype=ld)                      # the Thomas factors of rows 1 .. n-2
        dp = np.zeros(Yl.shape, dtype=ld)
        for i in range(1, n - 1):
            diag = ld(2.0) * (h[i - 1] + h[i])
            rhs = ld(6.0) * (slope[:, i] - slope[:, i - 1])
            den = diag - (h[i - 1] * cp[i - 1] if i > 1 else ld(0.0))
            cp[i] = (h[i] / den) if i < n - 2 else ld(0.0)
            dp[:, i] = (rhs - (h[i - 1] * dp[:, i - 1] if i > 1 else ld(0.0))) / den
        M[:, n - 2] = dp[:, n - 2]
        for i in range(n - 3, 0, -1):
            M[:, i] = dp[:, i] - cp[i] * M[:, i + 1]
    out = np.zeros((Y64.shape[0], xq.size))
    for k, q in enumerate(xq):
        i = int(np.clip(np.searchsorted(x64, q, side="right") - 1, 0, n - 2))
        if q == x64[i]:
            out[:, k] = Y64[:, i]
            continue
        if q == x64[i + 1]:
            out[:, k] = Y64[:, i + 1]
            continue
        hi, a, b = h[i], x[i + 1] - ld(q), ld(q) - x[i]
        val = (M[:, i] * a ** 3 + M[:, i + 1] * b ** 3) / (ld(6.0) * hi) + (Yl[:, i] - M[:, i] * hi * hi / ld(6.0)) * a / hi + \
            (Yl[:, i + 1] - M[:, i + 1] * hi * hi / ld(6.0)) * b / hi
        out[:, k] = val.astype(np.float64)
    return out


def dense_cost_ld(XC_dense, t_dense, thrustLimit, p, rho, mass, DU, TU):
    """addtime_reference.dense_cost with the trapezoid accumulated in long double.  Returns (cost, u): u is the float64 magnitude at
    every sample (addtime_reference.umag), for the clamp checks."""
    u = R.umag(np.asarray(XC_dense)[9:12], thrustLimit, p, rho, mass, DU, TU)
    t = np.asarray(t_dense, dtype=np.float64).astype(np.longdouble)
    ul = u.astype(np.longdouble)
    return float(np.sum(np.diff(t) * (ul[1:] + ul[:-1]) / np.longdouble(2.0))), u


def thrust_accel(thrustLimit, mass=MASS):
    """aL of the control law, DU/TU^2 (stateCostate_deriv.jl:33)."""
    return thrustLimit / mass / 1e3 * TU ** 2 / DU


# ---- the shapes of the sweep

# Single trajectories: n nodes -> n_desired samples of lto.densify.  S = n - 1 lanes in workgroups of 64.
#   2 -> 2, 2 -> 3, 2 -> 65, 3 -> 2      the smallest grids: no interior sample, one, a long chain in one lane, more nodes than samples
#   13 -> 5, 66 -> 7                     most segments own no sample (66 -> 7: a second workgroup with two lanes, one of them empty)
#   13 -> 13 on a LinRange grid          every sample is a node, bit for bit
#   13 -> 25                             every other sample is near a node
#   64 -> 65, 65 -> 64, 66 -> 129, 130 -> 257    S = 63, 64, 65, 129: the workgroup edge and the ragged last wavefront
SHAPES = [(2, 2), (2, 3), (2, 65), (3, 2), (13, 5), (66, 7), (13, 13), (13, 25), (64, 65), (65, 64), (66, 129), (130, 257)]
PS = (0.0, 1.0, 2.0, 1.5)
THRUSTS = (0.05, 10.0)
DIRS = (1.0, -1.0)
# Segment lengths.  An RK4 x 64 lane crosses a sample-free stretch in one 64-step hop, so the grids of the sparse shapes are short
# enough for RK4 x 64's own truncation over a whole segment to stay a decade under its bar against the adaptive reference; the
# dense shapes take test_densify_vs_oracle's lengths.  The seeds are ones at which the reference keeps every bar with a decade to
# spare against itself -- the oracle chained hop by hop against the oracle from the node, test_dense_reference_host.py -- so what
# a GPU comparison shows beyond that is the kernel's.
DT_DENSE, DT_SPARSE = (0.05, 0.25), (0.01, 0.04)

Case = collections.namedtuple("Case", "name n n_desired p thrust time_dir rho seed lin")


def _cases(seed0=240):
    out = []
    for s, (n, m) in enumerate(SHAPES):
        for v in range(2):                              # two parameter sets per shape: 24 sets cover the 16 (p, thrust, dir) triples
            k = 2 * s + v
            p, thrust, td = PS[k % 4], THRUSTS[(k // 4) % 2], DIRS[(k // 8) % 2]
            name = "%dto%d%s-p%g-thr%g-dir%+d" % (n, m, "lin" if (n, m) == (13, 13) else "", p, thrust, td)
            out.append(Case(name, n, m, p, thrust, td, (0.5, 0.1)[v], seed0 + k, (n, m) == (13, 13)))
    return out


CASES = _cases()


def case_problem(c):
    """(XC [12 x n], t [n], prm_l) of a case.  The sparse shapes (fewer samples than twice the nodes) take the short segments."""
    sparse = c.n_desired < 2 * c.n
    XC, T = synth.indirect_problem(c.n, seed=c.seed, dt_range=DT_SPARSE if sparse else DT_DENSE)
    XC, t = np.asfortranarray(XC[:, :, 0]), np.array(T[:, 0])
    if c.lin:
        t = R.linrange(t[0] + 0.1, t[-1], c.n)          # the library's own (1 - tau) a + tau b form: densify's samples are these nodes
    return XC, t, [MU, DU, TU, c.thrust, MASS, c.time_dir, c.p, c.rho]


def case_samples(c, t):
    """densify's samples and ranges for a case: (td [n_desired], first [S + 1])."""
    td = R.linrange(t[0], t[-1], c.n_desired)
    return td, segment_ranges(t, td, False)


# Batches: n = 23 nodes, B = 3 and 5 trajectories of mixed control-law classes, S = 66 and 110 lanes: the trajectory boundaries at
# lanes 22, 44, 66 and 88 fall inside wavefronts.  Every trajectory has its own sample count; trajectory 1 starts its samples
# behind its second node (no sample in its first segment); trajectory 0's samples end on the last grid point, which its last
# segment owns (the add-time form), the others' end before it, so final_state is a further hop there.  Seven samples on 22
# segments leave whole segments to one RK4 x 64 hop: the short segment lengths, as for the sparse single shapes.
BATCH_N = 23
BATCH_P = (1.0, 2.0, 0.0, 1.5, 1.0)
BATCH_THRUST = (0.05, 10.0, 10.0, 0.05, 10.0)
BATCH_DIR = (1.0, 1.0, -1.0, 1.0, -1.0)
BATCH_RHO = (0.5, 1.0, 1.0, 1.0, 0.1)
BATCH_COUNTS = (30, 7, 45, 23, 64)


def batch_problem(B, n_tgrids, seed0=70):
    """(XC [12 x n x B], T [n x n_tgrids], prm_l [B], td [B arrays], first [B S + 1] global, offsets [B + 1])."""
    n = BATCH_N
    XC, T = synth.indirect_problem(n, n_batch=B, seed=seed0 + B, dt_range=DT_SPARSE)
    T = np.asfortranarray(T[:, :n_tgrids])
    prm_l = [[MU, DU, TU, BATCH_THRUST[b], MASS, BATCH_DIR[b], BATCH_P[b], BATCH_RHO[b]] for b in range(B)]
    tds, firsts, off = [], [], [0]
    for b in range(B):
        t = T[:, b if n_tgrids > 1 else 0]
        lo = t[0] if b != 1 else t[1] + 0.25 * (t[2] - t[1])
        hi = t[-1] if b == 0 else t[-1] - 0.3 * (t[-1] - t[-2]) * (1 + b) / (1 + B)
        td = R.linrange(lo, hi, BATCH_COUNTS[b])
        tds.append(td)
        firsts.append(segment_ranges(t, td, True)[:-1] + off[-1])
        off.append(off[-1] + td.size)
    first = np.concatenate(firsts + [np.array([off[-1]], dtype=np.int32)]).astype(np.int32)
    return XC, T, prm_l, tds, first, off


# ---- addTimeFinal: the shapes of tests/test_add_time_shapes_gpu.py and a host restatement of the whole guess

# Re-mesh, n nodes and n_desired knots: n > n_desired at (30, 5), (65, 4), (65, 64); n - 1 divides n_desired - 1 at (3, 5), (4, 4),
# (4, 64), (65, 65), (65, 257), where every new node falls on a knot; (2, .) has no interior node.  The lane is c * K + b in
# workgroups of 64: K = 6 gives 72 lanes, K = 11 gives 132.
REMESH_PAIRS = [(2, 4), (2, 65), (3, 5), (3, 64), (4, 4), (4, 64), (4, 257), (30, 5), (30, 64), (30, 257), (65, 4), (65, 64), (65, 65),
                (65, 257)]
REMESH_K = (1, 6, 11)
# Snap: the winning candidate at the first and last index, either side of find_tau's 256-thread stride and of its wave edges.
SNAP_J = (0, 1, 63, 64, 255, 256, 257, 511, 512, 999, 1000)
# dt in TU: the coast moves the end by ~1e-11; the candidates are ~1e-3 apart, and 0 and 1000 (the table's two ends) 1.6e-9
SNAP_DT = 1e-11
# Cost: (p, rho, thrust N, lam_sigma, seed).  For p > 1 the magnitude (|lambda_v| / p)^(1 / (p - 1)) meets aL(0.05 N) = 0.0183 at
# |lambda_v| = 0.037 (p = 2), 0.20 (p = 1.5) and 1.0e-3 (p = 3): lam_sigma puts the costates on both sides of it.
COST_CASES = [(0.0, 1.0, 10.0, 0.5, 0), (1.0, 1.0, 10.0, 0.5, 0), (1.0, 0.1, 10.0, 0.5, 0), (2.0, 1.0, 0.05, 0.03, 0),
              (1.5, 1.0, 0.05, 0.15, 0), (3.0, 1.0, 0.05, 8e-4, 0)]
COST_N, COST_K, COST_M = 7, 3, (4, 65)


def arrival_table():
    """(Xf_times [100], Xf_states [6 x 100]) of the second halo orbit, the arrival side of synth.indirect_problem."""
    tab = synth.halo_orbits()[1]
    return np.linspace(0.0, 1.0, tab.shape[1]), np.asfortranarray(tab[:6])


def addtime_problem(n, seed=5, lam_sigma=0.1):
    """(XC [12 x n], t [n]): synth.indirect_problem's nodes, not a converged transfer."""
    XC, T = synth.indirect_problem(n, seed=seed, lam_sigma=lam_sigma)
    return np.asfortranarray(XC[:, :, 0]), np.array(T[:, 0])


def add_time_dts(K):
    from lowthrustopt_amd.constants import day
    return np.linspace(0.25, 2.0, K) * day / TU if K > 1 else np.array([0.5 * day / TU])


def oracle_dense(oracle, XC, t, prm_l, td):
    """The add-time form of the dense output by the oracle alone: every sample from its owning node, the last segment owning the
    last grid point."""
    first = segment_ranges(t, td, True)
    return dense_expected(oracle, XC, t, prm_l, td, first, DOP853, 0)[0]


def addtime_guess_host(oracle, XC, t, prm_l, dt, n_desired):
    """lto_indirect_add_time's guess by the oracle and this module alone: (G [12 x n], t_new [n], tau)."""
    times, tab = arrival_table()
    XCe, te = R.extended(XC, t, dt)
    td = R.linrange(te[0], te[-1], n_desired)
    Yd = oracle_dense(oracle, XCe, te, prm_l, td)
    t_new = R.linrange(te[0], te[-1], XC.shape[1])
    G = natural_spline_ld(td, Yd, t_new)
    tau, s = R.find_tau(times, tab, G[:6, -1])
    G[:6, -1] = s
    return G, t_new, tau


def clamp_sides(u, aL):
    """(samples clamped at aL, samples below it) of a p > 1 magnitude."""
    return int(np.count_nonzero(u == aL)), int(np.count_nonzero(u < aL))
