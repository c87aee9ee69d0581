"""Host reference for the dense output and the re-mesh of the 14-row variable-mass system (k_indirect_dense<14>, k_remesh_nodes<14>,
lto_indirect_remesh_mass_batch) -- CPU only, no library code under test.

The flow is the oracle's: oracle.indirect14 on a two-node pair whose second node is zero, so the defect IS the propagated state
(thrust_mass_reference.flow14 adds the next node back; with a zero node nothing is rounded).  The sample assignment is
dense_reference.segment_ranges, the grid rule remesh_reference.new_grid / sources / scan64, all by import.

Fixtures: nodes on ONE trajectory of the oracle's DOP853 flow at rtol = atol = 1e-13, started from the lifted first node of
synth.indirect_problem(n, seed=4, lam_sigma=0.1) with lambda_m = 0.4 and m0 = 1000 kg, on a non-uniform grid (segment lengths
uniform in [0.02, 0.2] TU, seeded), for the six parameter sets of SETS.  For p <= 1 lambda_m is shifted to lambda_m(tf) = 0 (it
does not feed back there); for p > 1 it is left alone (the shift would change the trajectory) and those fixtures serve the dense
and the guess comparisons only.  Admission (tests/test_mass_dense_host.py): defect <= 1e-12 max|X|, mass non-increasing, and every
p > 1 fixture at least CLAMP_CLEARANCE away from the clamp | |lambda_v| - p (cT / m)^(p-1) | at every node and sample.

Bars: relative PER ROW to max(1, max |reference row|) -- one global scale would let the 1000 kg mass row hide the others.  DOP853
1e-11 (from the node and hop by hop), RK4 1e-10 (hop by hop, against the oracle's RK4 with the same step count), the bars of
tests/dense_reference.TOL.  The mass row has an absolute bar besides: max(10 e_m, 64 eps m0) kg, e_m the reference's own
from-the-node against hop-by-hop difference of row 6 over DENSE_CASES (self_errors)."""
import collections
import functools

import numpy as np

import addtime_reference as A
import dense_reference as D
import remesh_reference as RM
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

RK4, DOP853 = D.RK4, D.DOP853
METHODS = D.METHODS                                   # name -> (method number, steps)
TOL = D.TOL                                           # dop853 1e-11, rk4x8 / rk4x64 1e-10
IDX12 = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]       # rows of the 12-row system inside the 14-row one
M0 = 1000.0
LAMBDA_M0 = 0.4
DT_RANGE = (0.02, 0.2)
CLAMP_CLEARANCE = 0.05
EPS = np.finfo(np.float64).eps

Set = collections.namedtuple("Set", "name thrust isp p rho")
SETS = (Set("p1", 0.05, 2000.0, 1.0, 1.0),
        Set("p1-rho0.1-10N", 10.0, 2000.0, 1.0, 0.1),
        Set("p2-10N", 10.0, 2000.0, 2.0, 1.0),                 # unclamped
        Set("p3", 0.05, 2000.0, 3.0, 1.0),                     # clamped throughout
        Set("p1.5-10N", 10.0, 2000.0, 1.5, 1.0),
        Set("p0-isp20", 0.05, 20.0, 0.0, 1.0))                 # 59 kg burnt over nine nodes


def prm_list(s, isp=None):
    """The parameter 8-tuple of a set, Isp in the mass slot."""
    return [MU, DU, TU, s.thrust, s.isp if isp is None else isp, 1.0, s.p, s.rho]


def oracle_mod():
    from oracle import oracle as O
    O.lib()
    return O


def flow14(O, y0, prm, tau, method=DOP853, steps=0):
    """The oracle's flow of a 14-row node over tau by (method, steps); DOP853 at 1e-13.  tau == 0: the node itself, bit for bit."""
    y0 = np.asarray(y0, dtype=np.float64)
    if tau == 0.0:
        return y0.copy()
    XC = np.asfortranarray(np.stack([y0, np.zeros(14)], axis=1))
    _, defect, rc = O.indirect14(XC, np.array([0.0, tau]), np.array(prm, dtype=np.float64), method, steps, 1e-13, 1e-13, want_stm=False)
    assert rc == 0
    return defect[:, 0].copy()


def grid(n, seed, lin=False):
    t = np.concatenate([[0.0], np.cumsum(np.random.default_rng(seed).uniform(DT_RANGE[0], DT_RANGE[1], n - 1))])
    if lin:                                           # the library's own LinRange form: densify's samples are these nodes
        t = A.linrange(t[0] + 0.1, t[-1], n)
    return t


@functools.lru_cache(maxsize=None)
def fixture(n, k, lin=False, isp=None, gseed=None):
    """(X [14 x n], t [n], prm) of parameter set k on n nodes; read-only, shared.  isp: in place of the set's; gseed: the seed of the
    grid (default 100 + n: the fixtures of one node count share their grid)."""
    O = oracle_mod()
    s = SETS[k]
    prm = prm_list(s, isp)
    XC, _ = synth.indirect_problem(n, seed=4, lam_sigma=0.1)
    t = grid(n, 100 + n if gseed is None else gseed, lin)
    X = np.zeros((14, n), order="F")
    X[IDX12, 0] = XC[:, 0, 0]
    X[6, 0] = M0
    X[13, 0] = LAMBDA_M0
    for i in range(n - 1):
        X[:, i + 1] = flow14(O, X[:, i], prm, t[i + 1] - t[i])
    if s.p <= 1:
        X[13] -= X[13, -1]
    X.setflags(write=False); t.setflags(write=False)
    return X, t, prm


def clamp_gap(Y, prm):
    """| |lambda_v| - p (cT / m)^(p-1) | per column of Y [14 x m]; p > 1 only."""
    p = prm[6]
    cT = prm[3] / 1e3 * prm[2] ** 2 / prm[1]
    return np.abs(np.linalg.norm(Y[10:13], axis=0) - p * (cT / Y[6]) ** (p - 1.0))


def fixture_defect(O, X, t, prm):
    _, d, rc = O.indirect14(np.asfortranarray(X), np.array(t), np.array(prm), O.DOP853_ADAPTIVE, 0, 1e-13, 1e-13, want_stm=False)
    assert rc == 0
    return d


# ---- the measures

def _cols(a):
    a = np.asarray(a, dtype=np.float64)
    return a if a.ndim == 2 else a[:, None]


def row_scale(ref):
    return np.maximum(1.0, np.nanmax(np.abs(_cols(ref)), axis=1))


def rel_rows(a, ref, scale=None, cols=None):
    """max over rows and the columns `cols` of |a - ref| / scale[row]; scale defaults to max(1, max |ref row|) over all columns the
    reference holds (NaN columns -- samples no segment owns -- are skipped)."""
    a, ref = _cols(a), _cols(ref)
    scale = row_scale(ref) if scale is None else scale
    if cols is not None:
        a, ref = a[:, cols], ref[:, cols]
    if ref.shape[1] == 0:
        return 0.0
    return float(np.nanmax(np.abs(a - ref) / scale[:, None]))


def mass_bar(e_m, m0=M0):
    """The absolute bar on the mass row in kg."""
    return max(10.0 * e_m, 64.0 * EPS * m0)


# ---- dense output: the expected states

def dense_expected(O, XC, t, prm, td, first, method, steps, Y=None, base=0):
    """dense_reference.dense_expected for 14 rows: (node_ref, hop_ref), each [14 x len(td)], NaN where no segment owns the sample.
    node_ref: the oracle's DOP853 flow of the owning node.  hop_ref: the flow by (method, steps) of the sample before it -- column
    j-1 of Y, the states to be checked, or of hop_ref itself when Y is None (the oracle chained alone) -- and of the node for the
    first sample of a segment.  A span of zero is the start itself."""
    td = np.asarray(td, dtype=np.float64)
    node_ref = np.full((14, td.size), np.nan)
    hop_ref = np.full((14, td.size), np.nan)
    for i in range(len(first) - 1):
        prev, tprev = XC[:, i], t[i]
        for j in range(first[i] - base, first[i + 1] - base):
            node_ref[:, j] = flow14(O, XC[:, i], prm, td[j] - t[i])
            hop_ref[:, j] = flow14(O, prev, prm, td[j] - tprev, method, steps)
            prev, tprev = (hop_ref if Y is None else Y)[:, j], td[j]
    return node_ref, hop_ref


def final_expected(O, XC, t, prm, td, first, method, steps, Y=None, base=0):
    """What final_state holds: the last segment carried on to t[-1]; (from the node, from the segment's last sample)."""
    i = len(first) - 2
    node_ref = flow14(O, XC[:, i], prm, t[i + 1] - t[i])
    prev, tprev = XC[:, i], t[i]
    if first[i + 1] > first[i]:
        j = first[i + 1] - base - 1
        src = Y if Y is not None else dense_expected(O, XC, t, prm, td, first, method, steps, None, base)[1]
        prev, tprev = src[:, j], td[j]
    return node_ref, flow14(O, prev, prm, t[i + 1] - tprev, method, steps)


def densify_expected(O, XC, t, prm, n_desired, method, steps, Y=None):
    """lto_indirect_densify_mass's output by the oracle: (td, node_ref [14 x n_desired], hop_ref), the final state in the last
    column.  Y: the device's output (hop_ref then hops from the device's own previous sample)."""
    td = A.linrange(t[0], t[-1], n_desired)
    first = D.segment_ranges(t, td, False)
    node_ref, hop_ref = dense_expected(O, XC, t, prm, td, first, method, steps, Y)
    node_ref[:, -1], hop_ref[:, -1] = final_expected(O, XC, t, prm, td, first, method, steps, Y)
    return td, node_ref, hop_ref


# Singles n -> n_desired, the parameter set of each and whether the grid is a LinRange.  The p > 1 sets sit on the short fixtures:
# 10 N burns 190 kg per TU at full throttle, and the clamp clearance has to hold along the whole fixture.
DenseCase = collections.namedtuple("DenseCase", "n n_desired k lin methods")
DENSE_CASES = (DenseCase(2, 2, 2, False, ("dop853", "rk4x64")),
               DenseCase(2, 65, 1, False, ("dop853", "rk4x64", "rk4x8")),
               DenseCase(3, 2, 3, False, ("dop853", "rk4x64")),            # an empty segment
               DenseCase(13, 5, 4, False, ("dop853", "rk4x64")),           # most segments empty
               DenseCase(13, 13, 5, True, ("dop853", "rk4x64")),           # every sample a node, bit for bit
               DenseCase(66, 129, 0, False, ("dop853", "rk4x64")))         # S = 65 crosses a 64-lane block
BATCH_SETS = (0, 2, 5)                                                     # p = 1, 2, 0 in one call
BATCH_N = 9
BATCH_COUNTS = (11, 4, 17)


def case_id(c):
    return "%dto%d%s-%s" % (c.n, c.n_desired, "lin" if c.lin else "", SETS[c.k].name)


@functools.lru_cache(maxsize=None)
def case_reference(c, name):
    """(td, node_ref, hop_ref) of a dense case by the oracle alone, chained hop by hop with METHODS[name]."""
    X, t, prm = fixture(c.n, c.k, c.lin)
    method, steps = METHODS[name]
    return densify_expected(oracle_mod(), X, t, prm, c.n_desired, method, steps)


@functools.lru_cache(maxsize=None)
def self_errors():
    """(e_node, e_m): the oracle chained hop by hop (DOP853) against the oracle from the node over DENSE_CASES -- the largest
    per-row relative difference, and the largest absolute difference of the mass row in kg."""
    e_node = e_m = 0.0
    for c in DENSE_CASES:
        _, node_ref, hop_ref = case_reference(c, "dop853")
        e_node = max(e_node, rel_rows(hop_ref, node_ref))
        e_m = max(e_m, float(np.abs(hop_ref[6] - node_ref[6]).max()))
    return e_node, e_m


@functools.lru_cache(maxsize=None)
def e_inf():
    """Isp -> infinity: the oracle's 14-row flow at Isp = 1e30, rows IDX12, against the oracle's 12-row flow of the same node with
    mass M0, over the segments of the nine-node fixtures of every set; per-row relative."""
    O = oracle_mod()
    worst = 0.0
    for k, s in enumerate(SETS):
        X, t, prm = fixture(9, k, isp=1e30)
        prm12 = [MU, DU, TU, s.thrust, M0, 1.0, s.p, s.rho]
        for i in range(8):
            y14 = flow14(O, X[:, i], prm, t[i + 1] - t[i])
            y12, rc, _, _ = O.flow_state_costate(X[IDX12, i], prm12, t[i + 1] - t[i], O.DOP853_ADAPTIVE)
            assert rc == 0
            worst = max(worst, rel_rows(y14[IDX12], y12))
    return worst


# ---- re-mesh: the expected guess

new_grid, sources, scan64 = RM.new_grid, RM.sources, RM.scan64
REMESH_SHAPES = ((9, 7), (9, 9), (9, 17), (66, 130), (130, 66))
# (n, n_new, parameter set) of the node comparisons: every set once at least; the p > 1 sets and 10 N on the nine-node fixtures
REMESH_NODE_CASES = ((9, 7, 1), (9, 7, 2), (9, 9, 3), (9, 17, 4), (9, 17, 5), (66, 130, 0), (130, 66, 0))
# the batch of the re-solve: p = (1, 1, 0), exactly consistent fixtures (lambda_m(tf) = 0), each on a grid of its own
REMESH_BATCH = ((9, 0, 1), (9, 1, 2), (9, 5, 3))          # (n, set, gseed)


def remesh_batch_problem():
    """(XC [14 x 9 x 3], T [9 x 3], [prm])."""
    fx = [fixture(n, k, gseed=g) for n, k, g in REMESH_BATCH]
    return (np.asfortranarray(np.stack([f[0] for f in fx], axis=2)), np.asfortranarray(np.stack([f[1] for f in fx], axis=1)),
            [f[2] for f in fx])


def guess_expected(O, XC, t, prm, t_out, method, steps):
    """(want [14 x n_new], src, span): new node k = the oracle's flow by (method, steps) of old node src[k] over span[k]."""
    src, span = sources(t, t_out)
    want = np.zeros((14, len(t_out)))
    for k in range(len(t_out)):
        want[:, k] = flow14(O, XC[:, src[k]], prm, span[k], method, steps)
    return want, src, span


def trajectory_expected(O, XC, t, prm, t_out):
    """The oracle's DOP853 flow from node 0 to every t_out[k], carried from one t_out to the next."""
    want = np.zeros((14, len(t_out)))
    want[:, 0] = XC[:, 0]
    for k in range(1, len(t_out)):
        want[:, k] = flow14(O, want[:, k - 1], prm, t_out[k] - t_out[k - 1])
    return want
