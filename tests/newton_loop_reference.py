"""Host reference of the decisions the indirect Newton loop takes on the device between its sweeps and its solve
(lto_indirect_solve_batch: k_soc_mask, k_trial_points, k_defect_norms, k_pick_alpha / k_take_trial, k_axpy_traj, k_end_pins).
Nothing here calls the library: the heavy operators (STM sweep + structured solve, defect sweep) come in as an `ops` object, the
decisions are restated in exact arithmetic.

Layouts (struct-of-arrays, as include/lto.h states them):
  nodes         X[c][b*n + k]                  trajectory b, node k
  trial points  Xt[c][(b*NA + a)*n + k]        trial a of trajectory b
  defect block  defect[c][b*seg + i]           segment i of trajectory b
The numpy arrays of this module are [rows x nodes x batch] (Julia's layout); to_soa / from_soa / trials_to_soa convert."""
import math
from fractions import Fraction

import numpy as np

NA = 20
# NewtonBatch (lto_host.hpp): alphas[a] = 0.1 + (1.0 - 0.1) / (n_alpha - 1) * a, the last one exactly 1.0
ALPHAS = np.array([0.1 + (1.0 - 0.1) / (NA - 1) * a for a in range(NA)])
ALPHAS[NA - 1] = 1.0

U = 2.0 ** -53          # unit round-off of float64

# Pinned entries, restated from the comment above k_end_pins: node 0 rows 0 .. nd/2-1 (r0, v0; 14 rows: also m0), node n-1 rows
# 0-5 (rf, vf), and for 14 rows node n-1 row 13 (lambda_m(tf)), which is set to 0 on entry.
PIN_FIRST = {12: (0, 1, 2, 3, 4, 5), 14: (0, 1, 2, 3, 4, 5, 6)}
PIN_LAST = {12: (0, 1, 2, 3, 4, 5), 14: (0, 1, 2, 3, 4, 5, 13)}
PIN_ZERO = {12: (), 14: (13,)}


def pinned_mask(nd, n):
    m = np.zeros((nd, n), dtype=bool)
    m[list(PIN_FIRST[nd]), 0] = True
    m[list(PIN_LAST[nd]), n - 1] = True
    return m


def apply_entry_pins(X):
    """What the loop does to its input before the first sweep: the entries held at 0 are set."""
    X = np.array(X, dtype=np.float64, order="F")
    for r in PIN_ZERO[X.shape[0]]:
        X[r, -1] = 0.0
    return X


# ------------------------------------------------------------------------------------------------ exact arithmetic
def fma_exact(a, d, x):
    """The correctly rounded a*d + x, elementwise with broadcasting: float(Fraction(a) * Fraction(d) + Fraction(x)).
    Where an operand is not finite, IEEE arithmetic decides (a*d + x in floats gives the same NaN / inf as the fma).  Where a is
    0 or +-2^k and the product neither overflows nor underflows, a*d is exact and a*d + x is rounded once: the same value
    (tests/test_newton_loop_reference_host.py holds this short cut against the Fraction form)."""
    a, d, x = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(d, dtype=np.float64), np.asarray(x, dtype=np.float64))
    out = np.empty(a.shape, dtype=np.float64)
    af, df, xf, of = a.ravel(), d.ravel(), x.ravel(), out.reshape(-1)
    with np.errstate(all="ignore"):
        plain = af * df + xf
        prod = af * df
    finite = np.isfinite(af) & np.isfinite(df) & np.isfinite(xf)
    pow2 = (np.frexp(np.abs(af))[0] == 0.5) | (af == 0.0)
    exact_prod = pow2 & np.isfinite(prod) & ((np.abs(prod) >= 1e-290) | (af == 0.0) | (df == 0.0))
    of[:] = plain
    for i in np.flatnonzero(finite & ~exact_prod):
        of[i] = fma_fraction(af[i], df[i], xf[i])
    return out


def fma_fraction(a, d, x):
    """One element, the form the issue states."""
    r = Fraction(float(a)) * Fraction(float(d)) + Fraction(float(x))
    if r == 0:
        # the sign of an exact zero: +0 unless both addends are -0 (round to nearest)
        p_neg = math.copysign(1.0, float(a)) * math.copysign(1.0, float(d)) < 0
        return -0.0 if (p_neg and math.copysign(1.0, float(x)) < 0) else 0.0
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def twice_rounded(a, d, x):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64) * np.asarray(d, dtype=np.float64) + np.asarray(x, dtype=np.float64)


def first_minimiser(e):
    """kernels_util.hip: best = 0; for a = 1 ..: if e[a] < e[best]: best = a.  A NaN in slot 0 stays, a NaN later never wins."""
    best = 0
    for a in range(1, len(e)):
        if e[a] < e[best]:
            best = a
    return best


def _two_square(v):
    """v*v = p + e exactly (Dekker / Veltkamp), for |v| in [1e-140, 1e140]."""
    p = v * v
    c = 134217729.0 * v
    hi = c - (c - v)
    lo = v - hi
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    return p, e


def sumsq_exact(v):
    """The exact sum of squares of all entries of v, correctly rounded (math.fsum of exact squares; Fraction where a square could
    underflow or overflow).  NaN if any entry is NaN, inf if any is infinite."""
    v = np.asarray(v, dtype=np.float64).ravel()
    if np.isnan(v).any():
        return math.nan
    if np.isinf(v).any():
        return math.inf
    av = np.abs(v[v != 0.0])
    if av.size == 0:
        return 0.0
    if av.min() < 1e-140 or av.max() > 1e140:
        return float(sum(Fraction(float(q)) ** 2 for q in av))
    p, e = _two_square(av)
    return math.fsum(p.tolist() + e.tolist())


def sumsq_fraction(v):
    return sum((Fraction(float(q)) ** 2 for q in np.asarray(v, dtype=np.float64).ravel()), Fraction(0))


def sumsq_rational(v):
    """The exact sum of squares as a Fraction; the float NaN / inf where an entry is NaN / infinite."""
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        return math.nan
    if np.isinf(v).any():
        return math.inf
    return sumsq_fraction(v)


def maxabs(v):
    """max |v|, NaN if any entry is NaN (k_defect_norms: a NaN defect must surface)."""
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        return math.nan
    return float(np.abs(v).max()) if v.size else 0.0


# ------------------------------------------------------------------------------------------------ layouts
def to_soa(A):
    """[rows x per x B] -> [rows x (B*per)], column b*per + k."""
    A = np.asarray(A, dtype=np.float64)
    return np.ascontiguousarray(A.transpose(0, 2, 1).reshape(A.shape[0], -1))


def from_soa(D, per, B):
    """[rows x >= B*per] -> [rows x per x B]."""
    D = np.asarray(D)
    return np.asfortranarray(D[:, :per * B].reshape(D.shape[0], B, per).transpose(0, 2, 1))


def trials_to_soa(Xt):
    """[rows x n x NA x B] -> [rows x (B*NA*n)], column (b*NA + a)*n + k."""
    Xt = np.asarray(Xt, dtype=np.float64)
    return np.ascontiguousarray(Xt.transpose(0, 3, 2, 1).reshape(Xt.shape[0], -1))


def trials_from_soa(D, per, na, B):
    """[rows x >= B*na*per] -> [rows x per x na x B]."""
    D = np.asarray(D)
    return np.ascontiguousarray(D[:, :B * na * per].reshape(D.shape[0], B, na, per).transpose(0, 3, 2, 1))


def trial_points(X, delta, alphas=ALPHAS):
    """[rows x n x B] -> [rows x n x NA x B]: fma_exact(alphas[a], delta, X)."""
    al = np.asarray(alphas, dtype=np.float64)
    return fma_exact(al[None, None, :, None], np.asarray(delta)[:, :, None, :], np.asarray(X)[:, :, None, :])


# ------------------------------------------------------------------------------------------------ NewtonBatch
def loop_counters(er, max_iter, tol=1e-10):
    """(status before the NaN rule, iterations, iterations done) of one trajectory as NewtonBatch::next and the loop's abort rule
    produce them, from er[j-1] = max |defect| after iteration j (as many entries as the trajectory can need)."""
    it, h_er, done = 0, 1.0, 0
    while True:
        if not (h_er > tol):
            return 0, it, done
        it += 1
        if it > max_iter:
            return 1, it, done
        h_er = er[done]
        done += 1
        if h_er > 1e3:
            it += 100


def still_active(er_prev, was_active, tol=1e-10):
    """Whether a trajectory does one more iteration after one that ended with max |defect| = er_prev."""
    return bool(was_active and er_prev > tol and not er_prev > 1e3)


# ------------------------------------------------------------------------------------------------ one iteration
class Replay:
    """What replay_iteration found: per trajectory the step, the decisions and the line search's sums."""

    def __init__(self, B):
        self.delta = None                       # [rows x n x B] the step with the correction where it was taken
        self.max_delta = [math.nan] * B          # max |xc_update| before the correction
        self.soc = [False] * B                   # second-order correction taken
        self.searched = [False] * B
        self.ss = [None] * B                     # 20 exact sums of squares (searched trajectories)
        self.alpha_ref = [0.0] * B               # 0 for a frozen trajectory
        self.accepted = [None] * B               # the step lengths a device pick may have (more than one: near tie)
        self.separation = [math.nan] * B         # (runner-up - minimum) / minimum of the searched trajectories


def replay_iteration(ops, X, iteration, active, adjoints_only, soc_threshold=1e-1):
    """Iteration `iteration` (1-based) of the loop from the state X [rows x n x B] after iteration - 1 iterations.
    ops.newton(X) -> delta (STM sweep + solve, keeps the factorisation), ops.resolve(d) -> delta from the stored factorisation,
    ops.defect(X) -> [rows x (n-1) x B], ops.trial_defect(Xt [rows x n x NA x B]) -> [rows x (n-1) x NA x B]."""
    X = np.asarray(X, dtype=np.float64)
    nd, n, B = X.shape
    r = Replay(B)
    delta = np.array(ops.newton(X), dtype=np.float64)
    pin = pinned_mask(nd, n)
    for b in range(B):
        if not active[b] or np.isnan(delta[:, :, b]).any():
            continue
        assert np.all(delta[:, :, b][pin] == 0.0), "the step moves a pinned entry (trajectory %d)" % b
        if adjoints_only:
            assert np.all(delta[:nd // 2, :, b] == 0.0), "adjoints-only step with a state update (trajectory %d)" % b
    r.max_delta = [maxabs(delta[:, :, b]) for b in range(B)]
    # second-order correction (indirect.jl:190-214; k_soc_mask): active, max |xc_update| < 0.1 and not NaN
    r.soc = [bool(active[b] and r.max_delta[b] == r.max_delta[b] and r.max_delta[b] < soc_threshold) for b in range(B)]
    if any(r.soc):
        d2 = ops.defect(X + delta)
        delta2 = np.asarray(ops.resolve(d2), dtype=np.float64)
        for b in range(B):
            if r.soc[b]:
                delta[:, :, b] = delta[:, :, b] + delta2[:, :, b]
    r.delta = delta
    # line search from iteration 4 (indirect.jl:300; k_trial_points, k_defect_norms, k_pick_alpha / k_take_trial)
    r.searched = [bool(active[b] and iteration > 3) for b in range(B)]
    if any(r.searched):
        dt = np.asarray(ops.trial_defect(trial_points(X, delta)))
        count = nd * (n - 1)
        for b in range(B):
            if not r.searched[b]:
                continue
            ss = [sumsq_rational(dt[:, :, a, b]) for a in range(NA)]
            best = first_minimiser(ss)
            r.ss[b] = ss
            r.alpha_ref[b] = float(ALPHAS[best])
            r.accepted[b] = [float(ALPHAS[best])]
            if isinstance(ss[best], Fraction):
                # a pick whose exact sum lies within relative 2 N 2^-53 of the minimum is one a correct device sum may take (an
                # exact tie too: the device's own rounding may separate the two)
                lim = ss[best] * (1 + Fraction(2 * count) * Fraction(U))
                r.accepted[b] = [float(ALPHAS[a]) for a in range(NA) if ss[a] <= lim]
                others = [ss[a] for a in range(NA) if a != best and ss[a] == ss[a]]
                if others and ss[best] > 0:
                    r.separation[b] = float((min(others) - ss[best]) / ss[best]) if min(others) != math.inf else math.inf
    for b in range(B):
        if active[b] and not r.searched[b]:
            r.alpha_ref[b] = 1.0
            r.accepted[b] = [1.0]
        elif not active[b]:
            r.alpha_ref[b] = 0.0
            r.accepted[b] = [0.0]
    return r


def apply_step(X, delta, alpha, X_entry):
    """X_{k+1}: fma_exact(alpha[b], delta, X) per trajectory, a frozen one (alpha 0) keeps X exactly whatever delta holds, then the
    pinned entries restored from the loop's entry state X_entry."""
    X = np.asarray(X, dtype=np.float64)
    nd, n, B = X.shape
    out = np.array(X, order="F")
    pin = pinned_mask(nd, n)
    for b in range(B):
        if alpha[b] != 0.0:
            out[:, :, b] = fma_exact(float(alpha[b]), delta[:, :, b], X[:, :, b])
        out[:, :, b][pin] = np.asarray(X_entry)[:, :, b][pin]
    return out
