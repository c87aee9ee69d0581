"""Host restatement of the trajectory-stacking initial guess (the block of CRTBP_Multishoot_direct_demo.jl:116-157):
plain numpy over a `flow(x, span)` callable.  The grid, the table spline and the 1001-candidate search are those of
addtime_reference.  The GPU tests compare lto_stack_guess_batch against it."""
import collections

import numpy as np

import addtime_reference as R

TAUS = np.arange(1001) / 1000.0

Stack = collections.namedtuple("Stack", "X t tau1 tau2_0 tau2 gap j n1 x1e xend d0 d1")


def wrap(tau):
    """The reference's wrap of a phase into [0, 1] (interpEndStates): one period at a time."""
    x = float(tau)
    while x > 1.0:
        x -= 1.0
    while x < 0.0:
        x += 1.0
    return x


def candidates(times, states):
    """The arrival table's spline at the 1001 candidates, [6 x 1001]."""
    return R.natural_spline(times, np.asarray(states)[:6], TAUS)


def stack(tau1, tof1, tof2, n, X0_times, X0_states, Xf_times, Xf_states, flow, S=None, x0=None):
    """The guess of one start.  flow(x [6], span > 0) -> x(span) [6].  S: candidates(Xf_times, Xf_states), if already at hand;
    x0: the departure spline at tau1, likewise (a caller that compares integrators passes the spline values under test).
    Returns Stack(X [6 x n], t [n], tau1 (wrapped), tau2_0, tau2, gap [2], j = the two winning candidates, n1 = nodes on arc 1,
    x1e = the end of arc 1, xend = node n-1 before the snap, d0 / d1 = the 1001 distances of the two searches)."""
    S = candidates(Xf_times, Xf_states) if S is None else S
    t = R.linrange(0.0, tof1 + tof2, n)
    X = np.zeros((6, n))
    w1 = wrap(tau1)
    x = R.natural_spline(X0_times, np.asarray(X0_states)[:6], [w1])[:, 0] if x0 is None else np.array(x0, dtype=np.float64)
    X[:, 0] = x
    n1 = int(np.count_nonzero(t < tof1))                  # strict (:122); t[0] = 0 < tof1, so n1 >= 1
    tcur = 0.0
    for k in range(1, n1):                                # node to node
        x = flow(x, t[k] - tcur)
        tcur = t[k]
        X[:, k] = x
    x1e = flow(x, tof1 - tcur) if tof1 > tcur else x
    j0, d0 = R.find_tau_from_samples(S, x1e)
    x = S[:, j0].copy()
    tcur = tof1
    for k in range(n1, n):
        if t[k] > tcur:
            x = flow(x, t[k] - tcur)
            tcur = t[k]
        X[:, k] = x
    xend = X[:, n - 1].copy()
    j1, d1 = R.find_tau_from_samples(S, xend)
    X[:, n - 1] = S[:, j1]
    return Stack(X, t, w1, TAUS[j0], TAUS[j1], np.array([d0[j0], d1[j1]]), (j0, j1), n1, x1e, xend, d0, d1)


def jacobi_constant(x, MU):
    """jacobiConstant (HelperFunctions.jl:10-15): C = x^2 + y^2 + 2 (1 - MU) / r1 + 2 MU / r2 - |v|^2, per column of x [6 x m]."""
    x = np.asarray(x, dtype=np.float64).reshape(6, -1)
    r1 = np.sqrt((x[0] + MU) ** 2 + x[1] ** 2 + x[2] ** 2)
    r2 = np.sqrt((x[0] - 1.0 + MU) ** 2 + x[1] ** 2 + x[2] ** 2)
    return x[0] ** 2 + x[1] ** 2 + 2.0 * (1.0 - MU) / r1 + 2.0 * MU / r2 - np.sum(x[3:6] ** 2, axis=0)


# The starts the GPU tests run (tests/test_stack_guess_gpu.py), vetted on the host (tests/test_stack_guess_host.py: no search of any
# of them is tied).  name -> (n, tau1, tof1 days, tof2 days): the smallest shapes at which the node / arc bookkeeping can go wrong.
CASES = {
    "n2": (2, 0.75, 10.0, 10.0),            # both nodes are end nodes; both arcs still run for the two searches
    "n3_mid": (3, 0.75, 10.0, 10.0),        # the middle node sits exactly at tof1: arc 2, zero span
    "n5_3_9": (5, 0.75, 3.0, 9.0),          # node 1 within rounding of tof1: whichever side the strict rule puts it
    "n5_4_8": (5, 0.75, 4.0, 8.0),          # arc 1 holds one interior node (3 days), arc 2 starts one day before its first node
    "n7_short": (7, 0.75, 1.0, 11.0),       # tof1 shorter than the first grid interval: arc 1 holds node 0 only
    "demo": (30, 0.75, 10.0, 10.0),         # the reference demo
    "wrap_hi": (5, 1.75, 4.0, 8.0),         # the wrap: same bits as n5_4_8
    "wrap_lo": (5, -0.25, 4.0, 8.0),
    # tof1 a thousandth of a day past a node: the end of arc 1 is a short hop from a stored node, so a host flow recovers it to
    # rounding and the junction search can be checked at its own precision
    "n3_late": (3, 0.75, 10.001, 9.999),
    "n30_late": (30, 0.6, 20.0 * 14.0 / 29.0 + 0.001, 20.0 * 15.0 / 29.0 - 0.001),
    # RK4 x 64 against the adaptive oracle: hops of 0.018 TU, the length of those the 1e-10 bar of the dense-output test was set on
    # (its 101 samples over twelve segments of 0.05 .. 0.25 TU); RK4's truncation error grows with the fifth power of the hop
    "rk4_short": (30, 0.75, 1.25, 1.0),
}
