"""CPU: a free time of flight in the direct method's free-end step -- the host reference step direct_qp_dense_free_tf against the
optimality conditions and against the pinned-tf step, the mirror loop with free tf on the CPU oracle, and the new C entry points'
argument checks."""
import ctypes as C

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import _lib, drivers, synth
from oracle import oracle as O

import direct_helpers as DH

C2 = (lto.DU / lto.TU) ** 2
ISP = 2000.0
DAY = lto.day / lto.TU


def _tf_problem(n, ns, seed, tau, shift):
    X, U, T = synth.direct_problem(n, nstate=ns, seed=seed)
    X, U, t = X[:, :, 0].copy(), U[:, :, 0].copy(), T[:, 0]
    tabs = DH.tables()
    a0, af = drivers.interpEndStates(tau[0] + shift[0], tau[1] + shift[1], *tabs)
    X[:6, 0], X[:6, -1] = a0, af
    rng = np.random.default_rng(seed)
    dV1, dV2 = 1e-4 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)
    Jt, dtf, d = DH.dtf(X, U, t)
    model = drivers.end_model(tau[0], tau[1], *tabs)
    return Jt, dtf, d, X, U, t, model, 1000.0, dV1, dV2


def _kkt_check(Jt, dtf, d, X, U, t, model, mass, dV1, dV2, beta, imp, tfb, sol):
    """Independent optimality check: feasibility, stationarity with least-squares multipliers, the signs of the active bounds.
    Returns the tuple of active bounds (-1 lower, 0 free, +1 upper) of (p1, p2, p3)."""
    s0, sf, g0, gf, c0, cf = model
    dx, du, d1, d2, p1, p2, p3, cost = sol
    step, tf_min, tf_max = tfb
    tf = t[-1]
    lo = np.array([-0.1, -0.1, max(-step, tf_min - tf)])
    hi = np.array([0.1, 0.1, min(step, tf_max - tf)])
    p = np.array([p1, p2, p3])
    assert np.all(p >= lo) and np.all(p <= hi)
    ns, _, S = Jt.shape
    n = S + 1
    w = np.zeros(n)
    w[:-1] += np.diff(t) / 2
    w[1:] += np.diff(t) / 2
    nz = ns * n + 3 * n + 9
    iu, iv, ip = ns * n, ns * n + 3 * n, ns * n + 3 * n + 6
    z = np.r_[dx.T.reshape(-1), du.T.reshape(-1), d1, d2, p]
    grad = np.zeros(nz)
    grad[iu:iv] = 2 * np.repeat(w, 3) * (U + du).T.reshape(-1)
    grad[iv:ip] = 2 * C2 * np.r_[dV1 + d1, dV2 + d2]
    grad[ip], grad[ip + 1] = beta * c0 * p1, beta * cf * p2
    A, b = [], []
    for i in range(S):
        r = np.zeros((ns, nz))
        r[:, ns * i:ns * (i + 2)] = Jt[:, :2 * ns, i]
        r[:, iu + 3 * i:iu + 3 * i + 6] = Jt[:, 2 * ns:, i]
        r[:, ip + 2] = dtf[:, i]
        A.append(r)
        b.append(-d[:, i])
    for k, s, g, dv, o in ((0, s0, g0, dV1, 0), (n - 1, sf, gf, dV2, 1)):
        r = np.zeros((6, nz))
        r[:, ns * k:ns * k + 6] = np.eye(6)
        r[3:, iv + 3 * o:iv + 3 * o + 3] = np.eye(3)
        r[:, ip + o] = -g
        A.append(r)
        b.append(s - X[:6, k] - np.r_[0, 0, 0, dv])
    if ns == 7:
        r = np.zeros((1, nz))
        r[0, 6] = 1
        A.append(r)
        b.append([mass - X[6, 0]])
    if not imp:
        r = np.zeros((6, nz))
        r[:, iv:ip] = np.eye(6)
        A.append(r)
        b.append(np.zeros(6))
    act = [(j, -1 if p[j] == lo[j] else 1) for j in range(3) if p[j] == lo[j] or p[j] == hi[j]]
    for j, _ in act:
        r = np.zeros((1, nz))
        r[0, ip + j] = 1
        A.append(r)
        b.append([0.0])
    A = np.vstack(A)
    b = np.concatenate([np.atleast_1d(v) for v in b])
    ne = A.shape[0] - len(act)
    res = A[:ne] @ z - b[:ne]
    assert np.abs(res).max() <= 1e-10 * max(1.0, np.abs(b).max())                  # feasibility
    D = 1.0 / np.maximum(np.abs(A).max(axis=0), 1e-300)
    lam, *_ = np.linalg.lstsq((A * D[None, :]).T, -grad * D, rcond=None)
    r = (A * D[None, :]).T @ lam + grad * D
    assert np.abs(r).max() <= 1e-8 * max(1.0, np.abs(grad * D).max())              # stationarity
    for (j, sgn), mu in zip(act, lam[ne:]):                                         # upper bound: mu >= 0, lower: mu <= 0
        assert sgn * mu >= -1e-8 * max(1.0, np.abs(lam).max())
    cost_ref = np.sum(w * np.sum((U + du) ** 2, axis=0)) + C2 * (np.sum((dV1 + d1) ** 2) + np.sum((dV2 + d2) ** 2)) + \
        beta * (c0 / 2 * p1 ** 2 + cf / 2 * p2 ** 2)
    assert abs(cost - cost_ref) <= 1e-10 * abs(cost_ref)
    kinds = [0, 0, 0]
    for j, sgn in act:
        kinds[j] = sgn
    return tuple(kinds), p3, lo[2], hi[2], step


CASES = [((0.3, 0.6), (0.02, -0.03)), ((0.3, 0.6), (0.4, 0.01)), ((0.2, 0.7), (-0.4, 0.4))]


@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
def test_dense_free_tf_step_satisfies_kkt(ns, imp):
    """beta = 0, 1, 100 on three problems, each with a wide step (p3 interior), a tight step (p3 at +-step) and absolute bounds just
    around tf (p3 at tf_min - tf or tf_max - tf); combinations with p1 or p2 at +-0.1 come from the problems' phase shifts."""
    seen = set()
    for k, (tau, shift) in enumerate(CASES):
        Jt, dtf, d, X, U, t, model, mass, dV1, dV2 = _tf_problem(6, ns, 11 + k, tau, shift)
        tf = t[-1]
        for tfb in ((50.0, t[0] + 1e-3, tf + 100.0), (1e-5, t[0] + 1e-3, tf + 100.0), (1.0, tf - 1e-6, tf + 1e-6)):
            for beta in (0.0, 1.0, 100.0):
                sol = drivers.direct_qp_dense_free_tf(Jt, dtf, d, X, U, t, *model, beta, mass, dV1, dV2, lto.DU, lto.TU, tf, tfb,
                                                      allowImpulsive=imp)
                kinds, p3, lo3, hi3, step = _kkt_check(Jt, dtf, d, X, U, t, model, mass, dV1, dV2, beta, imp, tfb, sol)
                cat = "interior" if kinds[2] == 0 else ("step" if abs(p3) == step else "absolute")
                seen.add((cat, kinds[0] != 0 or kinds[1] != 0))
                if not imp:
                    assert np.all(sol[2] == 0) and np.all(sol[3] == 0)
    cats = {c for c, _ in seen}
    assert cats == {"interior", "step", "absolute"}, seen
    assert any(pb for _, pb in seen), seen              # some case with p1 or p2 at its bound


@pytest.mark.parametrize("ns,imp", [(6, False), (7, True)])
def test_dense_free_tf_step_with_pinned_tf_is_the_free_step(ns, imp):
    """step = 0, or a zero tf column: the pinned-tf free step (dense, 1e-12).  And a free tf never costs more than a pinned one."""
    Jt, dtf, d, X, U, t, model, mass, dV1, dV2 = _tf_problem(7, ns, 3, (0.3, 0.6), (0.03, -0.02))
    tf = t[-1]
    for beta in (0.0, 1.0):
        ref = drivers.direct_qp_dense_free(Jt, d, X, U, t, *model, beta, mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
        for col, tfb in ((dtf, (0.0, t[0] + 1e-3, tf + 10)), (np.zeros_like(dtf), (0.2, t[0] + 1e-3, tf + 10))):
            sol = drivers.direct_qp_dense_free_tf(Jt, col, d, X, U, t, *model, beta, mass, dV1, dV2, lto.DU, lto.TU, tf, tfb,
                                                  allowImpulsive=imp)
            for a, b in zip(sol[:4], ref[:4]):
                assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
            assert abs(sol[4] - ref[4]) <= 1e-12 and abs(sol[5] - ref[5]) <= 1e-12
            assert abs(sol[7] - ref[6]) <= 1e-12 * abs(ref[6])
            assert abs(sol[6]) <= tfb[0]
        free = drivers.direct_qp_dense_free_tf(Jt, dtf, d, X, U, t, *model, beta, mass, dV1, dV2, lto.DU, lto.TU, tf,
                                               (DAY, t[0] + DAY, 40 * DAY), allowImpulsive=imp)
        assert free[7] <= ref[6] * (1 + 1e-12)


def test_oracle_tf_column_matches_the_central_difference():
    X, U, T = synth.direct_problem(8, seed=5)
    X, U, t = X[:, :, 0], U[:, :, 0], T[:, 0]
    _, dtf, _ = DH.dtf(X, U, t)
    fd = O.direct_dtf_fd(X, U, t, 10, lto.MU, lto.DU, lto.TU, ISP)
    assert np.abs(dtf - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())


def check_tf_history(hist, iters, tf0, tfb):
    """tf moves only on odd iterations, by at most alpha step, and stays in [tf_min, tf_max]."""
    step, tf_min, tf_max = tfb
    prev = tf0
    for k in range(iters):
        tf_k = hist[5, k]
        if k % 2 == 1:
            assert tf_k == prev
        assert abs(tf_k - prev) <= hist[2, k] * step * (1 + 1e-12)
        assert tf_min <= tf_k <= tf_max
        prev = tf_k


def test_mirror_loop_with_free_tf_converges_on_oracle():
    """The 8-node problem of the free-end mirror test with tf free (1-day step): the loop converges, tf moves, and the returned
    grid is t0 + (tau_grid + 1) / 2 (tf - t0) of the final tf."""
    n = 8
    X, U, T = synth.direct_problem(n, seed=5)
    X, U, t = X[:, :, 0].copy(), U[:, :, 0].copy(), T[:, 0]
    tabs = DH.tables()
    s0, sf = drivers.interpEndStates(0.32, 0.58, *tabs)
    X[:6, 0], X[:6, -1] = s0, sf
    tfb = drivers.tf_bounds_default(t[0], lto.TU)
    out, last = drivers.direct_loop_host(X, U, 0.3, 0.6, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, n, 10, 1000.0, ISP, *tabs,
                                         True, 0.0, False, 30, DH.OracleDirectOps(), verbose=False, tf_bounds=tfb)
    Xo, Uo, tau1, tau2, to, dV1, dV2, defect = out
    hist, iters = last["history"], last["iterations"]
    print("free-tf mirror (oracle, 8 nodes): status %d, %d iterations, tf %.9f -> %.9f TU" % (last["status"], iters, t[-1],
                                                                                               hist[5, iters - 1]))
    assert last["status"] == 0 and np.abs(defect).max() <= 1e-6
    assert hist.shape[0] == 6 and hist[5, iters - 1] != t[-1]
    check_tf_history(hist, iters, t[-1], tfb)
    tau_grid = (t - t[0]) / (t[-1] - t[0]) * 2 - 1
    tf = hist[5, iters - 1]
    assert np.array_equal(to, t[0] + (tau_grid + 1) / 2 * (tf - t[0]))
    d_o, _ = O.direct_defect(Xo, Uo, to, 10, lto.MU, lto.DU, lto.TU, ISP)
    assert np.abs(d_o).max() <= 1e-6


def test_mirror_loop_tf_bounds_none_and_zero_step_keep_the_pinned_loop():
    n = 8
    X, U, T = synth.direct_problem(n, seed=5)
    X, U, t = X[:, :, 0].copy(), U[:, :, 0].copy(), T[:, 0]
    tabs = DH.tables()
    args = (X, U, 0.3, 0.6, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, n, 10, 1000.0, ISP, *tabs, True, 0.0, False, 6,
            DH.OracleDirectOps())
    a, la = drivers.direct_loop_host(*args, verbose=False)
    b, lb = drivers.direct_loop_host(*args, verbose=False, tf_bounds=(0.0, t[0] + DAY, 40 * DAY))
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    k = la["iterations"]
    assert np.array_equal(la["history"][:, :k], lb["history"][:5, :k]) and np.all(lb["history"][5, :k] == t[-1])


def test_free_tf_entry_points_without_a_device():
    lib = lto.load_library()
    for name in ("lto_direct_qp_step_free_tf", "lto_direct_solve_free_tf_batch", "lto_direct_solve_free_tf"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert C.sizeof(_lib.LtoDirectTfBounds) == 24
    x = np.zeros(64)
    p = x.ctypes.data_as(C.c_void_p)
    t = np.linspace(0.0, 4.0, 4)
    pt = t.ctypes.data_as(C.c_void_p)
    prm = _lib.LtoDirectParams(lto.MU, lto.DU, lto.TU, ISP)
    tg = lto.direct_targets(np.zeros(6), np.zeros(6), 1000.0, np.zeros(3), np.zeros(3))
    em = lto.direct_end_model(np.zeros(6), np.zeros(6), 0.0, 0.0)
    ob = lto.DirectOrbits(*DH.tables())
    st = (C.c_int * 1)()
    good = lto.direct_tf_bounds(0.2, 1.0, 9.0)

    def step(tb, ns=6, n=4):
        return lib.lto_direct_qp_step_free_tf(None, ns, n, 1, p, p, pt, 1, 10, C.byref(prm), C.byref(tg), C.byref(em), p, C.byref(tb),
                                              1, 0, p, p, p, p, p)

    def solve(tb, ns=6, n=4):
        return lib.lto_direct_solve_free_tf_batch(None, ns, n, 1, p, p, pt, 1, 10, C.byref(prm), C.byref(ob.struct), C.byref(tg), 1,
                                                  p, p, C.byref(tb), 1, 0, 10, p, p, p, p, p, p, st, None, None)
    assert step(good) == _lib.LTO_ENULL and solve(good) == _lib.LTO_ENULL
    assert lib.lto_direct_solve_free_tf(None, 6, 4, p, p, pt, 10, C.byref(prm), C.byref(ob.struct), C.byref(tg), p, 0.0,
                                        C.byref(good), 1, 0, 10, p, p, p, p, p, p, st, None, None) == _lib.LTO_ENULL
    for bad in (lto.direct_tf_bounds(-0.1, 1.0, 9.0),          # step < 0
                lto.direct_tf_bounds(0.2, 1.0, 3.5),           # tf = 4 above tf_max
                lto.direct_tf_bounds(0.2, 4.5, 9.0),           # tf = 4 below tf_min
                lto.direct_tf_bounds(0.2, 0.0, 9.0),           # tf_min <= t0: an empty grid allowed
                lto.direct_tf_bounds(0.2, -1.0, 9.0)):
        assert step(bad) == _lib.LTO_EINVAL and solve(bad) == _lib.LTO_EINVAL
    for ns, n in ((5, 4), (8, 4), (6, 1)):
        assert step(good, ns, n) == _lib.LTO_EINVAL and solve(good, ns, n) == _lib.LTO_EINVAL
