"""The direct multiple-shooting loop on the device (lto_direct_solve_batch, lto_direct_solve_free_batch,
lto_direct_solve_free_tf_batch), one iteration at a time.

maxIter = k makes the loop do exactly k iterations (fewer for a trajectory that leaves earlier) and maxIter = 0 returns the start, so
the outputs of the run with maxIter = k are the device loop's state after k iterations and row k - 1 of its history is (max|defect|,
cost, alpha (, tau1, tau2 (, tf))) of iteration k.  For every k, direct_loop_reference.replay_iteration recomputes iteration k + 1 from
the device's own state k, twice: with the library's one-step entries and DirectPlan.defect at the loop's own shapes and every decision
in between on the host in exact arithmetic (the device-step layer, bit for bit), and with the CPU oracle's sweeps and the dense host
QPs (the independent layer, to the tolerances of the existing step and defect tests).  Nothing accumulates from step to step.

The problem sets are vetted on the CPU (tests/test_direct_loop_reference_host.py).  The quotas at the end are asserted over the
device's own runs, after the counts behind them are printed."""
import time

import numpy as np
import pytest

import direct_loop_reference as R
import lowthrustopt_amd as lto

pytestmark = pytest.mark.gpu

MARGIN = 1e-3                     # a searched pick is compared with the replay's when the replay's margin is at least this
SET_NAMES = ("A", "B", "C", "D", "E", "F")
FIELDS = ("X", "U", "dV", "t", "defect", "tau")

_SETS, _CASES = {}, {}


def sets():
    if not _SETS:
        _SETS.update(R.problem_sets())
    return _SETS


def solve(v, max_iter, ctx, kind=None):
    """One run of the variant's entry point: dict of X, U, dV [6 x B], t, defect, tau [2 x B], status, iters and hist
    [rows x maxIter x B] as the entry returns it (3, 5 or 6 rows)."""
    kind = kind or v.kind
    tg = [lto.direct_targets(np.zeros(6), np.zeros(6), v.mass, v.dV[:3, b], v.dV[3:, b]) for b in range(v.B)]
    common = (v.X, v.U, v.t_entry, v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp)
    if kind == "frozen":
        for b in range(v.B):
            s0, sf = R.drivers.interpEndStates(v.tau[0, b], v.tau[1, b], *v.tabs)
            tg[b] = lto.direct_targets(s0, sf, v.mass, v.dV[:3, b], v.dV[3:, b])
        X, U, dV, t, d, st, its, h = lto.direct_solve(*common, tg, allowImpulsive=v.allow_impulsive, maxIter=max_iter, ctx=ctx)
        tau = v.tau.copy()
    elif kind == "free":
        X, U, dV, t, d, tau, st, its, h = lto.direct_solve_free(*common, lto.DirectOrbits(*v.tabs), tg, v.tau, v.beta, flagEnd=True,
                                                                allowImpulsive=v.allow_impulsive, maxIter=max_iter, ctx=ctx)
    else:
        tb = [lto.direct_tf_bounds(*q) for q in v.tf_bounds]
        X, U, dV, t, d, tau, st, its, h = lto.direct_solve_free_tf(*common, lto.DirectOrbits(*v.tabs), tg, v.tau, v.beta, tb, flagEnd=True,
                                                                   allowImpulsive=v.allow_impulsive, maxIter=max_iter, ctx=ctx)
    return dict(X=X, U=U, dV=dV, t=t, defect=d, tau=tau, status=st, iters=its, hist=h)


def state_of(v, run, k):
    """The loop's state after k iterations from the run with maxIter = k: tf is the history's, the entry's before the first row."""
    B = v.B
    tf = np.full(B, v.t_entry[-1])
    if v.kind == "free_tf":
        for b in range(B):
            j = min(k, int(run["iters"][b]))
            if j > 0:
                tf[b] = run["hist"][5, j - 1, b]
    return R.State(run["X"], run["U"], run["dV"][:3].copy(), run["dV"][3:].copy(), run["tau"][0].copy(), run["tau"][1].copy(), tf, run["t"])


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def case(name, ctx):
    """Runs a set once per session: the device loop with maxIter = 0 .. K and both replays of every iteration from the device's own
    states.  Asserts nothing; the tests below read it."""
    if name in _CASES:
        return _CASES[name]
    v = sets()[name]
    t_start = time.perf_counter()
    full = solve(v, v.max_iter, ctx)
    count = [int(c) for c in full["iters"]]
    K = max(count)
    runs = [solve(v, k, ctx) for k in range(K + 1)]
    states = [state_of(v, runs[k], k) for k in range(K + 1)]
    hist = runs[K]["hist"]
    dev_be, cpu_be = R.DeviceStepBackEnd(ctx, v), R.OracleBackEnd(v.Isp)
    c = dict(v=v, full=full, count=count, K=K, runs=runs, states=states, hist=hist, dev=[], cpu=[], active=[], jac_defect=[], seconds={})
    try:
        c["defect0"] = dev_be.defect(v, v.X, v.U, states[0].t)
        t_dev = t_cpu = 0.0
        for k in range(K):
            active = [k < count[b] for b in range(v.B)]
            alpha = [float(hist[2, k, b]) if active[b] else 0.0 for b in range(v.B)]
            c["active"].append(active)
            t0 = time.perf_counter()
            c["jac_defect"].append(dev_be.jacobian_defect(v, states[k].X, states[k].U, states[k].t))
            c["dev"].append(R.replay_iteration(states[k], k + 1, v, dev_be, active, alpha))
            t1 = time.perf_counter()
            c["cpu"].append(R.replay_iteration(states[k], k + 1, v, cpu_be, active, alpha))
            t_dev, t_cpu = t_dev + t1 - t0, t_cpu + time.perf_counter() - t1
    finally:
        dev_be.close()
    # whether the loop's QP and the step entries' QP read the same defect bits at every state of this set (the second premise)
    c["premise"] = all(same(c["jac_defect"][k], runs[k]["defect"]) for k in range(K))
    c["seconds"] = dict(total=time.perf_counter() - t_start, device_replay=t_dev, cpu_replay=t_cpu)
    print("set %s (%s, nstate %d, B %d): device iterations %s, status %s; %.1f s (device replays %.1f s, CPU replays %.1f s)" % (
        name, v.kind, v.nstate, v.B, count, list(full["status"]), c["seconds"]["total"], t_dev, t_cpu))
    _CASES[name] = c
    return c


def tol_abs(ref, rel=1e-9):
    """The tolerance of the existing step tests for the device step against the dense host QP: 1e-9 relative to max(1, |.|)."""
    ref = np.asarray(ref, dtype=np.float64)
    return rel * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)


def close(a, ref, rel=1e-9):
    return float(np.abs(np.asarray(a) - np.asarray(ref)).max()) <= tol_abs(ref, rel)


@pytest.mark.parametrize("name", SET_NAMES)
def test_the_loop_and_the_step_entries_read_the_same_defect(gpu_ctx, name):
    """The loop's QP reads the defect of k_direct_defect (defect_out of the run with maxIter = k), the one-step entries the one
    k_direct_jacobian emits: bit-equal at every state of every set, i.e. at every shape and nstate used here, with U = 0 and U != 0."""
    c = case(name, gpu_ctx)
    worst = max(float(np.abs(c["jac_defect"][k] - c["runs"][k]["defect"]).max()) for k in range(c["K"]))
    print("set %s: largest |defect of the Jacobian sweep - defect of the defect sweep| over %d states: %.3e" % (name, c["K"], worst))
    assert same(c["defect0"], c["runs"][0]["defect"]), "maxIter = 0 returns the defect sweep of the start"
    for k in range(c["K"]):
        assert same(c["jac_defect"][k], c["runs"][k]["defect"]), (name, k)
    assert np.any(c["states"][c["K"] - 1].U != 0.0)


@pytest.mark.parametrize("name", SET_NAMES)
def test_leavers_and_counters(gpu_ctx, name):
    c = case(name, gpu_ctx)
    v, runs, count, K, hist = c["v"], c["runs"], c["count"], c["K"], c["hist"]
    # maxIter = 0 returns the start
    r0 = runs[0]
    assert same(r0["X"], v.X) and same(r0["U"], v.U) and same(r0["dV"], v.dV) and same(r0["tau"], v.tau)
    assert all(same(r0["t"][:, b], v.t_entry) for b in range(v.B))
    for b in range(v.B):
        er = list(hist[0, :count[b], b])
        assert not np.isnan(er).any()
        for k in range(K + 1):
            r = runs[k]
            status, its = R.loop_counters(er, k)
            assert (int(r["status"][b]), int(r["iters"][b])) == (status, its), (name, "counters", b, k)
            assert its == min(k, count[b])
            # the history of a shorter run is the longer run's, and rows past the count keep the wrapper's NaN fill
            assert same(r["hist"][:, :its, b], hist[:, :its, b]), (name, "history of maxIter = %d" % k, b)
            assert np.isnan(r["hist"][:, its:, b]).all(), (name, "history rows past the count", b, k)
            if k > count[b]:                               # a trajectory that has left never moves again
                for f in FIELDS:
                    assert same(r[f][..., b], runs[count[b]][f][..., b]), (name, "a trajectory that left moved", f, b, k)
        assert (int(c["full"]["status"][b]), int(c["full"]["iters"][b])) == (int(runs[K]["status"][b]), count[b])
        assert same(c["full"]["hist"][:, :count[b], b], hist[:, :count[b], b]) and np.isnan(c["full"]["hist"][:, count[b]:, b]).all()
    if name in ("E", "F"):                                 # stopped by maxIter: E at 16, F at 14
        assert list(c["full"]["status"]) == [1] and count == [v.max_iter] and v.max_iter == {"E": 16, "F": 14}[name]
    else:
        assert all(int(s) == 0 for s in c["full"]["status"])
    if name == "F":                                        # the one set whose impulses move, also on iterations with alpha < 1
        dV = np.array([runs[k]["dV"][:, 0] for k in range(K + 1)])
        assert all(np.all(dV[k + 1] != dV[k]) for k in range(K)) and sum(1 for k in range(K) if hist[2, k, 0] < 1.0) >= 2


@pytest.mark.parametrize("name", SET_NAMES)
def test_decisions(gpu_ctx, name):
    c = case(name, gpu_ctx)
    v, count, hist = c["v"], c["count"], c["hist"]
    for b in range(v.B):
        prev = np.array([v.tau[0, b], v.tau[1, b], v.t_entry[-1]])
        for k in range(count[b]):
            it, rep = k + 1, c["dev"][k]
            alpha = float(hist[2, k, b])
            if it <= R.SEARCH_AFTER:
                assert alpha == 1.0, (name, b, it, alpha)
            else:
                assert alpha in list(R.ALPHAS), (name, "alpha off the grid", b, it, alpha)
                if rep.margin[b] >= MARGIN:
                    assert alpha == float(R.ALPHAS[rep.pick[b]]), (name, "pick", b, it, alpha, rep.pick[b], rep.margin[b])
            if v.kind == "frozen":
                continue
            now = np.array([hist[3, k, b], hist[4, k, b], hist[5, k, b] if v.kind == "free_tf" else v.t_entry[-1]])
            if it % 2 == 0:                                # tau1, tau2 and tf change on odd iterations only
                assert same(now, prev), (name, "phases or tf moved on an even iteration", b, it)
            assert np.all(np.abs(now[:2] - prev[:2]) <= 0.1 * alpha * (1 + 1e-12))
            if v.kind == "free_tf":
                step, lo, hi = v.tf_bounds[b]
                assert lo <= now[2] <= hi and abs(now[2] - prev[2]) <= alpha * step * (1 + 1e-12), (name, "tf", b, it)
                if step == 0.0:
                    assert now[2] == v.t_entry[-1]
            prev = now


def test_a_pinned_tf_beside_a_free_one_is_its_free_end_run(gpu_ctx):
    """Set D's second trajectory has step = 0 beside one with a positive step: tf never moves and the whole run equals its
    lto_direct_solve_free_batch run bit for bit."""
    c = case("D", gpu_ctx)
    v, full = c["v"], c["full"]
    free = solve(v.single(1), v.max_iter, gpu_ctx, kind="free")
    k = c["count"][1]
    assert np.all(full["hist"][5, :k, 1] == v.t_entry[-1])
    assert (int(free["status"][0]), int(free["iters"][0])) == (int(full["status"][1]), k)
    worst = {f: float(np.abs(full[f][..., 1] - free[f][..., 0]).max()) for f in FIELDS}
    print("set D, step-0 trajectory against its free-end run: largest differences %s" % worst)
    assert same(full["hist"][:5, :k, 1], free["hist"][:, :k, 0])
    for f in FIELDS:
        assert same(full[f][..., 1], free[f][..., 0]), (f, worst[f])


@pytest.mark.parametrize("name", SET_NAMES)
def test_device_step_layer(gpu_ctx, name):
    """State k + 1 and history rows 0-1 are the replay's, bit for bit -- given that the loop and the step entries read the same
    defect bits (the test above); if they did not, the quantities that depend on the step are held to the independent layer's
    tolerance instead.  t_out is the host formula from the history's tf in either case."""
    c = case(name, gpu_ctx)
    v, runs, hist = c["v"], c["runs"], c["hist"]
    eq = same if c["premise"] else close
    for k in range(c["K"]):
        rep, nxt = c["dev"][k], runs[k + 1]
        for b in range(v.B):
            if not c["active"][k][b]:
                continue
            where = (name, "iteration %d" % (k + 1), "trajectory %d" % b, rep.kind[b])
            s = rep.state
            assert eq(nxt["X"][:, :, b], s.X[:, :, b]), where + ("X",)
            assert eq(nxt["U"][:, :, b], s.U[:, :, b]), where + ("U",)
            assert eq(nxt["dV"][:, b], np.r_[s.dV1[:, b], s.dV2[:, b]]), where + ("dV",)
            assert eq(nxt["tau"][:, b], [s.tau1[b], s.tau2[b]]), where + ("tau", nxt["tau"][:, b], s.tau1[b], s.tau2[b])
            assert eq(nxt["t"][:, b], s.t[:, b]), where + ("t_out",)
            assert eq(nxt["defect"][:, :, b], rep.defect[:, :, b]), where + ("defect_out",)
            assert eq(hist[0, k, b], rep.er[b]) and eq(hist[1, k, b], rep.cost[b]), where + ("history", hist[:2, k, b], rep.er[b], rep.cost[b])
            if v.kind != "frozen":
                assert eq(hist[3:5, k, b], [s.tau1[b], s.tau2[b]]), where + ("history tau",)
            if v.kind == "free_tf":
                assert eq(hist[5, k, b], s.tf[b]), where + ("tf", hist[5, k, b], s.tf[b])
                assert same(nxt["t"][:, b], v.t0 + (v.tau_grid + 1) / 2 * (hist[5, k, b] - v.t0)), where + ("t_out from the history's tf",)
                assert nxt["t"][-1, b] == hist[5, k, b]
            else:
                assert same(nxt["t"][:, b], v.t_fixed)


@pytest.mark.parametrize("name", SET_NAMES)
def test_independent_layer(gpu_ctx, oracle, name):
    """From the device's state k each time: max|defect| and defect_out against the oracle's defect at the device's own state k + 1
    (1e-12 max(1, 1e-2 max|X|), the direct-defect tolerance of test_gpu_fuzz.py), and X, U, dV, tau, tf and cost of state k + 1
    against the CPU replay (1e-9 relative to max(1, |.|))."""
    c = case(name, gpu_ctx)
    v, runs, hist = c["v"], c["runs"], c["hist"]
    worst = dict(defect=0.0, X=0.0, U=0.0, tau=0.0, tf=0.0, cost=0.0)
    fails = []
    for k in range(c["K"]):
        rep, nxt = c["cpu"][k], runs[k + 1]
        for b in range(v.B):
            if not c["active"][k][b]:
                continue
            where = (name, "iteration %d" % (k + 1), "trajectory %d" % b, rep.kind[b])
            d_o, _ = oracle.direct_defect(nxt["X"][:, :, b], nxt["U"][:, :, b], nxt["t"][:, b], v.nsteps, lto.MU, lto.DU, lto.TU, v.Isp)
            tol_d = 1e-12 * max(1.0, 1e-2 * float(np.abs(nxt["X"][:, :, b]).max()))
            e_d = max(float(np.abs(nxt["defect"][:, :, b] - d_o).max()), abs(float(hist[0, k, b]) - float(np.abs(d_o).max())))
            worst["defect"] = max(worst["defect"], e_d / tol_d)
            if e_d > tol_d:
                fails.append(where + ("defect", e_d, tol_d))
            s = rep.state
            pairs = [("X", nxt["X"][:, :, b], s.X[:, :, b]), ("U", nxt["U"][:, :, b], s.U[:, :, b]),
                     ("dV", nxt["dV"][:, b], np.r_[s.dV1[:, b], s.dV2[:, b]]), ("tau", nxt["tau"][:, b], np.array([s.tau1[b], s.tau2[b]])),
                     ("cost", hist[1, k, b], np.array(rep.cost[b]))]
            if v.kind == "free_tf":
                pairs.append(("tf", hist[5, k, b], np.array(s.tf[b])))
            for what, got, ref in pairs:
                e = float(np.abs(np.asarray(got) - ref).max()) / tol_abs(ref)
                if what in worst:
                    worst[what] = max(worst[what], e)
                if e > 1.0:
                    fails.append(where + (what, e))
            if rep.searched[b] and rep.margin[b] >= MARGIN:  # the oracle's own line search agrees where it is decided
                if float(hist[2, k, b]) != float(R.ALPHAS[rep.pick[b]]):
                    fails.append(where + ("pick", float(hist[2, k, b]), rep.pick[b], rep.margin[b]))
    print("set %s, independent layer: largest error / tolerance %s" % (name, {k_: "%.2e" % e for k_, e in worst.items()}))
    assert not fails, fails[:8]


@pytest.mark.parametrize("name", ("A", "B", "D"))
def test_every_trajectory_equals_its_single_run(gpu_ctx, name):
    c = case(name, gpu_ctx)
    v, full = c["v"], c["full"]
    for b in range(v.B):
        one = solve(v.single(b), v.max_iter, gpu_ctx)
        k = c["count"][b]
        assert (int(one["status"][0]), int(one["iters"][0])) == (int(full["status"][b]), k), (name, b)
        assert same(one["hist"][2, :k, 0], full["hist"][2, :k, b]), (name, "alpha", b)
        for row in range(full["hist"].shape[0]):
            assert close(full["hist"][row, :k, b], one["hist"][row, :k, 0], 1e-12), (name, "history row %d" % row, b)
        for f in FIELDS:
            assert close(full[f][..., b], one[f][..., 0], 1e-12), (name, f, b)


def test_the_sets_exercise_the_decisions(gpu_ctx):
    """The conditions that keep this module from passing vacuously, counted over the device's own runs."""
    per = {}
    inside_total, seconds = 0, 0.0
    for name in SET_NAMES:
        c = case(name, gpu_ctx)
        v, hist, count = c["v"], c["hist"], c["count"]
        t = per.setdefault(v.kind, dict(searched=0, below_one=0))
        searched = below = inside = skipped = beside = 0
        picks = []
        for k in range(R.SEARCH_AFTER, c["K"]):
            on = [b for b in range(v.B) if c["active"][k][b]]
            if on and len(on) < v.B:
                beside += 1
            for b in on:
                alpha = float(hist[2, k, b])
                searched += 1
                below += alpha < 1.0
                inside += 0.1 < alpha < 1.0
                skipped += not c["dev"][k].margin[b] >= MARGIN
                picks.append((b, k + 1, alpha, c["dev"][k].margin[b]))
        t["searched"] += searched
        t["below_one"] += below
        inside_total += inside
        seconds += c["seconds"]["total"]
        print("set %s (%s): device iterations %s, searched %d, picks below 1.0 %d, strictly inside %d, skipped for a margin under %g: %d, "
              "searched iterations with a frozen neighbour %d" % (name, v.kind, count, searched, below, inside, MARGIN, skipped, beside))
        for p in picks:
            print("   trajectory %d iteration %d: alpha %.4f, margin %.3e" % p)
        assert skipped <= 1, name
        if name in ("A", "B", "D"):
            assert beside >= 1, name
    print("per variant: %s; picks strictly inside (0.1, 1.0): %d; the sets took %.1f s" % (per, inside_total, seconds))
    assert set(per) == {"frozen", "free", "free_tf"}
    for kind, t in per.items():
        assert t["searched"] >= 4 and t["below_one"] >= 1, (kind, t)
    assert inside_total >= 2
