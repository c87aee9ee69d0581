"""CPU: the replay of one direct-loop iteration (tests/direct_loop_reference.py) with its independent back end, chained, against
drivers.direct_loop_host on the CPU oracle -- it must reproduce the mirror loop's history exactly -- and what makes the
problem sets worth running on the device: their iteration counts, the line search's picks and how well separated they are, a
trajectory that leaves before iteration 11 beside one that searches, and a free tf that touches its per-iteration step bound.
tests/test_direct_loop_steps_gpu.py runs the same sets through the device loop."""
import math

import numpy as np
import pytest

import direct_helpers as DH
import direct_loop_reference as R
import newton_loop_reference as NR

# the mirror loop on the oracle: iterations per trajectory, the searched picks (index into the ten alphas, from iteration 11 on)
# per trajectory, the smallest margin (second smallest / smallest sum - 1) of the set
EXPECTED = {
    "A": dict(iterations=[17, 3, 7], picks=[[9, 1, 2, 6, 9, 9, 9], [], []], margin=8.8e-3),
    "B": dict(iterations=[18, 12, 10], picks=[[8, 6, 0, 9, 0, 9, 0, 9], [0, 9], []], margin=4.3e-2),
    "C": dict(iterations=[12], picks=[[0, 9]], margin=1.2),
    "D": dict(iterations=[18, 10], picks=[[1, 9, 0, 9, 0, 9, 0, 9], []], margin=1.1e-1),
    "E": dict(iterations=[16], picks=[[1, 7, 0, 9, 0, 9]], margin=6.4e-3),
    "F": dict(iterations=[14], picks=[[5, 2, 1, 1]], margin=3.1e-2),      # frozen ends with impulses, target at tau2 + 0.25, maxIter 14
}
STATUS = {"A": [0, 0, 0], "B": [0, 0, 0], "C": [0], "D": [0, 0], "E": [1], "F": [1]}

_SETS = {}
_CHAINS = {}


def sets():
    if not _SETS:
        _SETS.update(R.problem_sets())
    return _SETS


def chain(name):
    """The replay chained from the entry state on the oracle, the whole batch at once: per trajectory the history rows, the picks
    and margins of its searched iterations, and the |tf step| / (alpha step) of its free-tf iterations."""
    if name in _CHAINS:
        return _CHAINS[name]
    v = sets()[name]
    be = R.OracleBackEnd()
    state = v.entry_state()
    B = v.B
    out = dict(rows=[[] for _ in range(B)], picks=[[] for _ in range(B)], margins=[[] for _ in range(B)], tf_ratio=[[] for _ in range(B)],
               kinds=[[] for _ in range(B)], active_at=[], final=None)
    active = [True] * B
    er = [1.0] * B
    for it in range(1, v.max_iter + 1):
        active = [active[b] and R.still_active(er[b]) for b in range(B)]
        if not any(active):
            break
        out["active_at"].append(list(active))
        rep = R.replay_iteration(state, it, v, be, active)
        for b in range(B):
            if not active[b]:
                continue
            out["rows"][b].append(rep.row[:, b].copy())
            out["kinds"][b].append(rep.kind[b])
            if rep.searched[b]:
                out["picks"][b].append(rep.pick[b])
                out["margins"][b].append(rep.margin[b])
            if rep.kind[b] == "free_tf":
                out["tf_ratio"][b].append(abs(rep.state.tf[b] - state.tf[b]) / (rep.alpha[b] * v.step_of(b)))
            er[b] = rep.er[b]
        state = rep.state
    out["final"] = state
    _CHAINS[name] = out
    return out


def test_the_grids_are_fixed_points_of_the_recomputation():
    """The loop sweeps its first iteration on the caller's grid and weights the QP on t1(t); the one-step entries take one grid.  The
    sets pass t1(t) of the demo grid, and t1(t1(t)) == t1(t) bit for bit for it and for its 18 / 20 / 22-day rescalings."""
    X, U, t, *_ = DH.demo().demo_problem()
    for tof in (None, 18.0, 20.0, 22.0):
        g = t if tof is None else t[0] + (t - t[0]) * (tof * R.DAY) / (t[-1] - t[0])
        g1 = R.fixed_grid(g)
        assert np.array_equal(R.fixed_grid(g1), g1), tof
        assert g1[0] == g[0] and g1[-1] == g[-1]
    for name, v in sets().items():
        assert np.array_equal(v.t_fixed, v.t_entry), name
        assert v.tau_grid[-1] == 1.0 and v.t0 + (v.tau_grid[-1] + 1) / 2 * (v.t_entry[-1] - v.t0) == v.t_entry[-1], name


def test_the_two_alpha_tables_agree_to_an_ulp():
    """NewtonBatch's table (0.1 + 0.9 / 9 a, the last forced to 1) and the mirror's LinRange differ by rounding at the most; the
    tests compare picks by index."""
    assert R.ALPHAS[0] == 0.1 and R.ALPHAS[-1] == 1.0 and R.ALPHAS_MIRROR[-1] == 1.0
    assert np.all(np.diff(R.ALPHAS) > 0)
    assert np.abs(R.ALPHAS - R.ALPHAS_MIRROR).max() <= 2.0 ** -52


def test_fma_of_the_device_step_layer_is_the_rounded_exact_value():
    rng = np.random.default_rng(0)
    a, d, x = R.ALPHAS[3], rng.standard_normal(50), rng.standard_normal(50)
    got = R.DeviceStepBackEnd.axpy(a, d, x)
    assert np.array_equal(got, [math.fma(a, di, xi) for di, xi in zip(d, x)] if hasattr(math, "fma") else
                          [NR.fma_fraction(a, di, xi) for di, xi in zip(d, x)])
    assert R.margin_of([4.0, 2.0, 3.0, math.nan]) == 0.5 and R.margin_of([0.0, 1.0]) == math.inf
    assert R.loop_counters([1.0, 1e-7], 5) == (0, 2) and R.loop_counters([1.0, 1e-7], 1) == (1, 1) and R.loop_counters([], 0) == (1, 0)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_chained_replay_reproduces_the_mirror_loop(name):
    v = sets()[name]
    ch = chain(name)
    ops = DH.OracleDirectOps(v.Isp)
    for b in range(v.B):
        out, last = v.mirror(b, ops)
        k, H = last["iterations"], last["history"]
        rows = np.array(ch["rows"][b]).T
        print("set %s trajectory %d: status %d, %d iterations, picks %s, margins %s" % (
            name, b, last["status"], k, ch["picks"][b], ["%.2e" % m for m in ch["margins"][b]]))
        assert rows.shape[1] == k, (name, b, rows.shape, k)
        assert np.array_equal(rows[:H.shape[0]], H[:, :k]), (name, b, "history")
        if v.tf_bounds is None:
            assert np.all(rows[5] == v.t_entry[-1])
        Xo, Uo, tau1, tau2, to, dV1, dV2, _ = out
        f = ch["final"]
        assert np.array_equal(f.X[:, :, b], Xo) and np.array_equal(f.U[:, :, b], Uo) and np.array_equal(f.t[:, b], to)
        assert (f.tau1[b], f.tau2[b]) == (tau1, tau2) and np.array_equal(f.dV1[:, b], dV1) and np.array_equal(f.dV2[:, b], dV2)
        assert last["status"] == STATUS[name][b]
        # alpha: 1 up to iteration 10, then the pick; tau and tf move on the odd iterations of the free variants only
        for it in range(1, k + 1):
            assert ch["kinds"][b][it - 1] == ("frozen" if (v.kind == "frozen" or it % 2 == 0) else
                                              ("free_tf" if v.step_of(b) > 0 else "free"))
            if it <= R.SEARCH_AFTER:
                assert rows[2, it - 1] == 1.0
        assert [float(R.ALPHAS_MIRROR[p]) for p in ch["picks"][b]] == list(rows[2, R.SEARCH_AFTER:])


@pytest.mark.parametrize("name", list(EXPECTED))
def test_the_sets_are_worth_running(name):
    v = sets()[name]
    ch = chain(name)
    exp = EXPECTED[name]
    its = [len(r) for r in ch["rows"]]
    margins = [m for ms in ch["margins"] for m in ms]
    print("set %s: iterations %s, picks %s, smallest margin %.3e" % (name, its, ch["picks"], min(margins)))
    assert its == exp["iterations"]
    assert ch["picks"] == exp["picks"]
    assert min(margins) >= 5e-3
    assert abs(min(margins) / exp["margin"] - 1.0) <= 0.06            # the table's two digits
    if name == "A":
        assert sum(1 for p in ch["picks"][0] if 0 < p < R.NA - 1) >= 2    # picks strictly inside (0.1, 1.0)
    if name in ("A", "B", "D"):
        # one trajectory leaves before iteration 11 while another searches
        assert any(n <= R.SEARCH_AFTER for n in its) and any(n > R.SEARCH_AFTER for n in its)
        at11 = ch["active_at"][R.SEARCH_AFTER]
        assert any(at11) and not all(at11)
    if name == "F":                                        # the impulses move, also where alpha < 1
        assert np.all(ch["final"].dV1[:, 0] != v.dV[:3, 0]) and np.all(ch["final"].dV2[:, 0] != v.dV[3:, 0])
        assert all(0 < p < R.NA - 1 for p in ch["picks"][0])
    if name == "D":
        assert ch["tf_ratio"][1] == [] and len(ch["tf_ratio"][0]) == 9
        assert any(abs(q - 1.0) <= 1e-12 for q in ch["tf_ratio"][0])     # |tf step| = alpha step: the bound is touched
        assert all(q <= 1.0 + 1e-12 for q in ch["tf_ratio"][0])
        assert np.all(np.array(ch["rows"][1])[:, 5] == v.t_entry[-1])
