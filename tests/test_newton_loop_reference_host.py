"""CPU: the host reference of the Newton loop's device decisions (tests/newton_loop_reference.py) against hand-made cases, and the
problems of tests/test_newton_loop_steps_gpu.py through the Python mirror of the loop (drivers._solve_indirect) and through the
reference's own replay, both on the oracle back end: the chosen inputs exercise the decisions before any GPU run."""
import math
from fractions import Fraction

import numpy as np
import pytest

import newton_loop_reference as R
import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers
from test_drivers import OracleOps
from test_newton_glue_gpu import FMA_SHAPES, PATTERNS, crafted_sums, fma_sensitive_elements
from test_newton_loop_steps_gpu import PRM12, PRM14, PRM_ABORT, problems_12, problems_14, problems_abort


# ------------------------------------------------------------------------------------------------ exact arithmetic
def test_fma_exact_on_cases_where_two_roundings_differ():
    e = 2.0 ** -30
    # (1 + e)^2 = 1 + 2e + e^2: the product rounds to 1 + 2e, the fused result keeps e^2
    assert R.fma_exact(1.0 + e, 1.0 + e, -(1.0 + 2.0 * e)) == e * e and (1.0 + e) * (1.0 + e) - (1.0 + 2.0 * e) == 0.0
    # 0.1 is 2^-54 * 0.1000...0055 above 1/10: 0.1 * 10 rounds to 1, the fused result is the excess
    assert R.fma_exact(0.1, 10.0, -1.0) == 2.0 ** -54 and 0.1 * 10.0 - 1.0 == 0.0
    # the product 3 (1 + 2^-52) = 3 + 1.5 ulp is a tie and rounds up to 3 + 2 ulp; the addend -0.25 ulp decides the fused result
    # the other way: 3 + 1.25 ulp rounds to 3 + 1 ulp, (3 + 2 ulp) - 0.25 ulp back to 3 + 2 ulp
    a, d, x, ulp = 3.0, 1.0 + 2.0 ** -52, -2.0 ** -53, 2.0 ** -51
    assert R.fma_exact(a, d, x) == 3.0 + ulp and a * d + x == 3.0 + 2.0 * ulp
    # broadcasting, the array form and the element form agree
    rng = np.random.default_rng(0)
    X, D = rng.standard_normal((3, 4, 2)), rng.standard_normal((3, 4, 2))
    got = R.fma_exact(R.ALPHAS[None, None, :, None], D[:, :, None, :], X[:, :, None, :])
    assert got.shape == (3, 4, 20, 2)
    assert got[1, 2, 5, 1] == R.fma_fraction(R.ALPHAS[5], D[1, 2, 1], X[1, 2, 1])
    assert np.sum(got != R.twice_rounded(R.ALPHAS[None, None, :, None], D[:, :, None, :], X[:, :, None, :])) > 20
    # the short cut for 0 and powers of two equals the Fraction form
    for a in (0.0, 1.0, -0.5, 2.0 ** -19, -4.0):
        x, d = rng.standard_normal(200), rng.standard_normal(200) * 10.0 ** rng.integers(-8, 8, 200)
        assert np.array_equal(R.fma_exact(a, d, x), [R.fma_fraction(a, d[i], x[i]) for i in range(200)])
    # what is not finite follows IEEE: 0 x NaN is NaN, inf stays inf; an exact zero is +0 unless both addends are -0
    got = R.fma_exact(0.0, np.array([np.nan, np.inf, 1.0, -1.0]), np.array([1.0, 1.0, np.inf, -0.0]))
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == np.inf and got[3] == 0.0 and math.copysign(1.0, got[3]) == -1.0
    assert math.copysign(1.0, R.fma_fraction(0.1, 0.0, 0.0)) == 1.0 and math.copysign(1.0, R.fma_fraction(-0.1, 0.0, -0.0)) == -1.0
    assert R.fma_fraction(1e308, 10.0, 1.0) == math.inf


def test_alphas_are_the_loops():
    """lto_host.hpp: alphas[a] = 0.1 + (1.0 - 0.1) / (n_alpha - 1) * a, the last set to 1.0 -- the twenty values written out."""
    stated = [0.1, 0.1473684210526316, 0.19473684210526315, 0.24210526315789474, 0.2894736842105263, 0.33684210526315794,
              0.38421052631578945, 0.43157894736842106, 0.4789473684210527, 0.5263157894736842, 0.5736842105263158,
              0.6210526315789474, 0.6684210526315789, 0.7157894736842105, 0.7631578947368421, 0.8105263157894737,
              0.8578947368421053, 0.9052631578947369, 0.9526315789473684, 1.0]
    assert R.ALPHAS.tolist() == stated and R.ALPHAS.dtype == np.float64 and len(R.ALPHAS) == R.NA == 20


def test_first_minimiser_nan_and_ties():
    nan, inf = math.nan, math.inf
    assert R.first_minimiser([3.0, 1.0, 2.0]) == 1 and R.first_minimiser([0.5, 1.0, 2.0]) == 0 and R.first_minimiser([3.0, 2.0, 1.0]) == 2
    assert R.first_minimiser([2.0, 1.0, 1.0, 3.0]) == 1                     # a tie: the first wins
    assert R.first_minimiser([nan, 1.0, 0.5]) == 0                          # a NaN in slot 0 stays
    assert R.first_minimiser([2.0, nan, 1.0, nan]) == 2                     # a NaN later never wins
    assert R.first_minimiser([nan, nan, nan]) == 0
    assert R.first_minimiser([inf, inf, 7.0, inf]) == 2 and R.first_minimiser([inf, inf]) == 0 and R.first_minimiser([4.0]) == 0
    rng = np.random.default_rng(1)
    for na in (1, 2, 20, 64):                                                # the patterns of the GPU sweep are what their names say
        ss = crafted_sums(na, len(PATTERNS), rng)
        best = [R.first_minimiser(row) for row in ss]
        assert best[0] == 0 and best[1] == na - 1 and best[2] == na // 2 and best[3] == na // 3 and best[4] == 0 and best[6] == 0
        assert best[7] == na // 2 and (na <= 2 or (best[5] == 2 and not np.isnan(ss[5, 2])))
        assert np.isnan(ss[4, 0]) and np.isnan(ss[6]).all() and np.isinf(ss[7]).sum() == na - 1


def test_norms_exact():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((7, 33)) * 10.0 ** rng.integers(-9, 9, size=(7, 33))
    assert R.sumsq_exact(v) == float(R.sumsq_fraction(v))
    assert R.sumsq_exact(np.full(5, 1e-160)) == float(5 * Fraction(1e-160) ** 2) > 0.0
    assert R.sumsq_exact(np.full((3, 3), -0.0)) == 0.0 and R.maxabs(np.full((3, 3), -0.0)) == 0.0
    assert math.isnan(R.sumsq_exact([1.0, math.nan])) and math.isnan(R.maxabs([1.0, math.nan, math.inf]))
    assert R.sumsq_exact([1.0, -math.inf]) == math.inf and R.maxabs([1.0, -math.inf]) == math.inf
    assert R.maxabs([-3.0, 2.0]) == 3.0
    assert isinstance(R.sumsq_rational([1.5, 2.0]), Fraction) and R.sumsq_rational([1.5, 2.0]) == Fraction(25, 4)
    assert math.isnan(R.sumsq_rational([math.nan, math.inf])) and R.sumsq_rational([1.0, math.inf]) == math.inf


def test_layouts_and_pins():
    A = np.arange(2 * 3 * 4, dtype=float).reshape(2, 3, 4)                  # [rows x per x B]
    s = R.to_soa(A)
    assert s[1, 2 * 3 + 1] == A[1, 1, 2] and np.array_equal(R.from_soa(np.hstack([s, np.zeros((2, 5))]), 3, 4), A)
    T = np.arange(2 * 3 * 5 * 4, dtype=float).reshape(2, 3, 5, 4)           # [rows x n x NA x B]
    st = R.trials_to_soa(T)
    assert st[1, (3 * 5 + 2) * 3 + 1] == T[1, 1, 2, 3] and np.array_equal(R.trials_from_soa(st, 3, 5, 4), T)
    m12, m14 = R.pinned_mask(12, 5), R.pinned_mask(14, 5)
    assert m12[:6, 0].all() and m12[:6, 4].all() and m12.sum() == 12
    assert m14[:7, 0].all() and m14[:6, 4].all() and m14[13, 4] and not m14[6, 4] and m14.sum() == 14
    X = np.ones((14, 5, 2))
    assert np.all(R.apply_entry_pins(X)[13, 4] == 0.0) and R.apply_entry_pins(X).sum() == X.sum() - 2
    assert np.array_equal(R.apply_entry_pins(np.ones((12, 5, 2))), np.ones((12, 5, 2)))


def test_loop_counters_follow_newton_batch():
    assert R.loop_counters([], 0) == (1, 1, 0)                               # maxIter = 0: at the limit at once
    assert R.loop_counters([1e-3, 1e-12], 5) == (0, 2, 2)                    # converged after two iterations
    assert R.loop_counters([1e-3, 1e-5, 1e-6], 3) == (1, 4, 3)               # the limit: iterations = maxIter + 1
    assert R.loop_counters([math.nan], 5) == (0, 1, 1)                       # NaN leaves like a converged one (status 2 comes later)
    assert R.loop_counters([1e-3, 2e3], 10) == (1, 103, 2)                   # abort: the count jumps by 100
    assert R.still_active(1e-3, True) and not R.still_active(1e-11, True) and not R.still_active(math.nan, True)
    assert not R.still_active(2e3, True) and not R.still_active(1e-3, False)


def test_trial_point_inputs_tell_the_fma_from_two_roundings():
    count = fma_sensitive_elements(FMA_SHAPES)
    print("trial points: %d elements of the small shapes differ between the fma and two roundings" % count)
    assert count >= 100


# ------------------------------------------------------------------------------------------------ the problems, on the CPU
class RecordingOps(OracleOps):
    """OracleOps that logs the mirror's calls: per iteration one stm, a defect if the correction is taken, the line search's
    sums, and the defect check."""

    def __init__(self, O):
        super().__init__(O)
        self.log = []

    def defect(self, XC, t, params):
        self.log.append(("defect",))
        return super().defect(XC, t, params)

    def stm(self, XC, t, params):
        self.log.append(("stm",))
        return super().stm(XC, t, params)

    def defect_batch_sumsq(self, XC_batch, t, params):
        er = np.array([np.sum(OracleOps.defect(self, XC_batch[:, :, b], t, params) ** 2) for b in range(XC_batch.shape[2])])
        order = np.sort(er)
        self.log.append(("search", float(np.linspace(0.1, 1.0, 20)[int(np.argmin(er))]), float((order[1] - order[0]) / order[0])))
        return er

    def iterations(self):
        its = []
        for e in self.log[1:]:                                               # (the first entry is the defect of the start)
            if e[0] == "stm":
                its.append(dict(defects=0, search=None))
            elif e[0] == "defect":
                its[-1]["defects"] += 1
            else:
                its[-1]["search"] = e[1:]
        return [dict(soc=i["defects"] == 2, search=i["search"]) for i in its]


class HostOps:
    """The replay's operators on the oracle back end with dense host linear algebra (12 or 14 rows)."""

    def __init__(self, O, nd, t, prm):
        self.O, self.nd, self.t, self.prm = O, nd, np.asarray(t, dtype=np.float64), list(prm)
        self.adjoints_only = False
        self.fact = None

    def _sweep(self, X1, want_stm):
        if self.nd == 12:
            if want_stm:
                Phi, d, rc = self.O.indirect_jacobian(X1, self.t, self.prm, self.O.DOP853_ADAPTIVE)
            else:
                (d, _, rc), Phi = self.O.indirect_defect(X1, self.t, self.prm, self.O.DOP853_ADAPTIVE), None
        else:
            Phi, d, rc = self.O.indirect14(X1, self.t, self.prm, self.O.DOP853_ADAPTIVE, want_stm=want_stm)
        return Phi, d

    def _solve(self, b, d):
        Jm, free = self.fact[b]
        out = np.zeros(free.size)
        if np.isfinite(Jm).all() and np.isfinite(d).all():
            rhs = -d.reshape(-1, order="F")
            out[free] = np.linalg.solve(Jm, rhs) if Jm.shape[0] == Jm.shape[1] else np.linalg.lstsq(Jm, rhs, rcond=None)[0]
        else:
            out[:] = np.nan
        return out.reshape(self.nd, -1, order="F")

    def newton(self, X):
        nd, n, B = X.shape
        free = ~R.pinned_mask(nd, n)
        if self.adjoints_only:
            free[:nd // 2] = False
        free = free.reshape(-1, order="F")
        self.fact, out = [], np.zeros(X.shape)
        for b in range(B):
            Phi, d = self._sweep(np.asfortranarray(X[:, :, b]), True)
            J = lto.indirect_scatter(Phi) if nd == 12 else lto.indirect_scatter_mass(Phi)
            self.fact.append((J[:, free], free))
            out[:, :, b] = self._solve(b, d)
        return out

    def resolve(self, d):
        return np.stack([self._solve(b, d[:, :, b]) for b in range(d.shape[2])], axis=2)

    def defect(self, X):
        return np.stack([self._sweep(np.asfortranarray(X[:, :, b]), False)[1] for b in range(X.shape[2])], axis=2)

    def trial_defect(self, Xt):
        nd, n, na, B = Xt.shape
        out = np.zeros((nd, n - 1, na, B))
        for b in range(B):
            for a in range(na):
                out[:, :, a, b] = self._sweep(np.asfortranarray(Xt[:, :, a, b]), False)[1]
        return out


def host_loop(ops, XC, adjoints_only, K):
    """The loop built from the reference's replay alone: per iteration and trajectory (alpha, SOC taken, searched, separation,
    near tie, max |defect|)."""
    nd, n, B = XC.shape
    ops.adjoints_only = adjoints_only
    X_entry = R.apply_entry_pins(XC)
    X = X_entry.copy()
    active = [True] * B
    rows = [[] for _ in range(B)]
    for it in range(1, K + 1):
        if not any(active):
            break
        was = list(active)
        rep = R.replay_iteration(ops, X, it, active, adjoints_only)
        X = R.apply_step(X, rep.delta, rep.alpha_ref, X_entry)
        d = ops.defect(X)
        for b in range(B):
            if was[b]:
                e = R.maxabs(d[:, :, b])
                rows[b].append(dict(alpha=rep.alpha_ref[b], soc=rep.soc[b], searched=rep.searched[b], separation=rep.separation[b],
                                    near_tie=rep.searched[b] and len(rep.accepted[b]) > 1, er=e))
                active[b] = R.still_active(e, True)
    return X, rows


def quotas(rows_per_trajectory):
    q = dict(searched=0, below_one_separated=0, alpha_one=0, near_tie=0, soc_taken=0, soc_skipped=0)
    for rows in rows_per_trajectory:
        for r in rows:
            q["soc_taken" if r["soc"] else "soc_skipped"] += 1
            if r["searched"]:
                q["searched"] += 1
                if r["near_tie"]:
                    q["near_tie"] += 1
                elif r["alpha"] == 1.0:
                    q["alpha_one"] += 1
                elif r["separation"] >= 0.01:
                    q["below_one_separated"] += 1
    return q


@pytest.fixture(scope="module")
def mirror_12(oracle):
    """The four 12-row problems through drivers._solve_indirect on the oracle back end."""
    XC, t = problems_12(oracle)
    out = []
    for b in range(XC.shape[2]):
        ops = RecordingOps(oracle)
        X, d, status = drivers._solve_indirect(np.array(XC[:, :, b], order="F"), t, XC.shape[1], lto.make_params(*PRM12), False, 10, ops, False)
        out.append((status, ops.iterations(), X))
    return out


def test_the_12_row_problems_exercise_the_decisions_in_the_mirror(mirror_12):
    rows = [[dict(soc=i["soc"], searched=i["search"] is not None, alpha=i["search"][0] if i["search"] else 1.0,
                  separation=i["search"][1] if i["search"] else math.nan, near_tie=bool(i["search"]) and i["search"][1] < 1e-12)
             for i in its] for _, its, _ in mirror_12]
    q = quotas(rows)
    iters = [len(its) for _, its, _ in mirror_12]
    print("mirror, 12 rows: iterations %s, %s" % (iters, q))
    for b, r in enumerate(rows):
        print("   trajectory %d: %s" % (b, [("%.3f" % i["alpha"], "soc" if i["soc"] else "-", "%.1e" % i["separation"]) for i in r]))
    assert all(status == 0 for status, _, _ in mirror_12)
    assert 8 <= min(iters[:3]) and max(iters[:3]) <= 10 and iters[3] <= 3
    assert q["below_one_separated"] >= 6 and q["alpha_one"] >= 3 and q["soc_taken"] >= 4 and q["soc_skipped"] >= 4
    assert q["near_tie"] <= 0.2 * q["searched"]
    assert max(iters[:3]) - iters[3] >= 2                                    # frozen for two or more iterations beside an active one


def test_the_replay_walks_the_mirrors_path_on_12_rows(oracle, mirror_12):
    """The loop built from replay_iteration and apply_step alone (exact fma, exact sums, the library's step lengths) against the
    independent mirror: the same correction decisions, the same picks wherever the runner-up is clear, the same solution."""
    XC, t = problems_12(oracle)
    X, rows = host_loop(HostOps(oracle, 12, t, PRM12), XC, False, 10)
    q = quotas(rows)
    print("replay, 12 rows: iterations %s, %s" % ([len(r) for r in rows], q))
    for b, (status, its, X_mirror) in enumerate(mirror_12):
        assert len(rows[b]) == len(its)
        for r, i in zip(rows[b], its):
            assert r["soc"] == i["soc"] and r["searched"] == (i["search"] is not None)
            if r["searched"] and r["separation"] >= 1e-6:
                assert r["alpha"] == i["search"][0]
        assert rows[b][-1]["er"] <= 1e-10 and np.abs(X[:, :, b] - X_mirror).max() < 1e-9
    assert q["below_one_separated"] >= 6 and q["alpha_one"] >= 3 and q["soc_taken"] >= 4 and q["soc_skipped"] >= 4


def test_the_other_cases_on_the_cpu(oracle):
    """Adjoints only, 14 rows and the NaN / diverging batch through the replay on the oracle back end: they search, the
    diverging start leaves after its first iteration, its healthy neighbour converges."""
    XC, t = problems_12(oracle)
    _, rows = host_loop(HostOps(oracle, 12, t, PRM12), XC, True, 10)
    qa = quotas(rows)
    print("replay, 12 rows, adjoints only: iterations %s, %s" % ([len(r) for r in rows], qa))
    X14, t14 = problems_14(oracle)
    X, rows = host_loop(HostOps(oracle, 14, t14, PRM14), X14, False, 10)
    q14 = quotas(rows)
    print("replay, 14 rows: iterations %s, last max |defect| %s, %s" % ([len(r) for r in rows], ["%.1e" % r[-1]["er"] for r in rows], q14))
    assert q14["below_one_separated"] >= 3 and all(r[-1]["er"] <= 1e-10 for r in rows)
    assert np.all(X[13, -1] == 0.0) and np.array_equal(X[0:7, 0], X14[0:7, 0]) and np.array_equal(X[0:6, -1], X14[0:6, -1])
    # (without the NaN start: the oracle's adaptive integrator spends minutes on a NaN trajectory; the device does not)
    Xa, ta = problems_abort(oracle)
    assert np.isnan(Xa[:, :, 0]).sum() == 1 and np.isfinite(Xa[:, :, 1:]).all()
    _, rows = host_loop(HostOps(oracle, 12, ta, PRM_ABORT), Xa[:, :, 1:], False, 6)
    print("replay, diverging / healthy: max |defect| %s" % [["%.1e" % r["er"] for r in tr] for tr in rows])
    assert len(rows[0]) == 1 and rows[0][0]["er"] > 1e3
    assert 2 <= len(rows[1]) <= 6 and rows[1][-1]["er"] <= 1e-10
