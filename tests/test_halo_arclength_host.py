"""CPU checks for the pseudo-arclength continuation: the independent reference (tests/halo_arclength_reference.py) finds
what the CPU prototype of the feature found -- the halo bifurcation of the L2 Lyapunov family between members 12 and 13, the two
branch points, the packaged halo orbits on the southern L2 branch --; every input the GPU tests use (tests/test_halo_arclength_gpu.py)
is far from a decision's edge at both of the reference's tolerance settings, and the reference's own spread between them stays below
a tenth of every bound the device is held to; the drivers' host arithmetic on made-up arrays; the argument checks the Python layer
makes before any library call; the new entry point is declared and exported."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import halo_arclength_reference as AR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import _lib, drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

TOL, MAX_ITER = 1e-12, 15


def test_the_l2_lyapunov_family_bifurcates_between_members_12_and_13():
    fam = AR.lyapunov_family(2, MU)
    assert all(m.status == 0 for m in fam) and max(m.iterations for m in fam) <= 3
    assert AR.family_bifurcations(fam) == [13]
    # in the 3-unknown form with z0 = 0 the second row of DF is (0, e, 0) exactly: z0 stays 0 and the tangent stays in the plane
    assert all(m.state[2] == 0.0 and m.tangent[1] == 0.0 for m in fam)


@pytest.mark.parametrize("which, x0, vy0, C, P", [(2, 1.12038624, 0.17604042, 3.152118903, 3.415530893),
                                                 (1, 0.8233909, 0.1263264, 3.174351954, 2.742994069)])
def test_the_branch_points(which, x0, vy0, C, P):
    bp, trials = AR.halo_branch(which, MU)
    fam = AR.lyapunov_family(which, MU)
    print("L%d: x0 %.10f vy0 %.10f C %.10f P %.10f, trials %s" % (which, bp.state[0], bp.state[4], bp.jacobi, bp.period, trials))
    assert len(trials) <= 8 and abs(bp.det) < 1e-9 * abs(fam[AR.family_bifurcations(fam)[0] - 1].det)
    assert abs(bp.jacobi - C) < 1e-8 and abs(bp.period - P) < 1e-8
    assert abs(bp.state[0] - x0) < 1e-7 and abs(bp.state[4] - vy0) < 1e-7 and bp.state[2] == 0.0
    # the step off the plane lands on z0 = +-ds exactly: the third equation is z0 - z0_pred = 0 and linear
    for z in (1.0, -1.0):
        for ds, steps in ((1e-3, 2), (1e-2, 4)):
            m = AR.switched(which, z, ds, MU)
            assert m.status == 0 and m.iterations <= steps and abs(m.state[2] - z * ds) < 1e-15


def test_the_southern_l2_branch_passes_through_the_packaged_orbits():
    halo = AR.case_march(AR.cases(MU)["halo_L2"], 0, MU)
    assert all(m.status == 0 and m.halvings == 0 and 3 <= m.iterations <= 6 for m in halo)
    z0 = np.array([m.state[2] for m in halo])
    assert AR.family_folds(halo, 1) == [12] and abs(z0.min() + 0.0756) < 1e-3        # the fold of z0
    for tb in synth.halo_orbits():
        packaged = HR.seed_of(np.asarray(tb[:6], dtype=float))
        k = int(np.argmin([abs(m.state[0] - packaged[0]) for m in halo]))
        start = halo[k].state.copy()
        start[0] = packaged[0]
        got = HR.correct(start, HR.HOLD_X0, MU)
        own = HR.correct(packaged, HR.HOLD_X0, MU)
        print("member %d: %.2e from the packaged seed, %.2e from the orbit the corrector makes of it" % (
            k, np.abs(got.state - packaged).max(), np.abs(got.state - own.state).max()))
        assert got.status == 0 and np.abs(got.state - packaged).max() < 1e-7 and np.abs(got.state - own.state).max() < 1e-12


@pytest.mark.parametrize("cls", AR.CLASSES)
def test_the_gpu_cases_are_not_marginal_and_the_spread_is_a_tenth_of_the_bounds(cls):
    bound = AR.BOUNDS[cls]
    worst, steps = np.zeros(4), 0
    for case in (c for c in AR.cases(MU).values() if c.cls == cls):
        for b in range(AR.N_BATCH):
            a, l = AR.case_march(case, b, MU), AR.case_march(case, b, MU, loose=True)
            # every member is accepted at its first attempt in <= max_iter - 2 steps at both settings
            for m in a + l:
                assert m.status == 0 and m.halvings == 0 and m.iterations <= MAX_ITER - 2, (case.name, b)
            assert [np.sign(m.det) for m in a] == [np.sign(m.det) for m in l]
            worst = np.maximum(worst, AR.differences(a, l))
            steps = max(steps, max(m.iterations for m in a))
    print("%s: spread state %.2e tangent %.2e period %.2e det %.2e (bounds %s), at most %d steps" % ((cls,) + tuple(worst) + (bound, steps)))
    assert np.all(worst < 0.1 * np.array(bound)), (worst, bound)


def test_the_lyapunov_march_of_the_gpu_test_flips_where_the_base_does():
    case = AR.cases(MU)["lyapunov3_L2"]
    for b in range(AR.N_BATCH):
        for loose in (False, True):
            got = AR.case_march(case, b, MU, loose=loose)
            flips = AR.family_bifurcations(got)
            assert len(flips) == 1 and 12 <= flips[0] <= 14, (b, flips)
            # no member sits on the bifurcation: |det| there is a thousand times the bound on det
            assert min(abs(m.det) for m in got) > 1e3 * AR.BOUNDS["lyapunov3"][3] * max(abs(m.det) for m in got)


@pytest.mark.parametrize("name", ["halve", "grow", "nogrow", "dsmin"])
def test_the_step_control_cases_are_not_marginal(name):
    case = AR.step_cases(MU)[name]
    cos_min, fast = case.kw.get("cos_min", 0.0), case.kw.get("fast_iter", 3)
    for b in range(case.seeds.shape[1]):
        runs = [AR.step_march(case, b, MU), AR.step_march(case, b, MU, loose=True)]
        if "t_max" in case.kw:                               # the flights that end at t_max miss it by more than 1e-3
            runs += [AR.step_march(case, b, MU, t_max=case.kw["t_max"] + s) for s in (-1e-3, 1e-3)]
        first = [(k, ds, m.status, m.iterations) for k, ds, m in runs[0][1]]
        print(name, b, first, [(m.status, m.halvings, m.ds) for m in runs[0][0]])
        for got, trace in runs:
            assert [(k, ds, m.status, m.iterations) for k, ds, m in trace] == first
            for k, ds, m in trace:
                if m.status == 0:
                    assert m.iterations <= MAX_ITER - 2
                    hist = m.history
                    # the count of steps is safe: the last residual is a tenth of tol and the one before ten times tol -- or one
                    # step more would change no decision (the seed's own correction, member 0 of a march from a direction, never
                    # changes ds)
                    safe = (hist[-1] < 0.1 * TOL or case.kw.get("grow", 1.0) == 1.0 or (k == 0 and not case.tangent)
                            or (m.iterations <= fast) == (m.iterations + 1 <= fast))
                    assert safe and (len(hist) == 1 or hist[-2] > 10.0 * TOL), (k, hist)
                    assert cos_min == 0.0 or m.dots > cos_min + AR.COS_MARGIN
                elif m.status == 4:
                    assert m.dots < cos_min - AR.COS_MARGIN
                else:
                    assert m.status == 2                     # no other kind of failure is relied on
    got = [AR.step_march(case, b, MU)[0] for b in range(case.seeds.shape[1])]
    # the spread of the members the GPU test compares, against the bounds of the case's class
    for b, a in enumerate(got):
        pairs = [(x, y) for x, y in zip(a, AR.step_march(case, b, MU, loose=True)[0]) if x.status == 0]
        if pairs:
            d = np.array(AR.differences([p[0] for p in pairs], [p[1] for p in pairs]))
            print("%s orbit %d: spread state %.2e tangent %.2e period %.2e det %.2e" % ((name, b) + tuple(d)))
            assert np.all(d < 0.1 * np.array(AR.BOUNDS[case.cls]))
    if name == "halve":
        assert [(m.status, m.halvings, m.ds) for m in got[0]] == [(0, 1, 0.08), (0, 1, 0.04)]
    elif name == "grow":
        assert [m.ds for m in got[0]] == [0.0, 0.005, 0.005 * 1.5, 0.005 * 1.5 * 1.5, 0.012, 0.012]
    elif name == "nogrow":
        assert [m.ds for m in got[0]] == [0.0] + [0.005] * 5
    else:
        assert [(m.status, m.halvings) for m in got[0]] == [(4, 0), (2, 0), (2, 0)] and got[0][0].ds == 0.02
        assert np.isnan(got[0][1].ds) and all(m.status == 0 for m in got[1])


def test_the_status_inputs_are_what_the_gpu_test_takes_them_for():
    sw = AR.switched(2, -1.0, 1e-2, MU)
    u, t = sw.state[[0, 2, 4]], sw.tangent
    # cos_min = 0.9999: the first step of 0.02 up the halo branch turns the tangent by 26 degrees, a step of 1e-3 along the planar
    # family by less than 0.1 degree (1 - cos < 1e-5, a tenth of 1 - cos_min)
    for tl in ({}, {"rtol": AR.LOOSE[0], "atol": AR.LOOSE[1]}):
        m = AR.attempt(u, t, 0.02, False, False, MU, cos_min=0.9999, **tl)
        assert m.status == 4 and m.dots < 0.9499
        f0 = AR.lyapunov_family(2, MU)[0]
        g = AR.attempt(f0.state[[0, 2, 4]], f0.tangent, 1e-3, False, False, MU, cos_min=0.9999, **tl)
        assert g.status == 0 and 1.0 - g.dots < 1e-5
        # sing_tol = 0.999: |det| / the product of the row norms of [DF; t] is far below
        F, DF, _ = AR.system(u + 0.02 * t, False, MU, **tl)
        J = np.vstack([DF, t])
        assert abs(np.linalg.det(J)) / np.prod(np.linalg.norm(J, axis=1)) < 0.9
        assert AR.attempt(u, t, 0.02, False, False, MU, sing_tol=0.999, **tl).status == 3
        # t_max = 1.0 is before the half period (1.7)
        assert AR.attempt(u, t, 0.02, False, False, MU, t_max=1.0, **tl).status == 2
    # a direction perpendicular to the planar family's tangent, exactly: (0, 1, 0)
    lyap = AR.lyapunov_orbit(2, MU)
    assert [m.status for m in AR.march(lyap, [0.0, 1.0, 0.0], 0.01, 2, True, MU)] == [2, 2]
    assert [m.status for m in AR.march(lyap, [0.0, 0.0, 0.0], 0.01, 2, True, MU)] == [2, 2]
    assert [m.status for m in AR.march(lyap, [0.0, np.nan, 1.0], 0.01, 2, True, MU)] == [2, 2]


def test_driver_arithmetic():
    nan = np.nan
    K = 7
    states = np.zeros((6, K))
    tang = np.array([[1.0, 0.5, -0.5, -1.0, nan, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, -1.0, 1.0, 1.0, -2.0]])
    det = np.array([-3.0, -1.0, 2.0, 1.0, -1.0, nan, 1.0])
    fam = drivers.HaloFamily(states, np.ones(K), np.zeros(K), np.zeros(K, dtype=int), np.zeros(K, dtype=int), tang, det, np.full(K, 0.01))
    assert drivers.family_bifurcations(fam) == [2, 4]                       # a NaN member is no sign change
    assert drivers.family_folds(fam) == {"x0": [2], "z0": [], "vy0": [3, 4, 6]}
    assert drivers._sign_changes([1.0, 0.0, -1.0]) == []                     # a zero is no sign change either
    old = drivers.HaloFamily(states, np.ones(K), np.zeros(K), np.zeros(K, dtype=int), np.zeros(K, dtype=int))
    assert old.tangent is None and old.det is None and old.ds is None       # the natural-parameter marches fill five fields
    for f in (drivers.family_bifurcations, drivers.family_folds):
        with pytest.raises(ValueError):
            f(old)
    with pytest.raises(ValueError):
        drivers.family_bifurcations(fam._replace(det=np.zeros((K, 2))))
    # the secant's next point: the zero of the line through the last two
    assert drivers._secant_next(0.0, -1.0, 0.01, 1.0) == 0.005
    assert abs(drivers._secant_next(0.01, 1.0, 0.005, 0.25) - (0.005 - 0.25 * (-0.005) / (-0.75))) < 1e-18
    for bad_k in (0, K, 1, 3):                                               # out of range, or no sign change there
        with pytest.raises(ValueError):
            drivers.halo_branch_point(fam, bad_k)
    with pytest.raises(ValueError):
        drivers.halo_branch_point(old, 2)
    with pytest.raises(ValueError):
        drivers.halo_family_arclength(np.ones(6), 4, 0.01, None)


def test_halo_arclength_rejects_malformed_input_before_any_library_call(monkeypatch):
    def no_context():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lto.hotpath, "default_context", no_context)
    up = [0.0, 0.0, 1.0]
    for bad in (np.zeros(5), np.zeros((5, 3)), np.zeros((6, 2, 2)), np.zeros((6, 0)), 1.0):
        with pytest.raises(ValueError):
            lto.halo_arclength(bad, 4, 0.01, up)
    for bad_dir in (np.zeros(2), np.zeros((3, 3)), np.zeros((2, 2)), 1.0):
        with pytest.raises(ValueError):
            lto.halo_arclength(np.ones((6, 2)), 4, 0.01, bad_dir)
    with pytest.raises(ValueError):
        lto.halo_arclength(np.ones(6), 4, 0.01, np.ones((3, 1)))          # a table of directions needs a batch of seeds
    for bad_ds in (0.0, -0.01, np.nan, np.inf, [0.01, 0.01], np.ones((1, 1))):
        with pytest.raises(ValueError):
            lto.halo_arclength(np.ones(6), 4, bad_ds, up)
    with pytest.raises(ValueError):
        lto.halo_arclength(np.ones((6, 2)), 4, [0.01, 0.01, 0.01], up)
    for n in (0, -1):
        with pytest.raises(ValueError):
            lto.halo_arclength(np.ones(6), n, 0.01, up)
    for kw in ({"ds_min": 0.0}, {"ds_min": 0.02, "ds_max": 0.01}, {"ds_max": np.inf}, {"ds_min": np.nan}, {"grow": 0.5}, {"grow": np.nan},
               {"grow": np.inf}, {"fast_iter": -1}, {"cos_min": 1.0}, {"cos_min": -0.1}, {"cos_min": np.nan}, {"max_iter": -1},
               {"tol": 0.0}, {"tol": np.nan}, {"t_max": np.inf}, {"t_max": 0.0}, {"sing_tol": 1.0}, {"sing_tol": np.nan}):
        with pytest.raises(ValueError):
            lto.halo_arclength(np.ones(6), 4, 0.01, up, **kw)
    with pytest.raises(AssertionError):
        lto.halo_arclength(np.ones(6), 4, 0.01, up)                       # well-formed input does go on to the library


def test_the_new_entry_is_declared_and_exported():
    name = "lto_halo_arclength_batch"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 30
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lto.h")).read()
    assert ("int %s(" % name) in header
    # one parameter per comma of the prototype, as many as the ctypes signature has
    proto = header[header.index("int %s(" % name):]
    assert proto[:proto.index(");")].count(",") + 1 == len(_lib.SIGNATURES[name][1])
    assert hasattr(ctypes.CDLL(lto.LIB_PATH), name)
    assert callable(lto.halo_arclength) and lto.HaloArclength._fields == (
        "state", "tangent", "det", "ds", "halvings", "period", "jacobi", "resid", "iterations", "history", "status")
    assert lto.load_library().lto_version() == 102
