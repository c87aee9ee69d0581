"""CPU checks for the invariant-manifold calls: the independent reference (tests/manifold_reference.py) against
itself at looser tolerances -- for every quantity the GPU tests (tests/test_manifold_gpu.py) compare, its own spread between
(rtol, atol) = (1e-13, 1e-14) and (1e-11, 1e-12) has to stay below a tenth of the bound the device is held to, each bound being ten
times the spread seen, rounded up to a power of ten -- a sanity check of the reference, and the argument checks the Python layer
makes before any library call.

The eigen step has no tolerance to loosen: its reference is a 50-digit solve of the same M.  Its bounds are ten times, rounded up,
what a backward-stable binary64 eigen-solve (LAPACK through numpy) misses that reference by on the same matrices: 1e-15 and 1e-11
relative in lambda_u and lambda_s, 3e-16 and 5e-14 in the vectors -- what the number format can give on these M, whoever solves."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.hotpath import manifold_seeds, section_flight, state_match  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

# ---- the bounds of tests/test_manifold_gpu.py
GPU_LAM_U_REL, GPU_LAM_S_REL, GPU_VEC_U, GPU_VEC_S = 1e-14, 1e-10, 1e-14, 1e-12      # eigen step against the 50-digit solve
GPU_SEED_X, GPU_SEED_V = 1e-10, 1e-9          # orbit points and unit vectors at the phases (spread 6.4e-12, 1.1e-11)
GPU_RK4_X, GPU_RK4_V = 1e-10, 1e-10           # RK4 x 4000 against DOP853 (2.1e-12, 2.4e-12 between the two in the reference)
GPU_Y0_T, GPU_Y0_X = 1e-9, 1e-9               # y = 0, first and second crossing, eps 1e-3 (spread 7.8e-11, 5.1e-11)
GPU_X1MU_T, GPU_X1MU_X = 1e-8, 1e-8           # x = 1 - MU, first crossing, eps 1e-2 (spread 3.1e-10, 3.0e-10)
GPU_SAMPLES = 1e-8                            # 5 samples of the y = 0 arcs (spread 1.8e-10)
GPU_SHORT_X = 1e-10                           # the state at t_max = +-0.5 (spread 1.01e-12)
GPU_DC = 1e-11                                # Jacobi drift of an arc (the issue's)
EPS_Y0, EPS_X1MU = 1e-3, 1e-2
T_MAX = 12.0


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def synthetic_M(kind):
    """Q D Q^-1 with reciprocal pairs: 'negative' lambda_u = -30; 'complex' a dominant pair 40 e^{+-i}; 'nan' one NaN entry."""
    rng = np.random.RandomState(7)
    Q = np.eye(6) + 0.3 * rng.uniform(-1.0, 1.0, (6, 6))
    c, s = np.cos(1.0), np.sin(1.0)
    D = np.zeros((6, 6))
    if kind == "complex":
        D[:2, :2] = 40.0 * np.array([[c, -s], [s, c]])
        D[2:4, 2:4] = np.array([[c, s], [-s, c]]) / 40.0
        D[4, 4], D[5, 5] = 2.0, 0.5
    else:
        D[0, 0], D[1, 1] = -30.0, -1.0 / 30.0
        D[2, 2], D[3, 3] = 2.0, 0.5
        D[4:, 4:] = np.array([[c, -s], [s, c]])
    M = Q @ D @ np.linalg.inv(Q)
    if kind == "nan":
        M[2, 3] = np.nan
    return M


def test_reference_eigen_pair_and_what_binary64_gives(orbits):
    mats = [o[2] for o in orbits] + [synthetic_M("negative")]
    for i, M in enumerate(mats):
        e = MR.eig_pair(M)
        lam, V = np.linalg.eig(M)
        iu, i_s = np.argmax(np.abs(lam)), np.argmin(np.abs(lam))
        d = (abs(lam[iu].real - e.lam_u) / abs(e.lam_u), abs(lam[i_s].real - e.lam_s) / abs(e.lam_s),
             np.abs(MR.sign_rule(V[:, iu].real) - e.v_u).max(), np.abs(MR.sign_rule(V[:, i_s].real) - e.v_s).max())
        print("M %d: lambda_u %.12g lambda_s %.12g, lambda_u lambda_s - 1 = %.2e; LAPACK off by %.1e %.1e (relative), vectors %.1e %.1e"
              % (i, e.lam_u, e.lam_s, e.lam_u * e.lam_s - 1.0, *d))
        assert d[0] <= 0.1 * GPU_LAM_U_REL and d[1] <= 0.1 * GPU_LAM_S_REL and d[2] <= 0.1 * GPU_VEC_U and d[3] <= 0.1 * GPU_VEC_S
        assert abs(np.linalg.norm(e.v_u) - 1.0) < 1e-15 and abs(np.linalg.norm(e.v_s) - 1.0) < 1e-15
        assert e.v_u[0] > 0.0 and e.v_s[0] > 0.0
    assert abs(MR.eig_pair(mats[2]).lam_u + 30.0) < 1e-12
    assert MR.eig_pair(synthetic_M("complex")) is None and MR.eig_pair(synthetic_M("nan")) is None
    for k, vx in ((0, 0.046), (1, 0.098)):                       # safely away from the sign rule's edge
        assert abs(MR.eig_pair(orbits[k][2]).v_u[0] - vx) < 1e-3


def test_stable_vector_is_the_mirrored_unstable_one(orbits):
    S = np.diag([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    for k, (_, _, M) in enumerate(orbits):
        e = MR.eig_pair(M)
        d = np.abs(e.v_s - MR.sign_rule(S @ e.v_u)).max()
        print("orbit %d: |v_s - S v_u| = %.2e" % (k + 1, d))
        assert d < 1e-9


@pytest.mark.parametrize("k", [0, 1])
def test_seed_spread_is_a_tenth_of_the_gpu_bounds(orbits, k):
    _, X, V = MR.shared_seeds(orbits, k, 8, MU)
    _, Xl, Vl = MR.shared_seeds(orbits, k, 8, MU, *MR.LOOSE)
    eX, eV = np.abs(X - Xl).max(), np.abs(V - Vl).max()
    print("orbit %d, 8 phases: spread X %.2e, V %.2e" % (k + 1, eX, eV))
    assert eX <= 0.1 * GPU_SEED_X and eV <= 0.1 * GPU_SEED_V
    assert np.array_equal(X[:, 0, 0], orbits[k][0]) and np.array_equal(X[:, 1, 0], orbits[k][0])      # tau = 0 flies nothing


def _rk4(f, w, span, n):
    h = span / n
    for _ in range(n):
        k1 = f(0.0, w)
        k2 = f(0.0, w + 0.5 * h * k1)
        k3 = f(0.0, w + 0.5 * h * k2)
        k4 = f(0.0, w + h * k3)
        w = w + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return w


@pytest.mark.parametrize("k", [0, 1])
def test_rk4_spread_is_a_tenth_of_the_gpu_bound(orbits, k):
    """RK4 with 4 000 steps per flight against DOP853 at 1e-13, in the reference: phases 1/3 and 2/3, both kinds."""
    s, P, M = orbits[k]
    e = MR.eig_pair(M)
    eX = eV = 0.0
    for tau in (1.0 / 3.0, 2.0 / 3.0):
        for kind, v in enumerate((e.v_u, e.v_s)):
            x, vv = MR.transport(s, P, v, tau, kind, MU)
            span = tau * P if kind == 0 else (1.0 - tau) * P
            w = _rk4(MR.rhs12(MU, 1.0 if kind == 0 else -1.0), np.concatenate([s, v]), span, 4000)
            eX = max(eX, np.abs(w[:6] - x).max())
            eV = max(eV, np.abs(w[6:] / np.linalg.norm(w[6:]) - vv).max())
    print("orbit %d: RK4 x 4000 against DOP853: X %.2e, V %.2e" % (k + 1, eX, eV))
    assert eX <= 0.1 * GPU_RK4_X and eV <= 0.1 * GPU_RK4_V


def _flight_spread(orbits, eps, axis, value, n_cross, sec_dir=0):
    Y, sign = MR.vetted_starts(orbits, eps, MU)
    et = ex = 0.0
    times = []
    for i in range(64):
        a = MR.shared_flight(Y[:, i], sign[i] * T_MAX, axis, value, MU, sec_dir, n_cross)
        b = MR.shared_flight(Y[:, i], sign[i] * T_MAX, axis, value, MU, sec_dir, n_cross, *MR.LOOSE)
        assert a.status == 0 and b.status == 0 and a.count == n_cross, i          # the share of cases left out is zero
        et, ex = max(et, abs(a.t_end - b.t_end)), max(ex, np.abs(a.x_end - b.x_end).max())
        times.append(abs(a.t_end))
    return et, ex, min(times), max(times)


@pytest.mark.parametrize("n_cross,sec_dir", [(2, 0), (1, 0), (1, 1), (1, -1)])
def test_y0_flight_spread_is_a_tenth_of_the_gpu_bounds(orbits, n_cross, sec_dir):
    et, ex, t0, t1 = _flight_spread(orbits, EPS_Y0, 1, 0.0, n_cross, sec_dir)
    print("y = 0, crossing %d, direction %d, eps %g, 64 arcs: |t| in [%.2f, %.2f], spread t %.2e, x %.2e" % (n_cross, sec_dir, EPS_Y0, t0, t1, et, ex))
    assert et <= 0.1 * GPU_Y0_T and ex <= 0.1 * GPU_Y0_X
    assert t1 < 3.1


def test_x1mu_flight_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    et, ex, t0, t1 = _flight_spread(orbits, EPS_X1MU, 0, 1.0 - MU, 1)
    print("x = 1 - MU, first crossing, eps %g, 64 arcs: |t| in [%.2f, %.2f], spread t %.2e, x %.2e" % (EPS_X1MU, t0, t1, et, ex))
    assert et <= 0.1 * GPU_X1MU_T and ex <= 0.1 * GPU_X1MU_X


def test_sample_and_short_arc_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    Y, sign = MR.vetted_starts(orbits, EPS_Y0, MU)
    es = eh = 0.0
    for i in range(0, 64, 5):
        a = MR.shared_flight(Y[:, i], sign[i] * T_MAX, 1, 0.0, MU, 0, 2)
        A, B = MR.flight_samples(Y[:, i], a.t_end, 5, MU), MR.flight_samples(Y[:, i], a.t_end, 5, MU, *MR.LOOSE)
        es = max(es, np.abs(A - B).max())
        h, hl = MR.flight(Y[:, i], sign[i] * 0.5, 1, 0.0, MU, 0, 0), MR.flight(Y[:, i], sign[i] * 0.5, 1, 0.0, MU, 0, 0, *MR.LOOSE)
        eh = max(eh, np.abs(h.x_end - hl.x_end).max())
    print("5 samples to the second y = 0 crossing: spread %.2e; the state at t = +-0.5: %.2e" % (es, eh))
    assert es <= 0.1 * GPU_SAMPLES and eh <= 0.1 * GPU_SHORT_X


def test_vetted_x1mu_set_reaches_the_section_and_passes_the_moon_on_both_sides_of_r_min(orbits):
    """The eps 1e-3 set of the status tests: every arc reaches x = 1 - MU before |t| = 12, and the closest step end to the Moon is
    well inside 0.05 for some and well outside for the others (none within 5 % of it, so the device's own steps decide alike)."""
    Y, sign = MR.vetted_starts(orbits, EPS_Y0, MU)
    cl = []
    for i in range(64):
        a = MR.shared_flight(Y[:, i], sign[i] * T_MAX, 0, 1.0 - MU, MU, 0, 1)
        assert a.status == 0 and abs(a.t_end) <= 8.7
        cl.append(a.closest[1])
    cl = np.array(cl)
    print("closest step ends to the Moon: %s" % np.sort(np.round(cl, 4)))
    assert np.any(cl < 0.05) and np.any(cl > 0.05)
    assert not np.any(np.abs(cl - 0.05) < 0.05 * 0.05)


def test_match_reference_rule():
    A = np.array([[0.0, 0, 0, 0, 0, 0]]).T
    Bs = np.array([[1.0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 0, 0, 0], [0.5, 0, 0, 0, 0, 0], [0.5, 0, 0, 0, 0, 0], [0.0, 0, 0, 0.1, 0, 0]]).T
    idx, d, dr, dv = MR.match(A, Bs, 10.0)
    assert idx[0] == 2 and d[0] == 0.5 and dr[0] == 0.5 and dv[0] == 0.0
    idx, d, dr, dv = MR.match(A, Bs, 1.0)
    assert idx[0] == 4 and d[0] == 0.1
    idx, d, _, _ = MR.match(A, Bs * np.nan, 1.0)
    assert idx[0] == -1 and np.isnan(d[0])


def test_hotpath_rejects_malformed_input_before_any_library_call(monkeypatch):
    def no_context():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lto.hotpath, "default_context", no_context)
    s, M = np.zeros(6), np.eye(6)
    for bad in (dict(state0=np.zeros(5)), dict(state0=np.zeros((6, 0))), dict(M=np.eye(5)), dict(M=np.zeros((6, 6, 1))),
                dict(state0=np.zeros((6, 2))), dict(period=[1.0, 2.0]), dict(tau=[]), dict(tau=[0.0, np.nan]), dict(eps=0.0),
                dict(eps=np.inf), dict(integ=lto.integrator(lto.RKF78_FIXED, steps=4)), dict(integ=lto.integrator(lto.RK4, steps=0))):
        kw = dict(state0=s, period=1.0, M=M, tau=[0.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            manifold_seeds(**kw)
    for bad in (dict(y0=np.zeros(5)), dict(y0=np.zeros((6, 2, 2))), dict(t_max=0.0), dict(t_max=np.nan), dict(t_max=[1.0, 2.0]),
                dict(section=("w", 0.0)), dict(section=(6, 0.0)), dict(section=(1, np.inf)), dict(section=1), dict(sec_dir=2),
                dict(n_cross=-1), dict(n_samples=1), dict(n_samples=-2), dict(r_min=(0.0,)), dict(r_min=(-1.0, 0.0)),
                dict(r_min=(0.0, np.nan)), dict(integ=lto.integrator(lto.RKF78_ADAPTIVE)), dict(integ=lto.integrator(lto.RK4))):
        kw = dict(y0=s, t_max=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            section_flight(**kw)
    for bad in (dict(A=np.zeros(5)), dict(Bs=np.zeros(6)), dict(Bs=np.zeros((6, 0))), dict(A=np.zeros((6, 0))), dict(w=-1.0),
                dict(w=np.nan)):
        kw = dict(A=s, Bs=np.zeros((6, 3)))
        kw.update(bad)
        with pytest.raises(ValueError):
            state_match(**kw)
    with pytest.raises(ValueError):
        drivers.halo_manifold((s, 1.0, M), 8, branches="u+x-")
    with pytest.raises(ValueError):
        drivers.halo_manifold((s, 1.0, np.eye(5)), 8)
    with pytest.raises(ValueError):
        drivers.halo_manifold((s, 1.0, M), 0)
