"""GPU shape sweep of the manifold calls: the paths of k_manifold_eigen, k_manifold_transport / k_manifold_starts,
k_section_flight and k_state_match that tests/test_manifold_gpu.py does not reach.

  eigen     spectra whose stable vector is not the mirrored unstable one, so the inverse iteration and the 6 x 6 LU do the work;
            all 720 P M P^T of one matrix, which take every row exchange; batches over the 64-lane block's edge; the power
            iteration's cap met by a real spectrum; the sign rule's second clause
  seeds     up to 128 (phase, orbit) records and 65 orbits
  sections  the axes z, vx, vy, vz; the third crossing; a direction with the second crossing; the Earth's r_min
  match     ties across waves and across a thread's passes

Every reference is independent of the product (tests/manifold_reference.py); every bound and every input set is a named constant or
a vetted set of tests/test_manifold_shapes_host.py (or of tests/test_manifold_host.py), which derives it from the references alone.
manifold_reference.eigen_restatement is printed for the log and is never an expected value.

Figures measured on an MI355X are in DESIGN 4.26."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import test_manifold_host as H  # noqa: E402
import test_manifold_shapes_host as HS  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

pytestmark = pytest.mark.gpu

STATE0 = np.array([1.1, 0.02, 0.05, 0.01, 0.2, -0.03])            # any finite state: with tau = 0 nothing is flown
EPS = 1e-3


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def _eigen(ctx, mats):
    """The eigen step alone on a list of matrices: (lam [2 x B], V [6 x 2 x B], status [B], the whole result)."""
    B = len(mats)
    r = lto.manifold_seeds(np.repeat(STATE0[:, None], B, axis=1), np.ones(B), np.stack(mats, axis=2), [0.0], eps=EPS, ctx=ctx)
    return r.lam, r.V[:, :, 0, :], r.status, r


def _record(r, b):
    return r.lam[:, b], r.X[..., b], r.V[..., b], r.starts[..., b], r.status[b]


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def _check_pair(lam, V, e, bounds, worst):
    d = HS.misses(lam[0], lam[1], V[:, 0], V[:, 1], e)
    np.maximum(worst, d, out=worst)
    assert np.all(d <= np.array(bounds)), (d, bounds)
    for kind in range(2):
        assert abs(np.linalg.norm(V[:, kind]) - 1.0) <= 1e-15 and V[0, kind] > 0.0


@pytest.fixture(scope="module")
def classes():
    """[(class, M, 50-digit pair)] of the converging classes, solved once."""
    return [(name, M, HS.shared_pair((name, M[0, 0]), M)) for name, M in HS.converging_matrices()]


@pytest.fixture(scope="module")
def singles(gpu_ctx, classes):
    """Every converging matrix in a call of its own."""
    return [_eigen(gpu_ctx, [M])[3] for _, M, _ in classes]


# ------------------------------------------------------------------------------------------------------------------- 1. eigen step
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_eigen_sweep_over_the_spectrum_classes(gpu_ctx, classes, B):
    pick = [classes[(b + B) % len(classes)] for b in range(B)]      # B = 1 does not always see the first class
    lam, V, status, r = _eigen(gpu_ctx, [M for _, M, _ in pick])
    worst = {}
    assert np.all(status == 0)
    for b, (name, M, e) in enumerate(pick):
        _check_pair(lam[:, b], V[:, :, b], e, HS.EIGEN_BOUNDS[name], worst.setdefault(name, np.zeros(4)))
        assert np.array_equal(r.X[:, 0, 0, b], STATE0) and np.array_equal(r.X[:, 1, 0, b], STATE0)       # nothing is flown
        assert np.array_equal(r.starts[..., b], MR.starts_of(r.X[..., b], r.V[..., b], EPS))
    for name, w in worst.items():
        print("B %3d, class %-6s lambda_u %.1e lambda_s %.1e (relative), v_u %.1e v_s %.1e against 50 digits" % (B, name, *w))


@pytest.mark.parametrize("which", list(HS.FAMILIES))
def test_every_row_exchange_of_the_lu(gpu_ctx, which):
    """All 720 P M P^T of one matrix in one call: between them they take all 15 exchanges of two rows and no exchange at every
    step (asserted by the host file); each is held to P applied to the 50-digit vectors of M.  `detuned`: lambda_s lies 1e-3 off
    1 / lambda_u, so v_s is the work of three to four solves; with the exact shift a single solve of the nearly singular system
    returns v_s from any right-hand side, and a solve that exchanges the wrong rows cannot be told from a right one."""
    M0 = HS.family_matrix(which)
    e0 = HS.shared_pair(which, M0)
    lam, V, status, _ = _eigen(gpu_ctx, [MR.permuted(M0, perm) for perm in HS.PERMS])
    hist = {}
    for perm in HS.PERMS:
        for k, p in enumerate(MR.eigen_restatement(MR.permuted(M0, perm)).pivots[:5]):
            hist[(k, p)] = hist.get((k, p), 0) + 1
    print("the restatement's exchanges (k, p): members")
    for k in range(5):
        print("  k = %d: " % k + "  ".join("p = %d: %3d" % (p, hist.get((k, p), 0)) for p in range(k, 6)))
    worst = np.zeros(4)
    assert np.all(status == 0)
    for b, perm in enumerate(HS.PERMS):
        _check_pair(lam[:, b], V[:, :, b], MR.permuted_pair(e0, perm), HS.EIGEN_BOUNDS[which], worst)
    print(which + ", 720 orbits: lambda_u %.1e lambda_s %.1e (relative), v_u %.1e v_s %.1e against 50 digits" % tuple(worst))


def test_cap_and_status_across_the_block_edge(gpu_ctx, classes, singles):
    """A real spectrum that is merely slow meets the cap like the complex pair does; status 1 and NaN exactly on the records without
    a usable pair, at the first lane, inside a wave, at the last lane of the block and the first of the next; the good records are
    what their single calls give, bit for bit."""
    nh = HS.not_hyperbolic()
    bad = {0: HS.matrix(HS.SLOW[0]), 31: nh[0], 63: H.synthetic_M("complex"), 64: H.synthetic_M("nan"),
           5: HS.matrix(HS.SLOW[1]), 17: nh[1], 40: nh[2]}
    mats = [bad[b] if b in bad else classes[b % len(classes)][1] for b in range(65)]
    lam, V, status, r = _eigen(gpu_ctx, mats)
    want = np.array([1 if b in bad else 0 for b in range(65)])
    print("status 1 on lanes %s" % np.nonzero(status)[0])
    assert np.array_equal(status, want)
    for b in range(65):
        if b in bad:
            assert all(np.all(np.isnan(a)) for a in _record(r, b)[:4]), b
        else:
            assert _same(_record(r, b), _record(singles[b % len(classes)], 0)), b
    for b, M in bad.items():                                        # and each of them alone
        assert _eigen(gpu_ctx, [M])[2][0] == 1, b


def test_zero_first_row_takes_the_sign_rules_second_clause(gpu_ctx):
    """After one multiplication by an M whose first row is zero the iterate's x is exactly 0, so v_u's sign is set by its largest
    component.  No non-singular M reaches this clause (lambda v_x = 0 needs lambda = 0), and a monodromy matrix has det 1: this is
    a finite input, not an orbit's.  v_s is held up to its sign only."""
    e = HS.zero_row_pair()
    lam, V, status, _ = _eigen(gpu_ctx, [HS.zero_row_matrix()])
    vu, vs = V[:, 0, 0], V[:, 1, 0]
    d = (abs(lam[0, 0] - e.lam_u) / abs(e.lam_u), np.abs(vu - e.v_u).max(), min(np.abs(vs - e.v_s).max(), np.abs(vs + e.v_s).max()))
    print("zero first row: v_u = %s, lambda_u %.1e (relative), v_u %.1e, v_s %.1e up to sign" % (vu, *d))
    assert status[0] == 0
    assert vu[0] == 0.0 and vu[np.argmax(np.abs(vu))] > 0.0
    assert np.all(np.array(d) <= np.array(HS.ZERO_ROW_BOUNDS))
    assert abs(np.linalg.norm(vu) - 1.0) <= 1e-15 and abs(np.linalg.norm(vs) - 1.0) <= 1e-15


# ------------------------------------------------------------------------------------------------------------------------- 2. seeds
def _orbit_batch(orbits, B):
    ks = [b % 2 for b in range(B)]
    return (ks, np.array([orbits[k][0] for k in ks]).T, np.array([orbits[k][1] for k in ks]), np.stack([orbits[k][2] for k in ks], axis=2))


@pytest.mark.parametrize("n_phase,B", [(13, 5), (64, 1), (1, 65), (21, 3)])
def test_seeds_across_a_block(gpu_ctx, orbits, n_phase, B):
    ks, S, P, M = _orbit_batch(orbits, B)
    tau = np.arange(n_phase) / float(n_phase)
    r = lto.manifold_seeds(S, P, M, tau, eps=EPS, ctx=gpu_ctx)
    one = [lto.manifold_seeds(S[:, k:k + 1], P[k:k + 1], M[:, :, k:k + 1], tau, eps=EPS, ctx=gpu_ctx) for k in range(min(B, 2))]
    assert np.all(r.status == 0)
    eX = eV = 0.0
    for b, k in enumerate(ks):
        lam, X, V = MR.shared_seeds(orbits, k, n_phase, MU)
        eX, eV = max(eX, np.abs(r.X[..., b] - X).max()), max(eV, np.abs(r.V[..., b] - V).max())
        assert abs(r.lam[0, b] - lam[0]) <= H.GPU_LAM_U_REL * abs(lam[0]) and abs(r.lam[1, b] - lam[1]) <= H.GPU_LAM_S_REL * abs(lam[1])
        assert np.array_equal(r.starts[..., b], MR.starts_of(r.X[..., b], r.V[..., b], EPS))       # of the call's own X and V, bit for bit
        assert np.abs(np.linalg.norm(r.V[..., b], axis=0) - 1.0).max() <= 1e-15
        assert _same(_record(r, b), _record(one[k], 0)), b
    print("n_phase %d, B %d (%d records): X %.2e, V %.2e against the reference" % (n_phase, B, n_phase * B, eX, eV))
    assert eX <= H.GPU_SEED_X and eV <= H.GPU_SEED_V


def test_a_nan_period_fails_all_phases_of_its_orbit_alone(gpu_ctx, orbits):
    ks, S, P, M = _orbit_batch(orbits, 5)
    tau = np.arange(13) / 13.0
    good = lto.manifold_seeds(S, P, M, tau, eps=EPS, ctx=gpu_ctx)
    Pn = P.copy()
    Pn[2] = np.nan
    r = lto.manifold_seeds(S, Pn, M, tau, eps=EPS, ctx=gpu_ctx)
    assert list(r.status) == [0, 0, 2, 0, 0]
    assert all(np.all(np.isnan(a)) for a in _record(r, 2)[:4]) and r.X[..., 2].shape == (6, 2, 13)
    for b in (0, 1, 3, 4):
        assert _same(_record(r, b), _record(good, b)), b


# ----------------------------------------------------------------------------------------------------------------- 3. section axes
def _starts(orbits):
    Y, sign = MR.vetted_starts(orbits, HS.EPS_Y0, MU)
    return np.asfortranarray(Y), sign * HS.T_MAX


FLIGHT_FIELDS = ("x_end", "t_end", "count", "dC", "status")


def _same_flights(a, b, pick=slice(None)):
    return all(np.array_equal(np.asarray(getattr(a, f))[..., pick], np.asarray(getattr(b, f))[..., pick], equal_nan=True) for f in FLIGHT_FIELDS)


@pytest.mark.parametrize("n_cross", HS.N_CROSS)
@pytest.mark.parametrize("name,axis", HS.AXES)
def test_flights_to_the_other_axes(gpu_ctx, orbits, name, axis, n_cross):
    keep, refs, _, _, _ = HS.section_set(orbits, axis, n_cross)
    Y, T = _starts(orbits)
    r = lto.section_flight(Y, T, section=(name, 0.0), n_cross=n_cross, ctx=gpu_ctx)
    by_number = lto.section_flight(Y, T, section=(axis, 0.0), n_cross=n_cross, ctx=gpu_ctx)
    assert _same_flights(r, by_number)
    et = ex = 0.0
    for i in np.nonzero(keep)[0]:
        assert r.status[i] == 0 and r.count[i] == refs[i].count == n_cross, (i, r.status[i], r.count[i])
        assert np.sign(r.t_end[i]) == np.sign(T[i])
        et, ex = max(et, abs(r.t_end[i] - refs[i].t_end)), max(ex, np.abs(r.x_end[:, i] - refs[i].x_end).max())
    print("%-2s = 0, crossing %d, %d arcs: t %.2e, x %.2e against the reference; |g| at the end <= %.1e; Jacobi drift <= %.1e"
          % (name, n_cross, keep.sum(), et, ex, np.abs(r.x_end[axis, keep]).max(), r.dC[keep].max()))
    assert et <= HS.GPU_AXIS_T[n_cross] and ex <= HS.GPU_AXIS_X[n_cross]
    assert np.abs(r.x_end[axis, keep]).max() <= 1e-13
    assert r.dC[keep].max() <= H.GPU_DC


@pytest.mark.parametrize("sec_dir", [1, -1])
def test_second_crossing_of_one_direction(gpu_ctx, orbits, sec_dir):
    """sec_dir with n_cross = 2 on y = 0, forward and backward arcs in one call: two crossings counted, both in the sense asked for
    in the order the flight visits them (the first one's from the same call with n_cross = 1)."""
    keep, refs, _, _ = HS.directed_set(orbits, sec_dir)
    Y, T = _starts(orbits)
    r = lto.section_flight(Y, T, section=("y", 0.0), sec_dir=sec_dir, n_cross=2, ctx=gpu_ctx)
    first = lto.section_flight(Y, T, section=("y", 0.0), sec_dir=sec_dir, n_cross=1, ctx=gpu_ctx)
    assert np.any(T[keep] > 0.0) and np.any(T[keep] < 0.0)
    et = ex = 0.0
    for i in np.nonzero(keep)[0]:
        assert r.status[i] == 0 and r.count[i] == 2 and first.status[i] == 0 and first.count[i] == 1, i
        assert np.sign(r.x_end[4, i] * np.sign(T[i])) == sec_dir and np.sign(first.x_end[4, i] * np.sign(T[i])) == sec_dir
        assert abs(first.t_end[i]) < abs(r.t_end[i]) and np.sign(r.t_end[i]) == np.sign(T[i])
        et, ex = max(et, abs(r.t_end[i] - refs[i].t_end)), max(ex, np.abs(r.x_end[:, i] - refs[i].x_end).max())
    print("y = 0, second crossing of direction %+d, %d arcs: t %.2e, x %.2e against the reference" % (sec_dir, keep.sum(), et, ex))
    assert et <= HS.GPU_Y0_DIR2_T and ex <= HS.GPU_Y0_DIR2_X
    assert np.abs(r.x_end[1, keep]).max() <= 1e-13


def test_the_earths_r_min_ends_the_arcs_the_reference_says(gpu_ctx, orbits):
    thr, near, keep, gap, _ = HS.earth_threshold(orbits)
    name, n_cross = HS.R_MIN_SET
    Y, T = _starts(orbits)
    base = lto.section_flight(Y, T, section=(name, 0.0), n_cross=n_cross, ctx=gpu_ctx)
    q = lto.section_flight(Y, T, section=(name, 0.0), n_cross=n_cross, r_min=(thr, 0.0), ctx=gpu_ctx)
    print("r_min[0] = %.4f (a gap of %.0f %%): status 3 on arcs %s, the reference's scan on %s"
          % (thr, 100.0 * gap, np.nonzero(q.status == 3)[0], np.nonzero(near & keep)[0]))
    assert np.array_equal((q.status == 3)[keep], near[keep])
    inside, outside = near & keep, ~near & keep
    d_earth = np.sqrt((q.x_end[0] + MU) ** 2 + q.x_end[1] ** 2 + q.x_end[2] ** 2)
    assert np.all(d_earth[inside] < thr) and np.all(np.abs(q.t_end[inside]) < np.abs(base.t_end[inside]))
    assert _same_flights(q, base, outside) and np.all(base.status[outside] == 0)


# ------------------------------------------------------------------------------------------------------------------------- 4. match
@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("nB", [255, 256, 257, 513])
def test_match_ties_across_waves_and_passes(gpu_ctx, nB, below):
    """Row 0's winner sits at j and again 64 further (another wave) and 256 further (the same thread's next pass), where nB has
    room; `below`: the winner is the last state and its copies sit 64 and 256 before it.  The lowest index wins."""
    rng = np.random.RandomState(7000 + nB)
    A, Bs = rng.uniform(-1.0, 1.0, (6, 3)), rng.uniform(-1.0, 1.0, (6, nB))
    j0 = int(MR.match(A, Bs, 1.0)[0][0])
    j = nB - 1 if below else 0
    Bs[:, [j, j0]] = Bs[:, [j0, j]]                                 # row 0's winner now sits at j
    copies = [c for c in ((j - 64, j - 256) if below else (j + 64, j + 256)) if 0 <= c < nB]
    for c in copies:
        Bs[:, c] = Bs[:, j]
    idx, d, dr, dv = MR.match(A, Bs, 1.0)
    assert len(copies) >= 1 and idx[0] == min(copies + [j])
    r = lto.state_match(np.asfortranarray(A), np.asfortranarray(Bs), ctx=gpu_ctx)
    print("nB %d, winner at %d, copies at %s: index %d" % (nB, j, copies, r.index[0]))
    assert np.array_equal(r.index, idx)
    assert np.array_equal(r.dist, d) and np.array_equal(r.dr, dr) and np.array_equal(r.dv, dv)
