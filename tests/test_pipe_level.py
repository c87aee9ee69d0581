"""The coefficient record of the three pipeline sweeps (LTO_KERNEL_PIPE8, _PIPE32, _PIPE48; pipe_common.hpp, CoefRecord and
pipe_coef_build).  The record leaves out the two exact zeros of the always-thrust-limited laws of the 14-dim system (d mdot / d m,
d lambda_m_dot / d lambda_m), and the 14-dim record is built with the stage weight already in its roots (dynamics.hpp,
coef14_weighted) instead of a product per stored value.

Every form is forced and compared with the per-lane kernel (var_col12 / var_col14 on rhs12 / rhs14: none of the code above) and
with the CPU oracle's fixed-step RK4, at the bounds of test_pipe_col_step.py: 1e-12 on the defect, 1e-11 relative on Phi.  Shapes:
S = 1 (one lane row), 13 (a partly filled workgroup of pipe8), 16 (exactly one), 17 (one and a shadow workgroup), and for the 32- and
48-segment forms also 31, 33 and 49; steps = 1 (no full phase), 2, 3 (odd: the tail step), 64 and 257 (across the 3^-256 rescale).
14-dim with p = 2 is the class that keeps lambda_m in the record (mm, Ll); pipe32 is not built for it (its stages do not pair) and
is left out there.  The references of a shape are computed once and shared by the three forms.

The two defect figures.  Against the per-lane kernel: max |d - d1| / max(1, max |d1|), as in test_pipe_col_step.py.  Against the oracle
the same bound, 1e-12, per row and relative to that row of the integrated end state y(t1) = defect + x_{i+1} (at least 1): the
defect is the small difference of two states, its rounding error is that of y(t1), and the mass row of the 14-dim system is of the
order 1000 -- there two correct implementations of RK4 differ by a few ulp of 1000 after 64 steps (this form and the per-lane
kernel alike: 1.5e-12 absolute at 14-dim, p = 1, S = 13, 64 steps, where they agree with each other to 2e-16), which is 1.5e-15 of
the state.  test_pipe8_edges.py measures its oracle defect against the end state for the same reason."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu

NAMES = {"pipe8": "pipeline8", "pipe32": "pipeline32", "pipe48": "pipeline48", "per_lane": "per-lane"}
SIZES = {"pipe8": (1, 13, 16, 17), "pipe32": (1, 13, 16, 17, 31, 33, 49), "pipe48": (1, 13, 16, 17, 31, 33, 49)}
CLASSES = [(nd, p) for nd in (12, 14) for p in (0.0, 1.0, 2.0)]
FORMS = [(k, nd, p) for k in ("pipe8", "pipe32", "pipe48") for nd, p in CLASSES if not (k == "pipe32" and nd == 14 and p > 1.0)]
SENTINEL = 7.0
BOUND_DEFECT, BOUND_PHI = 1e-12, 1e-11


def thrust(p):
    return 10.0 if p > 1.0 else 0.05


def problem(ndim, n, nb=1, seed=5):
    XC, T = synth.indirect_problem(n, n_batch=nb, seed=seed)
    if ndim == 14:
        X = np.zeros((14, n, nb), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        return X, T, 2000.0
    return XC, T, 1000.0


def sweep(ctx, kernel, ndim, prms, X, T, steps):
    """One STM sweep of a batch [ndim][n][nb], Phi and the defect prefilled with the sentinel."""
    import torch
    n, nb = X.shape[1], X.shape[2]
    S = (n - 1) * nb
    plan = lto.IndirectPlan(ctx, n, nb, prms if nb > 1 else prms[0], lto.integrator(lto.RK4, steps=steps), ndim=ndim)
    plan.set_kernel({"pipe8": plan.KERNEL_PIPE8, "pipe32": plan.KERNEL_PIPE32, "pipe48": plan.KERNEL_PIPE48, "per_lane": plan.KERNEL_PER_LANE}[kernel])
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    Phi = torch.full((ndim * ndim, S), SENTINEL, dtype=torch.float64, device="cuda")
    d = torch.full((ndim, S), SENTINEL, dtype=torch.float64, device="cuda")
    plan.jacobian(Xd, n * nb, td, nb, Phi, S, d, S)
    torch.cuda.synchronize()
    assert plan.last_kernel() == NAMES[kernel]
    plan.close()
    return Phi.cpu().numpy(), d.cpu().numpy()


_refs = {}


def references(ctx, oracle, ndim, p, steps, S):
    """(Phi, defect) of the per-lane kernel and of the oracle for one shape, [column * ndim + row][segment]; computed once."""
    key = (ndim, p, steps, S)
    if key not in _refs:
        X, T, slot = problem(ndim, S + 1)
        prm = [MU, DU, TU, thrust(p), slot, 1.0, p, 1.0]
        P1, d1 = sweep(ctx, "per_lane", ndim, [lto.make_params(*prm)], X, T, steps)
        Xh, t = np.asfortranarray(X[:, :, 0]), np.ascontiguousarray(T[:, 0])
        fn = oracle.indirect14 if ndim == 14 else oracle.indirect_jacobian
        Po, do, rc = fn(Xh, t, prm, oracle.RK4, steps)
        assert rc == 0
        Po = np.ascontiguousarray(Po.transpose(1, 0, 2)).reshape(ndim * ndim, S)      # Phi[row, column, segment] -> [column][row]
        y1 = np.maximum(1.0, np.abs(do + Xh[:, 1:]).max(axis=1))                        # per row: magnitude of the end state
        for a in (P1, d1, Po, do, y1):
            a.setflags(write=False)
        _refs[key] = (P1, d1, Po, do, y1)
    return _refs[key]


def figures(P, d, Pr, dr):
    return np.abs(d - dr).max() / max(1.0, np.abs(dr).max()), np.abs(P - Pr).max() / np.abs(Pr).max()


@pytest.mark.parametrize("kernel,ndim,p", FORMS)
@pytest.mark.parametrize("steps", [1, 2, 3, 64, 257])
def test_forced_form_agrees_with_the_per_lane_kernel_and_the_oracle(gpu_ctx, oracle, kernel, ndim, p, steps):
    for S in SIZES[kernel]:
        X, T, slot = problem(ndim, S + 1)
        P, d = sweep(gpu_ctx, kernel, ndim, [lto.make_params(MU, DU, TU, thrust(p), slot, 1.0, p, 1.0)], X, T, steps)
        assert np.all(np.isfinite(P)) and np.all(np.isfinite(d)), S
        assert not np.any(P == SENTINEL) and not np.any(d == SENTINEL), S               # every entry written
        P1, d1, Po, do, y1 = references(gpu_ctx, oracle, ndim, p, steps, S)
        e_d1, e_p1 = figures(P, d, P1, d1)
        e_do, e_po = (np.abs(d - do).max(axis=1) / y1).max(), np.abs(P - Po).max() / np.abs(Po).max()
        print("pipe_level %s ndim=%d p=%g S=%d steps=%d: per-lane defect %.3e Phi %.3e, oracle defect %.3e Phi %.3e (bounds %g, %g)"
              % (kernel, ndim, p, S, steps, e_d1, e_p1, e_do, e_po, BOUND_DEFECT, BOUND_PHI))
        assert e_d1 < BOUND_DEFECT and e_do < BOUND_DEFECT, S
        assert e_p1 < BOUND_PHI and e_po < BOUND_PHI, S


@pytest.mark.parametrize("kernel,ndim,p", FORMS)
def test_zero_lambda_v_gives_finite_coefficients(gpu_ctx, kernel, ndim, p):
    """lambda_v = 0 at a node: the first stage of that segment has |lambda_v| = 0, where 1 / |lambda_v| is taken as 0 -- lhat and the
    weighted ua, ub are zeros, not NaN."""
    S, steps, node = 17, 3, 5
    X, T, slot = problem(ndim, S + 1)
    X = X.copy(order="F")
    lv = 10 if ndim == 14 else 9
    X[lv:lv + 3, node, 0] = 0.0
    prms = [lto.make_params(MU, DU, TU, thrust(p), slot, 1.0, p, 1.0)]
    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T, steps)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(d))
    P1, d1 = sweep(gpu_ctx, "per_lane", ndim, prms, X, T, steps)
    e_d, e_p = figures(P, d, P1, d1)
    print("pipe_level zero lambda_v %s ndim=%d p=%g: defect %.3e Phi %.3e" % (kernel, ndim, p, e_d, e_p))
    assert e_d < BOUND_DEFECT and e_p < BOUND_PHI


@pytest.mark.parametrize("kernel,ndim,p", FORMS)
def test_nan_span_gives_nan_in_every_entry_of_phi(gpu_ctx, kernel, ndim, p):
    """A segment whose span is NaN: every entry of its Phi is NaN, the unit columns pipe8 and pipe32 do not integrate included; the
    other segments are untouched by it."""
    S, steps, bad = 17, 3, 6
    X, T, slot = problem(ndim, S + 1)
    prms = [lto.make_params(MU, DU, TU, thrust(p), slot, 1.0, p, 1.0)]
    P0, d0 = sweep(gpu_ctx, kernel, ndim, prms, X, T, steps)
    T = T.copy()
    T[bad, 0] = np.nan                                  # the spans of segments bad - 1 and bad
    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T, steps)
    nan_seg = np.zeros(S, dtype=bool)
    nan_seg[[bad - 1, bad]] = True
    assert np.all(np.isnan(P[:, nan_seg]))
    assert np.array_equal(P[:, ~nan_seg], P0[:, ~nan_seg]) and np.array_equal(d[:, ~nan_seg], d0[:, ~nan_seg])


@pytest.mark.parametrize("kernel,ndim", [(k, nd) for k in ("pipe8", "pipe32", "pipe48") for nd in (12, 14) if not (k == "pipe32" and nd == 14)])
def test_mixed_p1_p2_batch_every_launch_stores_its_own_segments_only(gpu_ctx, kernel, ndim):
    """Two trajectories of 17 segments, p = 1 and p = 2, in one call: one launch per class over the whole batch (the class boundary
    inside a workgroup of every form; 14-dim: a record without and a record with mm / Ll).  Each trajectory swept alone comes out
    the same bit for bit."""
    n, steps = 18, 3
    X, T, slot = problem(ndim, n, nb=2, seed=17)
    prms = [lto.make_params(MU, DU, TU, thrust(p), slot, 1.0, p, 1.0) for p in (1.0, 2.0)]
    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T, steps)
    assert not np.any(P == SENTINEL) and not np.any(d == SENTINEL) and np.all(np.isfinite(P)) and np.all(np.isfinite(d))
    for b in range(2):
        Pb, db = sweep(gpu_ctx, kernel, ndim, [prms[b]], np.asfortranarray(X[:, :, b:b + 1]), np.asfortranarray(T[:, b:b + 1]), steps)
        assert np.array_equal(P[:, b * (n - 1):(b + 1) * (n - 1)], Pb), b
        assert np.array_equal(d[:, b * (n - 1):(b + 1) * (n - 1)], db), b
