"""CPU: the host mirror of the costates of the direct transcription (drivers.direct_costates_dense) against the
multiplier part of qp_reference's refined KKT solution, on the three synthetic families, ns 6 and 7, S in {1, 2, 5, 17}, impulses
off and on; the sign convention pinned on the reference's own solution; and the new entry points in the binding tables.

Bar of the mirror.  The mirror and the reference's plain float64 solve are two host LU solves of one well-conditioned system
(condition estimate <= COND_BOUND after equilibration), so they land within a constant of each other: the bar is 100 x the
reference's own error estimate for the multipliers (its plain float64 solve against its refined one), largest over the family's
cases, and that estimate itself must stay below ERR_FLOOR.  Measured here (multipliers, relative 2-norm; printed by the tests):
  family        mirror      host float64    bar = 100 x host
  orthogonal    2.4e-15     4.3e-15         4.3e-13
  scaled        5.8e-15     4.1e-14         4.1e-12
  permutation   5.4e-16     1.1e-15         1.1e-13
"""
import ctypes
import os

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, _lib

import costates_reference as CR
import qp_reference as QR

SIZES = [1, 2, 5, 17]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family", QR.FAMILIES)
def test_mirror_multipliers_match_the_refined_reference(family):
    host_m, host_l = CR.host_errors(SIZES, family)
    assert host_m < QR.ERR_FLOOR and host_l < QR.ERR_FLOOR
    bar_m, bar_l = 100 * host_m, 100 * host_l
    worst = 0.0
    for S in SIZES:
        for ns in (6, 7):
            for imp in (False, True):
                s, ref = CR.case(family, ns, S, imp)
                Lam, mult, res = drivers.direct_costates_dense(s.Jt, s.d, s.X, s.U, s.t, *s.targets, 1.0, 1.0, allowImpulsive=imp)
                em, el = QR.rel(mult, ref.mult), QR.rel(Lam, ref.Lambda)
                worst = max(worst, em)
                assert Lam.shape == (ns, S + 1) and mult.shape == (ns, S)
                assert em <= bar_m and el <= bar_l, (family, ns, S, imp, em, el, bar_m, bar_l)
                assert res <= bar_l and (S > 1 or res == 0.0), (family, ns, S, imp, res)
    print("\ncostates host %s: mirror %.2e, host float64 %.2e (Lambda %.2e), bar %.2e" % (family, worst, host_m, host_l, bar_m))


@pytest.mark.parametrize("family", QR.FAMILIES)
def test_sign_convention_on_the_references_own_solution(family):
    """Lambda_k = E_k' l_k = -F_{k-1}' l_{k-1} at every interior node of the refined solution: the QP's stationarity in dx_k, a
    row of K z = rhs with a zero right-hand side.  The refined multipliers carry a relative error below ERR_FLOOR, so the row's
    residual stays below 2 ns ERR_FLOOR max|E, F| max|l|.  And the multipliers are not zero: -2 w (u + du) = G' l + H' l (the
    stationarity in du, same sign) is checked against the refined du on node 0, where only G_0' l_0 enters."""
    for S in SIZES:
        for ns in (6, 7):
            s, ref = CR.case(family, ns, S, False)
            assert np.abs(ref.mult).max() > 0
            if S > 1:
                r = np.abs(ref.El[:, 1:] + ref.Fl[:, :-1]).max()
                assert float(r) <= 2 * ns * QR.ERR_FLOOR * np.abs(s.Jt[:, :2 * ns]).max() * np.abs(ref.mult).max(), (family, ns, S, float(r))
            step, _ = s.sys.frozen(s.d, s.X, s.U, *s.targets)
            w0 = QR.weights(s.t)[0]
            lhs = -2.0 * w0 * (s.U[:, 0] + step.dU[:, 0])
            rhs = s.Jt[:, 2 * ns:2 * ns + 3, 0].T @ ref.mult[:, 0]
            assert np.abs(lhs - rhs).max() <= 1e-9 * max(np.abs(lhs).max(), np.abs(rhs).max()), (family, ns, S)
            # the two expressions of the node costates, and the end nodes' definitions
            lam, _ = drivers.costates_from_multipliers(s.Jt, ref.mult)
            assert QR.rel(lam, ref.Lambda) <= 1e-14
            assert np.array_equal(ref.Lambda[:, -1], (-ref.Fl[:, -1]).astype(np.float64))


def test_costates_from_direct_with_injected_ops():
    """The driver on an injected back end (the synthetic blocks as its Jacobian): XC = (X; c^2 Lambda) of the mirror."""
    s, ref = CR.case("orthogonal", 6, 5, False)

    class Ops:
        def jacobian(self, X, U, t, nsteps):
            return s.Jt, s.d
    s0, sf, mass, dV1, dV2 = s.targets
    XC = drivers.costates_from_direct(s.X, s.U, s.t, 10, mass, 2000.0, lto.MU, 1.0, 1.0, s0, sf, dV1, dV2, ops=Ops())
    c = lto.costate_scale(1.0, 1.0)
    assert c == 1e-6
    assert XC.shape == (12, 6) and np.array_equal(XC[:6], s.X)
    assert QR.rel(XC[6:] / (c * c), ref.Lambda) <= 100 * max(ref.err_lambda, np.finfo(np.float64).eps)
    last = drivers.costates_from_direct.last
    assert last["status"] == 0 and QR.rel(last["mult"], ref.mult) <= 100 * max(ref.err_mult, np.finfo(np.float64).eps)
    with pytest.raises(NotImplementedError):
        drivers.costates_from_direct(np.zeros((7, 6)), s.U, s.t, 10, mass, 2000.0, lto.MU, 1.0, 1.0, ops=Ops())


def test_entry_points_are_bound_everywhere():
    lib = ctypes.CDLL(lto.LIB_PATH)
    julia = open(os.path.join(ROOT, "julia", "LowThrustOptHIP.jl")).read()
    for name in ("lto_direct_costates_dev", "lto_direct_costates_batch", "lto_direct_costates"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "entry(ctx, :direct_costates)" in julia
    assert len(_lib.SIGNATURES["lto_direct_costates_batch"][1]) == len(_lib.SIGNATURES["lto_direct_costates"][1]) + 3
    assert hasattr(lto.DirectPlan, "costates") and callable(lto.direct_costates)
    # argument checks that answer without a device
    assert lib.lto_direct_costates_dev(None, None, None, 0, None, 0, None, 0, None) == _lib.LTO_ENULL
    fn = lib.lto_direct_costates_batch
    fn.restype, fn.argtypes = _lib.SIGNATURES["lto_direct_costates_batch"]
    assert fn(None, 5, 30, 1, None, None, None, 1, 10, None, None, 1, 0, None, None, None, None, None) == _lib.LTO_EINVAL
    assert fn(None, 6, 30, 1, None, None, None, 1, 10, None, None, 1, 0, None, None, None, None, None) == _lib.LTO_ENULL
