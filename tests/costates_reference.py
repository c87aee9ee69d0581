"""The multiplier part of qp_reference's refined KKT solution, for the costates of the direct transcription.

Helper module of the tests, not a test file; qp_reference.py is imported as it stands.  QpSystem orders its constraints with the S
linearised defects first (row ns i + a = component a of defect i), and its KKT system reads 2 Q z + A' nu = -2 q: the sign of
kernels_direct_qp.hip (grad cost + A' l = 0).  So the multipliers of the defects are nu[:ns S], and with E_i, F_i the first two
column blocks of Jt the node costates are Lambda_k = E_k' l_k (k < n - 1), Lambda_{n-1} = -F_{n-2}' l_{n-2}, formed here in long
double from the refined solution.  The same quantities of the plain float64 solve give the host error the device bars are multiples
of."""
import numpy as np

import qp_reference as QR

LD = QR.LD


def lambdas(Jt, l):
    """(E' l [ns, S], F' l [ns, S]) in the precision of l."""
    ns = Jt.shape[0]
    J = Jt.astype(l.dtype)
    return np.einsum("rci,ri->ci", J[:, :ns, :], l), np.einsum("rci,ri->ci", J[:, ns:2 * ns, :], l)


class Costates:
    """mult [ns, S], Lambda [ns, n] (float64, rounded from the refined long-double values), El, Fl (long double), and the errors
    of the plain float64 host solve against them: err_mult, err_lambda (relative 2-norms)."""


def reference(s):
    """Costates of one qp_reference.Synthetic (its targets, its impulse setting)."""
    qs = s.sys
    z, z0 = qs.solve(qs.rhs0(s.d, s.X, s.U, *s.targets))
    ns, S = qs.ns, qs.S
    out = Costates()
    l = z[qs.nz:qs.nz + ns * S].reshape(S, ns).T
    l0 = z0[qs.nz:qs.nz + ns * S].reshape(S, ns).T
    out.El, out.Fl = lambdas(s.Jt, l)
    lam = np.concatenate([out.El, -out.Fl[:, -1:]], axis=1)
    El0, Fl0 = lambdas(s.Jt, l0)
    lam0 = np.concatenate([El0, -Fl0[:, -1:]], axis=1)
    out.mult_ld = l
    out.mult, out.Lambda = l.astype(np.float64), lam.astype(np.float64)
    out.err_mult, out.err_lambda = QR.rel(l0, out.mult), QR.rel(lam0, out.Lambda)
    return out


_CACHE = {}


def case(family, ns, S, imp, seed=None, g=None):
    """The synthetic system of one shape and its reference costates, computed once per run: (Synthetic, Costates).  The scaled
    family takes its three magnitudes in turn over S."""
    key = (family, ns, S, bool(imp), seed, g)
    if key not in _CACHE:
        f = QR.FAMILIES.index(family)
        gg = (QR.SCALED_G[S % 3] if family == "scaled" else 1.0) if g is None else g
        s = QR.synthetic(family, ns, S, (4000 * S + 10 * ns + 2 * imp + f) if seed is None else seed, imp, g=gg)
        _CACHE[key] = (s, reference(s))
    return _CACHE[key]


def host_errors(sizes, family):
    """The largest error of the plain float64 host solve over the sweep of one family: (multipliers, Lambda)."""
    em = el = 0.0
    for S in sizes:
        for ns in (6, 7):
            for imp in (False, True):
                r = case(family, ns, S, imp)[1]
                em, el = max(em, r.err_mult), max(el, r.err_lambda)
    return em, el
