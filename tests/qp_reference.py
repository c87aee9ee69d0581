"""Host reference for the QP step of the direct method (kernels_direct_qp.hip): the frozen step and the free-end / free-tf steps.

Helper module of the tests, not a test file.  One trajectory: unknowns z = (dx node-major [ns n], du node-major [3 n], the two
impulse updates [6]); constraints A z = b in this order: the S linearised defects, the pins of node 0 and node n-1 (6 each, the
velocity rows carry the impulse update), the initial mass (ns = 7) and, without impulses, d1 = d2 = 0.  The KKT matrix
K = [[2 Q, A'], [A, 0]] is assembled sparse from triplets, equilibrated as the host code does (20 Ruiz sweeps, started from the kernels' own
scaling; the factors are then rounded to powers of two, so that D K D is exact) and factored once by splu.  Every right-hand side is solved in float64 and then
refined with residuals b - K z formed in long double from the triplets of the UNSCALED matrix; `solve` returns both, and the gap
between them is the reference's own error estimate (and the error of a plain float64 host solve, which the bars of
test_direct_qp_shapes_gpu.py are multiples of).

Free steps: p stays out of the factored system.  The constraint right-hand side is linear in p (b = b0 + g0 p1 at node 0's pins,
+ gf p2 at node n-1's, - dtf p3 in the defect rows), so z(p) = z0 + sum_j z_j p_j from 3 or 4 refined solves on the one
factorisation, and the reduced cost phi(p) = phi0 + G.p + p'Hp/2 is formed in long double.  The 2- or 3-dimensional box problem is
solved by enumerating the 3^k active sets (each coordinate free, at its lower or at its upper bound): a set is accepted when its
free coordinates lie in the box and the reduced gradient has the right sign at its active bounds; the accepted point of smallest
phi wins, ties go to the smaller max(|p1|/0.1, |p2|/0.1, |p3|/step) and then to the earlier set (include/lto.h).

Synthetic frozen systems (`synthetic`): the device entry takes any Jac and defect, so three families give any segment count
without a sweep -- `orthogonal`, `scaled` and `permutation`, described at `synthetic`.  Every system is drawn again (seed + 7919 k)
until the 1-norm condition estimate of its equilibrated KKT matrix is at most COND_BOUND.  Only numpy and scipy."""
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
P_BOUND = 0.1
COND_BOUND = 1e8            # 1-norm condition estimate of the equilibrated KKT matrix of a synthetic system
ERR_FLOOR = 1e-11           # the reference's own error estimate (relative, per block) stays below this on every synthetic system
FAMILIES = ("orthogonal", "scaled", "permutation")
SCALED_G = (2.0 ** -20, 1.0, 2.0 ** 10)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def weights(t):
    """Trapezoid weight of every node."""
    t = np.asarray(t, dtype=np.float64)
    w = np.zeros(t.size)
    w[:-1] += np.diff(t) / 2
    w[1:] += np.diff(t) / 2
    return w


def _matvec_ld(K, x):
    """K x in long double from K's triplets (CSR: rows in order)."""
    prod = K.data.astype(LD) * x.astype(LD)[K.indices]
    starts = K.indptr[:-1]
    nonempty = K.indptr[1:] > starts
    out = np.zeros(K.shape[0], dtype=LD)
    if prod.size:
        out[nonempty] = np.add.reduceat(prod, starts[nonempty])
    return out


class Step:
    """One update: dX [ns, n], dU [3, n], dV [6] (exact zeros without impulses), cost; p, on_bound for the free steps."""

    def __init__(self, dX, dU, dV, cost, p=None, on_bound=None):
        self.dX, self.dU, self.dV, self.cost, self.p, self.on_bound = dX, dU, dV, cost, p, on_bound


class QpSystem:
    """The KKT matrix of one trajectory (it depends on the Jacobian blocks, the grid, the impulse switch and c2 = (DU/TU)^2 only),
    factored once; then any number of right-hand sides."""

    def __init__(self, Jt, t, imp, c2, refine=3):
        Jt = np.asarray(Jt, dtype=np.float64)
        self.ns, _, self.S = Jt.shape
        ns, S = self.ns, self.S
        self.n = n = S + 1
        self.imp, self.c2, self.refine = bool(imp), float(c2), refine
        self.t = np.asarray(t, dtype=np.float64)
        self.w = weights(self.t)
        self.nz = nz = ns * n + 3 * n + 6
        self.iu, self.iv = iu, iv = ns * n, ns * n + 3 * n
        self.Q = np.r_[np.zeros(ns * n), np.repeat(self.w, 3), self.c2 * np.ones(6)]
        # defect rows: row ns i + a, columns of x_i, x_{i+1} (contiguous) and of u_i, u_{i+1} (contiguous)
        i = np.arange(S)[None, None, :]
        a = np.arange(ns)[:, None, None]
        c = np.arange(2 * ns + 6)[None, :, None]
        rows = np.broadcast_to(ns * i + a, Jt.shape)
        cols = np.broadcast_to(np.where(c < 2 * ns, ns * i + c, iu + 3 * i + c - 2 * ns), Jt.shape)
        ri, ci, vv = [rows.reshape(-1)], [cols.reshape(-1)], [Jt.reshape(-1)]
        r0 = ns * S
        self.row_pin0, self.row_pinf = r0, r0 + 6
        for k, o in ((0, 0), (n - 1, 3)):
            ri += [r0 + np.arange(6), r0 + 3 + np.arange(3)]
            ci += [ns * k + np.arange(6), iv + o + np.arange(3)]
            vv += [np.ones(6), np.ones(3)]
            r0 += 6
        if ns == 7:
            ri.append([r0]); ci.append([6]); vv.append([1.0])
            r0 += 1
        if not self.imp:
            ri.append(r0 + np.arange(6)); ci.append(iv + np.arange(6)); vv.append(np.ones(6))
            r0 += 6
        self.m = r0
        A = sp.csr_matrix((np.concatenate(vv), (np.concatenate(ri), np.concatenate(ci))), shape=(r0, nz))
        self.A = A
        self.K = sp.bmat([[sp.diags(2.0 * self.Q), A.T], [A, None]], format="csr")
        self.K.sort_indices()
        # start of the Ruiz sweeps: the scaling of the kernels (g = max |G|, |H|, w = max dt: du ~ 1 / g, multipliers ~ 2 w / g^2)
        # written symmetrically.  Every row of the unscaled matrix already has largest entry ~ 1, so sweeps started from D = 1 stay
        # there and leave a condition number ~ 1 / g^2
        gm = float(np.abs(Jt[:, 2 * ns:, :]).max())
        gm = gm if gm > 0 else 1.0
        sw = np.sqrt(2.0 * float(np.diff(self.t).max()))
        D = np.r_[np.full(ns * n, gm / sw), np.full(3 * n, 1.0 / sw), np.full(6, gm / sw), np.full(r0, sw / gm)]
        absK = abs(self.K)
        for _ in range(20):
            Ks = sp.diags(D) @ absK @ sp.diags(D)
            D = D / np.sqrt(np.maximum(Ks.max(axis=1).toarray().ravel(), 1e-300))
        self.D = np.exp2(np.round(np.log2(D)))
        self.Ks = (sp.diags(self.D) @ self.K @ sp.diags(self.D)).tocsc()
        self.lu = spla.splu(self.Ks)

    def cond1(self):
        """1-norm condition estimate of the equilibrated matrix."""
        N = self.Ks.shape[0]
        inv = spla.LinearOperator((N, N), matvec=self.lu.solve, rmatvec=lambda x: self.lu.solve(x, trans="T"))
        return float(spla.onenormest(self.Ks) * spla.onenormest(inv))

    def solve(self, rhs):
        """K sol = rhs: returns (refined [long double], plain float64 solve)."""
        rhs = np.asarray(rhs, dtype=np.float64)
        z0 = self.lu.solve(rhs * self.D) * self.D
        z = z0.astype(LD)
        for _ in range(self.refine):
            r = rhs.astype(LD) - _matvec_ld(self.K, z)
            z = z + (self.lu.solve((r * self.D).astype(np.float64)) * self.D).astype(LD)
        return z, z0

    # ---- right-hand sides
    def rhs0(self, d, X, U, s0, sf, mass, dV1, dV2):
        d, X, U = (np.asarray(v, dtype=np.float64) for v in (d, X, U))
        dV1, dV2 = np.asarray(dV1, dtype=np.float64), np.asarray(dV2, dtype=np.float64)
        q = np.r_[np.zeros(self.ns * self.n), (U * self.w[None, :]).T.reshape(-1), self.c2 * dV1, self.c2 * dV2]
        b = [-d.reshape(-1, order="F"), np.asarray(s0) - X[:6, 0] - np.r_[0.0, 0.0, 0.0, dV1],
             np.asarray(sf) - X[:6, -1] - np.r_[0.0, 0.0, 0.0, dV2]]
        if self.ns == 7:
            b.append([mass - X[6, 0]])
        if not self.imp:
            b.append(np.zeros(6))
        return np.r_[-2.0 * q, np.concatenate(b)]

    def _rhs_rows(self, row0, v):
        r = np.zeros(self.nz + self.m)
        r[self.nz + row0:self.nz + row0 + len(v)] = v
        return r

    def blocks(self, z):
        """z -> (dX [ns, n], dU [3, n], dV [6]) in float64; dV exact zeros without impulses."""
        z = np.asarray(z)
        ns, n = self.ns, self.n
        dV = z[self.iv:self.iv + 6].astype(np.float64) if self.imp else np.zeros(6)
        return z[:ns * n].reshape(n, ns).T.astype(np.float64), z[self.iu:self.iv].reshape(n, 3).T.astype(np.float64), dV

    def cost(self, z, U, dV1, dV2):
        """sum_k w_k |u_k + du_k|^2 + c2 (|dV1 + d1|^2 + |dV2 + d2|^2) in long double."""
        u = np.asarray(U, dtype=np.float64).astype(LD) + np.asarray(z)[self.iu:self.iv].astype(LD).reshape(self.n, 3).T
        dv = np.r_[dV1, dV2].astype(LD) + (np.asarray(z)[self.iv:self.iv + 6].astype(LD) if self.imp else 0)
        return np.sum(self.w.astype(LD)[None, :] * u * u) + LD(self.c2) * np.sum(dv * dv)

    def _gap(self, z, z0):
        """Largest relative 2-norm gap between the refined and the plain solve over the blocks dX, dU (and dV with impulses)."""
        a, b = self.blocks(z), self.blocks(z0)
        # a block that is pinned to zero (dX of dz/dp3 on two nodes) holds rounding only: left out, judged in the equilibrated unknowns
        y = np.asarray(z).astype(np.float64) / self.D
        ya, tiny = self.blocks(y), 1e-12 * np.linalg.norm(y[:self.nz])
        return max([rel(b[k], a[k]) for k in range(3 if self.imp else 2) if np.linalg.norm(ya[k]) > tiny] or [0.0])

    def frozen(self, d, X, U, s0, sf, mass, dV1, dV2):
        """The frozen step.  Returns (Step, err): err is the gap between the plain float64 solve and the refined one (the largest
        relative error over dX, dU, dV and the cost)."""
        z, z0 = self.solve(self.rhs0(d, X, U, s0, sf, mass, dV1, dV2))
        c, c0 = self.cost(z, U, dV1, dV2), self.cost(z0, U, dV1, dV2)
        err = max(self._gap(z, z0), float(abs(c - c0) / max(abs(c), LD(1e-300))))
        return Step(*self.blocks(z), float(c)), err

    def free(self, d, X, U, s0, sf, mass, dV1, dV2, g0, gf, c0n, cfn, beta, dtf=None, tf_bounds=None):
        """The free-end step (dtf None: p = (p1, p2)) or the free-tf step (p = (p1, p2, p3); tf_bounds = (step, tf_min, tf_max),
        tf = t[-1]).  Returns a FreeReference."""
        return FreeReference(self, d, X, U, s0, sf, mass, dV1, dV2, g0, gf, c0n, cfn, beta, dtf, tf_bounds)


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in long double (k <= 3); None when a pivot vanishes."""
    A, b = A.astype(LD).copy(), b.astype(LD).copy()
    k = len(b)
    for c in range(k):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if A[piv, c] == 0:
            return None
        A[[c, piv]], b[[c, piv]] = A[[piv, c]], b[[piv, c]]
        for r in range(c + 1, k):
            f = A[r, c] / A[c, c]
            A[r] -= f * A[c]
            b[r] -= f * b[c]
    x = np.zeros(k, dtype=LD)
    for c in range(k - 1, -1, -1):
        x[c] = (b[c] - A[c, c + 1:] @ x[c + 1:]) / A[c, c]
    return x


class FreeReference:
    """z0, dz/dp_j, the reduced quadratic and the box solution of one free step.
      p [k], on_bound [k]   the solution; a coordinate on a bound is the float64 bound value itself
      step                  Step at p (dX, dU, dV, cost with the beta term)
      err                   largest gap between the plain and the refined solves over the k + 1 right-hand sides (relative, per block)
      p_err [k]             |p of the plain float64 solves - p| / (hi - lo): the float64 host route's error in p
      ambiguous             the second-best active set's phi is within the reference's own error of the best one's: p is not
                            determined to the bar, check `optimality(p)` instead
      lo, hi [k]            the box (float64, formed as the device forms it)"""

    def __init__(self, sys_, d, X, U, s0, sf, mass, dV1, dV2, g0, gf, c0n, cfn, beta, dtf, tf_bounds):
        self.sys = s = sys_
        self.U, self.dV1, self.dV2 = np.asarray(U, dtype=np.float64), np.asarray(dV1, dtype=np.float64), np.asarray(dV2, dtype=np.float64)
        k = self.k = 2 if dtf is None else 3
        rhs = [s.rhs0(d, X, U, s0, sf, mass, dV1, dV2), s._rhs_rows(s.row_pin0, np.asarray(g0, dtype=np.float64)),
               s._rhs_rows(s.row_pinf, np.asarray(gf, dtype=np.float64))]
        if k == 3:
            rhs.append(s._rhs_rows(0, -np.asarray(dtf, dtype=np.float64).reshape(-1, order="F")))
        sols = [s.solve(r) for r in rhs]
        self.err = max(s._gap(z, z0) for z, z0 in sols)
        self.diag = np.r_[beta * c0n, beta * cfn, 0.0][:k].astype(LD)
        lo, hi = [-P_BOUND, -P_BOUND], [P_BOUND, P_BOUND]
        self.pscale = [1 / P_BOUND, 1 / P_BOUND]
        if k == 3:
            step, tf_min, tf_max = (float(v) for v in tf_bounds)
            tf = float(s.t[-1])
            lo.append(max(-step, tf_min - tf))
            hi.append(min(step, tf_max - tf))
            self.pscale.append(1 / step if step > 0 else 0.0)
        self.lo, self.hi = np.array(lo), np.array(hi)
        self.Z = [z for z, _ in sols]
        self.phi0, self.G, self.H = self._quadratic(self.Z)
        self.p, self.on_bound, best, second = self._box(self.phi0, self.G, self.H)
        phi0_, G_, H_ = self._quadratic([z0.astype(LD) for _, z0 in sols])
        p_plain, ob_plain, best_plain, _ = self._box(phi0_, G_, H_)
        self.p_err = np.abs(p_plain - self.p) / np.maximum(self.hi - self.lo, 1e-300)
        # the reference's own error in phi: the plain solves' phi against the refined one at the same p, and the rounding of phi
        self.phi_err = float(abs(self._phi(phi0_, G_, H_, self.p.astype(LD)) - best)) + 8 * np.finfo(np.float64).eps * float(abs(best))
        self.ambiguous = bool(ob_plain != self.on_bound) or (second is not None and float(second - best) <= self.phi_err)
        zp = self.Z[0] + sum(self.Z[j + 1] * LD(self.p[j]) for j in range(k))
        cost = s.cost(zp, self.U, self.dV1, self.dV2) + np.sum(self.diag * self.p.astype(LD) ** 2) / 2
        self.step = Step(*s.blocks(zp), float(cost), self.p, self.on_bound)

    def _quadratic(self, Z):
        """phi0, G [k], H [k, k] of phi(p) = cost(z0 + sum z_j p_j) + sum_j diag_j p_j^2 / 2, in long double."""
        s, k = self.sys, self.k
        Q = s.Q.astype(LD)
        U, dV = self.U, np.r_[self.dV1, self.dV2]
        q = np.r_[np.zeros(s.ns * s.n), (U * s.w[None, :]).T.reshape(-1), s.c2 * dV].astype(LD)
        if not s.imp:                                # the impulse updates are pinned to zero: their (refined) values are rounding
            Z = [np.r_[z[:s.iv], np.zeros(6, dtype=LD), z[s.iv + 6:]] for z in Z]
        zs = [z[:s.nz] for z in Z]
        g0 = Q * zs[0] + q
        G = np.array([2 * (zs[j + 1] @ g0) for j in range(k)], dtype=LD)
        H = np.array([[2 * (zs[i + 1] @ (Q * zs[j + 1])) for j in range(k)] for i in range(k)], dtype=LD) + np.diag(self.diag)
        return s.cost(Z[0], U, self.dV1, self.dV2), G, H

    @staticmethod
    def _phi(phi0, G, H, p):
        return phi0 + G @ p + (p @ (H @ p)) / 2

    def _box(self, phi0, G, H):
        """Enumerate the active sets.  Returns (p float64, on_bound tuple, phi of the best, phi of the second best DIFFERENT point
        among the sets' feasible points (free coordinates clamped into the box), or None)."""
        k = self.k
        lo, hi = self.lo.astype(LD), self.hi.astype(LD)
        accepted, others = [], []
        for order, pat in enumerate(itertools.product((0, -1, 1), repeat=k)):
            free = [j for j in range(k) if pat[j] == 0]
            p = np.array([0 if pat[j] == 0 else (lo[j] if pat[j] < 0 else hi[j]) for j in range(k)], dtype=LD)
            if free:
                x = _solve_ld(H[np.ix_(free, free)], -(G[free] + H[np.ix_(free, range(k))] @ p))
                if x is None or not np.all(np.isfinite(x.astype(np.float64))):
                    continue
                p[free] = x
            inside = all(lo[j] <= p[j] <= hi[j] for j in free)
            g = G + H @ p
            signs = all((g[j] >= 0) if pat[j] < 0 else (g[j] <= 0) for j in range(k) if pat[j])
            pc = np.minimum(np.maximum(p, lo), hi)
            # a free coordinate that lands on a bound is that bound (the device clamps its edge minimisers)
            on = tuple(int(pat[j]) if pat[j] else (-1 if pc[j] == lo[j] else 1 if pc[j] == hi[j] else 0) for j in range(k))
            f = self._phi(phi0, G, H, pc)
            m = max(float(abs(pc[j])) * self.pscale[j] for j in range(k))
            (accepted if inside and signs else others).append((f, m, order, pc, on))
        if not accepted:
            raise np.linalg.LinAlgError("qp_reference: no active set satisfies the optimality conditions")
        accepted.sort(key=lambda c: c[:3])
        f, _, _, pc, on = accepted[0]
        p64 = np.array([(self.lo[j] if on[j] < 0 else self.hi[j]) if on[j] else float(pc[j]) for j in range(k)])
        rest = [c[0] for c in accepted[1:] + others if c[4] != on]
        return p64, on, f, (min(rest) if rest else None)

    def gradient(self, p):
        """The reduced gradient G + H p at any p (float64)."""
        return (self.G + self.H @ np.asarray(p, dtype=np.float64).astype(LD)).astype(np.float64)

    def optimality(self, p, tol=1e-9):
        """Largest violation of the optimality conditions of the box problem at p, in units of the gradient change that moving p
        by tol of the box width causes (sum_i |H_ji| tol (hi_i - lo_i)): <= 1 means p is optimal to `tol` of the box.  p outside the
        box: inf."""
        p = np.asarray(p, dtype=np.float64)
        if np.any(p < self.lo) or np.any(p > self.hi):
            return np.inf
        g = self.gradient(p)
        unit = np.abs(self.H.astype(np.float64)) @ (tol * (self.hi - self.lo)) + 1e-300
        worst = 0.0
        for j in range(self.k):
            if p[j] == self.lo[j] and p[j] == self.hi[j]:
                continue
            v = -g[j] if p[j] == self.lo[j] else g[j] if p[j] == self.hi[j] else abs(g[j])
            worst = max(worst, v / unit[j])
        return worst


# ---- synthetic systems of the frozen step
def _haar(ns, rng):
    q, r = np.linalg.qr(rng.standard_normal((ns, ns)))
    return q * np.sign(np.diag(r))[None, :]


def _draw(family, ns, S, rng, g):
    n = S + 1
    Jt = np.zeros((ns, 2 * ns + 6, S), order="F")
    Jt[:, ns:2 * ns, :] = -np.eye(ns)[:, :, None]
    if family == "permutation":
        for i in range(S):
            Jt[rng.permutation(ns), np.arange(ns), i] = rng.choice([-1.0, 1.0], size=ns)
            Jt[rng.permutation(ns)[:6], 2 * ns + np.arange(6), i] = rng.choice([-1.0, 1.0], size=6)   # six different rows
        ints = lambda *shape: rng.integers(-3, 4, size=shape).astype(np.float64)      # noqa: E731
        d, X, U = ints(ns, S), ints(ns, n), ints(3, n)
        t = np.concatenate([[0.0], np.cumsum(rng.choice([0.5, 1.0, 2.0], size=S))])
        tgt = (X[:6, 0] + ints(6), X[:6, -1] + ints(6), (X[6, 0] if ns == 7 else 0.0) + 2.0, ints(3), ints(3))
        return Jt, d, X, U, t, tgt
    for i in range(S):
        Jt[:, :ns, i] = _haar(ns, rng)
    Jt[:, 2 * ns:, :] = g * rng.standard_normal((ns, 6, S))
    if family == "scaled":                      # segment lengths spread over a factor 1e3 within the grid, both ends reached
        e = rng.uniform(-3.0, 0.0, size=S)
        e[rng.integers(0, S)] = 0.0
        if S > 1:
            e[(int(np.argmax(e)) + 1 + rng.integers(0, S - 1)) % S] = -3.0
        dt = g * g * 10.0 ** e
    else:
        dt = rng.uniform(0.05, 0.2, size=S)
    t = np.concatenate([[0.0], np.cumsum(dt)])
    d, X, U = rng.standard_normal((ns, S)), rng.standard_normal((ns, n)), rng.standard_normal((3, n)) / g
    tgt = (X[:6, 0] + 0.1 * rng.standard_normal(6), X[:6, -1] + 0.1 * rng.standard_normal(6),
           (X[6, 0] if ns == 7 else 0.0) + 0.5, 0.1 * rng.standard_normal(3), 0.1 * rng.standard_normal(3))
    return Jt, d, X, U, t, tgt


class Synthetic:
    """One synthetic frozen system: Jt [ns, 2 ns + 6, S], d [ns, S], X [ns, n], U [3, n], t [n], targets (s0, sf, mass, dV1, dV2),
    its factored QpSystem (`sys`), the condition estimate and the number of draws it took."""


def synthetic(family, ns, S, seed, imp, c2=1.0, g=1.0):
    """Blocks [E | F | G | H] of one trajectory with a matching grid:
      orthogonal    E Haar-random orthogonal, F = -I, G and H standard normal, dt uniform in [0.05, 0.2];
      scaled        as orthogonal with G, H multiplied by g (SCALED_G: 2^-20, 1, 2^10) and segment lengths g^2 10^e, e in [-3, 0]
                    with both ends reached within the grid; U is divided by g.  du is then ~ 1 / g and the control cost
                    w |u|^2 stays comparable to the impulse cost at every g (with dt ~ 1 the impulses would be cheaper by g^2 and
                    the KKT matrix ill conditioned).  The power-of-two scale factors of qp_scale differ by many binades
                    between trajectories of one batch;
      permutation   E a signed permutation, F = -I, G and H exactly one +-1 per column (in six different rows), dt in {1/2, 1, 2}, small-integer defects,
                    states, controls and targets: exact zeros below the diagonal, the trivial-reflection branch of qp_householder.
    Drawn again with seed + 7919 k until the condition estimate of the equilibrated KKT matrix is <= COND_BOUND."""
    for k in range(200):
        rng = np.random.default_rng(seed + 7919 * k)
        Jt, d, X, U, t, tgt = _draw(family, ns, S, rng, g if family == "scaled" else 1.0)
        try:
            qs = QpSystem(Jt, t, imp, c2)
            cond = qs.cond1()
        except RuntimeError:                    # splu: exactly singular (a permutation system whose controls miss a state)
            continue
        if np.isfinite(cond) and cond <= COND_BOUND:
            out = Synthetic()
            out.family, out.Jt, out.d, out.X, out.U, out.t, out.targets, out.sys, out.cond, out.draws = family, Jt, d, X, U, t, tgt, qs, cond, k + 1
            return out
    raise RuntimeError("no well-conditioned %s system at ns=%d S=%d imp=%s" % (family, ns, S, imp))
