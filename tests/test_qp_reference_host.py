"""CPU: the host reference of the direct method's QP step (qp_reference.py) against the dense host routes of drivers.py on oracle
Jacobians, its synthetic generators at every size of the device sweep, the two-node case, and the caps the device sweep of the free
steps relies on (test_direct_qp_shapes_gpu.py), checked here with oracle blocks.

N2_FINDING.  n = 2 (one segment): both nodes are pinned, so the step has to close the one defect with the two controls (and the
impulses).  Without impulses the host KKT system is square in the constraints: ns = 6 has six defect rows against the six control
unknowns, ns = 7 seven against six controls and the free final mass.  On the oracle's blocks of synth.direct_problem(2) the
equilibrated KKT matrix has 1-norm condition estimates (printed by test_two_nodes)
    ns = 6: 2e+03 .. 4e+03 without impulses, 1e+02 .. 2e+02 with;      ns = 7: 3e+06 .. 5e+06 without impulses, 1e+04 with,
smallest / largest |diagonal of R| of its QR 1.8e-02, 6.2e-02, 8.3e-05 and 6.9e-03 at the least: far above the kernel's 1e-13, so n = 2 is a
SOLVABLE case of the sweep for both ns and both impulse settings (the controls reach the state through G, H ~ dt, dt^2 / 2)."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers

import direct_helpers as DH
import qp_reference as QR
from test_direct_qp_shapes_gpu import SIZES, BATCHES, BATCH_MIX, free_problems, free_reference, free_sizes

C2 = (lto.DU / lto.TU) ** 2
DENSE_BAR = 1e-9            # the dense route against the refined reference: the bar the direct-method tests hold the device to


def _oracle_blocks(X, U, T, b):
    Jt, dtf, d = DH.dtf(X[..., b], U[..., b], T[:, b])
    return Jt, dtf, d


@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("n", [3, 17, 30])
def test_frozen_reference_matches_dense_route(ns, imp, n):
    X, U, T, tg, em, tb, betas, host = free_problems("free", n, ns, n + ns)
    for b in (0, 3):
        Jt, _, d = _oracle_blocks(X, U, T, b)
        (s0, sf, *_), mass, dV1, dV2, _ = host[b]
        hx, hu, h1, h2, hc = drivers.direct_qp_dense(Jt, d, X[..., b], U[..., b], T[:, b], s0, sf, mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
        ref, err = QR.QpSystem(Jt, T[:, b], imp, C2).frozen(d, X[..., b], U[..., b], s0, sf, mass, dV1, dV2)
        gaps = [QR.rel(hx, ref.dX), QR.rel(hu, ref.dU), abs(hc - ref.cost) / abs(ref.cost)] + ([QR.rel(np.r_[h1, h2], ref.dV)] if imp else [])
        print("\nfrozen n=%d ns=%d imp=%d b=%d: dense - reference %.2e, reference's own error %.2e" % (n, ns, imp, b, max(gaps), err))
        assert err < QR.ERR_FLOOR and max(gaps) <= DENSE_BAR
        if not imp:
            assert np.all(ref.dV == 0)


@pytest.mark.parametrize("variant", ["free", "free_tf"])
@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("n", [3, 17, 30])
def test_free_reference_matches_dense_route(variant, ns, imp, n):
    """All five beta / bound settings: the same active set with identical bound values, p and the update within the dense route's
    own error."""
    X, U, T, tg, em, tb, betas, host = free_problems(variant, n, ns, n + ns)
    for b in range(5):
        Jt, dtf, d = _oracle_blocks(X, U, T, b)
        model, mass, dV1, dV2, tfb = host[b]
        if variant == "free":
            hx, hu, h1, h2, *hp, hc = drivers.direct_qp_dense_free(Jt, d, X[..., b], U[..., b], T[:, b], *model, betas[b], mass, dV1, dV2,
                                                                   lto.DU, lto.TU, allowImpulsive=imp)
        else:
            hx, hu, h1, h2, *hp, hc = drivers.direct_qp_dense_free_tf(Jt, dtf, d, X[..., b], U[..., b], T[:, b], *model, betas[b], mass, dV1,
                                                                      dV2, lto.DU, lto.TU, T[-1, b], tfb, allowImpulsive=imp)
        ref = free_reference(variant, Jt, dtf, d, X[..., b], U[..., b], T[:, b], imp, host[b] + (betas[b],))
        hp = np.array(hp)
        half = np.maximum((ref.hi - ref.lo) / 2, 1e-300)
        print("\n%s n=%d ns=%d imp=%d b=%d: p %s dense %s on_bound %s ambiguous %d err %.2e" % (variant, n, ns, imp, b, ref.p, hp, ref.on_bound,
                                                                                           ref.ambiguous, ref.err))
        assert ref.err < QR.ERR_FLOOR
        assert ref.optimality(ref.p) <= 1.0
        if ref.ambiguous:
            assert ref.optimality(hp) <= 1.0
            continue
        for j in range(len(hp)):
            if ref.on_bound[j]:
                assert hp[j] == ref.p[j] == (ref.lo[j] if ref.on_bound[j] < 0 else ref.hi[j])
            else:
                assert ref.lo[j] < hp[j] < ref.hi[j] or ref.lo[j] == ref.hi[j]
        assert (np.abs(hp - ref.p) / half).max() <= DENSE_BAR
        st = ref.step
        assert QR.rel(hx, st.dX) <= DENSE_BAR and QR.rel(hu, st.dU) <= DENSE_BAR and abs(hc - st.cost) <= DENSE_BAR * abs(st.cost)
        if imp:
            assert QR.rel(np.r_[h1, h2], st.dV) <= DENSE_BAR
        else:
            assert np.all(st.dV == 0)


@pytest.mark.parametrize("S", SIZES)
def test_generators_are_well_conditioned_at_every_size(S):
    """Every family (the scaled one at its three magnitudes), ns 6 and 7, impulses on and off: the condition bound holds (by
    construction: `synthetic` re-draws) and the reference's own error estimate is below ERR_FLOOR."""
    worst = {}
    for f, family in enumerate(QR.FAMILIES):
        for g in (QR.SCALED_G if family == "scaled" else (1.0,)):
            for ns in (6, 7):
                for imp in (False, True):
                    s = QR.synthetic(family, ns, S, 1000 * S + 10 * ns + 2 * imp + f, imp, g=g)
                    ref, err = s.sys.frozen(s.d, s.X, s.U, *s.targets)
                    assert s.cond <= QR.COND_BOUND and err < QR.ERR_FLOOR, (family, g, ns, imp, s.cond, err)
                    w = worst.get(family, (0.0, 0.0, 0))
                    worst[family] = (max(w[0], s.cond), max(w[1], err), max(w[2], s.draws))
                    if family == "permutation":      # integers in, and the structure the family is for
                        E, GH = s.Jt[:, :ns], s.Jt[:, 2 * ns:]
                        assert np.all(np.abs(E).sum(axis=0) == 1) and np.all(np.abs(E).sum(axis=1) == 1) and np.all(np.abs(GH).sum(axis=0) == 1)
                        assert np.all(s.d == np.round(s.d))
                    if family == "scaled":
                        dt = np.diff(s.t)
                        assert S == 1 or dt.max() / dt.min() >= 999.0
    print("\nqp generators S=%d: %s" % (S, {k: "cond %.1e err %.1e draws %d" % v for k, v in worst.items()}))


def test_batch_mix_systems_exist():
    for S, B in BATCHES:
        for ns in (6, 7):
            for imp in (False, True):
                for b, (f, g) in enumerate(BATCH_MIX[:B]):
                    assert QR.synthetic(f, ns, S, 77 + 13 * b + ns + imp, imp, g=g).cond <= QR.COND_BOUND


def test_two_nodes():
    """N2_FINDING of the module docstring: n = 2 on oracle blocks is well conditioned for both ns and both impulse settings."""
    for ns in (6, 7):
        X, U, T, tg, em, tb, betas, host = free_problems("free_tf", 2, ns, 2 + ns)
        for imp in (False, True):
            for b in range(5):
                Jt, dtf, d = _oracle_blocks(X, U, T, b)
                qs = QR.QpSystem(Jt, T[:, b], imp, C2)
                r = np.abs(np.diag(np.linalg.qr(qs.Ks.toarray(), mode="r")))
                print("\nn=2 ns=%d imp=%d b=%d: cond1 %.1e, min/max |diag R| %.1e" % (ns, imp, b, qs.cond1(), r.min() / r.max()), end="")
                assert r.min() > 1e-9 * r.max() and qs.cond1() < 1e8
                for variant in ("free", "free_tf"):
                    ref = free_reference(variant, Jt, dtf, d, X[..., b], U[..., b], T[:, b], imp, host[b] + (betas[b],))
                    assert ref.err < QR.ERR_FLOOR and ref.optimality(ref.p) <= 1.0


_ORACLE_SWEEP = {}      # (variant, S) -> [cases, optimality-only cases, active bounds per coordinate]


def _oracle_case(S):
    """One size of the device test's free sweep on oracle blocks, both variants (done once per run)."""
    if ("free", S) not in _ORACLE_SWEEP:
        n = S + 1
        for ns in (6, 7):
            prob = {v: free_problems(v, n, ns, n + ns) for v in ("free", "free_tf")}
            X, U, T = prob["free"][:3]
            blocks = [_oracle_blocks(X, U, T, b) for b in range(5)]
            for variant in ("free", "free_tf"):
                _, _, _, tg, em, tb, betas, host = prob[variant]
                for imp in (False, True):
                    for b in range(5):
                        Jt, dtf, d = blocks[b]
                        ref = free_reference(variant, Jt, dtf, d, X[..., b], U[..., b], T[:, b], imp, host[b] + (betas[b],))
                        c = _ORACLE_SWEEP.setdefault((variant, S), [0, 0, np.zeros(3, dtype=int)])
                        c[0] += 1
                        c[1] += int(ref.ambiguous)
                        if not ref.ambiguous:
                            c[2][:len(ref.p)] += np.abs(np.array(ref.on_bound))
    return [_ORACLE_SWEEP[v, S] for v in ("free", "free_tf")]


@pytest.mark.parametrize("S", free_sizes())
def test_free_sweep_size_on_oracle_blocks(S):
    """Every (variant, n): at least one trajectory that the device test compares directly."""
    assert all(c[1] < c[0] for c in _oracle_case(S))


def test_free_sweep_caps_hold_on_oracle_blocks():
    for S in free_sizes():
        _oracle_case(S)
    cases = sum(c[0] for c in _ORACLE_SWEEP.values())
    only = sum(c[1] for c in _ORACLE_SWEEP.values())
    active = sum(c[2] for c in _ORACLE_SWEEP.values())
    print("\nfree sweep on oracle blocks: %d cases, %d by the optimality conditions only, active bounds %s" % (cases, only, active))
    assert 10 * only <= cases                                        # at most one case in ten
    assert np.all(active > 0)                                        # p1, p2 and p3 each on a bound somewhere
