"""The host reference of the block-bidiagonal Newton system (bvp_reference.py) that the device shape sweep is checked against:
agreement with dense solve / lstsq at small S in all four variants, the synthetic Phi generators, and the pinned-column masks
against the library's scatter."""
import numpy as np
import pytest

import bvp_reference as R

SIZES = [1, 2, 15, 16, 17, 31, 33, 40]


@pytest.mark.parametrize("family", sorted(R.GENERATORS))
@pytest.mark.parametrize("nd,adjoints_only", R.VARIANTS)
def test_refined_solution_matches_dense(nd, adjoints_only, family):
    for S in SIZES:
        Phi, d = R.GENERATORS[family](nd, S, 100 + S, adjoints_only)
        ref = R.BvpReference(Phi, adjoints_only)
        Jf = R.dense_free(Phi, adjoints_only)
        # the refined solution of two right-hand sides (as the factor solve and the re-solve use it)
        for dd in (d, 0.5 * d + 0.01):
            x, err = ref.solve(dd)
            b = -dd.reshape(-1, order="F")
            xd = np.linalg.lstsq(Jf, b, rcond=None)[0] if adjoints_only else np.linalg.solve(Jf, b)
            xv = x.reshape(-1, order="F")
            scale = max(1.0, np.abs(xd).max())
            assert np.abs(xv[ref.free_flat] - xd).max() < 1e-13 * scale, (S, family)
            assert np.all(xv[~ref.free_flat] == 0.0)
            assert err < 1e-12 * scale
            # its long-double residual (square) / normal equations (least squares) is at round-off
            assert ref.backward_error(x, dd) < 1e-14 * max(1.0, np.abs(b).max()) * scale


@pytest.mark.parametrize("nd,adjoints_only", R.VARIANTS)
def test_generators(nd, adjoints_only):
    for S in (1, 2, 17, 40):
        Phi, d = R.random_orthogonal_blocks(nd, S, 7 + S, adjoints_only)
        assert Phi.shape == (nd, nd, S) and d.shape == (nd, S)
        for i in range(S):
            assert np.abs(Phi[:, :, i].T @ Phi[:, :, i] - np.eye(nd)).max() < 1e-14
        Phi2, d2 = R.random_orthogonal_blocks(nd, S, 7 + S, adjoints_only)
        assert np.array_equal(Phi, Phi2) and np.array_equal(d, d2)          # seeded
        P, dp = R.signed_permutation_blocks(nd, S, 7 + S, adjoints_only)
        for i in range(S):
            B = P[:, :, i]
            assert set(np.unique(B)) <= {-1.0, 0.0, 1.0}
            assert np.all(np.abs(B).sum(axis=0) == 1) and np.all(np.abs(B).sum(axis=1) == 1)
        assert np.all(dp == np.round(dp)) and np.abs(dp).max() <= 3
        # the free matrices have full column rank, sigma_min above a floor (square systems: ~1/S, the chain of S blocks)
        for blocks in (Phi, P):
            sv = np.linalg.svd(R.dense_free(blocks, adjoints_only), compute_uv=False)
            floor = 0.1 if adjoints_only else 0.1 / S
            assert sv.min() > floor, (S, sv.min())
    # square variants: the boundary block of the product (pinned rows of the last node x free columns of the first node)
    if not adjoints_only:
        rows, cols = R._boundary_rows_cols(nd, False)
        for gen in R.GENERATORS.values():
            Phi, _ = gen(nd, 300, 3, False)
            prod = np.eye(nd)
            for i in range(300):
                prod = Phi[:, :, i] @ prod
            assert np.linalg.svd(prod[np.ix_(rows, cols)], compute_uv=False).min() >= R.SIGMA_FLOOR - 1e-9


@pytest.mark.parametrize("nd", [12, 14])
def test_pinned_masks_are_the_scatters_zero_columns(nd):
    for S in (1, 5):
        Phi, _ = R.random_orthogonal_blocks(nd, S, 11)
        J = R.scatter(Phi).toarray()
        zero_cols = ~np.any(J != 0.0, axis=0)
        assert np.array_equal(zero_cols, R.pinned_mask(nd, S + 1).reshape(-1, order="F"))
        n = S + 1
        expect = np.zeros((nd, n), bool)
        expect[:6, 0] = expect[:6, -1] = True
        if nd == 14:
            expect[6, 0] = expect[13, -1] = True
        assert np.array_equal(R.pinned_mask(nd, n), expect)
        # adjoints-only drops every state column as well: 6 (12-dim) or 7 (14-dim) costates per node, the last node's lambda_m pinned
        fa = R.free_mask(nd, n, True)
        assert not fa[:nd // 2].any()
        assert fa.sum() == (nd // 2) * n - (1 if nd == 14 else 0)
        assert fa.sum(axis=0)[-1] == 6 and fa.sum(axis=0)[0] == nd // 2
