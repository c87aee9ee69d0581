"""CPU: the product's device formulas (lowthrustopt_amd/csrc/dynamics.hpp) compiled for the host with a stub
hip_runtime.h and checked against the oracle: RHS values, F * column against the dual-number / finite-difference
Jacobian, explicit vs fused single-column path, 12- and 14-dim, every control-law mode."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PM_P0, PM_P1, PM_P2, PM_PGEN = 0, 1, 2, 3     # dynamics.hpp PMode: one compiled control law per class


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostchk") / "libdynchk.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_stub"),
                           "-I", os.path.join(ROOT, "lowthrustopt_amd", "csrc"), "-o", out,
                           os.path.join(HERE, "host_stub", "dynamics_check.cpp")])
    return C.CDLL(out)


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def tp_vec(ndim, thr, mass_or_isp, td, p, rho):
    """TrajParams exactly as lto_indirect_plan.hip::make_traj_params fills it."""
    aL = thr / mass_or_isp / 1e3 * (TU * TU) / DU if ndim == 12 else 0.0
    cT = thr / 1e3 * (TU * TU) / DU
    kt = td * 1e3 * DU / (TU * mass_or_isp * 9.81) if ndim == 14 else 0.0
    return np.array([aL, 1 / (2 * rho), 1 / rho, p, (1 / p if p != 0 else 0.0), (1 / (p - 1) if p > 1 else 0.0), td, MU, cT, kt])


CASES = [(1.0, 1.0, 0.05, 0.1, PM_P1), (1.0, 1e-2, 0.05, 1.0, PM_P1), (1.0, 1e-4, 10.0, 1.0, PM_P1), (2.0, 1.0, 10.0, 0.1, PM_P2),
         (2.0, 1.0, 0.05, 1.0, PM_P2), (1.5, 1.0, 10.0, 0.3, PM_PGEN), (0.0, 1.0, 0.05, 0.1, PM_P0),
         (0.0, 1.0, 10.0, 1.0, PM_P0), (3.0, 1.0, 10.0, 0.1, PM_PGEN), (1.2, 0.5, 0.001, 0.5, PM_PGEN)]


@pytest.mark.parametrize("td", [1.0, -1.0])
def test_device_formulas_12(chk, oracle, td):
    assert chk.chk_sizeof_tp() == 80
    rng = np.random.default_rng(0)
    H1 = synth.halo_orbits()[0]
    for p, rho, thr, lam, pm in CASES:
        y = np.concatenate([H1[:, rng.integers(0, 99)], lam * rng.standard_normal(6)])
        prm = [MU, DU, TU, thr, 1000.0, td, p, rho]
        tp = tp_vec(12, thr, 1000.0, td, p, rho)
        col = rng.standard_normal(12)
        d = np.zeros(12); dc = np.zeros(12); df = np.zeros(12); dcf = np.zeros(12)
        chk.chk_rhs12(P(y), P(tp), pm, P(d), P(col), P(dc), P(df), P(dcf))
        ref = oracle.rhs_state_costate(y, prm)
        J = oracle.rhs_state_costate_jac(y, prm)
        sc = max(1.0, np.abs(ref).max())
        assert np.abs(d - ref).max() < 5e-14 * sc and np.abs(df - ref).max() < 5e-14 * sc
        Jc = J @ col
        scj = max(1.0, np.abs(J).max() * np.abs(col).max())
        assert np.abs(dc - Jc).max() < 1e-12 * scj and np.abs(dcf - Jc).max() < 1e-12 * scj


def test_device_formulas_14(chk, oracle):
    rng = np.random.default_rng(1)
    H1 = synth.halo_orbits()[0]
    for p, rho, thr, lam, pm in CASES:
        y = np.concatenate([H1[:, rng.integers(0, 99)], [990.0], lam * rng.standard_normal(6), [0.3]])
        prm = [MU, DU, TU, thr, 2000.0, 1.0, p, rho]
        tp = tp_vec(14, thr, 2000.0, 1.0, p, rho)
        col = rng.standard_normal(14)
        d = np.zeros(14); dc = np.zeros(14); df = np.zeros(14); dcf = np.zeros(14)
        chk.chk_rhs14(P(y), P(tp), pm, P(d), P(col), P(dc), P(df), P(dcf))
        ref = oracle.rhs_state_costate_mass(y, prm)
        assert np.abs(d - ref).max() < 5e-14 * max(1.0, np.abs(ref).max())
        # fused base + one column (the COLS = 1 kernel of the BASELINE configs[1] sweep) == the general path
        assert np.abs(df - d).max() < 5e-14 * max(1.0, np.abs(ref).max())
        assert np.abs(dcf - dc).max() < 1e-12 * max(1.0, np.abs(dc).max())
        J = np.zeros((14, 14))
        for c in range(14):          # central differences of the oracle RHS (FD noise ~1e-9 relative)
            h = 1e-6 * max(1.0, abs(y[c]))
            yp = y.copy(); yp[c] += h
            ym = y.copy(); ym[c] -= h
            J[:, c] = (oracle.rhs_state_costate_mass(yp, prm) - oracle.rhs_state_costate_mass(ym, prm)) / (yp[c] - ym[c])
        Jc = J @ col
        assert np.abs(dc - Jc).max() < 2e-8 * max(1.0, np.abs(J).max() * np.abs(col).max())


@pytest.mark.parametrize("ndim", [12, 14])
def test_lean_base_rhs_of_the_pipeline_kernel(chk, ndim):
    """rhs*_base (the pipeline kernel's base wave: dyadic G lambda_v, short-depth exp, no variational by-products) gives
    the slopes of the one-piece rhs* used by the other kernel families."""
    rng = np.random.default_rng(2)
    H1 = synth.halo_orbits()[0]
    for td in (1.0, -1.0):
        for p, rho, thr, lam, pm in CASES:
            if ndim == 12:
                y = np.concatenate([H1[:, rng.integers(0, 99)], lam * rng.standard_normal(6)])
                tp = tp_vec(12, thr, 1000.0, td, p, rho)
            else:
                y = np.concatenate([H1[:, rng.integers(0, 99)], [990.0], lam * rng.standard_normal(6), [0.3]])
                tp = tp_vec(14, thr, 2000.0, td, p, rho)
            da = np.zeros(ndim); db = np.zeros(ndim)
            chk.chk_base(ndim, P(y), P(tp), pm, P(da), P(db))
            assert np.all(np.isfinite(db))
            assert np.abs(da - db).max() <= 5e-14 * max(1.0, np.abs(da).max())


def test_by_products_path_of_the_cooperative_kernel(chk):
    """rhs12_base_parts (base lane: lean RHS + by-products c_b, 1/d_b, ua, ub, 1/n) and coef12_from_parts (column lanes:
    G, H, U rebuilt from them without reciprocal square roots or the control law) give the slopes and the 17 variational
    coefficients of the one-piece rhs12<PM, true>, for every control-law class, both time directions, rho down to 1e-4."""
    rng = np.random.default_rng(4)
    H1 = synth.halo_orbits()[0]
    for td in (1.0, -1.0):
        for p, rho, thr, lam, pm in CASES:
            y = np.concatenate([H1[:, rng.integers(0, 99)], lam * rng.standard_normal(6)])
            tp = tp_vec(12, thr, 1000.0, td, p, rho)
            da = np.zeros(12); db = np.zeros(12); va = np.zeros(17); vb = np.zeros(17)
            chk.chk_parts12(P(y), P(tp), pm, P(da), P(va), P(db), P(vb))
            assert np.all(np.isfinite(vb)) and np.all(np.isfinite(db))
            assert np.abs(da - db).max() <= 5e-14 * max(1.0, np.abs(da).max())
            assert np.abs(va - vb).max() <= 1e-13 * max(1.0, np.abs(va).max())


def test_two_lanes_per_state_forms_of_the_cooperative_kernel(chk):
    """rhs12_base_half evaluated as lane A (r, v) and as lane B (lambda_v, lambda_r) assembles the slopes of the one-piece
    rhs12 with the same by-products in both lanes, and var_col12_top / var_col12_bottom (fed the other half's first triple)
    assemble F * column of var_col12 -- every control-law class, both time directions, rho down to 1e-4."""
    rng = np.random.default_rng(6)
    H1 = synth.halo_orbits()[0]
    for td in (1.0, -1.0):
        for p, rho, thr, lam, pm in CASES:
            y = np.concatenate([H1[:, rng.integers(0, 99)], lam * rng.standard_normal(6)])
            col = rng.standard_normal(12)
            tp = tp_vec(12, thr, 1000.0, td, p, rho)
            da = np.zeros(12); ca = np.zeros(12); db = np.zeros(12); cb = np.zeros(12); parts = np.zeros(14)
            chk.chk_halves12(P(y), P(col), P(tp), pm, P(da), P(ca), P(db), P(cb), P(parts))
            assert np.all(np.isfinite(db)) and np.all(np.isfinite(cb))
            assert np.array_equal(parts[:7], parts[7:])                  # both lanes publish the same by-products
            assert np.abs(da - db).max() <= 5e-14 * max(1.0, np.abs(da).max())
            assert np.abs(ca - cb).max() <= 1e-13 * max(1.0, np.abs(ca).max())
