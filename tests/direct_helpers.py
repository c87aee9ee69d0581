"""Helpers the direct-method tests share: the halo orbit tables, the relative error, the halo demo module and a CPU back end of
the direct loop on the oracle's sweeps (test infrastructure)."""
import importlib.util
import os

import numpy as np

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISP = 2000.0


def tables():
    tabs = synth.halo_orbits()
    return np.linspace(0, 1, tabs[0].shape[1]), tabs[0], np.linspace(0, 1, tabs[1].shape[1]), tabs[1]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def demo():
    spec = importlib.util.spec_from_file_location("halo_direct_demo", os.path.join(ROOT, "examples", "halo_direct_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dtf(X, U, t):
    """The tf column from the oracle: d defect_i / d h_i times h_i / (tf - t0) (every segment length scales with tf - t0)."""
    Jt, dh, d = O.direct_jacobian_dual(X, U, t, 10, lto.MU, lto.DU, lto.TU, ISP)
    return Jt, dh * (np.diff(t) / (t[-1] - t[0]))[None, :], d


class OracleDirectOps:
    """CPU back end of the direct loop: the oracle's sweeps, with the tf column (jacobian_tf) at Isp = ISP and 10 steps."""

    def __init__(self, Isp=ISP):
        self.Isp = Isp

    def defect(self, X, U, t, nsteps):
        return O.direct_defect(X, U, t, nsteps, lto.MU, lto.DU, lto.TU, self.Isp)

    def jacobian(self, X, U, t, nsteps):
        Jt, _, d = O.direct_jacobian_dual(X, U, t, nsteps, lto.MU, lto.DU, lto.TU, self.Isp)
        return Jt, d

    def jacobian_tf(self, X, U, t, nsteps):
        return dtf(X, U, t)

    def defect_batch_sumsq(self, Xb, Ub, t, nsteps):
        return np.array([np.sum(self.defect(Xb[:, :, k], Ub[:, :, k], t, nsteps)[0] ** 2) for k in range(Xb.shape[2])])
