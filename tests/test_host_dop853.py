"""CPU: the product's adaptive DOP853 lane driver (lowthrustopt_amd/csrc/dop853_lane.hpp) compiled for the host with the stub
hip_runtime.h: one ballistic CRTBP flight against scipy's DOP853, the hooked form against the plain one, and the ways a flight
ends without a result (span, max_steps, NaN)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.integrate import solve_ivp

from lowthrustopt_amd.constants import MU

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
Y0 = np.array([1.12, 0.0, 0.03, 0.0, 0.18, 0.0])
SPAN, TOL = 3.0, 1e-13
NACC, NREJ = 37, 1          # what run_dop853 took for this flight before the drivers became one body
MAX_REC = 64


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostdop") / "libdopchk.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-attributes", "-I", os.path.join(HERE, "host_stub"),
                           "-I", os.path.join(ROOT, "lowthrustopt_amd", "csrc"), "-o", out,
                           os.path.join(HERE, "host_stub", "dop853_check.cpp")])
    lib = C.CDLL(out)
    lib.chk_dop853_plain.restype = C.c_double
    lib.chk_dop853_hooked.restype = C.c_double
    return lib


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def plain(chk, y0=Y0, span=SPAN, max_steps=100000):
    y = np.zeros(6)
    cnt = (C.c_long * 4)()
    ret = chk.chk_dop853_plain(P(np.ascontiguousarray(y0)), C.c_double(MU), C.c_double(span), C.c_double(TOL), max_steps, P(y), cnt)
    return ret, y, list(cnt)[:3]


def hooked(chk, stop_at=0, y0=Y0, span=SPAN, max_steps=100000):
    y = np.zeros(6)
    cnt = (C.c_long * 4)()
    rec = np.full((MAX_REC, 14), np.nan)
    ret = chk.chk_dop853_hooked(P(np.ascontiguousarray(y0)), C.c_double(MU), C.c_double(span), C.c_double(TOL), max_steps, stop_at,
                                P(y), cnt, P(rec), MAX_REC)
    return ret, y, list(cnt), rec


def crtbp(t, y):
    x, yy, z, vx, vy, vz = y
    r1 = ((x + MU) ** 2 + yy * yy + z * z) ** 1.5
    r2 = ((x + MU - 1) ** 2 + yy * yy + z * z) ** 1.5
    return [vx, vy, vz, x + 2 * vy - (1 - MU) * (x + MU) / r1 - MU * (x + MU - 1) / r2,
            yy - 2 * vx - (1 - MU) * yy / r1 - MU * yy / r2, -(1 - MU) * z / r1 - MU * z / r2]


def test_against_scipy(chk):
    """The driver as it was before the unification, built the same way, is within 1.27e-14 (max abs over the six components) of
    scipy's DOP853 at the same tolerances, in 37 accepted and 1 rejected steps: the bound is ten times that."""
    ref = solve_ivp(crtbp, (0.0, SPAN), Y0, method="DOP853", rtol=TOL, atol=TOL).y[:, -1]
    ret, y, (nacc, nrej, calls) = plain(chk)
    err = np.abs(y - ref).max()
    print("max abs difference to scipy", err, "steps", nacc, nrej)
    assert ret == 1.0
    assert err < 1.3e-13
    assert (nacc, nrej) == (NACC, NREJ)


def test_noop_hook_equals_no_hook(chk):
    ret0, y0, (nacc0, nrej0, calls0) = plain(chk)
    ret, y, (nacc, nrej, calls, hooks), rec = hooked(chk)
    assert ret == ret0 == 1.0
    assert y.tobytes() == y0.tobytes()
    assert (nacc, nrej, calls) == (nacc0, nrej0, calls0)
    assert hooks == nacc                                        # once per accepted step
    assert rec[0, 2:8].tobytes() == Y0.tobytes()
    for k in range(1, hooks):                                   # call k starts where call k - 1 ended
        assert rec[k, 2:8].tobytes() == rec[k - 1, 8:14].tobytes()
        assert rec[k, 0] == rec[k - 1, 0] + rec[k - 1, 1]
    assert rec[hooks - 1, 8:14].tobytes() == y.tobytes()
    assert rec[hooks - 1, 0] + rec[hooks - 1, 1] >= SPAN        # the last step reaches the span
    assert rec[hooks - 2, 0] + rec[hooks - 2, 1] < SPAN


def test_hook_stops_the_flight(chk):
    ret, y, (nacc, nrej, calls, hooks), rec = hooked(chk, stop_at=5)
    assert ret == 2.0
    assert hooks == 5 and nacc == 4
    assert y.tobytes() == rec[4, 2:8].tobytes()                 # the state the stopping call was handed: the step's start


def test_span_zero_negative_nan(chk):
    ret, y, (nacc, nrej, calls) = plain(chk, span=0.0)
    assert ret == 1.0 and y.tobytes() == Y0.tobytes() and (nacc, nrej, calls) == (0, 0, 0)
    ret, y, (nacc, nrej, calls, hooks), _ = hooked(chk, span=0.0)
    assert ret == 1.0 and y.tobytes() == Y0.tobytes() and (nacc, nrej, calls, hooks) == (0, 0, 0, 0)
    for span in (-1.0, float("nan")):
        for ret, y, cnt in (plain(chk, span=span), hooked(chk, span=span)[:3]):
            assert ret == 0.0 and np.all(np.isnan(y)) and cnt[:3] == [0, 0, 0]


def test_max_steps_used_up(chk):
    for ret, y, cnt in (plain(chk, max_steps=5), hooked(chk, max_steps=5)[:3]):
        assert ret == 0.0 and np.all(np.isnan(y))
        assert cnt[0] + cnt[1] == 5


def test_nan_in_the_start(chk):
    for c in range(6):
        y0 = Y0.copy()
        y0[c] = np.nan
        for ret, y, cnt in (plain(chk, y0=y0), hooked(chk, y0=y0)[:3]):
            assert ret == 0.0 and np.all(np.isnan(y))
            assert cnt[0] + cnt[1] == 1
