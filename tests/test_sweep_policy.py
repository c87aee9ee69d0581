"""csrc/sweep_policy.hpp on the CPU: which kernel form an indirect sweep runs -- the forced selectors and their fallbacks, the 44 / 48
form of the large-batch pipeline, the stream corner, the lanes per segment of the defect sweep and the statistics verdict -- as
literal expectations at 256 CUs and the default cost table (tests/cabi/sweep_policy_check.cpp).  Header-only host C++: built with
g++, no GPU.  LTO_KERNEL_AUTO's table is the one tests/test_auto_kernel.py pins through the library; here its rows go through
resolve_stm, the function the STM sweep itself calls."""
import os
import subprocess

import pytest

from lowthrustopt_amd.hotpath import IndirectPlan
from test_auto_kernel import BOUNDARY_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = IndirectPlan.KERNEL_NAMES      # LTO_KERNEL_* (include/lto.h) -> the family names lto.auto_kernel reports


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sweep_policy") / "sweep_policy_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fno-exceptions", os.path.join(ROOT, "tests", "cabi", "sweep_policy_check.cpp"), "-o", path])
    return path


def test_sweep_policy_literal_expectations(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sweep policy ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("ndim,S,method,steps,want", BOUNDARY_CASES)
def test_resolve_stm_auto_at_the_round_boundaries(exe, ndim, S, method, steps, want):
    out = subprocess.run([exe, "0", str(ndim), str(method), str(steps), "2", str(S)], capture_output=True, text=True)      # pm = 2: p = 1
    assert out.returncode == 0, out.stdout + out.stderr
    assert FAMILY[int(out.stdout)] == want


def test_the_policy_header_is_device_free():
    """No HIP and no context in the header: g++ alone compiles it (above), and nothing it includes is the GPU runtime's."""
    src = open(os.path.join(ROOT, "lowthrustopt_amd", "csrc", "sweep_policy.hpp")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes == ["<algorithm>", '"../../include/lto.h"'], includes

