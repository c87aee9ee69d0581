"""csrc/hostbuf.hpp on the CPU: the allocation-failure-as-a-value containers that replaced std::vector / std::unordered_map behind the
C ABI (round 5).  Header-only host C++: built with g++, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hostbuf_containers(tmp_path):
    exe = str(tmp_path / "hostbuf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fno-exceptions", os.path.join(ROOT, "tests", "cabi", "hostbuf_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "hostbuf ok" in out.stdout, out.stdout + out.stderr


def _host_units():
    """Every host translation unit of the library -- the Makefile's SRCS but the kernels_*.hip -- and the internal headers they share."""
    import re
    csrc = os.path.join(ROOT, "lowthrustopt_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")        # a wrapped list is one line
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    on_disk = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert sorted(srcs) == on_disk, (srcs, on_disk)                              # the whole list was read, and it is the directory
    units = [u for u in srcs if not u.startswith("kernels_")]
    assert {"lto_group.hip", "lto_comm.hip"} < set(units), units        # and at least one unit for the rest of the ABI
    assert all(u.startswith("lto_") for u in units), units              # the Makefile's SRCS holds kernels_*.hip and lto_*.hip only
    headers = sorted(f for f in os.listdir(csrc) if f.startswith("lto_") and f.endswith(".hpp"))      # internal headers of the host units
    return units + headers + ["hostbuf.hpp"]


def test_no_throwing_containers_left_behind_the_abi():
    """The translation units that implement the C ABI, and their internal headers, hold no std::vector / std::map / std::string /
    std::thread any more."""
    import re
    for unit in _host_units():
        src = open(os.path.join(ROOT, "lowthrustopt_amd", "csrc", unit)).read()
        code = re.sub(r"//[^\n]*", "", src)                       # comments may name what was replaced
        for bad in ("std::vector", "std::unordered_map", "std::map<", "std::string", "std::thread", "#include <vector>"):
            assert bad not in code, (unit, bad)
