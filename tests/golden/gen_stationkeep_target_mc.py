"""Writes tests/golden/stationkeep_target_mc.json: the vetting of the Monte Carlo that tests/test_stationkeep_target_gpu.py flies
(tests/test_stationkeep_target_host.py MONTE_CARLO: 16 runs, four burns a revolution, 20 revolutions), flown by the independent
reference (tests/stationkeep_reference.py flight, scipy DOP853, one solve per span) under the reference's own target-point law
(tests/stationkeep_target_reference.py) at (rtol, atol) = (1e-13, 1e-14) and (1e-12, 1e-13), and without a law.  About a minute and
a half on one core, which is why the result is kept.  Run from the repository root:  python tests/golden/gen_stationkeep_target_mc.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import stationkeep_target_reference as TR  # noqa: E402
import test_stationkeep_target_host as H  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def main():
    orbits = MR.packaged_orbits(synth.halo_orbits(), MU)
    m = H.MONTE_CARLO
    L = TR.law(orbits, 0, TR.TAUS4, MU)
    n_upd = 4 * m["n_rev"]
    inj, nav, exe = drivers.stationkeep_draws(m["n_runs"], n_upd, m["inj_sigma_r_km"], m["inj_sigma_v_ms"], m["nav_sigma_r_km"],
                                              m["nav_sigma_v_ms"], m["exe_sigma_frac"], m["exe_sigma_ms"], m["seed"], DU, TU)
    r_lost = m["r_lost_km"] / DU
    out = dict(monte_carlo=m, law={}, loose={}, free={})
    for name, G, tol in (("law", L.G, (TR.RTOL, TR.ATOL)), ("loose", L.G, TR.LOOSE), ("free", 0.0 * L.G, (TR.RTOL, TR.ATOL))):
        runs = [SR.flight(MU, L.X_ref, L.dt, G, L.X_ref[:, 0] + inj[:, b], m["n_rev"], nav[:, :, b], exe[:, :, b], r_lost=r_lost,
                          rtol=tol[0], atol=tol[1]) for b in range(m["n_runs"])]
        out[name] = dict(status=[int(r.status) for r in runs], lost_at=[int(r.lost_at) for r in runs],
                         n_burn=[int(r.n_burn) for r in runs], dv_total=[float(r.dv_total) for r in runs],
                         dev_r_max=[float(np.nanmax(r.dev[0])) for r in runs], x_final=[[float(v) for v in r.x_final] for r in runs],
                         dev_final=[[float(v) for v in r.dev_final] for r in runs])
        print(name, out[name]["status"], out[name]["lost_at"], "largest deviation %.2f km" % (max(out[name]["dev_r_max"]) * DU))
    with open(os.path.join(HERE, "stationkeep_target_mc.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
