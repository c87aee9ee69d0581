#!/usr/bin/env python3
"""Time the periodic-orbit calls on the device (lto_halo_correct_batch, lto_halo_table_batch) at B = 1 and B = 4096:
`lto_last_call_ms`, median of 10 calls after 3 warm-ups.  The seeds are the packaged orbit 1's, x0 spread over the march towards
orbit 2 (hold x0), so the orbits of a batch differ; the tables have 100 samples.  Prints one line per figure."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402


def median_call_ms(ctx, fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    return statistics.median([(fn(), ctx.last_call_ms())[1] for _ in range(reps)])


def main():
    ctx = lto.default_context(0)
    tabs = synth.halo_orbits()
    s1 = np.array(tabs[0][:6, 0])
    s1[[1, 3, 5]] = 0.0
    for B in (1, 4096):
        seeds = np.repeat(s1[:, None], B, axis=1)
        seeds[0] += 0.2 * (tabs[1][0, 0] - s1[0]) * np.arange(B) / float(B)      # a fifth of the way to orbit 2: a few Newton steps each
        c = lto.halo_correct(seeds, "x0", ctx=ctx)
        ms = median_call_ms(ctx, lambda: lto.halo_correct(seeds, "x0", ctx=ctx))
        print("halo_correct, B = %4d: lto_last_call_ms %.3f, status 0 for %d seeds, iterations %d .. %d"
              % (B, ms, int(np.count_nonzero(c.status == 0)), c.iterations.min(), c.iterations.max()))
        ok = c.status == 0
        state, period = np.asfortranarray(c.state[:, ok]), np.ascontiguousarray(c.period[ok])
        t = lto.halo_table(state, period, 100, ctx=ctx)
        ms = median_call_ms(ctx, lambda: lto.halo_table(state, period, 100, ctx=ctx))
        print("halo_table (100 samples), B = %4d: lto_last_call_ms %.3f, status 0 for %d orbits, worst closure %.2e"
              % (state.shape[1], ms, int(np.count_nonzero(t.status == 0)), float(np.max(t.closure))))


if __name__ == "__main__":
    main()
