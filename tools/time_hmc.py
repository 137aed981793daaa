#!/usr/bin/env python3
"""Cost of the lock-step HMC step (cel_slice_sample, param 3; k_hmc.h) on the benchmark field (BASELINE configs[2],
mixed10k_2048) with a resident split, beside the host loop that makes one gradient call per leapfrog step.  Also the acceptance
rates of the two presets on this field.  Diagnostic; not part of bench.py's contract.

    (python tools/time_hmc.py; python tools/time_hmc.py test12) > profiles/hmc_time.txt

Every time is the median of REPS calls after WARM warm-up calls (min and max beside it), wall-clock around the blocking call.
The catalogue is put back before every call, so that each call starts from the same state.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

WARM, REPS = 3, 15
ctx = cel.Context(0)
name = sys.argv[1] if len(sys.argv) > 1 else "mixed10k_2048"
if name == "test12":         # the two-band 96 x 112 scene of tests/test_hmc.py's engine test
    f = synth.SyntheticField(ctx, 12, 2, 96, 112, frac_gal=0.5, seed=23)
else:
    f = synth.SyntheticField.from_config(ctx, name)
print("%s: %d sources, %d bands, %d x %d; median of %d calls after %d warm-up calls (min .. max)" % (name, f.S, f.B, f.H, f.W, REPS, WARM))


def timed(label, fn, before=None, reps=REPS, warm=WARM):
    ts = []
    for k in range(warm + reps):
        if before is not None:
            before()
        t0 = time.perf_counter()
        out = fn()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    print("%-66s %9.3f ms  (%.3f .. %.3f)" % (label, np.median(ts), min(ts), max(ts)))
    return out


def model(engine):
    imgs = cel.ImageSet(ctx, f.bands, f.H, f.W)
    imgs.set_nelec(f.nelec)
    gf = celeste_mcmc.GibbsField(imgs, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W)
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=5, engine=engine)
    g.resample_photons()
    return g


g = model("auto")
start = (g.u.copy(), g.shape.copy())


def back(m=g):
    m.u, m.shape, m._hmc_p = start[0].copy(), start[1].copy(), None
    m._sources(m.fields[0])                     # (the upload is not part of the step)


for label, kw in (("library default (eps 0.5, 8 steps, scale-free mass)", {}), ("reference preset (eps 1e-5, 50 steps)", g.hmc_preset("reference"))):
    steps = kw.get("steps", 8)
    a0, e0 = g.timing["hmc_accepted"], g.timing["hmc_evals"]
    timed("device engine, %s" % label, lambda: g.resample_hmc(**kw), before=back)
    n = WARM + REPS
    run = int(np.sum(g.active & (g.typ < 2)))
    print("    acceptance %.3f (%d of %d updates), %d gradient evaluations per call"
          % ((g.timing["hmc_accepted"] - a0) / float(n * run), g.timing["hmc_accepted"] - a0, n * run, (g.timing["hmc_evals"] - e0) // n))
    t = []
    for L in (1, steps):
        k2 = dict(kw)
        k2["steps"] = L
        ts = []
        for k in range(WARM + REPS):
            back()
            t0 = time.perf_counter()
            g.resample_hmc(**k2)
            if k >= WARM:
                ts.append((time.perf_counter() - t0) * 1e3)
        t.append(np.median(ts))
    print("    per leapfrog step (median at %d steps - median at 1 step) / %d: %.3f ms" % (steps, steps - 1, (t[1] - t[0]) / (steps - 1)))

h = model("host")
timed("host loop (one mode-8 call per step), library default, 8 steps", lambda: h.resample_hmc(), before=lambda: back(h), reps=5, warm=1)
timed("host loop, 1 step", lambda: h.resample_hmc(steps=1), before=lambda: back(h), reps=5, warm=1)
