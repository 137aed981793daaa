#!/usr/bin/env python3
"""Cost of the masked sweep's steps on the device engine (ModelGibbs(mask="honour", mask_engine="device"): CEL_OPT_SAMPLER_MASK, the
observed-mass kernel on the samplers' job lists, k_mass_grad_masked) beside the host engine on the same masked field, and beside
the unmasked device engine on the same field with the NaNs filled -- what the mask itself costs.  The benchmark field (BASELINE
configs[2], mixed10k_2048) with 1 % of its pixels masked from a fixed seed.  Diagnostic; not part of bench.py's contract.

    python tools/time_sampler_mask.py > profiles/sampler_mask_time.txt
    python tools/time_sampler_mask.py test12            # the two-band 96 x 112 scene of tests/test_hmc.py's engine test

Steps: the location step, the shape step, the type move and the exact HMC update (grad_route dense and photons).  Every time is the
median of REPS calls after WARM warm-up calls (min and max beside it), wall-clock around the blocking call; the three models take
turns call by call, and each call starts from the same state (the catalogue is put back first).  --no-host leaves the host
engine out (its location step makes one launch and one readback per round of 10 000 chains).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

WARM, REPS = 3, 15
ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="mixed10k_2048")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--reps", type=int, default=REPS)
args = ap.parse_args()
REPS = args.reps
ctx = cel.Context(0)
if args.config == "test12":
    f = synth.SyntheticField(ctx, 12, 2, 96, 112, frac_gal=0.5, seed=23)
else:
    f = synth.SyntheticField.from_config(ctx, args.config)
mask = np.random.RandomState(2024).rand(*f.nelec.shape) < 0.01
print("%s: %d sources, %d bands, %d x %d, %d of %d pixels masked; median of %d calls after %d warm-up calls (min .. max)"
      % (args.config, f.S, f.B, f.H, f.W, int(mask.sum()), mask.size, REPS, WARM))
SLICE = dict(step_out=False, sigma=1e-3)


def model(nelec, route, **kw):
    imgs = cel.ImageSet(ctx, f.bands, f.H, f.W)
    imgs.set_nelec(nelec)
    npix = imgs.npix_observed() if kw.get("mask") == "honour" else None
    gf = celeste_mcmc.GibbsField(imgs, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W, npix_observed=npix)
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=5, conditional="exact",
                                hmc_conditional="exact", grad_route=route, slice_args=SLICE, **kw)
    g.resample_photons()
    return g


def models(route):
    masked = np.where(mask, np.nan, f.nelec)
    m = {"masked, device engine": model(masked, route, mask="honour", engine="auto", mask_engine="device"),
         "NaNs filled, device engine (no mask)": model(np.where(mask, 0.0, f.nelec), route, engine="auto")}
    if not args.no_host:
        m["masked, host engine"] = model(masked, route, mask="honour", engine="host")
    return m


def back(m, start):
    m.typ, m.u, m.shape, m._hmc_p = start[0].copy(), start[1].copy(), start[2].copy(), None
    m._sources(m.fields[0])                     # (the upload is not part of the step)


def interleaved(ms, step, label):
    ts = {k: [] for k in ms}
    start = {k: (m.typ.copy(), m.u.copy(), m.shape.copy()) for k, m in ms.items()}
    for i in range(WARM + REPS):
        for k, m in ms.items():
            back(m, start[k])
            t0 = time.perf_counter()
            step(m)
            if i >= WARM:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    for k in ms:
        print("%-28s %-40s %9.3f ms  (%.3f .. %.3f)" % (label, k, np.median(ts[k]), min(ts[k]), max(ts[k])))


ms = models("dense")
for k, m in ms.items():
    print("%-40s location %s, shape %s, type %s, hmc %s" % (k, "device" if m._device_engine_applies() and m.engine != "host" else "host",
          "device" if m._shape_engine_on_device() else "host", "device" if m._type_engine_on_device() else "host",
          "device" if m._hmc_engine_on_device() else "host"))
interleaved(ms, lambda m: m.resample_locations(), "location step")
interleaved(ms, lambda m: m.resample_shapes(), "shape step")
interleaved(ms, lambda m: m.resample_types(), "type move")
interleaved(ms, lambda m: m.resample_hmc(), "HMC update, dense route")
del ms
ms = models("photons")
interleaved(ms, lambda m: m.resample_hmc(), "HMC update, photons route")
