#!/usr/bin/env python3
"""Cost of the lock-step HMC step (cel_slice_sample, param 3; k_hmc.h) on the benchmark field (BASELINE configs[2],
mixed10k_2048) with a resident split, beside the host loop that makes one gradient call per leapfrog step.  Also the acceptance
rates of the two presets on this field.  Diagnostic; not part of bench.py's contract.

    (python tools/time_hmc.py --route both; python tools/time_hmc.py test12 --route both) > profiles/hmc_time.txt

--route dense | photons | both: where the step's gradients are summed (ModelGibbs(grad_route=)); both: the two routes in one
process, interleaved call by call.
--conditional reference | exact: exact = the step under the exact conditional (ModelGibbs(conditional="exact", hmc_conditional=
"exact"): CEL_OPT_GRAD_CONDITIONAL, k_mass_grad.h) BESIDE the reference's, in one process, the conditionals (and routes) taking
turns call by call:

    python tools/time_hmc.py --conditional exact --route both > profiles/hmc_exact_time.txt

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

import argparse  # noqa: E402

WARM, REPS = 3, 15
ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="mixed10k_2048")
ap.add_argument("--route", choices=("dense", "photons", "both"), default="dense")
ap.add_argument("--conditional", choices=("reference", "exact"), default="reference")
ap.add_argument("--no-host", action="store_true", help="leave out the host loop (one mode-8 call per step)")
args = ap.parse_args()
ROUTES = ("dense", "photons") if args.route == "both" else (args.route,)
CONDS = ("reference", "exact") if args.conditional == "exact" else ("reference",)
# a variant: (conditional, route); its label names the conditional only where there are two
ROUTES = tuple((c, r) for r in ROUTES for c in CONDS)


def vname(v):
    return v[1] if len(CONDS) == 1 else "%s conditional, %s" % v
ctx = cel.Context(0)
name = args.config
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


def model(engine, variant):
    cond, route = variant
    kw = dict(conditional="exact", hmc_conditional="exact") if cond == "exact" else {}
    imgs = cel.ImageSet(ctx, f.bands, f.H, f.W)
    imgs.set_nelec(f.nelec)
    gf = celeste_mcmc.GibbsField(imgs, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W)
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=5, engine=engine, grad_route=route, **kw)
    g.resample_photons()
    return g


g = {r: model("auto", r) for r in ROUTES}
start = (g[ROUTES[0]].u.copy(), g[ROUTES[0]].shape.copy())


def back(m):
    m.u, m.shape, m._hmc_p = start[0].copy(), start[1].copy(), None
    m._sources(m.fields[0])                     # (the upload is not part of the step)


def interleaved(kw):
    """median, min, max per route of WARM + REPS calls, the routes taking turns call by call"""
    ts = {r: [] for r in ROUTES}
    for k in range(WARM + REPS):
        for r in ROUTES:
            back(g[r])
            t0 = time.perf_counter()
            g[r].resample_hmc(**kw)
            if k >= WARM:
                ts[r].append((time.perf_counter() - t0) * 1e3)
    return ts


g0 = g[ROUTES[0]]
for label, kw in (("library default (eps 0.5, 8 steps, scale-free mass)", {}), ("reference preset (eps 1e-5, 50 steps)", g0.hmc_preset("reference"))):
    steps = kw.get("steps", 8)
    a0 = {r: (g[r].timing["hmc_accepted"], g[r].timing["hmc_evals"]) for r in ROUTES}
    ts = interleaved(kw)
    n = WARM + REPS
    run = int(np.sum(g0.active & (g0.typ < 2)))
    for r in ROUTES:
        print("%-66s %9.3f ms  (%.3f .. %.3f)" % ("device engine, %s route, %s" % (vname(r), label), np.median(ts[r]), min(ts[r]), max(ts[r])))
        acc, ev = g[r].timing["hmc_accepted"] - a0[r][0], g[r].timing["hmc_evals"] - a0[r][1]
        print("    acceptance %.3f (%d of %d updates), %d gradient evaluations per call" % (acc / float(n * run), acc, n * run, ev // n))
    k1 = dict(kw)
    k1["steps"] = 1
    t1 = interleaved(k1)
    for r in ROUTES:
        print("    %s route, per leapfrog step (median at %d steps - median at 1 step) / %d: %.3f ms"
              % (vname(r), steps, steps - 1, (np.median(ts[r]) - np.median(t1[r])) / (steps - 1)))

if not args.no_host:
    for r in ROUTES:
        h = model("host", r)
        timed("host loop (one mode-8 call per step), %s route, library default, 8 steps" % vname(r), lambda: h.resample_hmc(), before=lambda: back(h), reps=5, warm=1)
        timed("host loop, %s route, 1 step" % vname(r), lambda: h.resample_hmc(steps=1), before=lambda: back(h), reps=5, warm=1)
