#!/usr/bin/env python3
"""What the star <-> galaxy step costs (cel_slice_sample, param 2): BASELINE.json configs[2]'s field (10 000 mixed
sources x 5 bands x 2048^2) swept as `bench.py --workload gibbs10k` sweeps it, with sweep(types=True), in one process, two
settings interleaved sweep by sweep:

    1. the type step on the host engine    two slots per chain through patch_loglik_resident (+ _exact_terms): calls the
                                           library had before the move existed -- the yardstick
    2. the type step on the device         ImageSet.type_move: k_tm_fill, k_tm_jobs, k_prep, the likelihood kernels, k_tm_decide

Everything else of the sweep runs as it does by default (engine="auto") in both.

    python tools/type_move_cost.py [sweeps] [--exact]

Median and minimum wall clock of the type step and of the sweep; evaluations and accepted moves per sweep.  The two chains
start from the same state and seed and stay together bit for bit (asserted).

Diagnostic; not part of bench.py's contract (profiles/type_move_time.txt keeps a run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
sweeps = int(args[0]) if args else 20
conditional = "exact" if "--exact" in sys.argv else "reference"
SETTINGS = (("type step on the host", "host"), ("type step on the device", "device"))

chains = {}
for name, eng in SETTINGS:
    ctx = cel.Context(0)
    f = synth.SyntheticField.from_config(ctx, "mixed10k_2048", seed=42)
    gf = celeste_mcmc.GibbsField(f.images, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W)
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=1,
                                slice_args=dict(step_out=False, sigma=0.001), conditional=conditional)
    g.type_engine = eng
    chains[name] = (g, f)
g0, f0 = chains[SETTINGS[0][0]]
print("mixed10k_2048: S = %d, B = %d, %d x %d; conditional=%s; %d sweeps per setting after 2 warm-up sweeps, interleaved" % (
    f0.S, f0.B, f0.H, f0.W, conditional, sweeps))

wall = {name: [] for name in chains}
step = {name: [] for name in chains}
count = {name: dict(type_evals=0, type_accepted=0) for name in chains}
for r in range(sweeps + 2):
    for name, (g, f) in chains.items():
        for k in g.timing:
            g.timing[k] = 0
        t0 = time.perf_counter()
        g.sweep(types=True)
        g.log_likelihood()                                   # the chain's trace, as bench.py's step renders it
        dt = time.perf_counter() - t0
        if r >= 2:
            wall[name].append(1e3 * dt)
            step[name].append(1e3 * g.timing["type"])
            for k in count[name]:
                count[name][k] += g.timing[k]
    a, b = (chains[n][0] for n, _ in SETTINGS)
    for what in ("typ", "u", "fluxes", "shape"):
        assert np.array_equal(getattr(a, what), getattr(b, what)), (r, what)

print("wall clock, ms: median (minimum) of %d" % sweeps)
print("  %-26s %21s %21s %14s %14s" % ("setting", "type step", "sweep + trace", "evals / sweep", "accepted / sweep"))
for name in chains:
    print("  %-26s %10.3f (%8.3f) %10.2f (%8.2f) %14.0f %14.1f" % (
        name, np.median(step[name]), np.min(step[name]), np.median(wall[name]), np.min(wall[name]),
        count[name]["type_evals"] / sweeps, count[name]["type_accepted"] / sweeps))
h, d = (np.median(step[n]) for n, _ in SETTINGS)
print("type step: on the device %.3f ms = %.2f x the host engine's %.3f ms (the yardstick: must not exceed 1)" % (d, d / h, h))
print("galaxies in the catalogue: %d at the start, %d after %d sweeps" % (int((f0.src["type"] == 1).sum()), int((g0.typ == 1).sum()), sweeps + 2))
