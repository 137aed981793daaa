#!/usr/bin/env python3
"""What the exact conditional costs on the device slice engine (CEL_OPT_SLICE_CONDITIONAL): BASELINE.json
configs[2]'s field (10 000 mixed sources x 5 bands x 2048^2) swept as `bench.py --workload gibbs10k` sweeps it, in one
process, the three settings interleaved sweep by sweep:

    1. ModelGibbs(conditional="exact", engine="host")        the exact sweep as it ran before the option existed: the yardstick
    2. ModelGibbs(conditional="exact", engine="device")      cel_slice_sample under CEL_OPT_SLICE_CONDITIONAL = 1
    3. ModelGibbs(conditional="reference", engine="device")  cel_slice_locations (the default sweep)

    python tools/exact_slice_cost.py [sweeps] [--shapes]

Median and minimum wall clock per sweep and per step; rounds, evaluations and conditional-likelihood launches per sweep.
With --shapes every sweep ends with the galaxies' shape step (sweep(shapes=True)).  The three chains start from the same state
and seed but do not stay together (1 and 2 do, bit for bit: tests/test_slice_exact.py).

Diagnostic; not part of bench.py's contract (profiles/exact_slice_time.txt keeps a run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
sweeps = int(args[0]) if args else 20
shapes = "--shapes" in sys.argv
SETTINGS = (("exact, host engine", dict(conditional="exact", engine="host")),
            ("exact, device engine", dict(conditional="exact", engine="device")),
            ("reference, device engine", dict(conditional="reference", engine="device")))
STEPS = ("split", "flux", "location", "shape")
COUNTS = ("rounds", "evals", "loc_launches", "shape_rounds", "shape_evals")

chains = {}
for name, kw in SETTINGS:
    # a context and a field of its own per setting: the three resident splits live side by side
    ctx = cel.Context(0)
    f = synth.SyntheticField.from_config(ctx, "mixed10k_2048", seed=42)
    gf = celeste_mcmc.GibbsField(f.images, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W)
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=1,
                                slice_args=dict(step_out=False, sigma=0.001), **kw)
    chains[name] = (g, f)
g0, f0 = chains[SETTINGS[0][0]]
print("mixed10k_2048: S = %d, B = %d, %d x %d; %d sweeps per setting after 2 warm-up sweeps, interleaved; shape step %s" % (
    f0.S, f0.B, f0.H, f0.W, sweeps, "on" if shapes else "off"))

wall = {name: [] for name in chains}
step = {name: {k: [] for k in STEPS} for name in chains}
count = {name: {k: 0 for k in COUNTS} for name in chains}
for r in range(sweeps + 2):
    for name, (g, f) in chains.items():
        for k in g.timing:
            g.timing[k] = 0
        t0 = time.perf_counter()
        g.sweep(shapes=shapes)
        g.log_likelihood()                                   # the chain's trace, as bench.py's step renders it
        dt = time.perf_counter() - t0
        if r >= 2:
            wall[name].append(1e3 * dt)
            for k in STEPS:
                step[name][k].append(1e3 * g.timing.get(k, 0.0))
            for k in COUNTS:
                count[name][k] += g.timing.get(k, 0)


def fig(v):
    return "%8.2f (%8.2f)" % (np.median(v), np.min(v))


print("wall clock per sweep and per step, ms: median (minimum)")
print("  %-26s %19s %19s %19s %19s %19s" % ("setting", "sweep + trace", "split + sky", "flux", "location", "shape"))
for name in chains:
    print("  %-26s %19s %19s %19s %19s %19s" % (name, fig(wall[name]), fig(step[name]["split"]), fig(step[name]["flux"]),
                                               fig(step[name]["location"]), fig(step[name]["shape"])))
print("per sweep: location rounds, evaluations, round launches queued by the device engine (its launches per round: the")
print("likelihood kernels count as one); shape rounds, evaluations")
for name in chains:
    c = count[name]
    print("  %-26s %6.1f rounds %9.0f evaluations %6.1f queued rounds;  shape %6.1f rounds %9.0f evaluations" % (
        name, c["rounds"] / sweeps, c["evals"] / sweeps, c["loc_launches"] / sweeps, c["shape_rounds"] / sweeps, c["shape_evals"] / sweeps))
host, dev, ref = (SETTINGS[i][0] for i in range(3))
for k in ("location",) + (("shape",) if shapes else ()):
    h, d, rf = np.median(step[host][k]), np.median(step[dev][k]), np.median(step[ref][k])
    print("%s step: exact on the device %.2f ms = %.2f x the host engine's %.2f ms (the yardstick: must not exceed 1), %.2f x the "
          "reference conditional's %.2f ms on the device" % (k, d, d / h, h, d / rf if rf else float("nan"), rf))
print("launches per round of the exact conditional on the device: k_sg_propose, k_prep (with boxes), k_sg_cover, the likelihood "
      "kernels (dense and at the photons), k_patch_ll_hw<3> on the live chains' jobs, k_sg_exact_terms, k_sg_consume_exact; "
      "the reference conditional's round: k_sg_propose, k_prep (no boxes), the likelihood kernels, k_sg_consume")
