#!/usr/bin/env python3
"""The photon moments and the type move with either proposal, at BASELINE.json configs[2] (10 000 mixed sources x 5 bands x 2048^2).

    python tools/time_type_move.py [sweeps]        > profiles/type_move_moments.txt

1. ImageSet.photon_moments() (cel_slice_sample, param = CEL_SLICE_MOMENTS; k_moments.h) after a resident split made under CEL_OPT_PHOTON_LISTS = 0 (per
   patch, as the likelihoods read it), 1 (every patch at its photon list) and 2 (no lists: every patch densely): median and
   minimum wall clock of 20 calls.  The call's time holds the launch, the kernel and the S x B x 48 bytes that come back; the
   three results are compared with np.array_equal.
2. resample_types() with type_proposal="prior" and "moments", the same chain otherwise: median wall clock of the step
   (timing["type"]) over the sweeps, and of the proposal's host part alone (MomentProposal.__call__: the moments call, the centre
   map, the draws, the densities).
3. accepted moves per direction by the source's photons in the split (all bands), summed over the sweeps, under either proposal:
   on the catalogue as it is (every source correctly typed: a move should be rare) and on the same catalogue with EVERY source
   typed as a star (three sweeps: what the move is for).

Diagnostic; not part of bench.py's contract."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import _lib, celeste_mcmc, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
sweeps = int(args[0]) if args else 10
EDGES = np.array([0, 100, 300, 1000, 3000, 10000, 30000, 1e18])

ctx = cel.Context(0)
f = synth.SyntheticField.from_config(ctx, "mixed10k_2048", seed=42)
print("mixed10k_2048: S = %d, B = %d, %d x %d" % (f.S, f.B, f.H, f.W))

# ---- 1. the moments call ---------------------------------------------------------------------------------------------------------
print("\n1. ImageSet.photon_moments(): wall clock of the call, ms, median (minimum) of 20")
ref = None
for lists, name in ((0, "lists per patch (default)"), (1, "every patch at its list"), (2, "every patch densely")):
    ctx.set_option(_lib.CEL_OPT_PHOTON_LISTS, lists)
    f.images.render(f.sources, loglik=True)
    f.images.photon_split_resident(f.sources, seed=7)
    areas = f.images.sample_box_areas()
    f.images.photon_moments()
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        mom = f.images.photon_moments()
        ts.append(1e3 * (time.perf_counter() - t0))
    ref = mom if ref is None else ref
    assert np.array_equal(mom, ref)
    print("  CEL_OPT_PHOTON_LISTS = %d  %-28s %8.3f (%8.3f)   %d patches, %.2f GB of int32 pixels, %.1f M photons"
          % (lists, name, np.median(ts), np.min(ts), int((areas > 0).sum()), 4e-9 * areas.sum(), 1e-6 * mom[..., 0].sum()))
ctx.set_option(_lib.CEL_OPT_PHOTON_LISTS, 0)

# ---- 2. and 3. the type move -----------------------------------------------------------------------------------------------------
def run(prop, all_stars, n_sweeps):
    c = cel.Context(0)
    ff = synth.SyntheticField.from_config(c, "mixed10k_2048", seed=42)
    gf = celeste_mcmc.GibbsField(ff.images, list(range(ff.B)), ff.bands[:, 2], ff.bands[:, 1], ff.H * ff.W)
    typ0 = np.zeros_like(ff.src["type"]) if all_stars else ff.src["type"]
    shape0 = np.zeros_like(ff.src["shape"]) if all_stars else ff.src["shape"]
    g = celeste_mcmc.ModelGibbs([gf], typ0, ff.src["radec"], ff.flux5(), shape0, seed=1,
                                slice_args=dict(step_out=False, sigma=0.001), type_proposal=prop)
    warm = 0 if all_stars else 2
    step, host = [], []
    acc = np.zeros((2, EDGES.size - 1), dtype=np.int64)
    tried = np.zeros((2, EDGES.size - 1), dtype=np.int64)
    for r in range(n_sweeps + warm):
        g.resample_photons()
        g.resample_fluxes()
        g.resample_locations()
        if prop == "moments" and r >= warm:
            t0 = time.perf_counter()
            g.moment_proposal(g)
            host.append(1e3 * (time.perf_counter() - t0))
        before = g.typ.copy()
        g.timing["type"] = 0.0
        g.resample_types()
        g.sweeps += 1
        if r >= warm:
            step.append(1e3 * g.timing["type"])
            n = ff.images.sample_sums().sum(axis=1)
            k = np.clip(np.searchsorted(EDGES, n, side="right") - 1, 0, EDGES.size - 2)
            for d in (0, 1):
                sel = before == d
                tried[d] += np.bincount(k[sel], minlength=EDGES.size - 1)
                acc[d] += np.bincount(k[sel & (g.typ != before)], minlength=EDGES.size - 1)
    right = int((g.typ == ff.src["type"]).sum())
    return step, host, acc, tried, right


def show(table, n_sweeps):
    print("  %-22s" % "photons" + "".join("%16s" % ("%g-%s" % (EDGES[i], "%g" % EDGES[i + 1] if EDGES[i + 1] < 1e17 else "")) for i in range(EDGES.size - 1)))
    for prop in ("prior", "moments"):
        acc, tried, right = table[prop]
        for d, name in ((0, "star -> galaxy"), (1, "galaxy -> star")):
            print("  %-8s %-13s" % (prop, name) + "".join("%16s" % ("%d / %d" % (acc[d][i], tried[d][i])) for i in range(EDGES.size - 1)))
    for prop in ("prior", "moments"):
        print("  %-8s sources of the true type after the %d sweeps: %d of %d" % (prop, n_sweeps, table[prop][2], f.S))


print("\n2. resample_types(), ms, median (minimum) of %d sweeps after 2 warm-up sweeps" % sweeps)
table = {}
for prop in ("prior", "moments"):
    step, host, acc, tried, right = run(prop, False, sweeps)
    table[prop] = (acc, tried, right)
    print("  type_proposal=%-8s  step %8.3f (%8.3f)%s" % (
        prop, np.median(step), np.min(step),
        "   of which the proposal's host part alone (moments call + numpy) %8.3f (%8.3f)" % (np.median(host), np.min(host)) if host else ""))

print("\n3a. accepted / proposed by the source's photons in the split (all bands), %d sweeps, every source correctly typed at the start" % sweeps)
show(table, sweeps)
print("\n3b. the same with EVERY source typed as a star at the start (half are galaxies), 3 sweeps")
table = {}
for prop in ("prior", "moments"):
    table[prop] = run(prop, True, 3)[2:]
show(table, 3)
