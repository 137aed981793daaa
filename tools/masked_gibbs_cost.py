#!/usr/bin/env python3
"""What a mask costs the Gibbs sweep (CEL_OPT_HONOUR_MASK): BASELINE.json configs[2]'s field (10 000 mixed sources x
5 bands x 2048^2) with 1 % of the pixels masked (NaN counts), against the same field with 0 counts at those pixels, in one
process and interleaved.

    python tools/masked_gibbs_cost.py [rounds] [sweeps]

  1. the masked photon split twin (k_photon_split_hw_masked<int>) against its unmasked twin on the zero-filled set: the kernel's
     own time (CEL_OPT_PROFILE events), the split re-using the model image of a render as a sweep's does.  The zero-filled set
     takes the 16-bit photons-left plane when every count fits it; a second zero-filled set with ONE count raised above 65 535
     takes k_photon_split_hw<int, int>, the instantiation the masked twin shares its LDS footprint with.
  2. the observed-mass kernel (k_stamp_mass_masked) over all S B jobs against what it replaces on an unmasked set: the short cut
     from the split's own sums (k_mass_from_fx + leftovers), and the mass kernel proper (k_patch_ll_hw<3>) over the same jobs.
  3. a sweep of ModelGibbs(conditional="exact", engine="host") with mask="honour" on the masked set against the same sweep on
     the zero-filled set (wall clock; split + sky, flux, location shares).

Diagnostic; not part of bench.py's contract (profiles/masked_gibbs_time.txt keeps a run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

L = cel._lib
args = [a for a in sys.argv[1:] if not a.startswith("--")]
rounds = int(args[0]) if args else 10
sweeps = int(args[1]) if len(args) > 1 else 3
ctx = cel.Context(0)
f = synth.SyntheticField.from_config(ctx, "mixed10k_2048")
mask = np.random.RandomState(5).rand(f.B, f.H, f.W) < 0.01
zero = np.where(mask, 0.0, f.nelec)
big = zero.copy()
big[0, 0, 0] = 70000.0                      # one count beyond 16 bits: the int photons-left plane
sets = {"masked": cel.ImageSet(ctx, f.bands, f.H, f.W, nelec=np.where(mask, np.nan, f.nelec)),
        "zero-filled": cel.ImageSet(ctx, f.bands, f.H, f.W, nelec=zero),
        "zero-filled, int plane": cel.ImageSet(ctx, f.bands, f.H, f.W, nelec=big)}
print("mixed10k_2048: S = %d, B = %d, %d x %d; masked pixels per band %s; largest count %.0f" % (
    f.S, f.B, f.H, f.W, sets["masked"].masked.tolist(), zero.max()))
ctx.set_option(L.CEL_OPT_HONOUR_MASK, 1)


def timed(kernel, fn):
    """the mean time of `kernel`'s launches inside fn(), by the library's events"""
    ctx.profile(True)
    fn()
    ms, n = ctx.profile_get(kernel)
    ctx.profile(False)
    return ms, n


# ---- 1. the split twins, interleaved ---------------------------------------------------------------------------------------------
split = {k: [] for k in sets}
for r in range(rounds + 2):
    for name, im in sets.items():
        im.render(f.sources, loglik=True)                      # (the sweep's state: the split re-uses this model image)
        ms, n = timed("split", lambda: im.photon_split_resident(f.sources, 100 + r))
        if r >= 2:
            split[name].append(ms)
print("photon split kernel, %d interleaved rounds, median (min .. max) ms:" % rounds)
for name, v in split.items():
    print("  %-24s %.4f (%.4f .. %.4f)" % (name, np.median(v), np.min(v), np.max(v)))
ref = np.median(split["zero-filled, int plane"])
print("  masked twin / its unmasked twin (int plane): %.4f; / the zero-filled set as it ships: %.4f" % (
    np.median(split["masked"]) / ref, np.median(split["masked"]) / np.median(split["zero-filled"])))

# ---- 2. the observed mass against the short cut and against the mass kernel proper -------------------------------------------------
mass = {"observed (k_stamp_mass_masked)": [], "short cut (from the split's sums)": [], "mass kernel proper (k_patch_ll_hw<3>)": []}
wall = {k: [] for k in mass}
m_im, z_im = sets["masked"], sets["zero-filled"]
for r in range(rounds + 2):
    for name, im, prep in (("observed (k_stamp_mass_masked)", m_im, True), ("short cut (from the split's sums)", z_im, True),
                           ("mass kernel proper (k_patch_ll_hw<3>)", z_im, False)):
        im.render(f.sources, loglik=True)
        if prep:
            im.photon_split_resident(f.sources, 200 + r)
        else:
            ctx.set_option(L.CEL_OPT_SPLIT_REUSE, 1)       # no sums from the split: the kernel proper over all S B jobs
            im.photon_split_resident(f.sources, 200 + r)
        if im.stamp_mass_ready(f.sources) != name.startswith("short"):
            print("  (%s: the short cut's readiness is not what this leg expects)" % name)
        t0 = time.perf_counter()
        ms, n = timed("mass", lambda: im.stamp_mass(f.sources))
        dt = 1e3 * (time.perf_counter() - t0)
        if not prep:
            ctx.set_option(L.CEL_OPT_SPLIT_REUSE, 2)
        if r >= 2:
            mass[name].append(ms)
            wall[name].append(dt)
print("stamp masses of all %d (source, band) jobs, median kernel ms (call ms):" % (f.S * f.B))
for name in mass:
    print("  %-40s %.4f (%.3f)" % (name, np.median(mass[name]), np.median(wall[name])))

# ---- 3. the exact-conditional host-engine sweep -----------------------------------------------------------------------------------
ctx.set_option(L.CEL_OPT_HONOUR_MASK, 0)                      # (ModelGibbs sets it around its own calls)
print("ModelGibbs(conditional='exact', engine='host') sweeps, wall clock per sweep (after one warm-up sweep), %d sweeps:" % sweeps)
for name, im, kw in (("masked, mask='honour'", m_im, dict(mask="honour")), ("zero-filled", z_im, {})):
    gf = celeste_mcmc.GibbsField(im, list(range(f.B)), f.bands[:, 2], f.bands[:, 1], f.H * f.W, npix_observed=im.npix_observed())
    g = celeste_mcmc.ModelGibbs([gf], f.src["type"], f.src["radec"], f.flux5(), f.src["shape"], seed=1, engine="host",
                                conditional="exact", slice_args=dict(step_out=False, sigma=0.001), **kw)
    g.sweep()
    g.log_likelihood()
    for k in g.timing:
        g.timing[k] = 0
    t0 = time.perf_counter()
    for _ in range(sweeps):
        g.sweep()
        g.log_likelihood()
    dt = (time.perf_counter() - t0) / sweeps
    print("  %-24s %.1f ms per sweep: split + sky %.1f, flux %.1f, location %.1f (%d rounds, %d evaluations per sweep)" % (
        name, 1e3 * dt, 1e3 * g.timing["split"] / sweeps, 1e3 * g.timing["flux"] / sweeps, 1e3 * g.timing["location"] / sweeps,
        g.timing["rounds"] // sweeps, g.timing["evals"] // sweeps))
