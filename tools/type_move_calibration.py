#!/usr/bin/env python3
"""Calibration of the composed sweep with the type step on: is the posterior P(galaxy) the sweep reports the
frequency with which such a source IS a galaxy?

A scene drawn from the model's own priors -- types with prior odds 1, galaxy shapes from the shape prior
(ModelGibbs.sample_shape_prior), fluxes from the flux step's Gamma(a_0, 1 / b_0) prior, locations uniform on the frame,
counts Poisson about the rendered model image -- is swept from the truth with
ModelGibbs(conditional="exact", type_log_odds=0).sweep(shapes=True, types=True); a source's posterior P(galaxy) is the share
of the kept sweeps in which it is one.  Sources are binned by that share into five bins; a calibrated sampler puts the
share of true galaxies of a bin at the bin's mean posterior, within the binomial error -- if the shares were exact.  They are
not: a chain that changes type a dozen times in its run reports a noisy share, and binning by a noisy number overstates the
extremes (regression to the mean).  So the kept sweeps are cut in two halves: sources are binned by the share of the FIRST
half, and the table also gives the share of the SECOND half per bin.  The truth is one more draw from the posterior, as a
state far along the chain is: a calibrated sampler puts the true share at the second half's, whatever the noise of the first.

    python tools/type_move_calibration.py [sources] [sweeps] [scenes]

A record (profiles/type_move_calibration.txt keeps a run), not a gate: too long for a test."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_mcmc, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 150
sweeps = int(args[1]) if len(args) > 1 else 400
scenes = int(args[2]) if len(args) > 2 else 4
B, H, W = 3, 512, 512
A0, B0 = 2.0, 10.0                  # the flux prior: Gamma(2, rate 10), mean 0.2 nanomaggies (about 100 photons per band)
burn = sweeps // 4

post, later, truth = [], [], []
accepted = evals = 0
t0 = time.perf_counter()
for scene in range(scenes):
    ctx = cel.Context(0)
    f = synth.SyntheticField(ctx, S, B, H, W, frac_gal=0.5, seed=100 + scene, with_nelec=False)
    rs = np.random.RandomState(900 + scene)
    src = f.src
    typ = (rs.rand(S) < 0.5).astype(np.int32)
    proto = celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)))
    shape = proto.sample_shape_prior(5000 + scene, np.arange(S))
    pix = np.column_stack([rs.uniform(24, W - 24, S), rs.uniform(24, H - 24, S)])
    radec = synth.pixel2equa(f.bands[0], pix)
    flux5 = rs.gamma(A0, 1.0 / B0, size=(S, 5))
    calib, kappa = f.bands[:, 2], f.bands[:, 1]
    counts = flux5[:, :B] / calib[None, :] * kappa[None, :]
    f.sources.set(typ, radec, counts, shape)
    f.images.render(f.sources, loglik=False)
    nelec = rs.poisson(f.images.model_images()).astype(np.float64)
    f.images.set_nelec(nelec)
    gf = celeste_mcmc.GibbsField(f.images, list(range(B)), calib, kappa, H * W)
    g = celeste_mcmc.ModelGibbs([gf], typ, radec, flux5, shape, seed=7 + scene, flux_a_0=A0, flux_b_0=B0, conditional="exact",
                                type_log_odds=0.0)
    gal = np.zeros((2, S))
    half = burn + (sweeps - burn) // 2
    for k in range(sweeps):
        g.sweep(shapes=True, types=True)
        if k >= burn:
            gal[0 if k < half else 1] += g.typ == 1
    post.append(gal[0] / (half - burn))
    later.append(gal[1] / (sweeps - half))
    truth.append(typ == 1)
    accepted += g.timing["type_accepted"]
    evals += g.timing["type_evals"]
    if scene == 0:
        print("scene 0: median expected photons per (source, band) %.0f; engine of the type step: %s" % (
            np.median(counts), "device" if g._type_engine_on_device() else "host"))
post, later, truth = np.concatenate(post), np.concatenate(later), np.concatenate(truth)
print("%d scenes x %d sources on %d x %d x %d, %d sweeps each from the truth (the first %d dropped); %.1f s" % (
    scenes, S, B, H, W, sweeps, burn, time.perf_counter() - t0))
print("type step: %d proposals, %d accepted (%.2f %%)" % (evals // 2, accepted, 200.0 * accepted / max(evals, 1)))
print("reliability of the posterior P(galaxy), five bins by the share of the first half of the kept sweeps:")
print("  %-14s %8s %16s %16s %16s %10s" % ("bin", "sources", "share, 1st half", "share, 2nd half", "true galaxies", "z"))
edges = [0.0, 0.2, 0.4, 0.6, 0.8, 1.0 + 1e-12]
for lo, hi in zip(edges[:-1], edges[1:]):
    sel = (post >= lo) & (post < hi)
    n = int(sel.sum())
    if n == 0:
        print("  [%.1f, %.1f)     %8d" % (lo, min(hi, 1.0), 0))
        continue
    p, p2, q = post[sel].mean(), later[sel].mean(), truth[sel].mean()
    sd = np.sqrt(max((later[sel] * (1 - later[sel])).sum(), 1e-12)) / n
    print("  [%.1f, %.1f%s     %8d %16.3f %16.3f %16.3f %10.2f" % (lo, min(hi, 1.0), "]" if hi > 1 else ")", n, p, p2, q, (q - p2) / sd))
print("(z: (true share - the second half's share) / the binomial error of the bin at the second half's shares; the second")
print(" half's share carries Monte Carlo error of its own and is correlated with the first half's through the chain's memory)")
