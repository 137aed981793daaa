#!/usr/bin/env python3
"""Cost of the gradient form of the conditional log-likelihoods (cel_patch_loglik_multi, mode = 8 + m; k_patch_grad.h) on the
benchmark field (BASELINE configs[2], mixed10k_2048) with a resident split.  Diagnostic; not part of bench.py's contract.

    python tools/time_patch_grad.py [config] > profiles/patch_grad_time.txt

Every figure is the median of REPS calls after WARM warm-up calls (min and max beside it); wall-clock around the blocking call,
and for the device part the library's own event brackets (CEL_OPT_PROFILE) under CEL_K_PATCH_LL.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import celeste_galaxy_conditionals as gc  # noqa: E402
from desi_mcmc_amd import synth  # noqa: E402

WARM, REPS = 3, 15
ctx = cel.Context(0)
name = sys.argv[1] if len(sys.argv) > 1 else "mixed10k_2048"
f = synth.SyntheticField.from_config(ctx, name)
print("%s: %d sources, %d bands, %d x %d; median of %d calls after %d warm-up calls (min .. max)" % (name, f.S, f.B, f.H, f.W, REPS, WARM))


def timed(label, fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    print("%-58s %9.3f ms  (%.3f .. %.3f)" % (label, np.median(ts), min(ts), max(ts)))
    return out


def device_ms(fn, reps=REPS):
    """median of the time inside the CEL_K_PATCH_LL brackets of one call (profile_get gives the mean per bracket and their number)"""
    ms = []
    for _ in range(reps):
        ctx.profile(True)
        fn()
        mean, n = ctx.profile_get("patch_ll")
        ms.append(mean * n)
    ctx.profile(False)
    return np.median(ms), min(ms), max(ms)


# ---- the resident forms, one proposal per source (every source moved by ~0.2 px) ------------------------------------------
f.images.photon_split_resident(f.sources, seed=1)
rs = np.random.RandomState(0)
owner = np.arange(f.S, dtype=np.int32)
prop = cel.SourceSet(ctx, f.S, f.B).set(f.src["type"], f.src["radec"] + rs.normal(0.0, 2e-5, size=(f.S, 2)), f.src["counts"], f.src["shape"])
timed("resident mode 0 (value), %d proposals" % f.S, lambda: f.images.patch_loglik_resident(prop, owner))
timed("resident mode 8 (value + gradient), %d proposals" % f.S, lambda: f.images.patch_loglik_resident_grad(prop, owner))
d0 = device_ms(lambda: f.images.patch_loglik_resident(prop, owner))
d8 = device_ms(lambda: f.images.patch_loglik_resident_grad(prop, owner))
print("  device, CEL_K_PATCH_LL brackets: mode 0 %.3f ms (%.3f .. %.3f); mode 8 %.3f ms (%.3f .. %.3f); the gradient kernels alone ~ %.3f ms"
      % (d0 + d8 + (d8[0] - d0[0],)))
timed("resident mode 1 (value), %d proposals" % f.S, lambda: f.images.patch_loglik_resident(prop, owner, isolated=True))
timed("resident mode 9 (value + gradient), %d proposals" % f.S, lambda: f.images.patch_loglik_resident_grad(prop, owner, isolated=True))
d1 = device_ms(lambda: f.images.patch_loglik_resident(prop, owner, isolated=True))
d9 = device_ms(lambda: f.images.patch_loglik_resident_grad(prop, owner, isolated=True))
print("  device, CEL_K_PATCH_LL brackets: mode 1 %.3f ms (%.3f .. %.3f); mode 9 %.3f ms (%.3f .. %.3f); the gradient kernels alone ~ %.3f ms"
      % (d1 + d9 + (d9[0] - d1[0],)))

# ---- the HMC case: one source x five bands --------------------------------------------------------------------------------
gal = np.nonzero(f.src["type"] == 1)[0]
sig = f.src["shape"][gal, 1]
typical, largest = gal[np.argsort(sig)[len(gal) // 2]], gal[np.argmax(sig)]
images = synth.fits_images(f)
for label, s in (("typical", typical), ("largest", largest)):
    one = cel.SourceSet(ctx, 1, f.B).set(f.src["type"][s:s + 1], f.src["radec"][s:s + 1], f.src["counts"][s:s + 1], f.src["shape"][s:s + 1])
    Z_s, limits, keep, npx = [], [], [], 0
    for b in range(f.B):
        st, bx = f.images.stamps(one, b, scaled=True)
        if st[0] is None:
            continue
        Z_s.append(np.random.RandomState(100 + b).poisson(st[0]).astype(np.float64))
        limits.append(((int(bx[0, 0]), int(bx[0, 1])), (int(bx[0, 2]), int(bx[0, 3]))))
        keep.append(images[b])
        npx += st[0].size
    flux5 = np.zeros(5)
    flux5[:f.B] = f.src["flux"][s]
    th = np.concatenate([f.src["shape"][s], f.src["radec"][s], flux5])
    print("galaxy %d (%s: sigma %.2f arcsec, %d images, %d patch pixels)" % (s, label, f.src["shape"][s, 1], len(keep), npx))
    timed("  galaxy_source_like_grad, default (10 differences / image)", lambda: gc.galaxy_source_like_grad(th, Z_s, keep, limits=limits))
    timed("  galaxy_source_like_grad, analytic=True", lambda: gc.galaxy_source_like_grad(th, Z_s, keep, limits=limits, analytic=True))
    boxes = np.array([[lim[0][0], lim[0][1], lim[1][0], lim[1][1]] for lim in limits], dtype=np.int32)
    if len(keep) == f.B:
        timed("  one mode-10 launch, all %d bands (patch_loglik_grad)" % f.B, lambda: f.images.patch_loglik_grad(one, boxes, Z_s, mode=2))
        d = device_ms(lambda: f.images.patch_loglik_grad(one, boxes, Z_s, mode=2))
        print("    device, CEL_K_PATCH_LL brackets: %.3f ms (%.3f .. %.3f)" % d)
