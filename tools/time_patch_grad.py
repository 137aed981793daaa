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

import argparse  # noqa: E402
from desi_mcmc_amd import _lib  # noqa: E402

WARM, REPS = 3, 15
ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="mixed10k_2048")
ap.add_argument("--route", choices=("dense", "photons", "both"), default="dense",
                help="where the resident mode-8 gradient is summed (CEL_OPT_PHOTON_LISTS + 4 = photons); both: the two routes "
                     "interleaved call by call in this process, and nothing else")
args = ap.parse_args()
ctx = cel.Context(0)
name = args.config
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
lists0 = ctx.get_option(_lib.CEL_OPT_PHOTON_LISTS)


def set_route(route):
    ctx.set_option(_lib.CEL_OPT_PHOTON_LISTS, lists0 + (4 if route == "photons" else 0))


if args.route == "both":
    # the two routes call by call: warm-up calls of each, then REPS pairs; wall-clock and the CEL_K_PATCH_LL brackets of the same calls
    wall, devms, rows = {"dense": [], "photons": []}, {"dense": [], "photons": []}, {}
    for k in range(WARM + REPS):
        for route in ("dense", "photons"):
            set_route(route)
            ctx.profile(True)
            t0 = time.perf_counter()
            rows[route] = f.images.patch_loglik_resident_grad(prop, owner)
            dt = (time.perf_counter() - t0) * 1e3
            mean, n = ctx.profile_get("patch_ll")
            if k >= WARM:
                wall[route].append(dt)
                devms[route].append(mean * n)
    ctx.profile(False)
    set_route("dense")
    val = [(time.perf_counter(), f.images.patch_loglik_resident(prop, owner), time.perf_counter()) for _ in range(WARM + REPS)][WARM:]
    vms = [(c - a) * 1e3 for a, _, c in val]
    print("%-58s %9.3f ms  (%.3f .. %.3f)" % ("resident mode 0 (value), %d proposals" % f.S, np.median(vms), min(vms), max(vms)))
    for route in ("dense", "photons"):
        print("%-58s %9.3f ms  (%.3f .. %.3f)   device, CEL_K_PATCH_LL brackets: %.3f ms (%.3f .. %.3f)"
              % ("resident mode 8, %s route, %d proposals" % (route, f.S), np.median(wall[route]), min(wall[route]), max(wall[route]),
                 np.median(devms[route]), min(devms[route]), max(devms[route])))
    spread = max(max(wall[r]) - min(wall[r]) for r in wall)
    gain = np.median(wall["dense"]) - np.median(wall["photons"])
    print("dense - photons = %.3f ms; the larger of the two runs' own ranges = %.3f ms: %s"
          % (gain, spread, "the photon route is faster by more than that" if gain > spread else "NOT separated"))
    a, b = [np.column_stack(r[1:]) for r in (rows["dense"], rows["photons"])]
    print("largest |dense - photons| / column max over the rows: %.3g; values equal bit for bit: %s"
          % (np.max(np.abs(a - b) / np.max(np.abs(a), axis=0)), np.array_equal(rows["dense"][0], rows["photons"][0])))
    sys.exit(0)
set_route(args.route)
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
