#!/usr/bin/env python3
"""What a mask costs: the field render of BASELINE.json configs[2] (10 000 mixed sources x 5 bands x 2048^2) with 1 % of the
pixels masked (NaN counts) and with none, in one process; the masked twins of the gradient and E-step kernels against their
originals on the same scene; and the streaming rate of the stars2k_4096 render in the same session, to judge k_masked_ll by.

    python tools/masked_ll_cost.py [steps] [--no-stream-leg]

Prints the median step times (driver-timed wall clock of the synchronous call), k_masked_ll's own time (CEL_OPT_PROFILE
events on the dispatch), its bytes / time against 8 TB/s and against the streaming leg, and one line each for cel_loglik_grad
and cel_estep_stats.  Diagnostic; not part of bench.py's contract (profiles/masked_ll_time.txt keeps a run)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 20
ctx = cel.Context(0)
f = synth.SyntheticField.from_config(ctx, "mixed10k_2048")
mask = np.random.RandomState(5).rand(f.B, f.H, f.W) < 0.01
masked = cel.ImageSet(ctx, f.bands, f.H, f.W, nelec=np.where(mask, np.nan, f.nelec))
print("mixed10k_2048: S = %d, B = %d, %d x %d; masked pixels per band %s" % (f.S, f.B, f.H, f.W, masked.masked.tolist()))


def wall(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * np.median(ts), 1e3 * np.min(ts)


def events(fn, names):
    ctx.profile(True)
    for _ in range(n):
        fn()
    out = {k: ctx.profile_get(k) for k in names}
    ctx.profile(False)
    return out


npix = f.B * f.H * f.W
sets = (("unmasked", f.images), ("1 % masked", masked))
print("render + loglik, median (min) of %d steps:" % n)
for label, im in sets:
    med, mn = wall(lambda: im.render(f.sources, loglik=True))
    print("  %-12s %8.4f ms (%8.4f)" % (label, med, mn))
for label, im in sets:
    ev = events(lambda: im.render(f.sources, loglik=True), ("render", "reduce", "masked_ll"))
    print("  %-12s events, mean ms (launches): " % label + ", ".join("%s %.4f (%d)" % (k, v[0], v[1]) for k, v in ev.items()))
    if label != "unmasked":
        ms = ev["masked_ll"][0]
        rate = 16.0 * npix / (ms * 1e-3) / 1e12
        print("  k_masked_ll: %.4f ms for %.0f MB (16 B per pixel) = %.2f TB/s = %.2f of 8 TB/s" % (ms, 16.0 * npix / 1e6, rate, rate / 8.0))
        k_ms = ms

for name, call, key in (("loglik_grad", lambda im: im.loglik_grad(f.sources), "grad"), ("estep_stats", lambda im: im.estep_stats(f.sources), "estep")):
    row = []
    for label, im in sets:
        med, _ = wall(lambda: call(im))
        ev = events(lambda: call(im), (key,))
        row.append("%s %.3f ms (call %.3f)" % (label, ev[key][0], med))
    print("%s kernels, original against masked twin: %s" % (name, "; ".join(row)))

if "--no-stream-leg" not in sys.argv:
    masked.close()
    f.images.close()
    g = synth.SyntheticField.from_config(ctx, "stars2k_4096")
    ev = events(lambda: g.images.render(g.sources, loglik=True), ("render", "render_stars"))
    ms = max(ev["render"][0], ev["render_stars"][0])
    bytes_ = 16.0 * g.B * g.H * g.W
    rate = bytes_ / (ms * 1e-3) / 1e12
    print("stars2k_4096 render kernel: %.4f ms for %.0f MB = %.2f TB/s; k_masked_ll at that rate would take %.4f ms, it took %.4f (x %.2f)"
          % (ms, bytes_ / 1e6, rate, 16.0 * npix / (rate * 1e12) * 1e3, k_ms, k_ms / (16.0 * npix / (rate * 1e12) * 1e3)))
