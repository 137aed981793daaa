#!/usr/bin/env python3
"""What a gradient costs (cel_loglik_grad) next to a plain render on the same field: BASELINE.json configs[2] by default
(10 000 mixed sources x 5 bands x 2048^2, the benchmark field).

    python tools/time_loglik_grad.py [workload] [calls]

Prints, per call: the driver-timed wall clock (host perf_counter around the synchronous call) of a gradient and of a
render with the log-likelihood, and the HIP-event times of their kernels (CEL_OPT_PROFILE = 1: k_grad_src + k_grad_chain
as one bracket, the render's kernels by name).  Diagnostic; not part of bench.py's contract."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import synth  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "mixed10k_2048"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ctx = cel.Context(0)
f = synth.SyntheticField.from_config(ctx, name)
print("workload %s: S = %d, B = %d, %d x %d" % (name, f.S, f.B, f.H, f.W))


def wall(fn):
    fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * np.median(ts), 1e3 * np.min(ts)


render = lambda: f.images.render(f.sources, loglik=True)        # noqa: E731
grad = lambda: f.images.loglik_grad(f.sources)                   # noqa: E731
r_med, r_min = wall(render)
g_med, g_min = wall(grad)
print("driver-timed, median (min) of %d calls:" % n)
print("  render + loglik        %8.3f ms (%8.3f)" % (r_med, r_min))
print("  loglik_grad            %8.3f ms (%8.3f)   (render + loglik inside it)" % (g_med, g_min))

ctx.profile(True)
for _ in range(n):
    render()
rk = {k: ctx.profile_get(k) for k in ("prep", "bin", "render", "reduce")}
ctx.profile(True)
for _ in range(n):
    grad()
gk = {k: ctx.profile_get(k) for k in ("prep", "bin", "render", "reduce", "grad")}
ctx.profile(False)
print("CEL_OPT_PROFILE events, mean ms per launch (launches):")
print("  render call:  " + ", ".join("%s %.3f (%d)" % (k, v[0], v[1]) for k, v in rk.items()))
print("  grad call:    " + ", ".join("%s %.3f (%d)" % (k, v[0], v[1]) for k, v in gk.items()))
print("  k_grad_src + k_grad_chain per gradient: %.3f ms; render kernel per render: %.3f ms; ratio %.2f"
      % (gk["grad"][0], rk["render"][0], gk["grad"][0] / rk["render"][0]))
st = f.images.stats()
print("work: n_srcpix %.4g, n_gauss %.4g (Gaussian-pixels the gradient kernel tests)" % (st["n_srcpix"], st["n_gauss"]))
