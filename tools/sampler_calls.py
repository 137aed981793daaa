#!/usr/bin/env python3
"""What the device samplers return, call by call, for comparing two builds of the library (CEL_HIP_LIBRARY) -- for a change that
should touch their host code only.

    CEL_HIP_LIBRARY=$PWD/tools/bin/a.so python tools/sampler_calls.py a.npz
    python tools/sampler_calls.py b.npz                      (the shipped library)
    python tools/sampler_calls.py --compare a.npz b.npz      (no GPU; exit status 1 when a call differs)
    python tools/sampler_calls.py --launches a_kernel_trace.csv b_kernel_trace.csv       (two rocprofv3 --kernel-trace runs of it)

The scene is tests/test_slice_sample_contract.py's scene A (24 sources, 3 bands, 128 x 128, split seed 5), two chains left out by
chain_ids, one fixed seed.  cel_slice_sample's params 0 (location), 1 (shape), 2 (type move), 3 (HMC step), each under
CEL_OPT_SLICE_CONDITIONAL 0 and 1 (the HMC step is refused under 1: the refusal is the record), param 3 also under
CEL_OPT_GRAD_CONDITIONAL 1; the exact calls on the full-box split of the same seed.  Then cel_slice_locations.  Every call starts
from the scene's catalogue and goes to the C entry point directly: x, llh and all four stats words are kept.  The comparison is bit
for bit, NaNs included; of cel_slice_locations' stats only [0..2] are compared (its queued rounds depend on when the host wakes).
--launches: the ordered (kernel, grid, work-group) lists of two traced runs, up to cel_slice_locations' first launch (k_slice_init)
and over the whole run."""
import ctypes as C
import os
import sys

import numpy as np

S, B, SEED, SPLIT_SEED = 24, 3, 11, 5


def compare(a, b):
    a, b = np.load(a), np.load(b)
    names = sorted(set(a.files) | set(b.files))
    bad = []
    for n in names:
        if n not in a.files or n not in b.files:
            bad.append(n)
            continue
        x, y = a[n], b[n]
        if n == "locations.stats":
            x, y = x[:3], y[:3]
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(n)
    print("sampler calls: %d arrays of %d calls compared, %d differ %s" % (len(names), len(set(n.rsplit(".", 1)[0] for n in names)), len(bad), bad))
    return 1 if bad else 0


def launches(path):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dims = [k for k in rows[0] if k.startswith("Grid_Size") or k.startswith("Workgroup_Size")]
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in dims) for r in rows]


def compare_launches(a, b):
    a, b = launches(a), launches(b)
    cut = [next((i for i, r in enumerate(x) if r[0].startswith("k_slice_init")), len(x)) for x in (a, b)]
    same_head, same_all = a[:cut[0]] == b[:cut[1]], a == b
    print("launches: %d and %d; the two-slot samplers' %d and %d %s; the whole run %s"
          % (len(a), len(b), cut[0], cut[1], "equal" if same_head else "DIFFER", "equal" if same_all else "differs"))
    if not same_head:
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(cut))
        print("first difference at launch %d: %s | %s" % (i, a[i:i + 1], b[i:i + 1]))
    return 0 if same_head else 1


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
if len(sys.argv) == 4 and sys.argv[1] == "--launches":
    sys.exit(compare_launches(sys.argv[2], sys.argv[3]))

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import desi_mcmc_amd as cel  # noqa: E402
from desi_mcmc_amd import _lib as L, synth  # noqa: E402
from desi_mcmc_amd.util.infer.slicesample import ChainStreams  # noqa: E402

ctx = cel.Context(0)
f = synth.SyntheticField(ctx, S, B, 128, 128, frac_gal=0.5)
im, cat, src = f.images, f.sources, f.src
ids = np.random.RandomState(1000 + SEED).permutation(S).astype(np.int32)
ids[[3, 17]] = -1
streams = ChainStreams(SEED, np.where(ids < 0, 0, ids))
rs = np.random.RandomState(7)
out = {}


def split(full_box):
    ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1 if full_box else 0)
    cat.set(src["type"], src["radec"], src["counts"], src["shape"])
    im.photon_split_resident(cat, seed=SPLIT_SEED)
    ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)


def call(name, param, dirs, numdir, D, sigma, rounds, step_out=1, phi_max=180.0, slice_cond=0, grad_cond=0):
    cat.set(src["type"], src["radec"], src["counts"], src["shape"])
    x, llh, stats = np.full((S, D), -7.0), np.full(S, -7.0), np.full(4, -7, dtype=np.int64)
    ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, slice_cond)
    ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, grad_cond)
    rc = L.lib().cel_slice_sample(im._h, cat._h, param, ids.ctypes.data_as(L.c_int32_p), None if dirs is None else L.dptr(dirs), numdir,
                                  step_out, 1000, float(sigma), float(phi_max), C.c_uint64(SEED), rounds, L.dptr(x), L.dptr(llh),
                                  stats.ctypes.data_as(L.c_int64_p))
    ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 0)
    ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, 0)
    out[name + ".x"], out[name + ".llh"], out[name + ".stats"], out[name + ".rc"] = x, llh, stats, np.array([rc])
    print("%-28s rc %d stats %s  llh sum over the finite %.17g" % (name, rc, stats.tolist(), float(np.sum(llh[np.isfinite(llh)]))))


# the type move's rows (theta, sigma, phi, rho, h) and the HMC step's (momentum[6], inverse mass[6])
tm_rows = np.column_stack([rs.uniform(0.2, 0.8, S), rs.uniform(0.5, 3.0, S), rs.uniform(10, 170, S), rs.uniform(0.4, 0.9, S), rs.normal(0, 2, S)])
imass = np.full((S, 6), 1e-3)
imass[:, :2] = 1e-11
hmc_rows = np.ascontiguousarray(np.concatenate([rs.randn(S, 6) / np.sqrt(imass), imass], axis=1))
for cond in (0, 1):
    split(full_box=cond == 1)
    tag = "exact" if cond else "reference"
    call("param0 compwise " + tag, 0, None, 0, 2, 2e-6, 20000, slice_cond=cond)
    call("param0 dirs3 " + tag, 0, L.f64(streams.directions(3, 2)), 3, 2, 1e-3, 20000, slice_cond=cond)
    call("param1 compwise " + tag, 1, None, 0, 4, 0.05, 20000, slice_cond=cond)
    call("param1 dirs2 nostep " + tag, 1, L.f64(streams.directions(2, 4)), 2, 4, 0.05, 20000, step_out=0, slice_cond=cond)
    call("param2 " + tag, 2, tm_rows, 1, 5, 1.0, 1, step_out=0, phi_max=0.0, slice_cond=cond)
    call("param3 " + tag, 3, hmc_rows, 12, 12, 0.3, 3, step_out=0, slice_cond=cond)
    if cond:
        call("param3 exact gradient", 3, hmc_rows, 12, 12, 0.3, 3, step_out=0, grad_cond=1)

split(full_box=False)
radec, llh, stats = np.full((S, 2), -7.0), np.full(S, -7.0), np.full(4, -7, dtype=np.int64)
rc = L.lib().cel_slice_locations(im._h, cat._h, ids.ctypes.data_as(L.c_int32_p), 2e-6, C.c_uint64(SEED), 4000, L.dptr(radec), L.dptr(llh),
                                 stats.ctypes.data_as(L.c_int64_p))
out["locations.x"], out["locations.llh"], out["locations.stats"], out["locations.rc"] = radec, llh, stats, np.array([rc])
print("%-28s rc %d stats %s" % ("locations", rc, stats.tolist()))
np.savez(sys.argv[1], **out)
