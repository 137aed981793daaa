"""The device slice samplers, chain by chain, against the oracle's scalar restatement of the reference's `slicesample`.

ImageSet.slice_sample (cel_slice_sample, k_slice_gen.h: random directions, stepping out by doubling, the `acceptable` test,
the built-in shape prior, two proposal slots per chain) and ImageSet.slice_locations (cel_slice_locations, k_slice.h) are held
to oracle.slicesample_oracle.scalar_slicesample -- pinned bit for bit to a recorded run of the reference
(tests/test_slicesample.py) -- fed with

    the chain's own stream      ChainStreams(seed, ids), chain = the row; with `dirs`, ChainStreams(seed, ids).directions(numdir, D)
                                as ModelGibbs.resample_shapes draws them
    the device's own scorer     patch_loglik_resident of a ONE-row proposal set against the same resident split (bit-identical
                                however its jobs are dealt: test_conditional_loglik_does_not_depend_on_how_its_jobs_are_dealt); for
                                shapes plus galaxy_shape_prior_constrained(..., phi_max), -inf without a launch outside its support

and must return, bit for bit, `x` and `llh` of every chain that ran; the untouched row and a NaN `llh` of every chain that did
not; stats["evals"] = the points the chains asked for (1 for the first direction's level, 2 per round of the doubling loop, 1
per shrink step, 2 per halving of `acceptable` that looks at its ends -- points outside the prior included); stats["rounds"] =
slicesample_lockstep's on the same scorer.  Every option set asserts from the oracle's trace (scalar_slicesample(trace=)) that
it went where it claims to go, so that a trajectory match cannot pass vacuously.

Scene A: synth.SyntheticField(ctx, 24, 3, 128, 128, frac_gal=0.5), resident split of seed 5.  Every set at seeds 11 and 12,
chain ids a permutation of arange(24) with 8 of them -1 (those rows stay put and draw nothing).  Coverage summed over the seeds:

    param 0 (locations)
      wide              compwise, sigma 1e-3, step out / no step out
      narrow            compwise, sigma 2e-6, step out                 doubling set
      narrower          compwise, sigma 3e-7, step out                 doubling set
      dirs3             dirs numdir 3, sigma 2e-6, step out            doubling set
      cap2              compwise, sigma 3e-7, max_steps_out 2          capped set
      cap0              compwise, sigma 3e-7, max_steps_out 0          capped set (every direction, no doubling)
    param 1 (shapes), phi_max 180
      skew              dirs numdir 4, sigma 1.0, step out             prior set (slice_sample_skew's own call)
      compwise          compwise, sigma 0.05, step out                 doubling set, prior set
      cap3              dirs numdir 2, sigma 0.02, max_steps_out 3     capped set
      nostep            dirs numdir 3, sigma 0.05, no step out
      nostep, phi_max 0 the same without the prior

    doubling set: at least half the directions double three or more times;  capped set: at least half hit the cap;
    prior set: at least 20 points outside the support, a pair of interval ends with one of them outside and one with both

Scene B (two clumps): the same frame with nelec zero except two pixels per star, 3 photons each in every band, SEP = 8 pixels
apart along x about the star's pixel, every band's epsilon 1e-12; component-wise, stepping out, SIGMA_B = 2e-4 degrees.

MEASURED on the device, summed over the two seeds (directions; that doubled at all / three or more times / most doublings;
that hit the cap; halvings of `acceptable` that looked at their ends / most halvings; points outside the prior; pairs of ends
with one / both outside):

    param 0 wide        64;   0 /  0 /  0;   0;    0 /  0          (the no-step-out form: the same)
            narrow      64;  63 / 49 / 10;   0;   69 / 10
            narrower    64;  64 / 64 / 14;   0;  150 / 14
            dirs3       96;  94 / 71 / 15;   0;  111 / 15
            cap2        64;  64 /  0 /  2;  64;   66 /  2
            cap0        64;   0 /  0 /  0;  64;    0 /  0
    param 1 skew        60;  13 /  3 /  5;   0;    5 /  5;  134;  55 / 14
            compwise    60;  57 / 42 / 17;   0;  118 / 17;   79;  69 / 10
            cap3        30;  30 / 29 /  3;  24;   35 /  3;    5;   5 /  0
            nostep      45;   0 /  0 /  0;   0;    0 /  0;    0            (without the prior: the same)
    scene B            480 directions, 8 rejections by `acceptable` (see test_two_clumps_reject_in_acceptable)

`acceptable` rejects in scene B alone.  Of the three wrong libraries the contract was tried on, one computes something else:
`(l_out + u_out) <= max_steps_out` in k_sg_consume fails cap2, cap0 and cap3 (and passed the suite as it stood).  The other
two compute the same: `z > middle` for `z >= middle` in sg_accept_advance differs where a new point falls ON a middle -- the
halving then makes the point the interval's lower end, which is inside the slice, so the look at the ends cannot reject --
and the two ends of SG_ACCEPT swapped in k_sg_propose feed a test that is symmetric in them (and a prior slot that is swapped
with them).
"""
import numpy as np
import pytest

import desi_mcmc_amd  # noqa: F401
from desi_mcmc_amd.util.infer.slicesample import ChainStreams, slicesample_lockstep
from oracle.slicesample_oracle import DRAW_RAND, ReplayStream, scalar_slicesample

gpu = pytest.mark.gpu
S = 24
SPLIT_SEED = 5
SEEDS = (11, 12)
SEP, SIGMA_B, SEEDS_B = 8, 2e-4, (744, 1040, 1447, 2087, 2128)


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def clump_pixels(boxes, pix, sep):
    """the two pixels (xa, xb, y) of a star's clumps: `sep` apart along x about the star's pixel, moved along x where the
    frame cuts the star's box, strictly inside the box of every band (boxes (B, 4) = y0, y1, x0, x1); None: no room"""
    y0, y1, x0, x1 = boxes[:, 0].max(), boxes[:, 1].min(), boxes[:, 2].max(), boxes[:, 3].min()
    cx, cy = int(np.floor(pix[0])), int(np.floor(pix[1]))
    xa = cx - sep // 2
    xb = xa + sep
    if xa < x0 + 1:
        xa, xb = x0 + 1, x0 + 1 + sep
    if xb > x1 - 2:
        xa, xb = x1 - 2 - sep, x1 - 2
    cy = min(max(cy, y0 + 1), y1 - 2)
    if xa < x0 + 1 or not (y0 + 1 <= cy <= y1 - 2):
        return None
    return int(xa), int(xb), int(cy)


class Scene(object):
    """a synthetic field with a resident split, the one-row scorer over it and the oracle's runs, each computed once"""

    def __init__(self, cel, B=3, H=128, W=128, clump_sep=None, bands=None):
        from desi_mcmc_amd import synth
        self.cel, self.ctx, self.B = cel, cel.default_context(0), B
        f = self.f = synth.SyntheticField(self.ctx, S, B, H, W, frac_gal=0.5, with_nelec=clump_sep is None, bands=bands)
        self.src = f.src
        self.clumps = {}
        if clump_sep is not None:
            boxes, status = f.images.source_boxes(f.sources)
            nelec = np.zeros((B, H, W))
            for s in np.nonzero(self.src["type"] == 0)[0]:
                at = clump_pixels(boxes[:, s], self.src["pix"][s], clump_sep) if np.all(status[:, s] > 0) else None
                if at is not None:
                    self.clumps[int(s)] = at
                    nelec[:, at[2], at[0]] += 3.0
                    nelec[:, at[2], at[1]] += 3.0
            f.images.set_nelec(nelec)
            for b in range(B):
                f.images.set_epsilon(b, 1e-12)
        self.split()
        self.has_patch = f.images.sample_box_areas().sum(axis=1) > 0
        self.prop = cel.SourceSet(self.ctx, 16, B)
        self.values, self.runs, self.launches = {}, {}, 0

    def split(self):
        self.f.images.photon_split_resident(self.f.sources, seed=SPLIT_SEED)

    def reset(self):
        """the catalogue back at the start: both samplers move it in place"""
        self.f.sources.set(self.src["type"], self.src["radec"], self.src["counts"], self.src["shape"])

    def score(self, param, phi_max, s, x):
        """log-probability of chain s at x: the device's conditional log-likelihood of a one-row proposal (+ the shape prior)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = (param, phi_max, int(s), x.tobytes())
        v = self.values.get(key)
        if v is None:
            lp = 0.0
            if param and phi_max > 0.0:
                from desi_mcmc_amd.celeste_galaxy_conditionals import galaxy_shape_prior_constrained
                lp = float(galaxy_shape_prior_constrained(x[0], x[1], x[2], x[3], phi_max))
            if lp == -np.inf:
                v = -np.inf
            else:
                src = self.src
                self.prop.set(src["type"][s:s + 1], src["radec"][s:s + 1] if param else x[None, :], src["counts"][s:s + 1],
                              x[None, :] if param else src["shape"][s:s + 1])
                self.launches += 1
                v = lp + float(self.f.images.patch_loglik_resident(self.prop, np.array([s], dtype=np.int32))[0])
            self.values[key] = v
        return v

    def oracle(self, param, ids, seed, sigma, numdir=None, step_out=True, max_steps_out=1000, phi_max=180.):
        """-> dict(x, llh, ran, evals, rounds, dirs (the trace's direction records of every chain that ran))"""
        key = (param, ids.tobytes(), seed, sigma, numdir, step_out, max_steps_out, phi_max)
        if key in self.runs:
            return self.runs[key]
        x0 = self.src["shape" if param else "radec"]
        ran = (ids >= 0) & self.has_patch & ((self.src["type"] == 1) if param else True)
        clean = np.where(ids < 0, 0, ids)
        kw = dict(sigma=sigma, step_out=step_out, max_steps_out=max_steps_out, compwise=numdir is None, numdir=numdir or 2)
        streams = ChainStreams(seed, clean)
        x, llh, recs, evals = x0.copy(), np.full(S, np.nan), [], 0
        for s in np.nonzero(ran)[0]:
            tr = {}
            x[s], llh[s] = scalar_slicesample(x0[s].copy(), lambda p, s=s: self.score(param, phi_max, s, p), streams, s, trace=tr, **kw)
            recs += tr["directions"]
            evals += 1 + sum(2 * d["out_rounds"] + d["shrinks"] + 2 * d["end_pairs"] for d in tr["directions"])
        # the rounds of a lock-step run: the product's numpy engine on the same scorer (and the same trajectory, or the oracle
        # and the engine disagree before the device is asked)
        idx, st = np.nonzero(ran)[0], {}
        X, LL = slicesample_lockstep(x0[idx], lambda i, P: np.array([self.score(param, phi_max, idx[k], p) for k, p in zip(i, P)]),
                                     seed=seed, chain_ids=clean[idx], stats=st, **kw)
        assert np.array_equal(X, x[idx]) and np.array_equal(LL, llh[idx]) and st["evals"] == evals
        out = self.runs[key] = dict(x=x, llh=llh, ran=ran, evals=evals, rounds=st["rounds"], dirs=recs)
        return out

    def device(self, param, ids, seed, sigma, numdir=None, step_out=True, max_steps_out=1000, phi_max=180., resplit=False):
        self.reset()
        if resplit:
            self.split()
        dirs = None if numdir is None else ChainStreams(seed, np.where(ids < 0, 0, ids)).directions(numdir, 4 if param else 2)
        return self.f.images.slice_sample(self.f.sources, param, sigma, seed, dirs=dirs, step_out=step_out, max_steps_out=max_steps_out,
                                          phi_max=phi_max, chain_ids=ids)

    def check(self, got, want, param, what=""):
        x, llh, st = got
        ran, x0 = want["ran"], self.src["shape" if param else "radec"]
        assert ran.any()
        bad = np.nonzero(ran & (np.any(x != want["x"], axis=1) | (llh != want["llh"])))[0]
        assert bad.size == 0, (what, bad, x[bad], want["x"][bad], llh[bad], want["llh"][bad])
        assert np.array_equal(x[~ran], x0[~ran]) and np.all(np.isnan(llh[~ran])), what
        assert st["evals"] == want["evals"] and st["rounds"] == want["rounds"], (what, st, want["evals"], want["rounds"])
        now = self.f.sources.get()                   # the catalogue on the device moved with the chains, and nothing else did
        assert np.array_equal(now[3 if param else 1], x) and np.array_equal(now[1 if param else 3], self.src["radec" if param else "shape"])


def chain_ids(seed, n_out=S // 3):
    rs = np.random.RandomState(1000 + seed)
    ids = rs.permutation(S).astype(np.int32)
    ids[rs.permutation(S)[:n_out]] = -1
    return ids


def coverage(recs, what):
    n = len(recs)
    fig = dict(directions=n, doubled=sum(d["doublings"] > 0 for d in recs), doubled3=sum(d["doublings"] >= 3 for d in recs),
               most_doublings=max(d["doublings"] for d in recs), capped=sum(d["capped"] for d in recs),
               accept_calls=sum(d["accept_calls"] for d in recs), end_pairs=sum(d["end_pairs"] for d in recs),
               rejections=sum(d["rejections"] for d in recs), most_halvings=max(d["max_halvings"] for d in recs),
               outside=sum(d["outside"] for d in recs), one_outside=sum(d["pairs_one_outside"] for d in recs),
               both_outside=sum(d["pairs_both_outside"] for d in recs))
    print("COVERAGE %s: %s" % (what, fig))
    return fig


def assert_coverage(fig, kinds):
    if "doubling" in kinds:
        assert 2 * fig["doubled3"] >= fig["directions"], fig
    if "capped" in kinds:
        assert 2 * fig["capped"] >= fig["directions"], fig
    if "prior" in kinds:
        assert fig["outside"] >= 20 and fig["one_outside"] >= 1 and fig["both_outside"] >= 1, fig


@pytest.fixture(scope="module")
def scene_a(cel):
    return Scene(cel)


LOCATION_SETS = {
    "wide": (dict(sigma=1e-3), ()),
    "wide_nostep": (dict(sigma=1e-3, step_out=False), ()),
    "narrow": (dict(sigma=2e-6), ("doubling",)),
    "narrower": (dict(sigma=3e-7), ("doubling",)),
    "dirs3": (dict(sigma=2e-6, numdir=3), ("doubling",)),
    "cap2": (dict(sigma=3e-7, max_steps_out=2), ("capped",)),
    "cap0": (dict(sigma=3e-7, max_steps_out=0), ("capped",)),
}
SHAPE_SETS = {
    "skew": (dict(sigma=1.0, numdir=4), ("prior",)),
    "compwise": (dict(sigma=0.05), ("doubling", "prior")),
    "cap3": (dict(sigma=0.02, numdir=2, max_steps_out=3), ("capped",)),
    "nostep": (dict(sigma=0.05, numdir=3, step_out=False), ()),
    "nostep_noprior": (dict(sigma=0.05, numdir=3, step_out=False, phi_max=0.0), ()),
}


def run_sets(scene, param, name, opts, kinds, seeds=SEEDS):
    recs = []
    for seed in seeds:
        ids = chain_ids(seed)
        want = scene.oracle(param, ids, seed, **opts)
        scene.check(scene.device(param, ids, seed, **opts), want, param, (name, seed))
        recs += want["dirs"]
    fig = coverage(recs, "param %d %s" % (param, name))
    if opts.get("max_steps_out") == 0:
        assert fig["capped"] == fig["directions"] and fig["doubled"] == 0
    assert_coverage(fig, kinds)
    return fig


@gpu
@pytest.mark.parametrize("name", list(LOCATION_SETS))
def test_locations_through_the_general_sampler_follow_the_oracle(cel, scene_a, name):
    """param = 0 on scene A: every chain of cel_slice_sample takes the reference's trajectory, with stepping out and without,
    component-wise and along random directions, through many doublings and long `acceptable` loops, and stopped by the cap"""
    opts, kinds = LOCATION_SETS[name]
    run_sets(scene_a, 0, name, opts, kinds)


@gpu
@pytest.mark.parametrize("name", list(SHAPE_SETS))
def test_shapes_follow_the_oracle(cel, scene_a, name):
    """param = 1 on scene A: the galaxies' (theta, sigma, phi, rho) with the built-in prior (points outside its support are
    counted and never scored, one slot of a pair or both) and without it; the stars' rows stay put"""
    opts, kinds = SHAPE_SETS[name]
    fig = run_sets(scene_a, 1, name, opts, kinds)
    if opts.get("phi_max", 180.) <= 0:
        assert fig["outside"] == 0


@gpu
def test_two_clumps_reject_in_acceptable(cel):
    """Scene B: a clump star's location posterior has a mode at one clump and a shoulder or a second mode at the other, the
    only way `acceptable` can reject (the slice has to come apart between the start point and the new one, and a middle of
    the halving has to fall into the gap).  Every trajectory must match, and the seeds' rejections add up to at least 5.

    CHOSEN: SEP = 8 pixels, SIGMA_B = 2e-4 degrees -- the ends of the contract's ranges -- and the seeds SEEDS_B.
    MEASURED on the device (the oracle on the device's scorer, split of seed 5, which leaves the twelve clump stars 9 to 22
    of the 18 photons laid down for each: neighbouring sources share the clump pixels): rejections are rare.  Seeds 1 ... 3 000
    at SEP 8 / SIGMA 2e-4: 17 rejections in 14 seeds (867 000 evaluations); SIGMA 1e-4, seeds 1 ... 1 124: 8 in 8 seeds;
    SEP 7 / SIGMA 2e-4, seeds 1 ... 1 280: none.  (With the oracle's patch_loglik as scorer on a split that gives every photon
    to its star: 3 rejections in 300 seeds at SEP 8 / SIGMA 2e-4, none at 5e-5 ... 1.5e-4 nor at SEP 7 or 6; the PSF's skewed
    wide component leaves one mode and a shoulder 2.2 below it.)  The seeds are therefore the contract's "move the seed":
    744, 1040, 1447, 2087, 2128 are five of the 14 and hold 1 + 2 + 1 + 2 + 2 = 8 rejections in 480 directions."""
    scene = Scene(cel, clump_sep=SEP)
    rows = np.array(sorted(scene.clumps))
    assert rows.size >= 10
    sums = scene.f.images.sample_sums()
    print("scene B: photons of the clump stars (18 laid down for each): %s" % dict(zip(rows.tolist(), sums[rows].sum(axis=1).tolist())))
    assert np.all(sums[rows].sum(axis=1) <= 18.0 * 2) and sums[rows].sum() > 0
    ids = np.full(S, -1, dtype=np.int32)
    live = rows[sums[rows].sum(axis=1) > 0]                # (a star whose patch holds no photon has a flat posterior)
    ids[live] = live
    recs = []
    for seed in SEEDS_B:
        want = scene.oracle(0, ids, seed, sigma=SIGMA_B)
        scene.check(scene.device(0, ids, seed, sigma=SIGMA_B), want, 0, ("clumps", seed))
        recs += want["dirs"]
    fig = coverage(recs, "scene B sep %d sigma %g" % (SEP, SIGMA_B))
    assert fig["rejections"] >= 5, fig


@gpu
def test_the_location_engines_agree(cel, scene_a):
    """cel_slice_locations and cel_slice_sample(param 0, component-wise, no stepping out) on a fresh identical split with the
    same seed: the same `u` and `llh` bit for bit, both the oracle's"""
    for seed in SEEDS:
        ids = chain_ids(seed)
        want = scene_a.oracle(0, ids, seed, sigma=1e-3, step_out=False)
        scene_a.reset()
        scene_a.split()
        u, llh, st = scene_a.f.images.slice_locations(scene_a.f.sources, 1e-3, seed, chain_ids=ids)
        scene_a.check((u, llh, st), want, 0, ("slice_locations", seed))
        g = scene_a.device(0, ids, seed, sigma=1e-3, step_out=False, resplit=True)
        scene_a.check(g, want, 0, ("slice_sample", seed))
        assert np.array_equal(g[0], u) and np.array_equal(g[1], llh, equal_nan=True)


@gpu
@pytest.mark.parametrize("B,size", [(1, 128), (16, 96)])
def test_band_counts_one_and_sixteen(cel, B, size):
    """one band, and MAX_BANDS = 16 (k_slice_step runs 1024-thread blocks): both samplers against the oracle"""
    scene = Scene(cel, B=B, H=size, W=size)
    seed = SEEDS[0]
    ids = chain_ids(seed)
    want = scene.oracle(0, ids, seed, sigma=1e-3, step_out=False)
    scene.reset()
    scene.check(scene.f.images.slice_locations(scene.f.sources, 1e-3, seed, chain_ids=ids), want, 0, "slice_locations")
    for param, opts in ((0, dict(sigma=2e-6)), (1, dict(sigma=0.05, numdir=2))):
        scene.check(scene.device(param, ids, seed, **opts), scene.oracle(param, ids, seed, **opts), param, (B, param))


@gpu
def test_the_direct_evaluator_backs_the_samplers(cel):
    """CEL_OPT_KERNEL = 0 (k_patch_ll<int>, one slot per job): a location set and a shape set, the oracle's scorer taken under
    the same option"""
    from desi_mcmc_amd import _lib
    ctx = cel.default_context(0)
    before = ctx.get_option(_lib.CEL_OPT_KERNEL)
    ctx.set_kernel("direct")
    try:
        scene = Scene(cel)
        seed = SEEDS[1]
        ids = chain_ids(seed)
        for param, opts in ((0, dict(sigma=2e-6)), (1, dict(sigma=0.05))):
            scene.check(scene.device(param, ids, seed, **opts), scene.oracle(param, ids, seed, **opts), param, ("direct", param))
    finally:
        ctx.set_option(_lib.CEL_OPT_KERNEL, before)


@gpu
def test_the_direct_evaluator_backs_the_location_step(cel):
    """CEL_OPT_KERNEL = 0 under cel_slice_locations (its rounds score through the same launch as cel_slice_sample's): the
    oracle's run on the scorer taken under the same option, bit for bit as under the recurrence kernels"""
    from desi_mcmc_amd import _lib
    ctx = cel.default_context(0)
    before = ctx.get_option(_lib.CEL_OPT_KERNEL)
    ctx.set_kernel("direct")
    try:
        scene = Scene(cel)
        seed = SEEDS[1]
        ids = chain_ids(seed)
        want = scene.oracle(0, ids, seed, sigma=1e-3, step_out=False)
        scene.reset()
        scene.check(scene.f.images.slice_locations(scene.f.sources, 1e-3, seed, chain_ids=ids), want, 0, ("direct", "slice_locations"))
    finally:
        ctx.set_option(_lib.CEL_OPT_KERNEL, before)


@gpu
def test_failures_come_back_as_the_reference_raises_them(cel, scene_a):
    """a NaN log-likelihood (a NaN among one row's expected counts) and too few rounds come back as the reference's plain
    Exception("Slice sampler got a NaN") / as ValueError, from both samplers; the image set is as good as new afterwards.
    "Slice sampler shrank to zero!" is not provoked: new_z == 0 needs an interval that has collapsed onto the start point,
    and a point within rounding of the start point scores the start point's own value, which lies above the level (log U < 0),
    so it is accepted long before; no plain catalogue or image was found that reaches the branch, and the library gets no
    debug hook for it.  The host engine's own test covers the message."""
    sc, im = scene_a, scene_a.f.images
    seed = SEEDS[0]
    ids = np.arange(S, dtype=np.int32)
    row = int(np.nonzero(sc.src["type"] == 1)[0][0])            # a galaxy: it runs under either param
    bad = sc.src["counts"][row].copy()
    bad[sc.B - 1] = np.nan
    calls = (lambda: im.slice_locations(sc.f.sources, 1e-3, seed, chain_ids=ids),
             lambda: im.slice_sample(sc.f.sources, 0, 1e-3, seed, step_out=False, chain_ids=ids),
             lambda: im.slice_sample(sc.f.sources, 0, 2e-6, seed, chain_ids=ids),
             lambda: im.slice_sample(sc.f.sources, 1, 0.05, seed, chain_ids=ids))
    for call in calls:
        sc.reset()
        sc.f.sources.set_rows([row], sc.src["type"][row:row + 1], sc.src["radec"][row], bad, sc.src["shape"][row])
        with pytest.raises(Exception, match="got a NaN") as e:
            call()
        assert type(e.value) is Exception
    want = sc.oracle(0, ids, seed, sigma=1e-3, step_out=False)
    sc.reset()
    sc.check(im.slice_locations(sc.f.sources, 1e-3, seed, chain_ids=ids), want, 0, "after NaN: slice_locations")
    sc.check(sc.device(0, ids, seed, sigma=1e-3, step_out=False), want, 0, "after NaN: slice_sample")
    sc.check(sc.device(1, ids, seed, sigma=0.05), sc.oracle(1, ids, seed, sigma=0.05), 1, "after NaN: shapes")
    # rounds exhausted: the longest chain of the narrow set needs `rounds`; one fewer is refused, and nothing has moved
    narrow = sc.oracle(0, ids, seed, sigma=2e-6)
    sc.reset()
    with pytest.raises(ValueError, match="rounds"):
        im.slice_sample(sc.f.sources, 0, 2e-6, seed, chain_ids=ids, max_rounds=narrow["rounds"] - 1)
    assert np.array_equal(sc.f.sources.get()[1], sc.src["radec"])
    with pytest.raises(ValueError, match="rounds"):
        im.slice_locations(sc.f.sources, 1e-3, seed, chain_ids=ids, max_rounds=want["rounds"] - 1)
    assert np.array_equal(sc.f.sources.get()[1], sc.src["radec"])
    x, llh, st = im.slice_sample(sc.f.sources, 0, 2e-6, seed, chain_ids=ids, max_rounds=narrow["rounds"])     # exactly enough
    sc.check((x, llh, st), narrow, 0, "after too few rounds: slice_sample")
    sc.reset()
    sc.check(im.slice_locations(sc.f.sources, 1e-3, seed, chain_ids=ids, max_rounds=want["rounds"]), want, 0, "after too few rounds: slice_locations")


# ---- CPU calibration of the trace and of the contract's power ------------------------------------------------------------------

def _two_boxes(x, floor=-10.0):
    """0 where x[0] is in (-0.5, 0.5) u (3, 3.5) and x[1] in (-0.5, 0.5), `floor` elsewhere: bimodal in one axis"""
    return 0.0 if ((-0.5 < x[0] < 0.5 or 3.0 < x[0] < 3.5) and -0.5 < x[1] < 0.5) else floor


def _wrong_slicesample(init_x, logprob, stream, sigma, wrong):
    """the component-wise doubling update of slicesample.py:114-221 with the three `>=` of `acceptable` (:124, :129) as written
    (wrong=False) or as `>` (wrong=True): the test's own copy, for the one comparison below"""
    one = np.array([0])
    ge = (lambda p, q: p > q) if wrong else (lambda p, q: p >= q)
    rand = lambda: stream.uniform(one)[0]                     # noqa: E731
    order = np.argsort([rand() for _ in range(init_x.shape[0])], kind="stable")
    x = init_x.copy()
    for d in order:
        e = np.zeros(x.shape[0])
        e[d] = 1.0
        f = lambda z: logprob(e * z + x)                      # noqa: E731
        upper = sigma * rand()
        lower = upper - sigma
        level = np.log(rand()) + f(0.0)
        while f(lower) > level or f(upper) > level:
            if rand() < 0.5:
                lower -= upper - lower
            else:
                upper += upper - lower
        L0, U0 = lower, upper
        while True:
            z = (upper - lower) * rand() + lower
            v = f(z)
            ok = v > level
            L, U = L0, U0
            while ok and (U - L) > 1.1 * sigma:
                middle = 0.5 * (L + U)
                splits = (middle > 0 and ge(z, middle)) or (middle <= 0 and z < middle)
                if z < middle:
                    U = middle
                else:
                    L = middle
                if splits and ge(level, f(U)) and ge(level, f(L)):
                    ok = False
            if ok:
                break
            if z < 0:
                lower = z
            else:
                upper = z
        x, llh = e * z + x, v
    return x, llh


def test_trace_counts_what_it_claims_and_a_wrong_acceptable_changes_the_trajectory():
    """On a recorded stream (ReplayStream) and a target whose slice is two boxes along axis 0, the trace's counts are the hand
    count of the run, with the cap and without; and the contract has the power it is credited with: a copy of the update whose
    `acceptable` says `>` where the reference says `>=` accepts a point the reference rejects and ends somewhere else.  What
    parts the two here is `level >= logprob(end)` at equality.  `z >= middle` against `z > middle` alone parts NO trajectory:
    where the new point falls on a middle the halving makes it the interval's lower end, which is inside the slice, so the
    look at the ends cannot reject; the two differ by that one look (two evaluations), on an event of probability zero
    under the chains' continuous draws."""
    # axis 0 first (keys .2 < .7).  Axis 0: upper .75, lower -.25; level log .5; the interval doubles right, right, left to
    # (-4.25, 3.75) and both ends are outside.  New point 8 * .9375 - 4.25 = 3.25, in the second box: `acceptable` halves to
    # (-.25, 3.75), then to (1.75, 3.75), which parts the new point from the start, finds both ends outside: REJECTED; the
    # interval shrinks to (-4.25, 3.25).  New point 7.5 * .6 - 4.25 = .25: halved three times without a look at the ends, accepted.
    # Axis 1: upper .75, lower -.25; doubles left to (-1.25, .75); new point 2 * .5 - 1.25 = -.25; one halving; accepted.
    draws = [0.2, 0.7, 0.75, 0.5, 0.9, 0.9, 0.1, 0.9375, 0.6, 0.75, 0.5, 0.1, 0.5]
    tr = {}
    st = ReplayStream([DRAW_RAND] * len(draws), draws)
    x, llh = scalar_slicesample(np.zeros(2), _two_boxes, st, 0, sigma=1.0, trace=tr)
    assert st.exhausted() and llh == 0.0 and abs(x[0] - 0.25) < 1e-12 and x[1] == -0.25
    a, b = tr["directions"]
    assert (a["doublings"], a["out_rounds"], a["capped"], a["shrinks"]) == (3, 4, False, 2)
    assert (a["accept_calls"], a["end_pairs"], a["rejections"], a["max_halvings"]) == (2, 1, 1, 3)
    assert (a["outside"], a["pairs_one_outside"], a["pairs_both_outside"]) == (0, 0, 0)
    assert (b["doublings"], b["out_rounds"], b["capped"], b["shrinks"], b["accept_calls"], b["end_pairs"], b["rejections"],
            b["max_halvings"]) == (1, 2, False, 1, 1, 0, 0, 1)
    # what the trace adds changes neither the result nor the draws
    st2 = ReplayStream([DRAW_RAND] * len(draws), draws)
    x2, llh2 = scalar_slicesample(np.zeros(2), _two_boxes, st2, 0, sigma=1.0)
    assert np.array_equal(x, x2) and llh == llh2 and st2.exhausted()
    # the cap: max_steps_out = 2 stops axis 0 at (-.25, 3.75) with its lower end inside; the coin of the third doubling
    # becomes the new point 4 * .1 - .25 = .15
    tr = {}
    st = ReplayStream([DRAW_RAND] * len(draws), draws)
    scalar_slicesample(np.zeros(2), _two_boxes, st, 0, sigma=1.0, max_steps_out=2, trace=tr)
    a = tr["directions"][0]
    assert (a["doublings"], a["out_rounds"], a["capped"], a["shrinks"], a["rejections"]) == (2, 3, True, 1, 0)
    # a support: the same boxes with -inf outside, on the same draws: the doubling loop's four pairs of ends are
    # (in, out), (in, out), (in, out), (out, out); the rejecting halving sees (out, out); the other halvings look at nothing.
    # `outside` counts the points the reference's own short-circuit evaluation meets: the last pair of the loop and the rejecting pair
    tr = {}
    st = ReplayStream([DRAW_RAND] * len(draws), draws)
    scalar_slicesample(np.zeros(2), lambda p: 0.0 if _two_boxes(p) == 0.0 else -np.inf, st, 0, sigma=1.0, trace=tr)
    a = tr["directions"][0]
    assert (a["pairs_one_outside"], a["pairs_both_outside"], a["rejections"]) == (3, 2, 1) and a["outside"] == 4
    # the wrong `acceptable`: `>` for every `>=` of :119-131.  The target's floor is raised to the level itself, log .5: the
    # doubling loop (strict >) sees it outside as before; the reference rejects 3.25 (level >= both ends, with equality) and
    # ends axis 0 at .25; the wrong copy accepts 3.25, has one draw more left for axis 1 and ends it at -.4
    floor = float(np.log(0.5))
    raised = lambda p: _two_boxes(p, floor)                 # noqa: E731
    out = []
    for wrong in (False, True):
        st = ReplayStream([DRAW_RAND] * len(draws), draws)
        out.append(_wrong_slicesample(np.zeros(2), raised, st, 1.0, wrong))
        assert st.exhausted()
    st = ReplayStream([DRAW_RAND] * len(draws), draws)
    xs, ls = scalar_slicesample(np.zeros(2), raised, st, 0, sigma=1.0)
    assert np.array_equal(out[0][0], xs) and out[0][1] == ls                  # the copy as written IS the restatement
    assert abs(xs[0] - 0.25) < 1e-12 and xs[1] == -0.25
    assert out[1][0][0] == 3.25 and abs(out[1][0][1] + 0.4) < 1e-12           # the wrong one is somewhere else
