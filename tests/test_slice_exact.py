"""cel_slice_sample under CEL_OPT_SLICE_CONDITIONAL = 1: the exact conditional of ModelGibbs(conditional="exact") on the device.

1. Contract.  The scene of tests/test_slice_sample_contract.py (synth.SyntheticField(ctx, 24, 3, 128, 128, frac_gal=0.5), resident
   split of seed 5 -- made with CEL_OPT_SPLIT_FULL_BOX = 1, as the exact sweep makes it), seeds 11 and 12, the same chain ids.
   oracle.slicesample_oracle.scalar_slicesample per chain on that chain's stream, with a ONE-ROW exact scorer built from
   public calls: patch_loglik_resident of a one-row set + ModelGibbs._exact_terms' arithmetic on stamp_mass, source_boxes and
   photon_rects of that row (+ the shape prior for param 1).  x, llh, stats["evals"] and stats["rounds"] of
   slice_sample(..., conditional="exact") equal the oracle's exactly.
2. The match is not vacuous (asserted from the scorer's record and the scene, summed over the two seeds and the option sets):
   at least 20 points scored -inf by the cover test while the prior was finite; at least one chain's interval shrank because
   of such a point (counted in the sets that do not step out: there every point after a direction's level is a shrink
   proposal, and one that scores -inf is rejected and becomes the interval's new end); at least one (source, band) pair with
   has_patch false or an empty photon rectangle while the source runs; conditional="reference" on the same seed returns a
   different x for at least a quarter of the chains that ran.
3. ModelGibbs(conditional="exact"): engine="host" against engine="device" on a two-band 100 x 100 frame of 12 sources, three
   sweep(shapes=True): u, fluxes, shape bit for bit after every sweep, the evaluation counts equal; engine="auto" takes the device.
4. Refusals and hygiene.  5. CPU: the constructor and the option's number.

The scene as the contract file builds it gives every running source photons in every band, so the third condition of 2. was
not met (0 pairs); one galaxy that runs under both seeds is made faint in band 1 (1e-6 expected photons: no photon there).

MEASURED on the device, summed over seeds 11 and 12 and the five option sets (distinct points):

    points scored -inf by the cover test with a finite prior             87   (floor 20)
    ... of them rejected shrink proposals of the set without stepping out 39   (floor 1)
    (source, band) pairs without a patch or a photon, source running       1   (floor 1: the faint band)
    chains that ran (set "sweep") / moved elsewhere under "reference"     32 / 12   (floor: a quarter)
"""
import numpy as np
import pytest

import desi_mcmc_amd  # noqa: F401
from test_slice_sample_contract import S, SEEDS, Scene, chain_ids

gpu = pytest.mark.gpu

LOCATION_SETS = {
    "sweep": dict(sigma=1e-3, step_out=False),                  # the exact sweep's own call: component-wise, no stepping out
    "narrow": dict(sigma=2e-6),
    "dirs3": dict(sigma=2e-6, numdir=3),
}
SHAPE_SETS = {
    "skew": dict(sigma=1.0, numdir=4),
    "compwise": dict(sigma=0.05),
}


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


class ExactScene(Scene):
    """the contract's scene A with the split on whole boxes and the one-row EXACT scorer"""

    def __init__(self, cel):
        self.L = cel._lib
        super().__init__(cel)
        im = self.f.images
        # the contract's scene gives every running source photons in every band: one galaxy that runs under both seeds is made
        # faint in band 1 (1e-6 expected photons: the split hands it none there), so that a band without a photon is ignored
        # by the cover test of a chain that runs
        runs = np.all([chain_ids(seed) >= 0 for seed in SEEDS], axis=0) & (self.src["type"] == 1) & self.has_patch
        self.faint = int(np.nonzero(runs)[0][0])
        self.src["counts"][self.faint, 1] = 1e-6
        self.reset()
        self.split()
        self.has_patch = im.sample_box_areas().sum(axis=1) > 0
        self.rects = im.photon_rects()                              # (S, B, 4) = y0, y1, x0, x1
        self.patch = im.sample_box_areas() > 0                      # (S, B): ModelGibbs' has_patch
        self.wsum = np.array([im.band(b)[3:6].sum() for b in range(self.B)])
        self.exact_values = {}
        self.uncovered = set()         # points the cover test scored -inf while the prior was finite
        self.shrunk_by_cover = set()   # ... of them, in a run that does not step out (every such point is a rejected shrink proposal)
        self.no_step_out = False

    def split(self):
        ctx, L = self.ctx, self.L
        was = ctx.get_option(L.CEL_OPT_SPLIT_FULL_BOX)
        ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
        try:
            self.f.images.photon_split_resident(self.f.sources, seed=5)
        finally:
            ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, was)

    def score(self, param, phi_max, s, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = (param, phi_max, int(s), x.tobytes())
        if key in self.exact_values:
            if key in self.uncovered and self.no_step_out:
                self.shrunk_by_cover.add(key)
            return self.exact_values[key]
        lp = 0.0
        if param and phi_max > 0.0:
            from desi_mcmc_amd.celeste_galaxy_conditionals import galaxy_shape_prior_constrained
            lp = float(galaxy_shape_prior_constrained(x[0], x[1], x[2], x[3], phi_max))
        if lp == -np.inf:
            v = -np.inf
        else:
            src, im = self.src, self.f.images
            pc = src["counts"][s]
            self.prop.set(src["type"][s:s + 1], src["radec"][s:s + 1] if param else x[None, :], src["counts"][s:s + 1],
                          x[None, :] if param else src["shape"][s:s + 1])
            self.launches += 1
            ll = float(im.patch_loglik_resident(self.prop, np.array([s], dtype=np.int32))[0])
            # ModelGibbs._exact_terms for this one row, term by term
            mass = im.stamp_mass(self.prop)[0]
            e = 0.0
            for b in range(self.B):
                e += (pc[b] * (mass[b] - self.wsum[b])) * (1.0 if self.patch[s, b] else 0.0)
            e = -e
            bx, st = im.source_boxes(self.prop)                      # (B, 1, 4) = y0, y1, x0, x1; (B, 1)
            for b in range(self.B):
                r = self.rects[s, b]
                if not r[1] > r[0]:
                    continue                                         # no photon of the source in this band
                q = bx[b, 0]
                if not (st[b, 0] > 0 and q[0] <= r[0] and q[1] >= r[1] and q[2] <= r[2] and q[3] >= r[3]):
                    e = -np.inf
            if e == -np.inf:
                self.uncovered.add(key)
                if self.no_step_out:
                    self.shrunk_by_cover.add(key)
            ll += e
            v = lp + ll
        self.exact_values[key] = v
        return v

    def oracle(self, param, ids, seed, sigma, numdir=None, step_out=True, max_steps_out=1000, phi_max=180.):
        self.no_step_out = not step_out
        try:
            return super().oracle(param, ids, seed, sigma, numdir=numdir, step_out=step_out, max_steps_out=max_steps_out, phi_max=phi_max)
        finally:
            self.no_step_out = False

    def device(self, param, ids, seed, sigma, numdir=None, step_out=True, max_steps_out=1000, phi_max=180., conditional="exact"):
        from desi_mcmc_amd.util.infer.slicesample import ChainStreams
        self.reset()
        dirs = None if numdir is None else ChainStreams(seed, np.where(ids < 0, 0, ids)).directions(numdir, 4 if param else 2)
        return self.f.images.slice_sample(self.f.sources, param, sigma, seed, dirs=dirs, step_out=step_out, max_steps_out=max_steps_out,
                                          phi_max=phi_max, chain_ids=ids, conditional=conditional)


@pytest.fixture(scope="module")
def scene(cel):
    return ExactScene(cel)


def _run(scene, param, name, opts):
    for seed in SEEDS:
        ids = chain_ids(seed)
        want = scene.oracle(param, ids, seed, **opts)
        scene.check(scene.device(param, ids, seed, **opts), want, param, (name, seed))


@gpu
@pytest.mark.parametrize("name", list(LOCATION_SETS))
def test_locations_follow_the_oracle_on_the_exact_scorer(cel, scene, name):
    """param 0: x, llh, evals and rounds of slice_sample(conditional="exact") are the oracle's on the one-row exact scorer;
    chains with id -1 keep their row and get a NaN llh (Scene.check)"""
    _run(scene, 0, name, LOCATION_SETS[name])


@gpu
@pytest.mark.parametrize("name", list(SHAPE_SETS))
def test_shapes_follow_the_oracle_on_the_exact_scorer(cel, scene, name):
    """param 1, phi_max 180: the galaxies' shapes, the prior's -inf and the cover test's -inf side by side"""
    _run(scene, 1, name, SHAPE_SETS[name])


@gpu
def test_the_match_is_not_vacuous(cel, scene):
    """Conditions on the scene, from the scorer's record of the oracle's runs (every option set, both seeds; a set that has run
    already is read from the scene's cache).

    The figures of a run are in the module's docstring (and in the COVERAGE line of a run with -s)."""
    for param, sets in ((0, LOCATION_SETS), (1, SHAPE_SETS)):
        for name, opts in sets.items():
            for seed in SEEDS:
                scene.oracle(param, chain_ids(seed), seed, **opts)
    ran = np.zeros(S, bool)
    differ = n_ran = 0
    for seed in SEEDS:
        ids = chain_ids(seed)
        opts = LOCATION_SETS["sweep"]
        want = scene.oracle(0, ids, seed, **opts)
        ref = scene.device(0, ids, seed, conditional="reference", **opts)[0]
        ran |= want["ran"]
        n_ran += int(want["ran"].sum())
        differ += int(np.any(ref[want["ran"]] != want["x"][want["ran"]], axis=1).sum())
    held = scene.rects[..., 1] > scene.rects[..., 0]
    assert not held[scene.faint, 1] and held[scene.faint].any()
    odd_pairs = int(((~scene.patch | ~held) & ran[:, None]).sum())
    print("COVERAGE exact: uncovered points %d, of them rejected shrink proposals %d, (source, band) pairs without patch or photon %d, "
          "chains that ran %d, moved elsewhere under the reference's conditional %d"
          % (len(scene.uncovered), len(scene.shrunk_by_cover), odd_pairs, n_ran, differ))
    assert len(scene.uncovered) >= 20
    assert len(scene.shrunk_by_cover) >= 1
    assert odd_pairs >= 1
    assert 4 * differ >= n_ran


# ---- 3. the engines agree ---------------------------------------------------------------------------------------------------------
HF, WF, BF, SF = 100, 100, 2, 12


def _small_frame(cel):
    from desi_mcmc_amd import synth
    from test_masked_pixels import _fits_images, draw_counts
    ctx = cel.default_context(0)
    rs = np.random.RandomState(3)
    bands = synth.make_bands(HF, WF, BF)
    pix = np.column_stack([rs.uniform(10, 90, SF), rs.uniform(10, 90, SF)])
    typ = (np.arange(SF) % 2).astype(np.int32)
    shape = np.column_stack([rs.uniform(0.1, 0.9, SF), np.exp(rs.uniform(np.log(0.4), np.log(1.2), SF)), rs.uniform(0, 180, SF),
                             rs.uniform(0.3, 0.95, SF)])
    shape[typ == 0] = 0.0
    counts = np.exp(rs.uniform(np.log(300.0), np.log(3e4), size=(SF, BF)))
    nelec = draw_counts(cel, ctx, bands, HF, WF, typ, pix, counts, shape, 21)
    radec = synth.pixel2equa(bands[0], pix)
    flux = counts * bands[:, 2][None, :] / bands[:, 1][None, :]
    params = []
    for s in range(SF):
        fl = np.full(5, 3.0)
        fl[:BF] = flux[s]
        th = shape[s]
        kw = dict(theta=th[0], sigma=th[1], phi=th[2], rho=th[3]) if typ[s] == 1 else {}
        params.append(cel.SrcParams(u=radec[s], a=int(typ[s]), fluxes=fl, **kw))
    return lambda: [dict(zip("ug", _fits_images(bands, nelec, HF, WF)))], params


@gpu
def test_the_engines_agree_on_the_exact_sweep(cel):
    """ModelGibbs(conditional="exact"), host engine against device engine on the same seed: the chain's state bit for bit
    after each of three sweeps with shapes, the evaluation counts equal; "auto" is the device engine"""
    from desi_mcmc_amd import celeste_mcmc
    images, params = _small_frame(cel)
    g = {e: celeste_mcmc.ModelGibbs.from_images(images(), params, seed=4, conditional="exact", engine=e) for e in ("host", "device", "auto")}
    for sweep in range(3):
        for e in g:
            g[e].sweep(shapes=True)
        for e in ("device", "auto"):
            for name in ("u", "fluxes", "shape"):
                a, b = getattr(g["host"], name), getattr(g[e], name)
                assert np.array_equal(a, b), (sweep, e, name, np.nonzero(np.any(a != b, axis=1))[0])
            assert g[e].timing["evals"] == g["host"].timing["evals"] and g[e].timing["shape_evals"] == g["host"].timing["shape_evals"]
    assert g["host"].timing["evals"] > 0 and g["host"].timing["shape_evals"] > 0
    # what the device path alone fills: the launches of cel_slice_sample's rounds
    assert g["auto"].timing.get("loc_launches", 0) > 0 and g["device"].timing.get("loc_launches", 0) > 0
    assert "loc_launches" not in g["host"].timing
    assert np.any(g["host"].u != np.array([p.u for p in params]))


# ---- 4. refusals and hygiene ------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_hygiene(cel, scene):
    from desi_mcmc_amd import synth
    L = cel._lib
    ctx, im, srcs = scene.ctx, scene.f.images, scene.f.sources
    assert ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0
    with pytest.raises(ValueError):
        ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 2)
    assert ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0
    seed = SEEDS[0]
    ids = chain_ids(seed)
    opts = LOCATION_SETS["sweep"]
    # a reference call after an exact call: the bits of a reference call in a fresh context; the option reads 0 in between
    scene.device(0, ids, seed, **opts)
    assert ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0
    after = scene.device(0, ids, seed, conditional="reference", **opts)
    fresh_ctx = cel.Context(0)
    f2 = synth.SyntheticField(fresh_ctx, S, scene.B, 128, 128, frac_gal=0.5)
    f2.sources.set(scene.src["type"], scene.src["radec"], scene.src["counts"], scene.src["shape"])      # (the scene's faint band)
    fresh_ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    f2.images.photon_split_resident(f2.sources, seed=5)
    fresh_ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
    fresh = f2.images.slice_sample(f2.sources, 0, opts["sigma"], seed, step_out=False, chain_ids=ids)
    assert np.array_equal(after[0], fresh[0]) and np.array_equal(after[1], fresh[1], equal_nan=True) and after[2] == fresh[2]
    # the failed call restores the option too
    with pytest.raises(ValueError):
        im.slice_sample(srcs, 0, -1.0, seed, conditional="exact")
    assert ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0
    # cel_slice_locations does not read the option
    out = []
    for v in (0, 1):
        scene.reset()
        scene.split()
        ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, v)
        try:
            out.append(im.slice_locations(srcs, 1e-3, seed, chain_ids=ids))
        finally:
            ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 0)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1], equal_nan=True) and out[0][2] == out[1][2]
    # a masked set and a windowed set are refused under the exact conditional, before any launch
    f2.images.set_window(64, 512)
    with pytest.raises(ValueError, match="window"):
        f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, conditional="exact")
    assert fresh_ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0
    f2.images.set_window(0, 128)
    f2.images.photon_split_resident(f2.sources, seed=5)
    f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, conditional="exact")          # whole again: runs
    masked = np.zeros((scene.B, 128, 128))
    masked[0, 5, 7] = np.nan
    f2.images.set_nelec(masked)
    with pytest.raises(ValueError, match="masked"):
        f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, conditional="exact")
    assert fresh_ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 0


# ---- 5. CPU -----------------------------------------------------------------------------------------------------------------------
def test_the_exact_conditional_constructs_on_the_device_engine():
    import __graft_entry__ as ge
    ge.build()
    from desi_mcmc_amd import _lib, celeste_mcmc
    assert _lib.CEL_OPT_SLICE_CONDITIONAL == 18
    empty = ([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)))
    g = celeste_mcmc.ModelGibbs(*empty, conditional="exact", engine="device")
    # (no field: the device engines need exactly one -- the options are what is asked here)
    g.fields = [None]
    assert g._shape_engine_on_device() is True
    assert g._device_engine_applies() is True
    # shape_mass="exact" under the reference's conditional is a diagnostic setting of the host engine
    h = celeste_mcmc.ModelGibbs(*empty, shape_mass="exact")
    h.fields = [None]
    assert h._shape_engine_on_device() is False
    # mask="honour" keeps requiring the host engine
    with pytest.raises(ValueError, match="host"):
        celeste_mcmc.ModelGibbs(*empty, mask="honour", conditional="exact", engine="device")
