"""The device samplers of the exact conditional on a MASKED image set: CEL_OPT_SAMPLER_MASK = 21, cel_slice_sample params 0, 1, 2 under
CEL_OPT_SLICE_CONDITIONAL = 1 with the observed-mass kernel on the samplers' job lists, ImageSet.slice_sample / type_move(mask=
"honour"), ModelGibbs(mask="honour", mask_engine="device").

The scene is tests/test_slice_exact.py's ExactScene (128 x 128, 3 bands, 24 sources, full-box resident split of seed 5, seeds 11
and 12) with NaN written into nelec BEFORE the split and the split made under CEL_OPT_HONOUR_MASK.  The mask is built from the
scene's own boxes (MaskedMixin.build_mask):

  (a) the core pixel of one star and of one galaxy (band 0);
  (b) one whole chunk (32 columns x up to 64 rows, as k_stamp_mass_masked walks it) of the widest galaxy box, the one that does
      not hold the galaxy's core (band 0);
  (c) the row pair either side of a chunk seam (box rows 63 and 64) of the tallest box, and five rows of the columns behind the
      last full 32-column chunk of the widest box that does not end on one (band 1);
  (d) the band-1 box of a star that runs under both seeds, masked everywhere;
  (e) band 2 without a masked pixel;
  (f) 1 % of the remaining pixels of bands 0 and 1 (RandomState(77)).

1. chain by chain against the oracle's sampler on the one-row exact scorer taken under CEL_OPT_HONOUR_MASK
2. the type move restated from public calls (tests/test_type_move.py's restatement on the masked scene)
3. the match is not vacuous: scored with the UNMASKED mass the chains move elsewhere
4. ModelGibbs: host engine against engine="auto", mask_engine="device" over three sweeps with shapes and types
5. refusals and hygiene

MEASURED on the device (seeds 11 and 12, the "sweep" set for the control):

    chains that ran / ended elsewhere under the unmasked mass       32 / 16   (floor: a quarter)
    proposal boxes that reach the masked chunk of (b)                851   (floor 1); every source was scored, the one of (d) among them
    points the cover test scored -inf                                118
    type move, seeds 11 .. 14: chains that ran 57, accepted 3, proposals the cover test alone rejects 20
"""
import ctypes as C

import numpy as np
import pytest

import desi_mcmc_amd  # noqa: F401
import test_type_move as tt
from test_slice_exact import BF, HF, LOCATION_SETS, SHAPE_SETS, WF, ExactScene, _small_frame
from test_slice_sample_contract import S, SEEDS, chain_ids

gpu = pytest.mark.gpu
SETS = [(0, "sweep", LOCATION_SETS["sweep"]), (0, "narrow", LOCATION_SETS["narrow"]), (1, "skew", SHAPE_SETS["skew"])]


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def _option(ctx, key, value):
    import contextlib

    @contextlib.contextmanager
    def cm():
        was = ctx.get_option(key)
        ctx.set_option(key, value)
        try:
            yield
        finally:
            ctx.set_option(key, was)
    return cm()


def _chunks(box):
    """the chunks k_stamp_mass_masked walks a box (y0, y1, x0, x1) in: (y0, y1, x0, x1) each"""
    y0, y1, x0, x1 = (int(v) for v in box)
    return [(Y, min(Y + 64, y1), X, min(X + 32, x1)) for Y in range(y0, y1, 64) for X in range(x0, x1, 32)]


def build_mask(boxes, status, typ, pix, runs, shape_hw, seed=77):
    """the mask of kinds (a) - (f) from the catalogue's boxes (B, S, 4) = y0, y1, x0, x1 -> (mask (B, H, W), dict of what was chosen)"""
    Bn, (Hh, Ww) = boxes.shape[0], shape_hw
    m = np.zeros((Bn, Hh, Ww), dtype=bool)
    core = lambda s: (int(np.floor(pix[s, 1])), int(np.floor(pix[s, 0])))          # noqa: E731
    on_frame = lambda s: 0 <= core(s)[0] < Hh and 0 <= core(s)[1] < Ww             # noqa: E731
    ok = runs & np.all(status > 0, axis=0) & np.array([on_frame(s) for s in range(len(typ))])
    star, gal = np.nonzero(ok & (typ == 0))[0], np.nonzero(ok & (typ == 1))[0]
    pick = dict(star_a=int(star[0]), gal_a=int(gal[0]))
    for s in (pick["star_a"], pick["gal_a"]):                                      # (a)
        m[0][core(s)] = True
    nx, ny = boxes[..., 3] - boxes[..., 2], boxes[..., 1] - boxes[..., 0]
    gb = int(gal[np.argmax(nx[0, gal])])                                           # (b)
    ch = [c for c in _chunks(boxes[0, gb]) if c[3] - c[2] == 32 and not (c[0] <= core(gb)[0] < c[1] and c[2] <= core(gb)[1] < c[3])]
    assert len(_chunks(boxes[0, gb])) > 1 and ch, ("no galaxy box of several chunks", boxes[0, gb])
    pick.update(gal_b=gb, chunk=ch[0])
    m[0, ch[0][0]:ch[0][1], ch[0][2]:ch[0][3]] = True
    every = np.nonzero(ok)[0]
    gc = int(every[np.argmax(ny[1, every])])                                       # (c): the seam of the tallest box ...
    y0, y1, x0, x1 = (int(v) for v in boxes[1, gc])
    assert y1 - y0 > 64, ("no box with a seam between two row chunks", boxes[1, gc])
    m[1, y0 + 63:y0 + 65, x0:x1] = True
    ragged = every[(nx[1, every] > 32) & (nx[1, every] % 32 != 0)]                  # ... and the widest box that ends behind a full chunk
    assert ragged.size, "every box ends on a 32-column chunk"
    gt = int(ragged[np.argmax(nx[1, ragged])])
    y0, y1, x0, x1 = (int(v) for v in boxes[1, gt])
    tail = (y0 + 2, min(y0 + 7, y1), x0 + 32 * ((x1 - x0) // 32), x1)
    m[1, tail[0]:tail[1], tail[2]:tail[3]] = True
    pick.update(src_c=gc, src_tail=gt, tail=tail)
    sd = int([s for s in star if s != pick["star_a"]][0])                          # (d)
    q = boxes[1, sd]
    m[1, q[0]:q[1], q[2]:q[3]] = True
    pick.update(star_d=sd)
    rs = np.random.RandomState(seed)                                               # (f); (e): the last band stays clean
    m[:2] |= rs.rand(2, Hh, Ww) < 0.01
    assert not m[2:].any()
    # every source keeps, in some band, its core pixel and most of its box: it still holds photons there
    for s in np.nonzero(ok)[0]:
        keeps = [not m[b][core(s)] and m[b, boxes[b, s, 0]:boxes[b, s, 1], boxes[b, s, 2]:boxes[b, s, 3]].mean() < 0.25 for b in range(Bn)]
        assert any(keeps), s
    q = boxes[1, sd]
    assert m[1, q[0]:q[1], q[2]:q[3]].all()
    return m, pick


class MaskedMixin(object):
    """masks the scene a base class built (its field, catalogue and whole-box split), splits again under CEL_OPT_HONOUR_MASK and
    reads the split's tables again; the scorers below take the observed mass (control: the unmasked one)"""
    masked = False
    control = False

    def honour(self, on=True):
        return _option(self.ctx, self.L.CEL_OPT_HONOUR_MASK, 1 if on else 0)

    def split(self):
        with self.honour(self.masked):
            super().split()

    def mask_scene(self):
        f, im = self.f, self.f.images
        self.reset()
        boxes, status = im.source_boxes(f.sources)
        runs = np.all([chain_ids(seed) >= 0 for seed in SEEDS], axis=0) & self.has_patch
        self.mask, self.pick = build_mask(boxes, status, self.src["type"], self.src["pix"], runs, (f.H, f.W))
        self.cat_boxes = boxes
        im.set_nelec(np.where(self.mask, np.nan, f.nelec))
        assert list(im.masked) == [int(self.mask[b].sum()) for b in range(self.B)] and im.masked[-1] == 0
        self.masked = True
        self.split()
        self.patch = im.sample_box_areas() > 0
        self.has_patch = self.patch.any(axis=1)
        self.rects = im.photon_rects()
        sums = im.sample_sums()
        assert np.all(sums[runs].sum(axis=1) > 0) and sums[self.pick["star_d"], 1] == 0 and sums[self.pick["star_d"]].sum() > 0
        assert np.all(sums[self.mask_sources()].sum(axis=1) > 0)
        self.values, self.runs, self.exact_values, self.uncovered, self.shrunk_by_cover = {}, {}, {}, set(), set()
        self.seen_sources, self.boxes_on_chunk = set(), 0

    def mask_sources(self):
        return [self.pick[k] for k in ("star_a", "gal_a", "gal_b", "src_c", "src_tail", "star_d")]


class MaskedScene(MaskedMixin, ExactScene):
    def __init__(self, cel):
        super().__init__(cel)
        self.mask_scene()

    def score(self, param, phi_max, s, x):
        """ExactScene.score with the masses taken under CEL_OPT_HONOUR_MASK (control: with the option off -- the unmasked mass),
        and a record of whose points were scored and of the proposal boxes that reach the chunk of (b)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = (param, phi_max, int(s), x.tobytes(), self.control)
        if key in self.exact_values:
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
            with self.honour(not self.control):
                mass = im.stamp_mass(self.prop)[0]
            e = 0.0
            for b in range(self.B):
                e += (pc[b] * (mass[b] - self.wsum[b])) * (1.0 if self.patch[s, b] else 0.0)
            e = -e
            bx, st = im.source_boxes(self.prop)                      # (B, 1, 4) = y0, y1, x0, x1; (B, 1)
            for b in range(self.B):
                r = self.rects[s, b]
                if not r[1] > r[0]:
                    continue
                q = bx[b, 0]
                if not (st[b, 0] > 0 and q[0] <= r[0] and q[1] >= r[1] and q[2] <= r[2] and q[3] >= r[3]):
                    e = -np.inf
            if e == -np.inf:
                self.uncovered.add(key)
            elif not self.control:
                self.seen_sources.add(int(s))
                c, q = self.pick["chunk"], bx[0, 0]
                if st[0, 0] > 0 and q[0] < c[1] and q[1] > c[0] and q[2] < c[3] and q[3] > c[2]:
                    self.boxes_on_chunk += 1
            ll += e
            v = lp + ll
        self.exact_values[key] = v
        return v

    def oracle(self, param, ids, seed, sigma, **kw):
        runs = self.runs
        self.runs = runs.setdefault(("control", self.control), {})      # (the base class keys its runs by the arguments alone)
        try:
            return super().oracle(param, ids, seed, sigma, **kw)
        finally:
            self.runs = runs

    def device(self, param, ids, seed, sigma, numdir=None, step_out=True, max_steps_out=1000, phi_max=180., **kw):
        from desi_mcmc_amd.util.infer.slicesample import ChainStreams
        self.reset()
        dirs = None if numdir is None else ChainStreams(seed, np.where(ids < 0, 0, ids)).directions(numdir, 4 if param else 2)
        kw.setdefault("conditional", "exact")
        kw.setdefault("mask", "honour")
        return self.f.images.slice_sample(self.f.sources, param, sigma, seed, dirs=dirs, step_out=step_out, max_steps_out=max_steps_out,
                                          phi_max=phi_max, chain_ids=ids, **kw)


@pytest.fixture(scope="module")
def scene(cel):
    return MaskedScene(cel)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("param,name,opts", SETS, ids=[s[1] for s in SETS])
def test_chains_follow_the_oracle_on_the_masked_scorer(cel, scene, param, name, opts):
    """x, llh, evals and rounds of slice_sample(conditional="exact", mask="honour") are scalar_slicesample's on the one-row exact
    scorer taken under CEL_OPT_HONOUR_MASK; the options are the caller's again afterwards"""
    L = scene.L
    for seed in SEEDS:
        ids = chain_ids(seed)
        want = scene.oracle(param, ids, seed, **opts)
        scene.check(scene.device(param, ids, seed, **opts), want, param, (name, seed))
    for k in (L.CEL_OPT_SAMPLER_MASK, L.CEL_OPT_HONOUR_MASK, L.CEL_OPT_SLICE_CONDITIONAL):
        assert scene.ctx.get_option(k) == 0


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_match_is_not_vacuous(cel, scene):
    """the same chains scored with the UNMASKED mass (stamp_mass with CEL_OPT_HONOUR_MASK off) end elsewhere: at least a quarter of
    the chains that ran (tests/test_slice_exact.py's floor for its "reference" control); the source of (d) was scored, and a
    proposal's box reached the masked chunk of (b)"""
    opts = LOCATION_SETS["sweep"]
    differ = n_ran = 0
    for seed in SEEDS:
        ids = chain_ids(seed)
        want = scene.oracle(0, ids, seed, **opts)
        scene.control = True
        try:
            other = scene.oracle(0, ids, seed, **opts)
        finally:
            scene.control = False
        assert np.array_equal(want["ran"], other["ran"])
        n_ran += int(want["ran"].sum())
        differ += int(np.any(other["x"][want["ran"]] != want["x"][want["ran"]], axis=1).sum())
    print("COVERAGE masked: chains that ran %d, ended elsewhere under the unmasked mass %d; sources scored %s; proposal boxes on the "
          "masked chunk %d; points the cover test scored -inf %d" % (n_ran, differ, sorted(scene.seen_sources), scene.boxes_on_chunk,
                                                                     len(scene.uncovered)))
    assert 4 * differ >= n_ran
    assert scene.pick["star_d"] in scene.seen_sources
    assert scene.boxes_on_chunk >= 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
class MaskedTypeScene(MaskedMixin, tt.TypeScene):
    def __init__(self, cel):
        super().__init__(cel)
        self.mask_scene()

    def scores(self, typ, shape, conditional):
        with self.honour():
            return super().scores(typ, shape, conditional)


@pytest.fixture(scope="module")
def type_scene(cel):
    return MaskedTypeScene(cel)


@gpu
def test_every_type_decision_is_the_restated_one(cel, type_scene):
    """tests/test_type_move.py's restatement (its scores take stamp_mass under CEL_OPT_HONOUR_MASK here): log alpha, the accepted
    moves, typ, shape and every untouched row bit for bit"""
    scene = type_scene
    im, srcs = scene.f.images, scene.f.sources
    moved = ran_all = 0
    for seed in tt.SEEDS4:
        ids = chain_ids(seed)
        shapes, h, out = scene.proposals(seed, ids)
        want = scene.restate(ids, seed, shapes, h, "exact")
        scene.reset()
        typ, shape, la, st = im.type_move(srcs, shapes, h, seed, chain_ids=ids, conditional="exact", mask="honour")
        ran = want["ran"]
        print("TYPE MOVE masked seed %d: ran %d, accepted %d, cover-only %d" % (seed, ran.sum(), want["acc"].sum(), want["cover_only"].sum()))
        assert ran.any() and not ran[scene.off] and not ran[scene.t2] and (ids < 0).any()
        assert np.array_equal(la, want["la"], equal_nan=True), (seed, la, want["la"])
        assert np.array_equal(typ, want["typ"]) and np.array_equal(shape, want["shape"]), seed
        assert np.array_equal(typ[~ran], scene.src["type"][~ran]) and np.array_equal(shape[~ran], scene.src["shape"][~ran])
        assert np.all(np.isnan(la[~ran]))
        now = srcs.get()
        assert np.array_equal(now[0], typ) and np.array_equal(now[3], shape)
        assert st["evals"] == 2 * int(ran.sum()) and st["accepted"] == int(want["acc"].sum()) and st["launches"] >= 1
        moved += int(want["acc"].sum())
        ran_all += int(ran.sum())
        # the unmasked mass gives other odds for the sources beside a mask
        with scene.honour(False):
            other = tt.TypeScene.scores(scene, np.repeat(scene.src["type"], 2), np.repeat(scene.src["shape"], 2, axis=0), "exact")[2]
        mine = scene.scores(np.repeat(scene.src["type"], 2), np.repeat(scene.src["shape"], 2, axis=0), "exact")[2]
        assert np.any(other[0::2][ran] != mine[0::2][ran])
    assert moved >= 1 and ran_all >= 30
    scene.reset()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _masked_small_frame(cel):
    """tests/test_slice_exact.py's 100 x 100 two-band frame with a mask of the same kinds in band 0 (band 1 stays clean): the core
    pixel of one star and one galaxy, a 32-column chunk of the widest box, a seam row pair, one star's box, 1 % of the rest"""
    from desi_mcmc_amd import synth
    from test_masked_pixels import _fits_images
    images, params = _small_frame(cel)
    first = images()[0]
    nelec = np.stack([first[k].nelec for k in "ug"])
    bands = synth.make_bands(HF, WF, BF)
    ctx = cel.default_context(0)
    typ = np.array([p.a for p in params], dtype=np.int32)
    radec = np.array([p.u for p in params])
    iset = cel.ImageSet(ctx, bands, HF, WF)
    sset = cel.SourceSet(ctx, len(params), BF).set(typ, radec, np.full((len(params), BF), 1000.0),
                                                  np.array([[p.theta, p.sigma, p.phi, p.rho] if p.a == 1 else [0.] * 4 for p in params]))
    boxes, status = iset.source_boxes(sset)
    iset.close()
    pix = np.array([[0.5 * (boxes[0, s, 2] + boxes[0, s, 3]), 0.5 * (boxes[0, s, 0] + boxes[0, s, 1])] for s in range(len(params))])
    m = np.zeros((BF, HF, WF), dtype=bool)
    star, gal = np.nonzero(typ == 0)[0], np.nonzero(typ == 1)[0]
    for s in (star[0], gal[0]):
        m[0, int(pix[s, 1]), int(pix[s, 0])] = True
    gb = gal[np.argmax(boxes[0, gal, 3] - boxes[0, gal, 2])]
    y0, y1, x0, x1 = boxes[0, gb]
    m[0, y0:min(y0 + 64, y1), x0:min(x0 + 32, x1)] = True
    m[0, 63:65, :] = True
    q = boxes[0, star[1]]
    m[0, q[0]:q[1], q[2]:q[3]] = True
    m[0] |= np.random.RandomState(78).rand(HF, WF) < 0.01
    iv = np.where(m, 0.0, 1.0)
    return (lambda: [dict(zip("ug", _fits_images(bands, nelec, HF, WF, iv)))]), params, int(m.sum())


@gpu
def test_the_engines_agree_on_the_masked_sweep(cel):
    """ModelGibbs(conditional="exact", mask="honour"): engine="host" against engine="auto" with mask_engine="device", the chain's
    state bit for bit after each of three sweeps with shapes and types, the evaluation counts equal, "auto" on the device"""
    from desi_mcmc_amd import celeste_mcmc
    images, params, n_masked = _masked_small_frame(cel)
    kw = dict(seed=4, conditional="exact", mask="honour")
    g = dict(host=celeste_mcmc.ModelGibbs.from_images(images(), params, engine="host", **kw),
             auto=celeste_mcmc.ModelGibbs.from_images(images(), params, engine="auto", mask_engine="device", **kw))
    assert int(g["auto"].fields[0].iset.masked.sum()) == n_masked > 100
    assert g["auto"]._device_engine_applies() and g["auto"]._shape_engine_on_device() and g["auto"]._type_engine_on_device()
    assert not g["host"]._type_engine_on_device()
    for sweep in range(3):
        for e in g:
            g[e].sweep(shapes=True, types=True)
        for name in ("u", "fluxes", "shape", "typ"):
            a, b = getattr(g["host"], name), getattr(g["auto"], name)
            assert np.array_equal(a, b), (sweep, name, np.nonzero(a != b))
        for k in ("evals", "shape_evals", "type_evals", "type_accepted"):
            assert g["auto"].timing[k] == g["host"].timing[k], (sweep, k)
    assert g["host"].timing["evals"] > 0 and g["host"].timing["shape_evals"] > 0 and g["host"].timing["type_evals"] > 0
    assert g["auto"].timing.get("loc_launches", 0) > 0 and "loc_launches" not in g["host"].timing
    assert np.any(g["host"].u != np.array([p.u for p in params]))
    ctx = g["auto"].fields[0].iset.ctx
    for k in (cel._lib.CEL_OPT_SAMPLER_MASK, cel._lib.CEL_OPT_HONOUR_MASK, cel._lib.CEL_OPT_SLICE_CONDITIONAL):
        assert ctx.get_option(k) == 0


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _raw_sample(L, im, srcs, param, dirs, numdir, x, sigma=1e-3, rounds=20000):
    stats = np.zeros(4, dtype=np.int64)
    return L.lib().cel_slice_sample(im._h, srcs._h, param, None, None if dirs is None else L.dptr(dirs), numdir, 0, 0, sigma, 180.0,
                                    C.c_uint64(7), rounds, L.dptr(x), None, stats.ctypes.data_as(L.c_int64_p))


@gpu
def test_refusals_and_hygiene(cel, scene):
    from desi_mcmc_amd import synth
    L = scene.L
    ctx, im, srcs = scene.ctx, scene.f.images, scene.f.sources
    K, HM, SC, GC = L.CEL_OPT_SAMPLER_MASK, L.CEL_OPT_HONOUR_MASK, L.CEL_OPT_SLICE_CONDITIONAL, L.CEL_OPT_GRAD_CONDITIONAL
    assert ctx.get_option(K) == 0
    for start in (0.0, 1.0):
        ctx.set_option(K, start)
        for bad in (2.0, -1.0, 0.5, float("nan")):
            assert L.lib().cel_ctx_set_option(ctx._h, K, bad) == L.CEL_ERR_INVALID
            assert ctx.get_option(K) == start
    ctx.set_option(K, 0)
    seed, ids = SEEDS[0], chain_ids(SEEDS[0])
    shapes, h = np.tile([0.5, 1.0, 30.0, 0.5], (S, 1)), np.zeros(S)
    p0, imass = np.zeros((S, 6)), np.ones((S, 6))
    sent = np.full((S, 12), -7.25)

    def every_sampler(**kw):
        scene.reset()
        return [lambda: im.slice_locations(srcs, 1e-3, seed, chain_ids=ids),
                lambda: im.slice_sample(srcs, 0, 1e-3, seed, step_out=False, chain_ids=ids, **kw),
                lambda: im.slice_sample(srcs, 1, 1.0, seed, chain_ids=ids, **kw),
                lambda: im.type_move(srcs, shapes, h, seed, chain_ids=ids, **kw),
                lambda: im.hmc_step(srcs, p0, imass, 0.1, 2, seed, chain_ids=ids, **kw)]

    # the option off: every pinned refusal as it was, under either value of CEL_OPT_HONOUR_MASK and either conditional
    for hm in (0, 1):
        with _option(ctx, HM, hm):
            for conditional in ("reference", "exact"):
                for call in every_sampler(conditional=conditional)[1:] + every_sampler()[:1]:
                    with pytest.raises(ValueError, match="masked"):
                        call()
            with pytest.raises(ValueError, match="masked"):
                im.patch_loglik_resident_grad(scene.prop, np.zeros(scene.prop.S, dtype=np.int32), conditional="exact")
            with pytest.raises(ValueError, match="masked"):
                im.patch_loglik_resident(scene.prop, np.zeros(scene.prop.S, dtype=np.int32), isolated=True)
    # the option on without CEL_OPT_HONOUR_MASK: nothing is accepted
    with _option(ctx, K, 1):
        for call in every_sampler(conditional="exact"):
            with pytest.raises(ValueError, match="masked"):
                call()
    # both on: still refused before any launch (the outputs keep their sentinel) -- the reference's conditional, cel_slice_locations,
    # the isolated forms
    with _option(ctx, K, 1), _option(ctx, HM, 1):
        scene.reset()
        for param, dirs, numdir in ((0, None, 0), (1, None, 0), (2, np.ascontiguousarray(np.column_stack([shapes, h])), 1),
                                    (3, np.ascontiguousarray(np.column_stack([p0, imass])), 12)):
            assert _raw_sample(L, im, srcs, param, dirs, numdir, sent, sigma=0.1 if param == 3 else 1e-3, rounds=2 if param == 3 else 20000) == L.CEL_ERR_INVALID
            assert b"masked" in L.lib().cel_last_error() and np.all(sent == -7.25), param
        with pytest.raises(ValueError, match="masked"):
            im.slice_locations(srcs, 1e-3, seed, chain_ids=ids)
        with pytest.raises(ValueError, match="masked"):
            im.patch_loglik_resident(scene.prop, np.zeros(scene.prop.S, dtype=np.int32), isolated=True)
        with pytest.raises(ValueError, match="masked"):
            im.patch_loglik_resident_grad(scene.prop, np.zeros(scene.prop.S, dtype=np.int32), isolated=True)
        # ... and the exact conditional runs under the raw keys
        with _option(ctx, SC, 1):
            assert _raw_sample(L, im, srcs, 0, None, 0, sent) == L.CEL_OK
            assert not np.any(sent.ravel()[:2 * S] == -7.25) and np.all(sent.ravel()[2 * S:] == -7.25)
        sent[:] = -7.25
    # the wrappers refuse mask="honour" under the reference's conditional before any device call, and restore both options after a
    # call that raised
    for hm, k in ((0, 0), (1, 1)):
        with _option(ctx, HM, hm), _option(ctx, K, k):
            for call in every_sampler(conditional="reference", mask="honour")[1:]:
                with pytest.raises(ValueError, match="masked"):
                    call()
                assert ctx.get_option(HM) == hm and ctx.get_option(K) == k
            with pytest.raises(ValueError):
                im.slice_sample(srcs, 0, -1.0, seed, conditional="exact", mask="honour")             # a bad sigma: the library raises
            assert ctx.get_option(HM) == hm and ctx.get_option(K) == k and ctx.get_option(SC) == 0
            with pytest.raises(ValueError, match="mask must be"):
                im.slice_sample(srcs, 0, 1e-3, seed, conditional="exact", mask="ignore")
    # a windowed masked set: refused under both options (the exact conditional's own words)
    fresh_ctx = cel.Context(0)
    f2 = synth.SyntheticField(fresh_ctx, S, scene.B, 128, 128, frac_gal=0.5)
    f2.sources.set(scene.src["type"], scene.src["radec"], scene.src["counts"], scene.src["shape"])
    fresh_ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    out = {}
    for v in (0, 1):
        # a set without a NaN: params 0 - 3 return the same bits with the option 0 and 1
        res = []
        with _option(fresh_ctx, K, v), _option(fresh_ctx, HM, v):
            f2.sources.set(scene.src["type"], scene.src["radec"], scene.src["counts"], scene.src["shape"])
            f2.images.photon_split_resident(f2.sources, seed=5)
            res.append(f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, chain_ids=ids, conditional="exact"))
            res.append(f2.images.slice_sample(f2.sources, 1, 1.0, seed, chain_ids=ids, conditional="exact"))
            res.append(f2.images.type_move(f2.sources, shapes, h, seed, chain_ids=ids, conditional="exact"))
            res.append(f2.images.hmc_step(f2.sources, p0, 1e-12 * imass, 0.1, 2, seed, chain_ids=ids, conditional="exact"))
        out[v] = res
    for a, b in zip(out[0], out[1]):
        for x, y in zip(a[:-1], b[:-1]):
            assert np.array_equal(x, y, equal_nan=True)
        assert a[-1] == b[-1]                                        # rounds, evaluations, launches
    f2.images.set_window(64, 512)
    nan_win = f2.nelec.copy()
    nan_win[0, 5, 7] = np.nan
    f2.images.set_nelec(nan_win)
    with _option(fresh_ctx, HM, 1):
        f2.images.photon_split_resident(f2.sources, seed=5)
    with pytest.raises(ValueError, match="window"):
        f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, conditional="exact", mask="honour")
    with pytest.raises(ValueError, match="window"):
        f2.images.hmc_step(f2.sources, p0, imass, 0.1, 2, seed, conditional="exact", mask="honour")
    f2.images.set_window(0, 128)
    # new pixels: every sampler names the mask first while the option is off, the missing split once it is on
    f2.images.set_nelec(nan_win)
    calls = [lambda **kw: f2.images.slice_sample(f2.sources, 0, 1e-3, seed, step_out=False, conditional="exact", **kw),
             lambda **kw: f2.images.slice_sample(f2.sources, 1, 1.0, seed, conditional="exact", **kw),
             lambda **kw: f2.images.type_move(f2.sources, shapes, h, seed, conditional="exact", **kw),
             lambda **kw: f2.images.hmc_step(f2.sources, p0, imass, 0.1, 2, seed, conditional="exact", **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="masked"):
            call()
        with pytest.raises(ValueError, match="resident photon split"):
            call(mask="honour")
    for k in (K, HM, SC, GC):
        assert fresh_ctx.get_option(k) == 0 and ctx.get_option(k) == 0
    scene.reset()
