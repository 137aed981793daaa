"""The component cache of the general render (csrc/k_comps.h, k_render_hwc in csrc/k_render_hw.h, RecordStamps::comps_of_records in
csrc/field_state.h, CEL_OPT_COMP_CACHE).

A render that launches no k_prep builds every record's mixture components once (k_comps, counted under the "gmm" timing slot) and
this and every later such render loads them per tile entry instead of computing them.  The rows hold the bits the plain kernel
computes, so a render with the cache is, in every bit, the render without it; and the cache is read only while it is of exactly
the records that stand on the device.

Field.  2 bands under the rotated, per-band WCS of tests/_general_wcs.py on a 96 x 160 frame -- three tile columns, two and a half
tile rows (the last one ragged); CEL_OPT_TILE_PARTS = 1, or a frame this small would take the PARTS = 4 kernel and never reach the
cached one.  111 sources: 70 small galaxies inside the tile (1, 0), so that its list passes 64 entries and the prefetch crosses
the reload of the list indices; galaxies from 0.02" (below k_prep's floor) to 40" (every tile), centred off every edge, with
theta = 0 and theta = 1 (zero-amplitude components); stars on and off the frame.  `sharp`: band 1's first PSF component has the
covariance 0.012 I, so that the smallest galaxy's sharpest pair of groups takes the direct fallback (L < 4) and band 1's stars are
refused by the star pass and reach the general path -- with the components of their rows.
"""
import numpy as np
import pytest

from _general_wcs import general_bands

gpu = pytest.mark.gpu
B, H, W = 2, 160, 96
GAL = 75                      # the galaxy the state walk moves
SEED = 31


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def catalogue(bands):
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(SEED)
    pix, typ, shape, flux = [], [], [], []

    def add(x, y, t, theta=0.5, sigma=1.0, phi=30.0, rho=0.6, f=20.0):
        pix.append((x, y)); typ.append(t); shape.append((theta, sigma, phi, rho) if t else (0.0, 0.0, 0.0, 0.0)); flux.append(f)

    for _ in range(70):                                        # rows 0 .. 69: inside the tile of columns 32 .. 63, rows 0 .. 63
        add(rs.uniform(44.0, 52.0), rs.uniform(24.0, 40.0), 1, rs.uniform(0.05, 0.95), rs.uniform(0.2, 0.6), rs.uniform(0, 180), rs.uniform(0.3, 0.9),
            rs.uniform(2.0, 30.0))
    add(48.3, 80.7, 1, 0.4, 0.02, 10.0, 0.5, 50.0)             # 70: sub-pixel, below the 1/30" floor (sharp: the direct fallback)
    add(47.5, 79.5, 1, 0.6, 40.0, 75.0, 0.7, 4000.0)           # 71: spans every tile
    add(20.2, 140.1, 1, 0.0, 3.0, 120.0, 0.4, 300.0)           # 72: theta = 0 -- the six exp components have amplitude 0
    add(70.9, 30.3, 1, 1.0, 2.0, 50.0, 0.8, 200.0)             # 73: theta = 1 -- the eight dev components
    add(31.5, 63.5, 1, 0.3, 1.5, 0.0, 0.95, 100.0)             # 74: on a tile corner
    add(40.25, 100.75, 1, 0.5, 2.5, 140.0, 0.5, 150.0)         # 75: GAL
    for x, y in ((-3.2, 50.0), (W + 2.6, 90.0), (30.0, -4.1), (60.0, H + 3.3), (-6.0, -5.0), (W + 5.0, H + 6.0)):     # 76 .. 81: off every edge
        add(x, y, 1, rs.uniform(0.1, 0.9), rs.uniform(1.0, 5.0), rs.uniform(0, 180), rs.uniform(0.3, 0.9), 120.0)
    for _ in range(14):                                        # 82 .. 95: anywhere, a range of sizes
        add(rs.uniform(0, W), rs.uniform(0, H), 1, rs.uniform(0.05, 0.95), np.exp(rs.uniform(np.log(0.3), np.log(12.0))), rs.uniform(0, 180),
            rs.uniform(0.2, 0.95), rs.uniform(5.0, 500.0))
    for x, y in ((10.5, 12.5), (48.0, 33.0), (95.2, 159.1), (0.4, 70.0), (64.0, 128.0), (-2.0, 20.0), (33.3, 64.2), (80.1, 150.6)):   # 96 .. 103: stars
        add(x, y, 0, f=rs.uniform(5.0, 200.0))
    for _ in range(7):                                         # 104 .. 110
        add(rs.uniform(0, W), rs.uniform(0, H), 0, f=rs.uniform(5.0, 200.0))
    pix, typ, shape = np.array(pix), np.array(typ, dtype=np.int32), np.array(shape)
    flux = np.array(flux)[:, None] * np.array([1.0, 0.7])[None, :]
    counts = flux / bands[None, :, 2] * bands[None, :, 1]
    assert typ[GAL] == 1 and len(typ) == 111
    return [typ, synth.pixel2equa(bands[0], pix), counts, shape], pix


def make_field(cel, sharp):
    bands = general_bands(H, W, B)
    if sharp:
        bands[1, 12:16] = (0.012, 0.0, 0.0, 0.012)
    cat, pix = catalogue(bands)
    ctx = context(cel, 0)
    im = cel.ImageSet(ctx, bands, H, W)
    im.render(cel.SourceSet(ctx, len(cat[0]), B).set(*cat))
    nelec = np.random.RandomState(SEED + 1).poisson(im.model_images()).astype(np.float64)
    im.close()
    return dict(bands=bands, cat=cat, pix=pix, nelec=nelec)


def context(cel, cache, tail_log=None):
    ctx = cel.Context(0)
    ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, 1)
    ctx.set_option(cel._lib.CEL_OPT_COMP_CACHE, cache)
    if tail_log is not None:
        ctx.set_tail_log(tail_log)
    return ctx


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@gpu
@pytest.mark.parametrize("tail_log", [8.0, 24.0, 32.0])
@pytest.mark.parametrize("sharp", [False, True])
def test_cached_render_is_the_plain_render_in_every_bit(cel, tail_log, sharp):
    fld = make_field(cel, sharp)
    got = {}
    for cache in (0, 1):
        ctx = context(cel, cache, tail_log)
        assert ctx.get_option(cel._lib.CEL_OPT_COMP_CACHE) == cache
        im = cel.ImageSet(ctx, fld["bands"], H, W, nelec=fld["nelec"])
        ss = cel.SourceSet(ctx, len(fld["cat"][0]), B).set(*fld["cat"])
        out = []
        ctx.profile(1)
        im.render(ss)                                         # prepares: the plain kernel
        im.render(ss)                                         # builds the rows; the cached kernel from here on
        out.append(words(im.model_images()))
        ll, llb = im.render(ss, loglik=True)
        out += [words(im.model_images()), words(ll), words(llb)]
        ll, llb = im.render(ss, loglik=True, store=False)
        out += [words(ll), words(llb)]
        assert ctx.profile_get("prep")[1] == 1 and ctx.profile_get("gmm")[1] == cache
        im.set_window(32, H + 64)                             # a row window: the set holds rows 32 .. 32 + H of a taller frame
        im.render(ss)
        im.render(ss)
        out.append(words(im.model_images()))
        ll, llb = im.render(ss, loglik=True)
        out += [words(im.model_images()), words(ll), words(llb)]
        assert ctx.profile_get("prep")[1] == 2 and ctx.profile_get("gmm")[1] == 2 * cache
        ctx.profile(0)
        got[cache] = out
        assert im.stats()["n_tile_entries"] > 0
        im.close()
    assert got[1][0].max() > 0
    for i, (a, b) in enumerate(zip(got[0], got[1])):
        assert a.shape == b.shape and np.array_equal(a, b), "output %d differs between the cache on and off (tail_log %g, sharp %r)" % (i, tail_log, sharp)


class Walk(object):
    """one long-lived image set and catalogue with the cache on; after every step a render is counted (its k_prep and k_comps
    launches) and compared bit for bit with a fresh context's, image set's and catalogue's render with the option off"""

    def __init__(self, cel, fld):
        self.cel, self.f, self.L = cel, fld, cel._lib
        self.ctx = context(cel, 1)
        self.eps = fld["bands"][:, 0].copy()
        self.window = (0, H)
        self.cat = [np.array(a, copy=True) for a in fld["cat"]]
        self.pix = fld["pix"].copy()
        self.im = cel.ImageSet(self.ctx, fld["bands"], H, W, nelec=fld["nelec"])
        self.ss = cel.SourceSet(self.ctx, len(self.cat[0]), B).set(*self.cat)

    def fresh(self, cat):
        ctx = context(self.cel, 0)
        bands = self.f["bands"].copy()
        bands[:, 0] = self.eps
        im = self.cel.ImageSet(ctx, bands, H, W, nelec=self.f["nelec"])
        if self.window != (0, H):
            im.set_window(*self.window)
        ll, llb = im.render(self.cel.SourceSet(ctx, len(cat[0]), B).set(*cat), loglik=True)
        out = [words(im.model_images()), words(ll), words(llb)]
        im.close()
        return out

    def check(self, what, prep, comps, ss=None, cat=None, im=None, small_stars=0, dirty=False, loglik=True):
        ss, cat, im = ss or self.ss, cat or self.cat, im or self.im
        self.ctx.profile(1)
        r = im.render(ss, loglik=loglik)
        count = dict(prep=self.ctx.profile_get("prep")[1], comps=self.ctx.profile_get("gmm")[1], small_stars=self.ctx.profile_get("small_stars")[1],
                     dirty=im.last_render_dirty_tiles() >= 0)
        self.ctx.profile(0)
        want = dict(prep=prep, comps=comps, small_stars=small_stars, dirty=dirty)
        assert count == want, "%s: the render launched %r, expected %r" % (what, count, want)
        ref = self.fresh(cat)
        assert np.array_equal(words(im.model_images()), ref[0]), "%s: the model image differs from a fresh plain render's" % what
        if loglik:
            assert np.array_equal(words(r[0]), ref[1]) and np.array_equal(words(r[1]), ref[2]), "%s: the log-likelihood differs" % what

    def twice(self, what, **kw):
        """a state the set has not rendered yet: the first render prepares and takes the plain kernel, the second builds the rows"""
        self.check(what, 1, 0, **kw)
        self.check(what + ", again", 0, 1, **kw)


@gpu
def test_cache_is_built_once_per_record_generation_and_never_read_stale(cel):
    from desi_mcmc_amd import synth
    fld = make_field(cel, False)
    w = Walk(cel, fld)
    rs = np.random.RandomState(7)
    S = len(w.cat[0])
    w.check("1. first render", 1, 0)
    w.check("2. second render", 0, 1)
    w.check("3. third render", 0, 0)
    w.eps[0] *= 1.25
    w.im.set_epsilon(0, w.eps[0])
    w.check("4. a new sky level", 0, 0)
    w.check("4. without the log-likelihood", 0, 0, loglik=False)
    w.check("4. ... and with it again", 0, 0)
    # 5. one source moved by several pixels: the dirty-tile render prepares and takes the plain kernel; rows of the old position,
    # read by anyone, would show in the tiles it renders
    w.pix[GAL] += (5.5, 3.0)
    w.cat[1][GAL] = synth.pixel2equa(fld["bands"][0], w.pix[GAL:GAL + 1])[0]
    w.ss.set_rows(np.array([GAL]), w.cat[0][[GAL]], w.cat[1][[GAL]], w.cat[2][[GAL]], w.cat[3][[GAL]])
    w.check("5. set_rows of one source", 1, 0, dirty=True)
    w.check("6. the render after it", 0, 1)
    w.ss.set(*w.cat)
    w.twice("7. the whole catalogue uploaded again, identical values")
    other = [np.array(a, copy=True) for a in w.cat]
    other[1] = other[1][rs.permutation(S)]
    ss2 = cel.SourceSet(w.ctx, S, B).set(*other)
    w.twice("8. another catalogue object", ss=ss2, cat=other)
    w.twice("8. the first catalogue back")
    bands = fld["bands"].copy()
    bands[:, 0] = w.eps
    im2 = cel.ImageSet(w.ctx, bands, H, W, nelec=fld["nelec"])
    w.twice("9. a second image set of the same catalogue", im=im2)
    w.check("9. the first image set meanwhile: its own stamps", 0, 0)
    im2.close()
    w.window = (32, H + 64)
    w.im.set_window(*w.window)
    w.twice("10. another window")
    w.window = (0, H)
    w.im.set_window(*w.window)
    w.twice("10. the window back")
    big = [np.concatenate([a, a]) for a in w.cat]               # (the record buffer holds 1.25 S B + 64)
    big[1][S:] += 2e-4
    ss_big = cel.SourceSet(w.ctx, 2 * S, B).set(*big)
    w.twice("11. a catalogue that re-allocates the records", ss=ss_big, cat=big)
    w.twice("11. the first catalogue after it")
    # 12. 4 200 wide galaxies: past k_bin_direct's 4 096 sources, and ~15 tiles each against the list buffer's room: the render
    # overflows its lists, grows them and bins again
    n = 4200
    pix = np.column_stack([rs.uniform(0, W, n), rs.uniform(0, H, n)])
    wide = [np.ones(n, dtype=np.int32), synth.pixel2equa(fld["bands"][0], pix), np.tile(w.cat[2][GAL], (n, 1)) * rs.uniform(0.01, 0.1, (n, 1)),
            np.column_stack([rs.uniform(0.1, 0.9, n), rs.uniform(8.0, 12.0, n), rs.uniform(0, 180, n), rs.uniform(0.3, 0.9, n)])]
    ss_wide = cel.SourceSet(w.ctx, n, B).set(*wide)
    w.twice("12. a list-buffer overflow and its retry", ss=ss_wide, cat=wide)
    assert w.im.stats()["n_tile_entries"] > 30 * 2 * S            # (more entries than the buffer held: 30 tiles x 222 sources, from step 11)
    w.twice("12. the first catalogue after it")
    w.ctx.set_option(w.L.CEL_OPT_COMP_CACHE, 0)
    w.check("13. the option off", 0, 0)
    w.ctx.set_option(w.L.CEL_OPT_COMP_CACHE, 1)
    w.check("13. the option on again: the rows still stand", 0, 0)
    stars = [np.array(a[96:], copy=True) for a in w.cat]
    assert not stars[0].any()
    ss_st = cel.SourceSet(w.ctx, len(stars[0]), B).set(*stars)
    w.check("14. a star-only catalogue: the one-launch render", 0, 0, ss=ss_st, cat=stars, small_stars=1)
    w.twice("14. the mixed catalogue after it")
    w.im.close()
