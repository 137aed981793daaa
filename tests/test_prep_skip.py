"""No source preparation when the records and the tile lists still stand (FieldState::prep_stands in csrc/field_state.h, render_impl,
BIN_LEAVE in csrc/k_prep_bin.h).

k_prep's records are a function of the catalogue's rows, the bands' WCS and PSF tables, the window and the source count.  A general
render whose image set still holds the records of exactly this catalogue generation, and the lists its last render binned from
them, launches no k_prep, and its binning launch leaves every word as it is.  One long-lived image set and catalogue are taken
through every step that may or may not leave that promise standing.  After every step

  * the FIRST render runs under ctx.profile(1), and profile_get("prep")[1] must be 0 exactly where the skip is claimed and 1 where
    it is not;
  * model images, ll, per-band sums, stats(), source_boxes and estep_stats must equal, bit for bit, those of an image set and a
    catalogue created fresh in a fresh context for the same state.

Two fields, those of tests/test_prep_bin_reuse.py: (a) 4 400 mixed sources, 2 bands, 512 x 512 -- k_bin_fine_blk; (b) 60 mixed
sources, 2 bands, 128 x 192 -- k_bin_direct -- with one source off the frame, one star in a corner and one galaxy below k_prep's
1/30" floor.  CEL_OPT_TILE_PARTS = 1, so the dirty-tile render takes part in the set_rows steps.

Two steps need a word.  "The same catalogue rendered into a second image set and back": the second set's render must prepare (its
tables hold nothing), and it writes its OWN tables; the stamps are per image set, so the first set's records still stand when the
catalogue comes back, and the skip is claimed there (0).  "A star-only catalogue that takes k_small_stars": that kernel prepares
inside itself, so its render shows one `small_stars` launch and no `prep`; the mixed catalogue after it must prepare.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu
B = 2
FIELDS = {"fine": dict(S=4400, H=512, W=512, seed=11), "direct": dict(S=60, H=128, W=192, seed=12)}
OFF, CORNER, THIN, STAR, GAL = 0, 1, 2, 3, 4          # rows with a part to play
SIGMA_LOC = 1e-3


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def make_field(cel, name):
    from desi_mcmc_amd import synth
    f = FIELDS[name]
    S, H, W = f["S"], f["H"], f["W"]
    bands = synth.make_bands(H, W, B)
    src = synth.make_sources(S, H, W, bands, 0.5, f["seed"])
    typ, shape, counts, pix = src["type"].copy(), src["shape"].copy(), src["counts"].copy(), src["pix"].copy()
    typ[[OFF, CORNER, STAR]] = 0
    typ[[THIN, GAL]] = 1
    pix[OFF] = (-500.0, 80.0)
    pix[CORNER] = (1.5, 2.0)
    pix[STAR] = (W / 2 + 8.5, H / 2 + 4.5)                  # half-pixel positions: 1e-7 px keeps the box, 1.5 px shifts it
    pix[GAL] = (W / 2 - 20.5, H / 2 - 10.5)
    shape[THIN, 1] = 0.02                                  # below the 1/30 floor
    shape[typ == 0] = 0.0
    radec = synth.pixel2equa(bands[0], pix)
    ctx = cel.Context(0)
    im = cel.ImageSet(ctx, bands, H, W)
    im.render(cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape))
    lam = im.model_images()
    nelec = np.random.RandomState(f["seed"] + 1).poisson(lam).astype(np.float64)
    nelec2 = np.random.RandomState(f["seed"] + 2).poisson(lam).astype(np.float64)
    im.close()
    return dict(S=S, H=H, W=W, bands=bands, cat=[typ, radec, counts, shape], pix=pix, nelec=nelec, nelec2=nelec2)


def outputs(im, ss, ctx=None, count=None):
    """the first render (timed per kernel when `count` is a dict: its launches of k_prep and k_small_stars), then everything else"""
    if count is not None:
        ctx.profile(1)
    ll, llb = im.render(ss, loglik=True)
    if count is not None:
        count["prep"], count["small_stars"] = ctx.profile_get("prep")[1], ctx.profile_get("small_stars")[1]
        ctx.profile(0)
        count["dirty"] = im.last_render_dirty_tiles() >= 0          # the dirty-tile render took this one
    out = dict(ll=np.float64(ll), llb=llb, lam=im.model_images(), stats=np.array([v for _, v in sorted(im.stats().items())], dtype=np.float64))
    out["boxes"], out["status"] = im.source_boxes(ss)
    out["xtilde"], out["mass"], out["noise"] = im.estep_stats(ss)        # (a render of its own, then the walk over the tile lists)
    return out


class Pair(object):
    """the long-lived image set and catalogue, and what a fresh pair gives for the same state"""

    def __init__(self, cel, fld):
        self.cel, self.f = cel, fld
        self.L = cel._lib
        self.ctx = self.context()
        self.eps = fld["bands"][:, 0].copy()
        self.window = (0, fld["H"])
        self.nelec = fld["nelec"]
        self.cat = [np.array(a, copy=True) for a in fld["cat"]]
        self.pix = fld["pix"].copy()
        self.im = cel.ImageSet(self.ctx, fld["bands"], fld["H"], fld["W"], nelec=fld["nelec"])
        self.ss = cel.SourceSet(self.ctx, fld["S"], B).set(*self.cat)
        self.inc = 1

    def context(self):
        ctx = self.cel.Context(0)
        ctx.set_option(self.L.CEL_OPT_TILE_PARTS, 1)
        return ctx

    def radec_of(self, row):
        from desi_mcmc_amd import synth
        return synth.pixel2equa(self.f["bands"][0], self.pix[row:row + 1])[0]

    def prep_launches(self, ss=None, loglik=True):
        """one render of the long-lived set under the per-kernel timing: its k_prep launches"""
        self.ctx.profile(1)
        self.im.render(ss or self.ss, loglik=loglik)
        n = self.ctx.profile_get("prep")[1]
        self.ctx.profile(0)
        return n

    def check(self, what, prep, ss=None, cat=None, small_stars=0, dirty=False):
        ss, cat = ss or self.ss, cat or self.cat
        count = {}
        got = outputs(self.im, ss, self.ctx, count)
        want = dict(prep=prep, small_stars=small_stars, dirty=dirty)
        assert count == want, "%s: the first render gave %r, expected %r" % (what, count, want)
        ctx = self.context()
        ctx.set_option(self.L.CEL_OPT_INCREMENTAL, self.inc)
        bands = self.f["bands"].copy()
        bands[:, 0] = self.eps
        im = self.cel.ImageSet(ctx, bands, self.f["H"], self.f["W"], nelec=self.nelec)
        if self.window != (0, self.f["H"]):
            im.set_window(*self.window)
        want = outputs(im, self.cel.SourceSet(ctx, len(cat[0]), B).set(*cat))
        im.close()
        for k in want:
            assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), "%s: %s differs from a fresh image set's" % (what, k)
        return got

    def set_rows(self, rows):
        rows = np.asarray(rows)
        self.ss.set_rows(rows, self.cat[0][rows], self.cat[1][rows], self.cat[2][rows], self.cat[3][rows])

    def base(self):
        """a log-likelihood render of the current generation: image, partials, lists and records for the dirty-tile render to start
        from (check() ends on the E-step, which overwrites the partials)"""
        self.im.render(self.ss, loglik=True)

    def move(self, row, dx, dy=0.0):
        self.base()
        self.pix[row] += (dx, dy)
        self.cat[1][row] = self.radec_of(row)
        self.set_rows([row])


@gpu
@pytest.mark.parametrize("name", ["fine", "direct"])
def test_render_skips_k_prep_exactly_while_records_and_lists_stand(cel, name):
    fld = make_field(cel, name)
    p = Pair(cel, fld)
    rs = np.random.RandomState(5)
    S, H, W = fld["S"], fld["H"], fld["W"]
    first = p.check("first render", 1)
    # ---- the render must skip ----
    p.check("unchanged", 0)
    p.check("unchanged, again", 0)
    p.eps[0] *= 1.25
    p.im.set_epsilon(0, p.eps[0])
    p.check("set_epsilon", 0)
    p.nelec = fld["nelec2"]
    p.im.set_nelec(p.nelec)
    p.check("set_nelec with new pixels", 0)
    assert p.prep_launches(loglik=False) == 0
    p.check("render(loglik=False) then render(loglik=True), unchanged", 0)
    p.im.source_boxes(p.ss)
    p.check("source_boxes in between, records current", 0)
    # ---- the render must prepare ----
    b0 = p.check("before the moves", 0)["boxes"]
    p.move(STAR, 1e-7)
    b1 = p.check("set_rows of one row, inside its box (no binning runs)", 1, dirty=True)["boxes"]
    assert np.array_equal(b0, b1)
    p.check("unchanged after the move", 0)
    p.move(STAR, 1.5)
    b2 = p.check("set_rows of one row, the box shifts", 1, dirty=True)["boxes"]
    assert not np.array_equal(b1[:, STAR], b2[:, STAR]) and np.array_equal(np.delete(b1, STAR, 1), np.delete(b2, STAR, 1))
    # a plain render prepares, the log-likelihood behind it does not
    p.move(STAR, -1.5)
    assert p.prep_launches(loglik=False) == 1
    p.check("render(loglik=False) then render(loglik=True), after a move", 0)
    # source_boxes prepares the new generation itself; the render behind it must prepare again all the same: a k_prep outside a
    # render zeroed the cursor words and compared against no binning's step (records_written drops binned_S)
    p.move(STAR, 1.5)
    p.im.source_boxes(p.ss)
    p.check("source_boxes prepared the new generation itself", 1)
    # across a tile edge: the star's box comes to lie over the column W/2 between two 32-column tiles
    p.move(STAR, -(p.pix[STAR, 0] - (W / 2 + 0.5)))
    p.check("set_rows of one row, across a tile edge", 1, dirty=True)
    p.check("unchanged after the tile edge", 0)
    back = p.pix[STAR].copy()
    p.move(STAR, -600.0 - back[0])
    p.check("set_rows of one row, off the frame", 1, dirty=True)
    p.move(STAR, back[0] - p.pix[STAR, 0])
    p.check("set_rows of one row, back on the frame", 1, dirty=True)
    p.base()
    p.cat[0][STAR], p.cat[3][STAR] = 1, (0.5, 1.0, 20.0, 0.7)
    p.set_rows([STAR])
    p.check("set_rows of one row, star -> galaxy", 1, dirty=True)
    p.base()
    p.cat[0][STAR], p.cat[3][STAR] = 0, 0.0
    p.set_rows([STAR])
    p.check("set_rows of one row, galaxy -> star", 1, dirty=True)
    # 60 rows in two batches of 30 before one render: within the dirty-tile render's 64 rows
    rows60 = np.arange(5, 5 + 60) if S > 65 else np.arange(S)
    p.base()
    for batch in (rows60[:30], rows60[30:]):
        p.pix[batch] += rs.uniform(-1.5, 1.5, (len(batch), 2))
        for r in batch:
            p.cat[1][r] = p.radec_of(r)
        p.set_rows(batch)
    p.check("60 rows in two batches", 1, dirty=True)
    p.check("unchanged after the batches", 0)
    # more than 64 rows: the full render
    many = rs.choice(S, 70, replace=False) if S >= 70 else np.arange(S)
    p.cat[2][many] *= rs.uniform(0.5, 2.0, (len(many), 1))
    p.pix[many[:8]] += 0.75
    for r in many[:8]:
        p.cat[1][r] = p.radec_of(r)
    p.set_rows(many)
    if S >= 70:
        p.check("set_rows of more than 64 rows", 1)
    else:       # (field (b) holds 60 sources: every row, twice, so that 120 row changes lie between two renders)
        p.set_rows(many)
        p.check("set_rows of every row, twice", 1)
    p.ss.set(*p.cat)
    p.check("sources.set of the whole catalogue, identical values: a new generation", 1)
    p.check("unchanged after the upload", 0)
    # a second catalogue object into the set, and the first one after it
    other = [np.array(a, copy=True) for a in p.cat]
    other[1] = other[1][rs.permutation(S)]
    ss2 = cel.SourceSet(p.ctx, S, B).set(*other)
    p.check("a second catalogue object", 1, ss2, other)
    p.check("the first catalogue after it", 1)
    p.check("the second again", 1, ss2, other)
    p.check("the second, unchanged", 0, ss2, other)
    p.check("the first, second time", 1)
    # the same catalogue into a second image set (of the same context) and back: see the module docstring
    bands = fld["bands"].copy()
    bands[:, 0] = p.eps
    im2 = cel.ImageSet(p.ctx, bands, H, W, nelec=p.nelec)
    p.ctx.profile(1)
    ll2, _ = im2.render(p.ss, loglik=True)
    assert p.ctx.profile_get("prep")[1] == 1
    p.ctx.profile(0)
    got = p.check("back from a second image set", 0)
    assert np.float64(ll2).tobytes() == got["ll"].tobytes()
    im2.close()
    # another window and back
    p.window = (32, H + 64)
    p.im.set_window(*p.window)
    p.check("set_window to another window", 1)
    p.check("the window, unchanged", 0)
    p.window = (0, H)
    p.im.set_window(*p.window)
    p.check("set_window back", 1)
    # a photon split prepares nothing anew; a device slice-sampler round runs the box-less k_prep and moves the catalogue
    p.im.photon_split_resident(p.ss, 17)
    p.check("after a photon split of this generation", 0)
    p.im.photon_split_resident(p.ss, 18)
    p.im.slice_locations(p.ss, SIGMA_LOC, 19)
    moved = p.ss.get()
    assert not np.array_equal(moved[1], p.cat[1])
    p.cat = [np.array(a, copy=True) for a in moved]
    p.check("after a device slice-sampler round", 1)
    p.check("unchanged after the slice sampler", 0)
    # a flux step writes the device rows
    p.im.photon_split_resident(p.ss, 20)
    p.im.flux_conditionals(p.ss, 21, 5.0, 0.005, [0, 1], fld["bands"][:, 2].copy(), fld["bands"][:, 1].copy())
    fluxed = p.ss.get()
    assert not np.array_equal(fluxed[2], p.cat[2])
    p.cat = [np.array(a, copy=True) for a in fluxed]
    p.check("after a flux step", 1)
    p.check("unchanged after the flux step", 0)
    # the option off: never
    p.inc = 0
    p.ctx.set_option(p.L.CEL_OPT_INCREMENTAL, 0)
    p.check("option off", 1)
    p.check("option off, unchanged", 1)
    p.im.set_epsilon(1, p.eps[1])
    p.check("option off, set_epsilon", 1)
    p.inc = 1
    p.ctx.set_option(p.L.CEL_OPT_INCREMENTAL, 1)
    p.check("option on again: what the render with the option off left stands", 0)
    # a larger catalogue regrows the record buffer
    n_big = 2 * S                                           # (the buffer holds 1.25 S B + 64 records)
    big = [np.concatenate([a, a]) for a in p.cat]
    big[1][S:] += 2e-4
    ss_big = cel.SourceSet(p.ctx, n_big, B).set(*big)
    p.check("a larger catalogue", 1, ss_big, big)
    p.check("the larger catalogue, unchanged", 0, ss_big, big)
    p.check("the first after the larger", 1)
    # a star-only catalogue takes k_small_stars, then the mixed one again
    n_st = min(S, 300)
    stars = [np.array(a[:n_st], copy=True) for a in p.cat]
    stars[0][:] = 0
    stars[3][:] = 0.0
    ss_st = cel.SourceSet(p.ctx, n_st, B).set(*stars)
    p.check("a star-only catalogue", 0, ss_st, stars, small_stars=1)
    p.check("the star-only catalogue, again", 0, ss_st, stars, small_stars=1)
    p.check("the mixed catalogue after it", 1)
    p.check("the mixed catalogue, unchanged", 0)
    assert first["stats"][2] > 0                            # n_tile_entries: the lists were there to be walked
    p.im.close()
