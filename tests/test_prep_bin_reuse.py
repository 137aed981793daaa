"""Binning only when a box or a kind changed (csrc/k_prep_bin.h, k_bin2.h; ListStamps::binned_S in field_state.h).

k_prep compares, on the device and on every call, the (box, kind) it is about to store with what stands in the tables; the binning
kernels return at once when it found no difference and the host vouches that the lists in front of them were binned from exactly
that table.  One long-lived image set is taken through everything that can make that promise false; after every step its model
images, log-likelihoods, stats(), source boxes and E-step sums (which walk the tile lists) are compared BIT FOR BIT with an image
set created fresh in a fresh context for the same state.

Two fields: (a) 4 400 mixed sources, 2 bands, 512 x 512 -- above the 4 096 up to which k_bin_direct is taken, so k_bin_fine_blk
runs; (b) 60 mixed sources, 2 bands, 128 x 192 -- k_bin_direct -- with one source off the frame, one star in a corner and one
galaxy below k_prep's 1/30" floor.  Both contexts render with one block per tile (CEL_OPT_TILE_PARTS = 1), so the dirty-tile render
takes part in the set_rows steps.

Left out: a forced list overflow in the middle of the sequence -- the API has no way to start a set with a small list capacity.
(The retry path itself bins with force = 1 and is run by every first render whose first guess of the list size is too small.)

test_unchanged_binning_returns_at_once shows that the short cut is taken: the binning launch of a render with nothing changed
must take less than 0.6 of one whose box moved -- and the same with the option off must not.
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
    nelec = np.random.RandomState(f["seed"] + 1).poisson(im.model_images()).astype(np.float64)
    im.close()
    return dict(S=S, H=H, W=W, bands=bands, cat=[typ, radec, counts, shape], pix=pix, nelec=nelec)


def outputs(im, ss):
    ll, llb = im.render(ss, loglik=True)
    out = dict(ll=np.float64(ll), llb=llb, lam=im.model_images(), stats=np.array([v for _, v in sorted(im.stats().items())], dtype=np.float64))      # n_gauss, n_srcpix, n_tile_entries
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

    def check(self, what, ss=None, cat=None):
        ss, cat = ss or self.ss, cat or self.cat
        got = outputs(self.im, ss)
        ctx = self.context()
        ctx.set_option(self.L.CEL_OPT_INCREMENTAL, self.inc)
        bands = self.f["bands"].copy()
        bands[:, 0] = self.eps
        im = self.cel.ImageSet(ctx, bands, self.f["H"], self.f["W"], nelec=self.f["nelec"])
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


@gpu
@pytest.mark.parametrize("name", ["fine", "direct"])
def test_long_lived_set_equals_a_fresh_one_after_every_step(cel, name):
    fld = make_field(cel, name)
    p = Pair(cel, fld)
    rs = np.random.RandomState(3)
    S = fld["S"]
    first = p.check("first render")
    # 1. nothing changed, three times
    for k in range(3):
        p.check("1. nothing changed (%d)" % k)
    # 2. all fluxes changed, by set and by set_rows
    p.cat[2] = p.cat[2] * rs.uniform(0.5, 2.0, p.cat[2].shape)
    p.ss.set(*p.cat)
    p.check("2. fluxes by set")
    p.cat[2] = p.cat[2] * rs.uniform(0.5, 2.0, p.cat[2].shape)
    p.set_rows(np.arange(S))
    p.check("2. fluxes by set_rows")
    few = rs.choice(S, 5, replace=False)
    p.cat[2][few] *= 1.5
    p.set_rows(few)
    p.check("2. five fluxes by set_rows")
    # 3. one position moved by 1e-7 px: the same box
    b0 = p.check("before 3.")["boxes"]
    p.pix[STAR, 0] += 1e-7
    p.cat[1][STAR] = p.radec_of(STAR)
    p.set_rows([STAR])
    b1 = p.check("3. 1e-7 px")["boxes"]
    assert np.array_equal(b0, b1)
    # 4. one position moved by 1.5 px: the box shifts
    p.pix[STAR, 0] += 1.5
    p.cat[1][STAR] = p.radec_of(STAR)
    p.set_rows([STAR])
    b2 = p.check("4. 1.5 px")["boxes"]
    assert not np.array_equal(b1[:, STAR], b2[:, STAR]) and np.array_equal(np.delete(b1, STAR, 1), np.delete(b2, STAR, 1))
    p.pix[GAL, 1] -= 1.5
    p.cat[1][GAL] = p.radec_of(GAL)
    p.ss.set(*p.cat)                                        # ... and by a whole-catalogue upload
    p.check("4. 1.5 px by set")
    # 5. one galaxy's shape changed
    p.cat[3][GAL] = (0.3, 2.5, 70.0, 0.5)
    p.set_rows([GAL])
    p.check("5. shape")
    p.cat[3][THIN, 1] = 0.03                                # (still below the floor: the same record but for theta ... )
    p.set_rows([THIN])
    p.check("5. shape below the floor")
    # 6. a star turned galaxy and back, counts unchanged
    p.cat[0][STAR], p.cat[3][STAR] = 1, (0.5, 1.0, 20.0, 0.7)
    p.set_rows([STAR])
    p.check("6. star -> galaxy")
    p.cat[0][STAR], p.cat[3][STAR] = 0, 0.0
    p.set_rows([STAR])
    p.check("6. galaxy -> star")
    # 7. a new sky level
    p.eps[0] *= 1.25
    p.im.set_epsilon(0, p.eps[0])
    p.check("7. sky level")
    # 8. a new window and back
    p.window = (32, fld["H"] + 64)
    p.im.set_window(*p.window)
    p.check("8. window")
    p.check("8. window, again")
    p.window = (0, fld["H"])
    p.im.set_window(*p.window)
    p.check("8. window back")
    # 9. another catalogue object of the same S in between
    other = [np.array(a, copy=True) for a in p.cat]
    perm = rs.permutation(S)
    other[1] = other[1][perm]
    ss2 = cel.SourceSet(p.ctx, S, B).set(*other)
    p.check("9. another object", ss2, other)
    p.check("9. the first again")
    p.check("9. another object again", ss2, other)
    p.check("9. the first, second time")
    # 10. a catalogue of another S, then the first again
    fewer = [np.array(a[:S - 7], copy=True) for a in p.cat]
    ss3 = cel.SourceSet(p.ctx, S - 7, B).set(*fewer)
    p.check("10. another S", ss3, fewer)
    p.check("10. the first again")
    # 11. a photon split and a slice-sampler round in between: their partial k_prep writes the tables
    p.im.render(p.ss, loglik=True)
    p.im.photon_split_resident(p.ss, 17)
    p.check("11. after the split")
    p.im.photon_split_resident(p.ss, 18)
    p.im.slice_locations(p.ss, SIGMA_LOC, 19)
    moved = p.ss.get()
    assert not np.array_equal(moved[1], p.cat[1])
    p.cat = [np.array(a, copy=True) for a in moved]
    p.check("11. after the slice sampler")
    p.check("11. after the slice sampler, again")
    # 13. the option off, then on
    p.inc = 0
    p.ctx.set_option(p.L.CEL_OPT_INCREMENTAL, 0)
    p.check("13. option off")
    p.cat[2][few] *= 0.5
    p.set_rows(few)
    p.check("13. option off, fluxes")
    p.inc = 1
    p.ctx.set_option(p.L.CEL_OPT_INCREMENTAL, 1)
    p.check("13. option on")
    p.check("13. option on, again")
    assert first["stats"][2] > 0                            # n_tile_entries: the lists were there to be walked
    p.im.close()


@gpu
def test_unchanged_binning_returns_at_once(cel):
    """field (a), HIP-event time of the binning launch (ctx.profile(1), "bin"): 20 renders with nothing changed against 20 with
    one box shifted each time.  A real binning pass has a floor of 15-17 us, a launch whose blocks return takes a few: the
    unchanged median must be below 0.6 of the changed one; with CEL_OPT_INCREMENTAL off both bin, and the ratio is near 1."""
    fld = make_field(cel, "fine")
    p = Pair(cel, fld)

    def medians():
        p.im.render(p.ss, loglik=True)
        p.im.render(p.ss, loglik=True)
        t = {"same": [], "moved": []}
        for k in range(40):
            kind = "moved" if k % 2 else "same"
            if kind == "moved":
                p.pix[STAR, 0] += 1.5 if (k // 2) % 2 else -1.5
                p.cat[1][STAR] = p.radec_of(STAR)
                p.set_rows([STAR])
            p.ctx.profile(1)
            p.im.render(p.ss, loglik=True)
            ms, n = p.ctx.profile_get("bin")
            assert n == 1
            t[kind].append(ms)
        p.ctx.profile(0)
        return float(np.median(t["same"])), float(np.median(t["moved"]))

    same, moved = medians()
    print("binning launch, option on:  unchanged %.2f us, one box shifted %.2f us" % (same * 1e3, moved * 1e3))
    p.ctx.set_option(p.L.CEL_OPT_INCREMENTAL, 0)
    same0, moved0 = medians()
    print("binning launch, option off: unchanged %.2f us, one box shifted %.2f us" % (same0 * 1e3, moved0 * 1e3))
    assert same < 0.6 * moved, (same, moved)
    assert 0.8 < same0 / moved0 < 1.25, (same0, moved0)       # (the same kernel doing the same work twice: event jitter of 1-2 us on 17 and more)
    p.im.close()
