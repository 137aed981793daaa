"""Masked pixels (a NaN count: the pixel was not observed) in the field log-likelihood, its gradient and the E-step.

  1. the log-likelihood of a masked set under every render form: the model image is that of the set with finite counts, bit
     for bit, and ll_band is the exact sum over the unmasked pixels (k_masked_ll, a pass of its own behind the render)
  2. edges of the rule: a band masked everywhere, the per-band counts, no pass on a set without a NaN, negative counts are data
  3. the incremental render on a masked set;  4. row windows and owned rows
  5. the gradient's fill identity: r = 0 at a masked pixel, and r = lambda / lambda - 1 = 0 exactly at a pixel whose count is lambda
  6. the E-step's fill identity in all three forms (0 / lambda = 0 exactly) and the mass over the unmasked pixels
  7. d ll / d counts = xtilde / counts - mass with the mask on both sides;  8. the calls that refuse a masked set
"""
import math

import numpy as np
import pytest

from conftest import tail_log
from test_drop_contract import FIELD_FORMS, star_field
from test_drop_contract import H as HB, W as WB, NB
from test_loglik_grad import _scene
from test_loglik_grad import H as HG, W as WG, B as BG

pytestmark = pytest.mark.gpu

HA, WA, BA = 200, 150, 2          # frame A: 5 x 4 tiles of 32 x 64, a 22-column last tile column, an 8-row last tile row
EMPTY_TILE, SPARSE_TILE = (4, 1), (4, 2)          # (tx, ty) of the 32 x 64 layout: no source's box reaches column 128


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(cel):
    return cel.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


def mask_pattern(Hh, Ww, centres, block_at, whole_tile, sparse_tile, seed):
    """band 0's mask: the whole column 40; both sides of every tile seam at x in {31, 32, 63, 64}, y in {63, 64, 127, 128};
    the four frame corners (both ends of the last row and of the last column among them) and their neighbours along the last
    row and column; the pixel nearest each of `centres`; a 5 x 5 block; one whole 32 x 64 tile; three single pixels of another;
    1 % of the rest"""
    m = np.zeros((Hh, Ww), bool)
    m[:, 40] = True
    for y in (63, 64, 127, 128):
        for x in (31, 32, 63, 64):
            m[y, x] = True
    for y in (0, Hh - 1):
        for x in (0, Ww - 1):
            m[y, x] = True
    m[Hh - 1, 1] = m[Hh - 1, Ww - 2] = m[1, Ww - 1] = m[Hh - 2, Ww - 1] = True
    for cx, cy in centres:
        m[int(round(cy)), int(round(cx))] = True
    bx, by = int(round(block_at[0])), int(round(block_at[1]))
    m[by - 2:by + 3, bx - 2:bx + 3] = True
    tx, ty = whole_tile
    m[ty * 64:(ty + 1) * 64, tx * 32:(tx + 1) * 32] = True
    tx, ty = sparse_tile
    for dy, dx in ((0, 0), (17, 5), (40, 11)):
        m[ty * 64 + dy, tx * 32 + dx] = True
    m |= (~m) & (np.random.RandomState(seed).rand(Hh, Ww) < 0.01)
    return m


def sparse_mask(Hh, Ww, seed):
    return np.random.RandomState(seed).rand(Hh, Ww) < 0.01


def frame_a_catalogue():
    """24 stars and galaxies with centres in x in [8, 90], y in [8, 190] of frame A"""
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(11)
    S = 24
    bands = synth.make_bands(HA, WA, BA)
    pix = np.column_stack([rs.uniform(8, 90, S), rs.uniform(8, 190, S)])
    typ = (np.arange(S) % 2).astype(np.int32)                    # stars and galaxies alternate
    shape = np.column_stack([rs.uniform(0.1, 0.9, S), np.exp(rs.uniform(np.log(0.4), np.log(1.2), S)),
                             rs.uniform(0, 180, S), rs.uniform(0.3, 0.95, S)])
    shape[typ == 0] = 0.0
    counts = np.exp(rs.uniform(np.log(300.0), np.log(3e4), size=(S, BA)))
    return dict(bands=bands, typ=typ, pix=pix, radec=synth.pixel2equa(bands[0], pix), counts=counts, shape=shape, S=S)


def draw_counts(cel, ctx, bands, Hh, Ww, typ, pix, counts, shape, seed):
    """a Poisson draw of a render of the catalogue moved by 0.3 px and 5 %, as test_loglik_grad._scene does"""
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(seed)
    S, Bb = len(typ), bands.shape[0]
    iset = cel.ImageSet(ctx, bands, Hh, Ww)
    sset = cel.SourceSet(ctx, S, Bb).set(typ, synth.pixel2equa(bands[0], pix + rs.normal(0, 0.3, (S, 2))),
                                         counts * rs.uniform(0.95, 1.05, (S, Bb)), shape)
    iset.render(sset)
    nelec = rs.poisson(iset.model_images()).astype(np.float64)
    iset.close()
    return nelec


@pytest.fixture(scope="module")
def frame_a(cel, ctx):
    f = frame_a_catalogue()
    f["nelec"] = draw_counts(cel, ctx, f["bands"], HA, WA, f["typ"], f["pix"], f["counts"], f["shape"], 21)
    gal = int(np.nonzero(f["typ"] == 1)[0][4])                   # the 5 x 5 block sits on this galaxy
    f["block_gal"] = gal
    mask = np.zeros((BA, HA, WA), bool)
    mask[0] = mask_pattern(HA, WA, f["pix"][:6], f["pix"][gal], EMPTY_TILE, SPARSE_TILE, 5)
    mask[1] = sparse_mask(HA, WA, 6)
    f["mask"] = mask
    f["masked"] = np.where(mask, np.nan, f["nelec"])
    # no box reaches column 128: the tiles of the last tile column are empty
    probe = cel.ImageSet(ctx, f["bands"], HA, WA)
    boxes, status = probe.source_boxes(cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"]))
    probe.close()
    assert np.all(status > 0) and boxes[..., 3].max() <= 128, boxes[..., 3].max()
    f["boxes"] = boxes
    return f


@pytest.fixture(scope="module")
def frame_b(cel, ctx, orc):
    from desi_mcmc_amd import synth
    bands, typ, radec, counts, shape = star_field(orc)
    rs = np.random.RandomState(31)
    S = len(typ)
    iset = cel.ImageSet(ctx, bands, HB, WB)
    sset = cel.SourceSet(ctx, S, NB).set(typ, radec + rs.normal(0, 0.3 * 1.1e-4, (S, 2)), counts * rs.uniform(0.95, 1.05, (S, NB)), shape)
    iset.render(sset)
    nelec = rs.poisson(iset.model_images()).astype(np.float64)
    iset.close()
    mask = np.stack([sparse_mask(HB, WB, 40 + b) for b in range(NB)])
    pixc = np.array([[32.0, 64.0], [31.5, 63.5], [0.2, 100.0], [255.9, 10.0], [64.0, 0.0], [128.0, 255.5]])     # star_field's first six
    mask[0] = mask_pattern(HB, WB, np.clip(pixc, 0, [WB - 1, HB - 1]), (96.3, 96.7), (5, 2), (6, 1), 5)
    return dict(bands=bands, typ=typ, radec=radec, counts=counts, shape=shape, S=S, nelec=nelec, mask=mask,
                masked=np.where(mask, np.nan, nelec))


def _options(cel, ctx, layout=1, rows=32, parts=0, star_tiles=1):
    L = cel._lib
    ctx.set_option(L.CEL_OPT_TILE_LAYOUT, layout)      # (layout and rows are read when the image set is created)
    ctx.set_option(L.CEL_OPT_TILE_ROWS, rows)
    ctx.set_option(L.CEL_OPT_TILE_PARTS, parts)
    ctx.set_option(L.CEL_OPT_STAR_TILES, star_tiles)


def _exact_ll(nelec, lam):
    """per band: (math.fsum of n log(lambda) - lambda over the unmasked pixels, 256 * 2^-53 * sum |n log lambda| + lambda).
    The bound is derived: 1.5 ulp for the render's table log (the pass of its own uses the library log: 1 ulp), one rounding
    for the product, and the longest chain of additions of a fixed-order reduction -- k_masked_ll adds at most 64 rows per lane,
    6 shuffle steps and k_reduce's strided sums and tree, far below the 250 that 256 allows."""
    want, tol = [], []
    for b in range(nelec.shape[0]):
        ok = ~np.isnan(nelec[b])
        n, l = nelec[b][ok], lam[b][ok]
        t = n * np.log(l)
        want.append(math.fsum(t - l))
        tol.append(256 * 2.0 ** -53 * math.fsum(np.abs(t) + l))
    return np.array(want), np.array(tol)


def _check_masked_ll(cel, ctx, f, Hh, Ww, label):
    """the checks of test 1 on one form (the context's options are set by the caller)"""
    Bb = f["bands"].shape[0]
    srcs = cel.SourceSet(ctx, f["S"], Bb).set(f["typ"], f["radec"], f["counts"], f["shape"])
    finite = cel.ImageSet(ctx, f["bands"], Hh, Ww, nelec=f["nelec"])
    finite.render(srcs, loglik=True)
    lam_f = finite.model_images()
    im = cel.ImageSet(ctx, f["bands"], Hh, Ww, nelec=f["masked"])
    assert np.array_equal(im.masked, f["mask"].sum(axis=(1, 2)))
    tot, llb = im.render(srcs, loglik=True)
    lam = im.model_images()
    assert np.array_equal(lam, lam_f)
    want, tol = _exact_ll(f["masked"], lam)
    print("%s: |ll_band - fsum| / tol = %s" % (label, np.abs(llb - want) / tol))
    assert np.all(np.isfinite(llb)) and np.all(np.abs(llb - want) <= tol), (llb, want, tol)
    assert tot == llb.sum() or abs(tot - llb.sum()) <= 1e-15 * abs(tot)
    tot2, llb2 = im.render(srcs, loglik=True)                   # two renders in a row: the same bits
    assert tot2 == tot and np.array_equal(llb2, llb)
    tot3, llb3 = im.render(srcs, loglik=True, store=False)      # CEL_RENDER_NO_STORE: the same bits
    assert tot3 == tot and np.array_equal(llb3, llb)
    fresh = cel.ImageSet(ctx, f["bands"], Hh, Ww, nelec=f["masked"])
    tot4, llb4 = fresh.render(srcs, loglik=True, store=False)   # ... on a set that never stored an image either
    assert tot4 == tot and np.array_equal(llb4, llb)
    for s in (finite, im, fresh):
        s.close()


@pytest.mark.parametrize("form", FIELD_FORMS)
def test_masked_loglik_every_field_form(cel, ctx, frame_a, form):
    _options(cel, ctx, **form)
    try:
        _check_masked_ll(cel, ctx, frame_a, HA, WA, "frame A %s" % sorted(form.items()))
    finally:
        _options(cel, ctx)


@pytest.mark.parametrize("star_tiles,counter", [(0, "render"), (1, "small_stars"), (2, "render_stars")],
                         ids=["k_render_hw-star_pass", "k_small_stars", "k_render_stars"])
def test_masked_loglik_every_star_form(cel, ctx, frame_b, star_tiles, counter):
    _options(cel, ctx, star_tiles=star_tiles)
    try:
        ctx.profile(True)
        _check_masked_ll(cel, ctx, frame_b, HB, WB, "frame B star_tiles=%d" % star_tiles)
        assert ctx.profile_get(counter)[1] >= 1                  # the form the setting names did render
        assert ctx.profile_get("masked_ll")[1] >= 1
    finally:
        ctx.profile(False)
        _options(cel, ctx)


def test_edges_of_the_rule(cel, ctx, frame_a):
    f = frame_a
    srcs = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])
    # a band masked everywhere gives 0
    n = f["masked"].copy()
    n[0] = np.nan
    im = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=n)
    assert np.array_equal(im.masked, [HA * WA, f["mask"][1].sum()])
    _, llb = im.render(srcs, loglik=True)
    assert llb[0] == 0.0 and np.isfinite(llb[1]) and llb[1] != 0.0
    # the pass runs on a masked set only
    ctx.profile(True)
    try:
        clean = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["nelec"])
        assert np.array_equal(clean.masked, [0, 0])
        clean.render(srcs, loglik=True)
        assert ctx.profile_get("masked_ll")[1] == 0
        im.render(srcs, loglik=True)
        assert ctx.profile_get("masked_ll")[1] >= 1
    finally:
        ctx.profile(False)
    # set_nelec(invvar=): NaN where invvar == 0
    iv = np.where(f["mask"], 0.0, 2.5)
    clean.set_nelec(f["nelec"], invvar=iv)
    assert np.array_equal(clean.masked, f["mask"].sum(axis=(1, 2)))
    # a negative finite count is scored, not skipped
    n = f["masked"].copy()
    assert not f["mask"][1, 100, 20]
    n[1, 100, 20] = -3.0
    im.set_nelec(n)
    _, llb = im.render(srcs, loglik=True)
    lam = im.model_images()
    want, tol = _exact_ll(n, lam)
    assert np.all(np.abs(llb - want) <= tol)
    n[1, 100, 20] = np.nan
    im.set_nelec(n)
    _, llb_m = im.render(srcs, loglik=True)
    term = -3.0 * math.log(lam[1, 100, 20]) - lam[1, 100, 20]
    assert abs((llb[1] - llb_m[1]) - term) <= 2 * tol[1] and abs(term) > 1e6 * tol[1]
    im.close()
    clean.close()


def test_incremental_render_on_a_masked_set(cel, ctx, frame_a):
    """one part per tile: render, move three sources across the masked column and the masked block with set_rows, render
    again -- the dirty tiles' pixels, every tile's partial (the form that was built) -- against a fresh set's full render"""
    f = frame_a
    L = cel._lib
    ctx.set_option(L.CEL_OPT_TILE_PARTS, 1)
    try:
        im = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["masked"])
        srcs = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])
        im.render(srcs, loglik=True)
        near = np.argsort(np.abs(f["pix"][:, 0] - 40.0))[:2]                 # the two sources nearest the masked column
        rows = np.array(sorted(set(int(i) for i in near) | {f["block_gal"]}), np.int32)
        assert len(rows) == 3
        from desi_mcmc_amd import synth
        pix2 = f["pix"].copy()
        pix2[rows, 0] += np.where(pix2[rows, 0] < 40.0, 4.0, -4.0)           # across the column / into and out of the block
        pix2[rows, 1] += 1.5
        radec2 = synth.pixel2equa(f["bands"][0], pix2)
        srcs.set_rows(rows, f["typ"][rows], radec2[rows], f["counts"][rows], f["shape"][rows])
        tot, llb = im.render(srcs, loglik=True)
        assert im.last_render_dirty_tiles() > 0
        lam = im.model_images()
        fresh = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["masked"])
        srcs2 = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], radec2, f["counts"], f["shape"])
        tot_f, llb_f = fresh.render(srcs2, loglik=True)
        assert fresh.last_render_dirty_tiles() == -1
        assert tot == tot_f and np.array_equal(llb, llb_f)
        assert np.array_equal(lam, fresh.model_images())
        im.close()
        fresh.close()
    finally:
        ctx.set_option(L.CEL_OPT_TILE_PARTS, 0)


@pytest.mark.parametrize("tail,rtol", [("default", 1e-11), ("strict", 1e-13)])
def test_row_windows_add_up(cel, ctx, frame_a, tail, rtol):
    """frame A cut at row 128 (test_hip_parity._row_strips_body: set_window strips; test_owned_rows...: a halo with
    set_noise_rows), at that module's tolerances for unmasked strips: 1e-11 at the shipping threshold, 1e-13 at the strict one"""
    f = frame_a
    srcs = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])
    with tail_log(ctx, tail):
        whole = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["masked"])
        _, llb = whole.render(srcs, loglik=True)
        parts, strips = np.zeros(BA), []
        for y0, y1 in ((0, 128), (128, HA)):
            strip = cel.ImageSet(ctx, f["bands"], y1 - y0, WA, nelec=f["masked"][:, y0:y1])
            strip.set_window(y0, HA)
            assert np.array_equal(strip.masked, f["mask"][:, y0:y1].sum(axis=(1, 2)))
            _, p = strip.render(srcs, loglik=True)
            parts += p
            strips.append(p)
            strip.close()
        np.testing.assert_allclose(parts, llb, rtol=rtol)
        win = cel.ImageSet(ctx, f["bands"], HA - 64, WA, nelec=f["masked"][:, 64:])      # rows 64 ..., owning frame rows 128 ...
        win.set_window(64, HA)
        win.set_noise_rows(64, HA - 64)
        _, llw = win.render(srcs, loglik=True)
        np.testing.assert_allclose(llw, strips[1], rtol=1e-13)
        win.close()
        whole.close()


@pytest.fixture(scope="module")
def grad_scene(cel, ctx):
    """test_loglik_grad's scene (192 x 256 x 3) with the mask pattern scaled to its frame"""
    sc = _scene(cel, ctx)
    from oracle import oracle as orc
    cen = np.array([orc.equa2pixel(sc["bands"][0], sc["radec"][s]) for s in range(sc["S"])])
    gal = int(np.nonzero(sc["typ"] == 1)[0][3])
    mask = np.stack([sparse_mask(HG, WG, 50 + b) for b in range(BG)])
    mask[0] = mask_pattern(HG, WG, cen[:6], cen[gal], (7, 1), (7, 2), 5)
    sc["mask"] = mask
    sc["masked"] = np.where(mask, np.nan, sc["nelec"])
    sc["mset"] = cel.ImageSet(ctx, sc["bands"], HG, WG, nelec=sc["masked"])
    return sc


@pytest.mark.parametrize("T", ["default", 0.0], ids=["shipping", "T0"])
def test_gradient_fill_identity(cel, ctx, grad_scene, T):
    """r = 0 at a masked pixel; r = lambda / lambda - 1 = 0 exactly at a pixel whose count IS lambda: the masked set's gradient
    equals, bit for bit, that of the set whose masked counts are replaced by the model image there"""
    sc = grad_scene
    mset, sset = sc["mset"], sc["sset"]
    with tail_log(ctx, T):
        ll_r, _ = mset.render(sset, loglik=True)
        lam = mset.model_images()
        fset = cel.ImageSet(ctx, sc["bands"], HG, WG, nelec=np.where(sc["mask"], lam, sc["nelec"]))
        assert np.array_equal(fset.masked, [0] * BG)
        got = mset.loglik_grad(sset)
        want = fset.loglik_grad(sset)
        fset.close()
    assert got[0] == ll_r                                        # bit for bit the masked render's total
    for g, w in zip(got[1:], want[1:]):
        assert np.all(np.isfinite(g)) and np.array_equal(g, w)
    assert np.any(got[1] != 0.0) and np.any(got[2] != 0.0) and np.any(got[3] != 0.0)
    # ... and the mask matters: the zero-filled set's gradient is another one
    zset = cel.ImageSet(ctx, sc["bands"], HG, WG, nelec=np.where(sc["mask"], 0.0, sc["nelec"]))
    with tail_log(ctx, T):
        other = zset.loglik_grad(sset)
    zset.close()
    assert not np.array_equal(other[2], got[2])


def _estep_mask(f):
    """frame A's mask plus what the E-step test needs: five sources lose the right-hand part of their boxes in band 0 (20-60 %
    of the mass), one source loses every pixel of its box in band 0"""
    mask = f["mask"].copy()
    half = [1, 11, 20, 6, 8]         # (chosen with the oracle's patches: each loses 40-47 %, their boxes do not meet each other's centres)
    gone = 12
    for s in half:
        y0, y1, x0, x1 = f["boxes"][0, s]
        mask[0, y0:y1, int(round(f["pix"][s, 0])) + 1:x1] = True
    y0, y1, x0, x1 = f["boxes"][0, gone]
    mask[0, y0:y1, x0:x1] = True
    return mask, half, gone


@pytest.mark.parametrize("form", ["tiles", "per-source", "direct"])
def test_estep_fill_identity_and_masked_mass(cel, ctx, orc, frame_a, form):
    """xtilde and noise of the masked set equal, bit for bit, those of the set with 0 counts at the masked pixels (0 / lambda = 0
    exactly); the mass a source loses is the oracle's unit patch summed over the masked pixels of its box (strict threshold,
    the suite's 1e-10 stamp tolerance); a box masked everywhere gives mass 0 and xtilde 0"""
    f = frame_a
    L = cel._lib
    mask, half, gone = _estep_mask(f)
    srcs = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])
    if form == "per-source":
        ctx.set_option(L.CEL_OPT_DEBUG, 64)
    if form == "direct":
        ctx.set_kernel("direct")
    try:
        with tail_log(ctx, "strict"):
            mset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, np.nan, f["nelec"]))
            zset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, 0.0, f["nelec"]))
            xt, ms, nz = mset.estep_stats(srcs)
            xt0, ms0, nz0 = zset.estep_stats(srcs)
            assert np.array_equal(mset.model_images(), zset.model_images())
            ob = f["bands"].copy()
            for b in range(BA):
                ob[b, 36] = orc.checked_radius(ob[b], mset.band(b)[36])
            mset.close()
            zset.close()
    finally:
        ctx.set_option(L.CEL_OPT_DEBUG, 0)
        ctx.set_kernel("recurrence")
    assert np.all(np.isfinite(xt)) and np.array_equal(xt, xt0) and np.array_equal(nz, nz0)
    lost = np.zeros((f["S"], BA))
    for s in range(f["S"]):
        for b in range(BA):
            patch, (y0, y1), (x0, x1) = orc.source_patch(ob[b], HA, WA, f["typ"][s], f["radec"][s], f["shape"][s])
            assert np.array_equal(f["boxes"][b, s], [y0, y1, x0, x1])
            lost[s, b] = math.fsum(patch[mask[b, y0:y1, x0:x1]])
            assert abs(ms0[s, b] - math.fsum(patch.ravel())) <= 1e-10 * ms0[s, b]
    print("%s: max |mass lost - oracle| / mass = %.3g" % (form, np.max(np.abs((ms0 - ms) - lost) / ms0)))
    assert np.all(np.abs((ms0 - ms) - lost) <= 1e-10 * ms0)
    frac = 1.0 - ms[:, 0] / ms0[:, 0]
    assert np.sum((frac >= 0.2) & (frac <= 0.6)) >= 5, frac
    assert all(0.2 <= frac[s] <= 0.6 for s in half), frac[half]
    assert ms[gone, 0] == 0.0 and xt[gone, 0] == 0.0 and ms[gone, 1] > 0.5 and xt[gone, 1] > 0.0


def test_gradient_and_estep_agree_on_the_masked_scene(ctx, grad_scene):
    """d ll / d counts = xtilde / counts - mass (test_grad_counts_is_estep_identity_on_benchmark_field's form and 1e-9):
    fails when either side forgets the mask"""
    sc = grad_scene
    _, _, gc, _ = sc["mset"].loglik_grad(sc["sset"])
    xt, ms, _ = sc["mset"].estep_stats(sc["sset"])
    want = xt / sc["counts"] - ms
    assert np.all(np.isfinite(gc)) and np.all(np.abs(gc - want) <= 1e-9 * (xt / sc["counts"] + ms))
    xt0, ms0, _ = sc["iset"].estep_stats(sc["sset"])             # the unmasked scene: other sums
    assert np.any(np.abs(gc - (xt0 / sc["counts"] - ms0)) > 1e-6 * (xt0 / sc["counts"] + ms0))


def _fits_images(bands, nelec, Hh, Ww, invvar=None):
    from desi_mcmc_amd.fits_image import FitsImage
    out = []
    for b in range(bands.shape[0]):
        r = bands[b]
        out.append(FitsImage("ugriz"[b % 5], nelec[b], epsilon=r[0], kappa=r[1], calib=r[2], weights=r[3:6], means=r[6:12].reshape(3, 2),
                             covars=r[12:24].reshape(3, 2, 2), rho_n=r[24:26], phi_n=r[26:28], Ups_n=r[28:32].reshape(2, 2),
                             invvar=None if invvar is None else invvar[b], mask_invvar=invvar is not None))
    return out


def test_calls_that_do_not_honour_a_mask_refuse_it(cel, ctx, frame_a):
    from desi_mcmc_amd import celeste_mcmc, models
    L = cel._lib
    f = frame_a
    srcs = cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])
    one = cel.SourceSet(ctx, 1, BA).set(f["typ"][:1], f["radec"][:1], f["counts"][:1], f["shape"][:1])
    im = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["masked"])
    box = f["boxes"][:, 0]
    patches = [f["nelec"][b, box[b, 0]:box[b, 1], box[b, 2]:box[b, 3]] for b in range(BA)]
    params = [cel.SrcParams(u=f["radec"][s], a=0, fluxes=np.full(5, 20.0)) for s in range(3)]
    iv = np.where(f["mask"], 0.0, 1.0)

    def gibbs(invvar):
        imgs = _fits_images(f["bands"], f["nelec"], HA, WA, invvar)
        return celeste_mcmc.ModelGibbs.from_images([dict(zip("ug", imgs))], params, seed=1), imgs

    for call in (lambda: im.photon_split(srcs, 3), lambda: im.photon_split_resident(srcs, 3),
                 lambda: im.patch_loglik(one, box, patches, isolated=True), lambda: gibbs(iv)):
        with pytest.raises(L.CelesteHipError, match="masked"):
            call()
    # the library's own refusal (CEL_ERR_INVALID), for a caller of the C ABI
    import ctypes as C
    noise = np.zeros(BA)
    assert L.lib().cel_photon_split(im._h, srcs._h, C.c_uint64(3), None, None, L.CEL_DEVICE, L.dptr(noise)) == L.CEL_ERR_INVALID
    assert b"masked" in L.lib().cel_last_error()
    with pytest.raises(ValueError, match="masked"):
        models.Field(dict(zip("ug", _fits_images(f["bands"], f["nelec"], HA, WA, iv)))).resample_photons([])
    # the same calls on the unmasked set of the same context
    im.set_nelec(f["nelec"])
    assert np.array_equal(im.masked, [0, 0])
    _, _, noise = im.photon_split(srcs, 3)
    assert np.all(np.isfinite(noise))
    assert np.all(np.isfinite(im.photon_split_resident(srcs, 3)))
    assert np.all(np.isfinite(im.patch_loglik(one, box, patches, isolated=True)))
    g, imgs = gibbs(None)
    assert g.S == 3
    im.close()
