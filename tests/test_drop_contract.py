"""The drop rule's contract, pixel by pixel, against an exact sum of every term.

include/celeste_hip.h (CEL_OPT_TAIL_LOG): a mixture component is skipped on a tile only where its contribution stays below
eps * e^-T on the part of the tile its source covers; the per-source kernels use the source's own smallest value on the tile
in place of eps.  The parity tests check the result at the shipping thresholds (T = 24 / 32), where one wrongly dropped term is
1e-11 .. 1e-14 of eps and invisible under their 1e-9 / 1e-10 tolerances.  Here the threshold is LOW (T = 4 .. 20), so a term
that should have been kept is far above rounding, and every pixel is held between two exact bounds:

    lam_full - S_sub - tol  <=  lam_kernel  <=  lam_full + tol
    S_sub = sum of the pixel's terms t <= thr,    thr = eps_b e^-T (1 + DELTA)
    tol   = C_R * sum |t| + 4 ulp(lam_full)

lam_full is the exact sum (long double) of every (source, component) term t = counts * w_k * N(pixel; mu_k, Sigma_k) over the
source's box.  The right-hand bound catches a term added twice; the left-hand one a term above the threshold left out.

DELTA: the drop test and the row ends are computed with documented fp32 slack only.
  * quad_min_rect shrinks the minimum of the quadratic form by 0.99999: towards keeping, contributes nothing;
    its fp32 edge minimisers give a feasible point, so the form's value there is >= the minimum (second order).
  * Tk = T + __logf(|A|) - __logf(eps): (float) A and eps round by 6e-8 relative (6e-8 in the log), __logf's error is a
    few fp32 ulp of its result, |log| < 64 here: ulp 3.8e-6, so |dTk| < 4 * 4e-6 + 1.2e-7 < 2e-5.  A component dropped
    on that Tk is below eps e^-T e^(2e-5).
  * the row ends (quad_rows_on_columns, fp32) err by a few ulp of |cy| + |y| < 256 rows: < 1e-4 row, inside the 0.02 row
    margin, so every row inside the ellipse of the fp32 Tk is walked.
  So thr = eps e^-T e^(2e-5) suffices; DELTA = 1e-3 takes that with a factor 50 to spare and stays far below 1 (a
  drop test that is off by a factor e, Tk - 1, is 1.7).
C_R: the evaluator's relative rounding per term.  DESIGN 5: a seed's relative error is multiplied by the walk's row count, and
  the seed needs 1e-12 in r for the 64-row walk.  Seeds: exp_tab64 <= 4.34 ulp by its derivation (test_primitives.py, which
  asserts it; measured 2.30 ulp on the CPU, 2.23 on the device -- not the "<= 2 ulp" this line used to quote: 4.34 ulp = 4.8e-16
  is 5e-4 of C_R, which covers it unchanged), the quadratic form's argument |q| <= 600
  (Tk <= 300) rounds by < 600 ulp absolute = 7e-14 relative in exp; the recurrence g(y+1) = g(y) r(y), r(y+1) = r(y) q over
  at most 64 rows: 64^2 / 2 ulp = 2.3e-13; a pixel's adds (<= 200 accumulator adds) 200 ulp = 2e-14 of sum |t|.
  C_R = 1e-12 covers all of it, and is 2000 times below thr / eps = e^-20 = 2e-9 at the highest threshold that places
  edges (T = 20): a term wrongly dropped there is 2000 tol.  At T = 24 and 32 the bound still holds and still catches
  double counting, but a single lost tail term is within C_R of a bright pixel.

The geometry is built to sit on the edges (GeomField): components whose threshold ellipse ends within +-0.005 and +-0.03 row
of an integer row at each edge-placing T, ends on tile rows 31/32 and 63/64, boxes that begin on tile columns and rows, thin
rotated galaxies, compact galaxies under a sharp PSF (band 4), a galaxy below eps e^-T everywhere, and a crowded tile whose
list fills four parts of k_render_hw.
"""
import math

import numpy as np
import pytest

from conftest import tail_log
from _exact_terms import C_R, DELTA, LD, H, W, chunk_sub, components, patch_rel_err, source_terms

pytestmark = pytest.mark.gpu

NB = 5
T_ALL = (0, 4, 8, 12, 20, 24, 32)
T_EDGE = (4, 8, 12, 20)              # thresholds whose ellipse ends are placed on integer rows
EDGE_BAND = 2                        # the band whose ellipses are placed (r)
SHARP_BAND = 4                       # this band's PSF is narrowed to 0.3 pixel

# (case, T) -> the worst pixel's error in units of tol, beyond what the bound allows: max of (lam_full - lam_kernel - S_sub) / tol
# and (lam_kernel - lam_full) / tol; <= 1 passes.  Printed at the end of the module (pytest -s)
RATIOS = {}


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# the exact per-term reference: components, source_terms, patch_rel_err (_exact_terms.py, shared with test_conditional_contract.py)
class FieldRef(object):
    """lam_full, sum |t| and, per T, the sum of the terms at or below the field render's threshold -- per band and pixel; the
    unit patches for the E-step.  A source's terms are added in fp64 (<= 42 ulp of sum |t|: 1e-14, far inside C_R), the
    sources and the sky in long double"""

    def __init__(self, orc, bands, typ, radec, counts, shape, thresholds=T_ALL):
        B = bands.shape[0]
        Td = sorted(T for T in thresholds if T > 0)
        self.lam = np.zeros((B, H, W), LD)
        self.sabs = np.zeros((B, H, W))
        self.sub = {T: np.zeros((B, H, W)) for T in Td}
        self.units = [[None] * len(typ) for _ in range(B)]
        self.patch_err = 0.0
        for b in range(B):
            eps = bands[b, 0]
            thr_up = np.array([eps * math.exp(-T) * (1 + DELTA) for T in Td])[::-1]       # increasing
            pix, lev, val = [], [], []
            for s in range(len(typ)):
                r = source_terms(orc, bands[b], typ[s], radec[s], shape[s])
                if r is None:
                    continue
                (y0, y1, x0, x1), t, patch = r
                u = t.sum(axis=0)
                self.patch_err = max(self.patch_err, patch_rel_err(u, patch))
                self.units[b][s] = ((y0, y1, x0, x1), u)
                t = t * counts[s, b]
                self.lam[b, y0:y1, x0:x1] += LD(counts[s, b]) * u
                # level of a term: how many of the thresholds it is at or below (it is in S_sub[Td[j]] for j < level)
                at = np.abs(t)
                small = at <= thr_up[-1]
                if small.any():
                    kk, yy, xx = np.nonzero(small)
                    pix.append((yy + y0) * W + (xx + x0))
                    lev.append(len(Td) - np.searchsorted(thr_up, at[small], side="left"))
                    val.append(t[small])
                self.sabs[b, y0:y1, x0:x1] += at.sum(axis=0)
            if pix:
                pix, lev, val = np.concatenate(pix), np.concatenate(lev), np.concatenate(val)
                part = np.bincount(lev * (H * W) + pix, weights=val, minlength=(len(Td) + 1) * H * W).reshape(len(Td) + 1, H, W)
                acc = np.zeros((H, W))
                for j in range(len(Td), 0, -1):                  # S_sub[Td[j-1]] = the terms of level >= j
                    acc = acc + part[j]
                    self.sub[Td[j - 1]][b] = acc
            self.lam[b] += LD(eps)
        self.lam64 = self.lam.astype(np.float64)
        self.tol = C_R * self.sabs + 4 * np.spacing(self.lam64)


def check_field(ref, lam_k, T, case, drops=True):
    """the two-sided bound at every pixel; drops=False: nothing may be skipped (T = 0, the direct evaluator, stars)"""
    sub = ref.sub[T] if (drops and T > 0) else 0.0
    lo = (ref.lam - LD(1) * lam_k).astype(np.float64)      # what the kernel left out (>= 0 up to rounding)
    r_lo = float(np.max((lo - sub) / ref.tol))              # <= 1: lo <= S_sub + tol
    r_hi = float(np.max(-lo / ref.tol))
    RATIOS[(case, T)] = max(r_lo, r_hi, RATIOS.get((case, T), -np.inf))
    if r_lo > 1.0:
        b, y, x = np.unravel_index(np.argmax((lo - sub) / ref.tol), lo.shape)
        raise AssertionError("%s T=%g: a term above the threshold was left out: band %d pixel (y %d, x %d): lam_full %.17g kernel %.17g "
                             "S_sub %.3g tol %.3g (worst ratio %.3g)" % (case, T, b, y, x, ref.lam64[b, y, x], lam_k[b, y, x],
                                                                         np.broadcast_to(sub, lo.shape)[b, y, x], ref.tol[b, y, x], r_lo))
    if r_hi > 1.0:
        b, y, x = np.unravel_index(np.argmax(-lo / ref.tol), lo.shape)
        raise AssertionError("%s T=%g: the kernel exceeds the exact sum: band %d pixel (y %d, x %d): lam_full %.17g kernel %.17g tol %.3g"
                             % (case, T, b, y, x, ref.lam64[b, y, x], lam_k[b, y, x], ref.tol[b, y, x]))


# ---------------------------------------------------------------------------------------------------------------------
# the geometry
def _ellipse_end(orc, band, shape, u, k, T, cnt, end):
    """(y, x) of component k's threshold ellipse's top (end = +1) or bottom (-1) for the field render at T"""
    w, mu, cov = components(orc, band, 1, u, shape)
    det = cov[k, 0, 0] * cov[k, 1, 1] - cov[k, 0, 1] ** 2
    A = cnt * w[k] / (2 * math.pi * math.sqrt(det))
    Tk = T + math.log(abs(A) / band[0])
    if Tk <= 0:
        return None
    h = math.sqrt(2 * Tk * cov[k, 1, 1])
    return mu[k, 1] + end * h, mu[k, 0] + end * cov[k, 0, 1] * math.sqrt(2 * Tk / cov[k, 1, 1])


def _place(orc, band, shape, px, py, k, T, cnt, end, frac, row=None):
    """move the source in dec (y; rigid to first order) until component k's ellipse ends at an integer row + frac"""
    from desi_mcmc_amd import synth
    for _ in range(4):
        u = synth.pixel2equa(band, np.array([[px, py]]))[0]
        ye = _ellipse_end(orc, band, shape, u, k, T, cnt, end)[0]
        n = row if row is not None else math.floor(ye - frac + 0.5)
        py += (n + frac) - ye
    u = synth.pixel2equa(band, np.array([[px, py]]))[0]
    return u, _ellipse_end(orc, band, shape, u, k, T, cnt, end)


class GeomField(object):
    """5 bands of 256^2 with ~70 sources placed on the drop rule's edges (band EDGE_BAND)"""

    def __init__(self, orc):
        from desi_mcmc_amd import synth
        bands = synth.make_bands(H, W, NB)
        bands[SHARP_BAND, 12:24] *= 0.04                  # a sharp PSF (sigma ~0.3 px): compact galaxies, the general path for stars
        self.bands = bands
        bd = bands[EDGE_BAND]
        cnt_of = lambda flux: flux / bands[:, 2] * bands[:, 1]
        rs = np.random.RandomState(7)
        typ, radec, counts, shape, self.edges = [], [], [], [], []

        def add(t, u, flux, sh):
            typ.append(t)
            radec.append(np.asarray(u, float))
            counts.append(cnt_of(np.broadcast_to(np.asarray(flux, float), (NB,))))
            shape.append(np.asarray(sh, float))

        # (1) ellipse ends within +-0.005 / +-0.03 of an integer row, at the top and the bottom, for every edge-placing T
        cells = [(x, y) for y in (36.0, 100.0, 164.0, 228.0) for x in np.arange(16.0, 256.0, 32.0)]
        ci = 0
        for T in T_EDGE:
            for frac in (0.005, -0.005, 0.03, -0.03):
                for end in (1, -1):
                    px, py = cells[ci % len(cells)]
                    ci += 1
                    px += rs.uniform(-6, 6)
                    sh = [rs.uniform(0.1, 0.9), rs.uniform(0.6, 1.6), rs.uniform(0, 180), rs.uniform(0.25, 0.9)]
                    flux = rs.uniform(3.0, 12.0)
                    cnt = cnt_of(flux)[EDGE_BAND]
                    u0 = synth.pixel2equa(bd, np.array([[px, py]]))[0]
                    w, mu, cov = components(orc, bd, 1, u0, sh)
                    k = int(np.argmax(w / np.sqrt(np.linalg.det(cov))))         # the peak component: ends well inside the box
                    u, (ye, xe) = _place(orc, bd, sh, px, py, k, T, cnt, end, frac)
                    add(1, u, flux, sh)
                    self.edges.append(dict(T=T, frac=frac, end=end, y=ye, x=xe, k=k))
        # (2) ends on tile rows: the last row of a 32- and a 64-row tile, the first row of the next
        for (row, frac, px) in ((63, 0.005, 40.0), (64, 0.005, 104.0), (31, 0.005, 168.0), (32, -0.005, 232.0)):
            sh = [0.5, 1.0, 60.0, 0.6]
            cnt = cnt_of(6.0)[EDGE_BAND]
            u0 = synth.pixel2equa(bd, np.array([[px, row - 6.0]]))[0]
            w, mu, cov = components(orc, bd, 1, u0, sh)
            k = int(np.argmax(w / np.sqrt(np.linalg.det(cov))))
            u, (ye, xe) = _place(orc, bd, sh, px, row - 6.0, k, 8, cnt, 1, frac, row=row)
            add(1, u, 6.0, sh)
            self.edges.append(dict(T=8, frac=frac, end=1, y=ye, x=xe, k=k))
        # (3) a box that begins exactly on a tile column (32) and a tile row (64)
        sh = [0.4, 1.2, 20.0, 0.7]
        u = synth.pixel2equa(bd, np.array([[80.0, 150.0]]))[0]
        _, (y0, _), (x0, _) = orc.source_patch(bd, H, W, 1, u, sh)
        u = synth.pixel2equa(bd, np.array([[80.0 + (64 - x0), 150.0 + (128 - y0)]]))[0]
        _, (y0, _), (x0, _) = orc.source_patch(bd, H, W, 1, u, sh)
        self.box_on_tile = (y0, x0)
        add(1, u, 8.0, sh)
        # (4) thin, strongly rotated galaxies with a large b; compact ones (sharp in band SHARP_BAND)
        for (px, py, sh) in ((200.0, 60.0, [0.3, 3.0, 37.0, 0.12]), (60.0, 200.0, [0.7, 2.5, 128.0, 0.1]),
                             (130.0, 30.0, [0.5, 0.1, 10.0, 0.8]), (30.0, 120.0, [0.9, 0.05, 80.0, 0.5])):
            add(1, synth.pixel2equa(bd, np.array([[px, py]]))[0], 20.0, sh)
        # (5) a galaxy below eps e^-T everywhere at the low thresholds (Tk < 0 for every component at T <= 8)
        add(1, synth.pixel2equa(bd, np.array([[100.0, 20.0]]))[0], 1e-6, [0.5, 1.0, 0.0, 0.5])
        self.n_faint = len(typ) - 1
        # (6) a crowded tile (x 128..160, y 128..192): 40 sources, so k_render_hw's four parts all work and pairs of groups
        # overlap in all three nested phases
        for i in range(40):
            px, py = rs.uniform(130, 158), rs.uniform(130, 190)
            u = synth.pixel2equa(bd, np.array([[px, py]]))[0]
            if i % 5 == 0:
                add(0, u, rs.uniform(2, 30), [0, 0, 0, 0])
            else:
                add(1, u, rs.uniform(1, 30), [rs.uniform(0.05, 0.95), rs.uniform(0.3, 1.5), rs.uniform(0, 180), rs.uniform(0.2, 0.95)])
        # (7) a few lone stars
        for (px, py) in ((12.5, 12.5), (243.2, 20.7), (20.1, 240.9), (250.0, 250.0), (96.0, 64.0)):
            add(0, synth.pixel2equa(bd, np.array([[px, py]]))[0], 15.0, [0, 0, 0, 0])
        self.typ = np.array(typ, np.int32)
        self.radec = np.array(radec)
        self.counts = np.array(counts)
        self.shape = np.array(shape)


def star_field(orc):
    """a star-only catalogue: k_small_stars / k_render_stars / k_render_hw's star pass by CEL_OPT_STAR_TILES"""
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, NB)
    rs = np.random.RandomState(3)
    S = 40
    pix = np.column_stack([rs.uniform(-3, W + 3, S), rs.uniform(-3, H + 3, S)])
    pix[:8] = [[32.0, 64.0], [31.5, 63.5], [0.2, 100.0], [255.9, 10.0], [64.0, 0.0], [128.0, 255.5], [96.3, 96.7], [97.0, 96.0]]
    flux = np.exp(rs.uniform(0.0, np.log(200.0), (S, 1))) * np.ones((1, NB))
    return bands, np.zeros(S, np.int32), synth.pixel2equa(bands[0], pix), flux / bands[None, :, 2] * bands[None, :, 1], np.zeros((S, 4))


def _fix_radii(orc, bands, images):
    """the star radius: the oracle's own, after checking the library's (conftest-style, orc.checked_radius)"""
    out = bands.copy()
    for b in range(bands.shape[0]):
        out[b, 36] = orc.checked_radius(bands[b], images.band(b)[36])
    return out


@pytest.fixture(scope="module")
def geom(cel, orc):
    g = GeomField(orc)
    ctx = cel.Context(0)
    images = cel.ImageSet(ctx, g.bands, H, W)
    g.bands = _fix_radii(orc, g.bands, images)
    images.close()
    g.ref = FieldRef(orc, g.bands, g.typ, g.radec, g.counts, g.shape)
    return g


@pytest.fixture(scope="module")
def stars(cel, orc):
    bands, typ, radec, counts, shape = star_field(orc)
    ctx = cel.Context(0)
    images = cel.ImageSet(ctx, bands, H, W)
    bands = _fix_radii(orc, bands, images)
    images.close()
    return dict(bands=bands, typ=typ, radec=radec, counts=counts, shape=shape,
                ref=FieldRef(orc, bands, typ, radec, counts, shape))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nworst (error - allowance) / tol, by case and T:")
        for (case, T) in sorted(RATIOS, key=lambda k: (k[0], k[1])):
            print("  %-44s T=%-3g %.3g" % (case, T, RATIOS[(case, T)]))


# ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle(orc, geom, stars):
    """the reference's self-check: its per-term sums equal the oracle's unit patches and its field render to 1e-13"""
    for f in (dict(bands=geom.bands, typ=geom.typ, radec=geom.radec, counts=geom.counts, shape=geom.shape, ref=geom.ref), stars):
        assert f["ref"].patch_err <= 1e-13
        o_lam, _, _ = orc.render_field(f["bands"], H, W, f["typ"], f["radec"], f["counts"], f["shape"])
        np.testing.assert_allclose(f["ref"].lam64, o_lam, rtol=1e-13, atol=0)


def test_geometry_sits_on_the_edges(orc, geom):
    """the placed ends are where the test says they are, inside their boxes and the frame; the box-on-tile source and the faint
    source are what they claim"""
    bd = geom.bands[EDGE_BAND]
    for e, i in zip(geom.edges, range(len(geom.edges))):
        assert abs(e["y"] - round(e["y"]) - e["frac"]) < 1e-6, e
        _, (y0, y1), (x0, x1) = orc.source_patch(bd, H, W, 1, geom.radec[i], geom.shape[i])
        assert y0 + 1 <= e["y"] <= y1 - 2 and x0 <= e["x"] <= x1 - 1, (e, (y0, y1, x0, x1))
    assert {(e["T"], e["frac"], e["end"]) for e in geom.edges} >= {(T, f, s) for T in T_EDGE for f in (0.005, -0.005, 0.03, -0.03)
                                                                  for s in (1, -1)}
    assert {int(round(e["y"])) for e in geom.edges} >= {31, 32, 63, 64}
    assert geom.box_on_tile == (128, 64)
    w, mu, cov = components(orc, bd, 1, geom.radec[geom.n_faint], geom.shape[geom.n_faint])
    A = geom.counts[geom.n_faint, EDGE_BAND] * w / (2 * np.pi * np.sqrt(np.linalg.det(cov)))
    assert np.all(A < bd[0] * math.exp(-8))              # Tk < 0 for every component at T <= 8


def _render(cel, ctx, f, T, layout=1, rows=32, parts=0, star_tiles=1):
    ctx.set_option(cel._lib.CEL_OPT_TILE_LAYOUT, layout)      # (layout and rows are read when the image set is created)
    ctx.set_option(cel._lib.CEL_OPT_TILE_ROWS, rows)
    ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, parts)
    ctx.set_option(cel._lib.CEL_OPT_STAR_TILES, star_tiles)
    try:
        images = cel.ImageSet(ctx, f["bands"], H, W)
        srcs = cel.SourceSet(ctx, len(f["typ"]), NB).set(f["typ"], f["radec"], f["counts"], f["shape"])
        with tail_log(ctx, T):
            images.render(srcs)
        return images.model_images()
    finally:
        for key, v in ((cel._lib.CEL_OPT_TILE_LAYOUT, 1), (cel._lib.CEL_OPT_TILE_ROWS, 32), (cel._lib.CEL_OPT_TILE_PARTS, 0),
                       (cel._lib.CEL_OPT_STAR_TILES, 1)):
            ctx.set_option(key, v)


def _gdict(g):
    return dict(bands=g.bands, typ=g.typ, radec=g.radec, counts=g.counts, shape=g.shape)


# the kernel each setting reaches (celeste_hip.hip, cel_render_field's dispatch): layout 1 -> k_render_hw<false, PARTS>
# (PARTS by CEL_OPT_TILE_PARTS), layout 2 -> k_render_qw, layout 0 -> k_render<TILE_ROWS>
FIELD_FORMS = [
    pytest.param(dict(layout=1, parts=1), id="k_render_hw-parts1"),
    pytest.param(dict(layout=1, parts=2), id="k_render_hw-parts2"),
    pytest.param(dict(layout=1, parts=4), id="k_render_hw-parts4"),
    pytest.param(dict(layout=2, parts=1), id="k_render_qw"),
    pytest.param(dict(layout=0, rows=32, parts=1), id="k_render-rows32"),
    pytest.param(dict(layout=0, rows=64, parts=1), id="k_render-rows64"),
]


@pytest.mark.parametrize("form", FIELD_FORMS)
def test_field_render_keeps_every_term_above_the_threshold(cel, geom, form):
    ctx = cel.Context(0)
    case = "field:" + "-".join("%s%s" % kv for kv in sorted(form.items()))
    for T in T_ALL:
        lam = _render(cel, ctx, _gdict(geom), T, **form)
        check_field(geom.ref, lam, T, case)


def test_field_render_direct_drops_nothing(cel, geom):
    """set_kernel("direct"): k_render_hw with the direct evaluator, which never drops (variant 0)"""
    ctx = cel.Context(0)
    ctx.set_kernel("direct")
    for T in (0, 4, 8, 20):
        lam = _render(cel, ctx, _gdict(geom), T, parts=1)
        check_field(geom.ref, lam, T, "field:direct", drops=False)


@pytest.mark.parametrize("star_tiles,kernel", [(0, "k_render_hw star pass"), (1, "k_small_stars"), (2, "k_render_stars")],
                         ids=["k_render_hw-star_pass", "k_small_stars", "k_render_stars"])
def test_star_field_drops_nothing(cel, stars, star_tiles, kernel):
    """stars have no table and no drop: every T meets tol with nothing subtracted"""
    ctx = cel.Context(0)
    for T in T_ALL:
        lam = _render(cel, ctx, stars, T, star_tiles=star_tiles)
        check_field(stars["ref"], lam, T, "stars:" + kernel, drops=False)


def test_incremental_render_after_set_rows(cel, orc, geom):
    """k_render_hw's incremental form (CEL_OPT_INCREMENTAL, one part per tile): move three sources with set_rows, render again
    -- only the dirty tiles -- and hold the new field to the bound"""
    ctx = cel.Context(0)
    ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, 1)
    try:
        f = _gdict(geom)
        images = cel.ImageSet(ctx, f["bands"], H, W)
        srcs = cel.SourceSet(ctx, len(f["typ"]), NB).set(f["typ"], f["radec"], f["counts"], f["shape"])
        rows = np.array([0, 9, len(f["typ"]) - 10], np.int32)
        radec2 = f["radec"].copy()
        radec2[rows] += np.array([[1.3e-4, -0.7e-4], [-2.1e-4, 0.9e-4], [0.4e-4, 1.1e-4]])
        ref2 = FieldRef(orc, f["bands"], f["typ"], radec2, f["counts"], f["shape"], thresholds=(8,))
        with tail_log(ctx, 8):
            images.render(srcs)
            srcs.set_rows(rows, f["typ"][rows], radec2[rows], f["counts"][rows], f["shape"][rows])
            images.render(srcs)
            assert images.last_render_dirty_tiles() > 0          # the incremental form ran
            check_field(ref2, images.model_images(), 8, "field:incremental")
    finally:
        ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the per-source kernels (hw_source.h, HW_DROP_SELF): the threshold is the source's own smallest value on the rectangle
def test_unit_stamps_keep_every_term_above_the_source_floor(cel, orc, geom):
    ctx = cel.Context(0)
    f = _gdict(geom)
    images = cel.ImageSet(ctx, f["bands"], H, W)
    srcs = cel.SourceSet(ctx, len(f["typ"]), NB).set(f["typ"], f["radec"], f["counts"], f["shape"])
    for b in (EDGE_BAND, SHARP_BAND):
        refs = [source_terms(orc, f["bands"][b], f["typ"][s], f["radec"][s], f["shape"][s]) for s in range(len(f["typ"]))]
        for T in (4, 8, 12, 20, 32):
            ctx.set_option(cel._lib.CEL_OPT_TAIL_LOG_SOURCE, T)
            try:
                st, boxes = images.stamps(srcs, b)
            finally:
                ctx.set_option(cel._lib.CEL_OPT_TAIL_LOG_SOURCE, float("nan"))
            worst = -np.inf
            for s, r in enumerate(refs):
                if r is None:
                    assert st[s] is None
                    continue
                box, t, _ = r
                assert tuple(boxes[s]) == box
                full = t.sum(axis=0)
                sub = chunk_sub(t, T)                          # (a star's three components take the same table and drop test)
                tol = C_R * np.abs(t).sum(axis=0).astype(np.float64) + 4 * np.spacing(full.astype(np.float64))
                lo = (full - LD(1) * st[s]).astype(np.float64)
                r_lo, r_hi = float(np.max((lo - sub) / tol)), float(np.max(-lo / tol))
                worst = max(worst, r_lo, r_hi)
                assert r_lo <= 1.0, "stamp of source %d, band %d, T=%g: a term above the floor's threshold left out (%.3g)" % (s, b, T, r_lo)
                assert r_hi <= 1.0, "stamp of source %d, band %d, T=%g: above the exact sum (%.3g)" % (s, b, T, r_hi)
            RATIOS[("stamps:k_stamps_hw-band%d" % b, T)] = worst


def test_estep_sums_within_the_header_rule(cel, orc, geom):
    """cel_estep_stats at a low per-source threshold (the field render at T = 0: lambda is exact to tol): every pixel of a
    source's patch is within n_components e^-T of its exact value, from below -- so X~ and the mass are too"""
    ctx = cel.Context(0)
    f = _gdict(geom)
    ref = geom.ref
    nelec = np.random.RandomState(1).poisson(ref.lam64).astype(np.float64)
    images = cel.ImageSet(ctx, f["bands"], H, W, nelec=nelec)
    srcs = cel.SourceSet(ctx, len(f["typ"]), NB).set(f["typ"], f["radec"], f["counts"], f["shape"])
    S = len(f["typ"])
    xt_ex, ms_ex = np.zeros((S, NB), LD), np.zeros((S, NB), LD)
    for b in range(NB):
        for s in range(S):
            if ref.units[b][s] is None:
                continue
            (y0, y1, x0, x1), u = ref.units[b][s]
            ms_ex[s, b] = u.sum()
            xt_ex[s, b] = (u * LD(f["counts"][s, b]) / ref.lam[b, y0:y1, x0:x1] * nelec[b, y0:y1, x0:x1]).sum()
    K = np.where(f["typ"] == 0, 3, 42)[:, None]
    try:
        for T in (4, 8, 12, 20):
            ctx.set_option(cel._lib.CEL_OPT_TAIL_LOG, 0)
            ctx.set_option(cel._lib.CEL_OPT_TAIL_LOG_SOURCE, T)
            xt, ms, _ = images.estep_stats(srcs)
            rel = K * math.exp(-T) * (1 + DELTA)
            worst = -np.inf
            for got, ex, extra in ((xt, xt_ex, 2 * C_R), (ms, ms_ex, C_R)):     # (X~ divides by lambda: its rounding too)
                ex64 = ex.astype(np.float64)
                tol = extra * np.abs(ex64) + 4 * np.spacing(np.abs(ex64)) + 1e-300
                lo = (ex - LD(1) * got).astype(np.float64)
                r_lo, r_hi = np.max((lo - rel * np.abs(ex64)) / tol), np.max(-lo / tol)
                worst = max(worst, r_lo, r_hi)
                assert r_lo <= 1.0, "E-step T=%g: below exact by more than n_components e^-T (%.3g)" % (T, r_lo)
                assert r_hi <= 1.0, "E-step T=%g: above the exact sum (%.3g)" % (T, r_hi)
            RATIOS[("estep:k_estep", T)] = worst
    finally:
        ctx.set_tail_log("default")
