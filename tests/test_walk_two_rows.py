"""k_render_hw's column walk two rows per step, on the smallest frame where it can go wrong.

The nested walk (k_render_hw.h, rec_walk_n / rec_group_nested) carries R(y) = r(y) r(y+1) next to r and takes two rows per trip;
its three phases [ga, sa) [sa, sb) [sb, gb) each end on an odd row or an even one, and a phase that ends on an odd row hands
the state on by a single-row step.  A row lost or added twice at such a boundary, a second set seeded one row off, a state
advanced with the wrong power of q: each is a whole term, thousands of tol at a low threshold.  So the frame is one tile
column of two tile rows (W = 32, H = 128), the sources are a handful of galaxies, and every pixel is held to the bound of
test_drop_contract.py against the exact per-term sums of _exact_terms.py:

    lam_full - S_sub - tol  <=  lam  <=  lam_full + tol,     tol = C_R sum |t| + 4 ulp,  C_R = 1e-12

WHICH phase lengths occur is decided by the geometry, so the test works them out on the host (WalkModel: the kernel's own
rules -- drop test, rows on the tile's columns, slots by row count, pairs of twelve, the pair's second set -- in fp64, refusing
any geometry that sits within the kernel's fp32 margins of a decision) and asserts that all eight parity combinations of the
three phase lengths occur, with lengths 0, 1 and 2 among them; that ranges end on tile rows 63 and 64 and begin on row 64;
that a 64-row component shares a pair with one of at most two rows; that a pair takes more than one segment and one the direct
fallback.  The model is itself checked against the device: its component-rows and pairs per tile are what the kernel's work
counters report (CEL_OPT_TILE_TIMING).
"""
import contextlib
import math

import numpy as np
import pytest

from conftest import tail_log
from _exact_terms import C_R, DELTA, LD, components, patch_rel_err, source_terms

pytestmark = pytest.mark.gpu

H, W = 128, 32
TH, TW = 64, 32
T_HIGH, T_LOW = 32, 8
PROF_ORDER = (6, 7, 0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13)        # k_render.h, c_prof_order
# the kernel's lane k is PSF component k / 14, profile component PROF_ORDER[k % 14]; the oracle's table is profile-major
LANE_TO_ORACLE = np.array([PROF_ORDER[k % 14] * 3 + k // 14 for k in range(42)])
MARGIN_ROW = 5e-4           # a row end this close to where the kernel rounds it (fp32: < 1e-4 row) is refused
MARGIN_T = 1e-3             # a drop test this close to its threshold (fp32 logs: < 2e-5) is refused


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's walk rules on the host
def _quad_min_rect(a, b, c, x1, x2, y1, y2):
    if x1 <= 0.0 <= x2 and y1 <= 0.0 <= y2:
        return 0.0
    best = math.inf
    for X, Y in ((x1, y1), (x2, y2)):
        t = min(max(-b * X / c, y1), y2)
        best = min(best, a * X * X + (2.0 * b * X + c * t) * t)
        u = min(max(-b * Y / a, x1), x2)
        best = min(best, c * Y * Y + (2.0 * b * Y + a * u) * u)
    return best * 0.99999


def _rows_on_columns(a, b, c, R, x1, x2):
    det = a * c - b * b
    xs = b * math.sqrt(R / (det * a))
    xt, xb = min(max(-xs, x1), x2), min(max(xs, x1), x2)
    st = math.sqrt(max(c * R - det * xt * xt, 0.0))
    sb = math.sqrt(max(c * R - det * xb * xb, 0.0))
    return (-b * xb - sb) / c, (-b * xt + st) / c


def _seg_len(qc, T):
    return int(min((26.0768 - math.sqrt(T)) / math.sqrt(0.5 * qc) * 0.999, 4096.0))


def _nested_big(gA):
    return 3 if gA >= 5 else (2 if gA == 4 else gA)


class Pair(object):
    def __init__(self, rows, L):
        """rows: [(rlo, rhi)] of the pair's slots in slot order"""
        self.R = len(rows)
        self.gA = (self.R + 1) // 2
        self.nb = _nested_big(self.gA)
        self.L = L
        self.rows = rows
        self.ga, self.gb = min(r[0] for r in rows), max(r[1] for r in rows)
        small = rows[2 * self.nb:]
        s0, s1 = (min(r[0] for r in small), max(r[1] for r in small)) if small else (TH, 0)
        self.sa = min(max(s0, self.ga), self.gb)
        self.sb = max(min(s1, self.gb), self.sa)
        self.nested = self.gA >= 4 and self.gb - self.ga <= L
        self.direct = (not self.nested) and L < 4
        self.segments = 1 if (self.nested or self.direct) else -(-(self.gb - self.ga) // L)
        self.phases = (self.sa - self.ga, self.sb - self.sa, self.gb - self.sb) if self.nested else None
        self.comprows = ((self.gb - self.ga) * 2 * self.nb + (self.sb - self.sa) * (self.R - 2 * self.nb)) if self.nested \
            else (self.gb - self.ga) * self.R


class WalkModel(object):
    """what k_render_hw walks for a galaxy-only field at threshold T: per (band, tile row) the pairs of every source"""

    def __init__(self, orc, f, T):
        self.pairs = {}           # (band, ty) -> [Pair]
        self.kept = {}            # (band, ty, source) -> [(lane, rlo, rhi, first row unclipped, last row unclipped)]
        self.min_margin_row, self.min_margin_T = math.inf, math.inf
        for b in range(f["bands"].shape[0]):
            band = f["bands"][b]
            eps = band[0]
            for ty in range(H // TH):
                Y0 = ty * TH
                out = self.pairs.setdefault((b, ty), [])
                for s in range(len(f["typ"])):
                    assert f["typ"][s] == 1
                    patch, (by0, by1), (bx0, bx1) = orc.source_patch(band, H, W, 1, f["radec"][s], f["shape"][s])
                    if patch is None:
                        continue
                    ra, rb = max(by0, Y0) - Y0, min(by1, Y0 + TH) - Y0
                    if rb <= ra or min(bx1, TW) <= max(bx0, 0):
                        continue
                    xa, xb = float(max(bx0, 0)), float(min(bx1, TW) - 1)
                    ya, yb = float(Y0 + ra), float(Y0 + rb - 1)
                    w, mu, cov = components(orc, band, 1, f["radec"][s], f["shape"][s])
                    kept = []
                    for lane in range(42):
                        i = LANE_TO_ORACLE[lane]
                        cxx, cxy, cyy = cov[i, 0, 0], cov[i, 0, 1], cov[i, 1, 1]
                        det = cxx * cyy - cxy * cxy
                        qa, qb, qc = cyy / det, -cxy / det, cxx / det
                        A = f["counts"][s, b] * w[i] / (2 * math.pi * math.sqrt(det))
                        Tk = T + math.log(abs(A) / eps)
                        mx, my = mu[i]
                        half_qmin = 0.5 * _quad_min_rect(qa, qb, qc, xa - mx, xb - mx, ya - my, yb - my)
                        self.min_margin_T = min(self.min_margin_T, abs(half_qmin - Tk))
                        if not half_qmin <= Tk:
                            continue
                        ylo, yhi = _rows_on_columns(qa, qb, qc, 2.0 * max(Tk, 0.0), xa - mx, xb - mx)
                        lo_f, hi_f = (my - Y0) + ylo - 0.02, (my - Y0) + yhi + 0.02
                        first, last = math.ceil(lo_f), math.floor(hi_f)
                        for v, edge in ((lo_f, first), (hi_f, last)):
                            if ra - 1 <= edge <= rb:              # a rounding that the clip to the box's rows does not absorb
                                self.min_margin_row = min(self.min_margin_row, abs(v - round(v)))
                        rlo, rhi = max(ra, first), min(rb, last + 1)
                        if rhi <= rlo:
                            continue
                        kept.append((lane, rlo, rhi, first, last, _seg_len(qc, min(max(Tk, 1.0), 300.0))))
                    self.kept[(b, ty, s)] = kept
                    # slots: by class of eight rows, longest first; inside a class in lane order
                    order = sorted(kept, key=lambda c: (7 - min((c[2] - c[1] - 1) >> 3, 7), c[0]))
                    for p0 in range(0, len(order), 12):
                        grp = order[p0:p0 + 12]
                        out.append(Pair([(c[1], c[2]) for c in grp], min(c[5] for c in grp)))

    def check_margins(self):
        assert self.min_margin_row >= MARGIN_ROW, "a row end %.2g from its rounding: the model cannot vouch for it" % self.min_margin_row
        assert self.min_margin_T >= MARGIN_T, "a drop test %.2g from its threshold" % self.min_margin_T

    def counters(self, b, ty):
        ps = self.pairs[(b, ty)]
        return len(ps), sum(p.comprows for p in ps)


# ---------------------------------------------------------------------------------------------------------------------
# the field
SHARP_BAND = 1


def make_field():
    """two bands of 32 x 128; band 1's PSF narrowed to a tenth of a pixel (short segments, the direct fallback).  Galaxies
    (pixel x, y, flux in nmgy, shape): found by scanning positions with the model for the properties the tests assert"""
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, 2)
    bands[SHARP_BAND, 12:24] *= 0.005
    gal = GALAXIES
    pix = np.array([[g[0], g[1]] for g in gal])
    flux = np.array([g[2] for g in gal])
    f = dict(bands=bands, typ=np.ones(len(gal), np.int32), radec=synth.pixel2equa(bands[0], pix),
             counts=flux[:, None] / bands[None, :, 2] * bands[None, :, 1], shape=np.array([g[3] for g in gal], float))
    return f


GALAXIES = [
    # (x, y, flux, (theta, radius, angle, axis ratio))
    (21.79, 82.68, 15.64, (0.4, 0.94, 49.0, 0.9)),       # below the seam: ranges that begin on row 64; short phases; band 1: segments, direct
    (15.66, 38.19, 6.73, (0.31, 2.24, 56.1, 0.31)),      # above it: ranges whose last row is 63 and 64; an odd last phase
    (16.44, 38.8, 1.66, (0.12, 2.29, 79.4, 0.28)),       # three odd phases
    (17.86, 2.2, 13.52, (0.63, 5.69, 46.6, 0.79)),       # wide: 64-row components beside narrow ones
]


class Ref(object):
    """lam_full, sum |t| and S_sub per threshold, per band and pixel (FieldRef of test_drop_contract.py at this frame's size)"""

    def __init__(self, orc, f, thresholds):
        B = f["bands"].shape[0]
        self.lam = np.zeros((B, H, W), LD)
        self.sabs = np.zeros((B, H, W))
        self.sub = {T: np.zeros((B, H, W)) for T in thresholds}
        self.patch_err = 0.0
        for b in range(B):
            eps = f["bands"][b, 0]
            for s in range(len(f["typ"])):
                r = source_terms(orc, f["bands"][b], f["typ"][s], f["radec"][s], f["shape"][s], H=H, W=W)
                if r is None:
                    continue
                (y0, y1, x0, x1), t, patch = r
                u = t.sum(axis=0)
                self.patch_err = max(self.patch_err, patch_rel_err(u, patch))
                t = t * f["counts"][s, b]
                self.lam[b, y0:y1, x0:x1] += LD(f["counts"][s, b]) * u
                self.sabs[b, y0:y1, x0:x1] += np.abs(t).sum(axis=0)
                for T in thresholds:
                    thr = eps * math.exp(-T) * (1 + DELTA)
                    self.sub[T][b, y0:y1, x0:x1] += np.where(np.abs(t) <= thr, t, 0.0).sum(axis=0)
            self.lam[b] += LD(eps)
        self.lam64 = self.lam.astype(np.float64)
        self.tol = C_R * self.sabs + 4 * np.spacing(self.lam64)

    def check(self, lam_k, T, case):
        lo = (self.lam - LD(1) * lam_k).astype(np.float64)          # what the kernel left out (>= 0 up to rounding)
        r_lo = (lo - self.sub[T]) / self.tol
        r_hi = -lo / self.tol
        print("%s T=%g: worst (left out - S_sub) / tol %.3g, worst excess / tol %.3g" % (case, T, r_lo.max(), r_hi.max()))
        b, y, x = np.unravel_index(np.argmax(r_lo), lo.shape)
        assert r_lo.max() <= 1.0, "%s T=%g: a term above the threshold was left out: band %d pixel (y %d, x %d): lam_full %.17g kernel " \
            "%.17g S_sub %.3g tol %.3g (%.3g tol)" % (case, T, b, y, x, self.lam64[b, y, x], lam_k[b, y, x], self.sub[T][b, y, x],
                                                      self.tol[b, y, x], r_lo.max())
        b, y, x = np.unravel_index(np.argmax(r_hi), lo.shape)
        assert r_hi.max() <= 1.0, "%s T=%g: the kernel exceeds the exact sum: band %d pixel (y %d, x %d): lam_full %.17g kernel %.17g " \
            "tol %.3g (%.3g tol)" % (case, T, b, y, x, self.lam64[b, y, x], lam_k[b, y, x], self.tol[b, y, x], r_hi.max())


@pytest.fixture(scope="module")
def field(orc):
    f = make_field()
    f["ref"] = Ref(orc, f, (T_HIGH, T_LOW))
    f["model"] = {T: WalkModel(orc, f, T) for T in (T_HIGH, T_LOW)}
    return f


@contextlib.contextmanager
def tile_parts(cel, ctx, parts):
    """CEL_OPT_TILE_PARTS for the image sets made and the renders run inside: 1 = one wave per tile, k_render_hw<false, 1> (the
    benchmark's kernel, and the only one that renders incrementally); 0 = the library's rule (four parts on a frame this small)"""
    ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, parts)
    try:
        yield
    finally:
        ctx.set_option(cel._lib.CEL_OPT_TILE_PARTS, 0)


def _images(cel, ctx, f):
    return cel.ImageSet(ctx, f["bands"], H, W)


def _sources(cel, ctx, f):
    return cel.SourceSet(ctx, len(f["typ"]), f["bands"].shape[0]).set(f["typ"], f["radec"], f["counts"], f["shape"])


# ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle(orc, field):
    assert field["ref"].patch_err <= 1e-13
    o_lam, _, _ = orc.render_field(field["bands"], H, W, field["typ"], field["radec"], field["counts"], field["shape"])
    np.testing.assert_allclose(field["ref"].lam64, o_lam, rtol=1e-13, atol=0)


def test_geometry_reaches_every_boundary_of_the_walk(field):
    """from the geometry alone: the eight parity combinations of the three phase lengths, lengths 0, 1 and 2, the seams, the long
    walk beside a short one, more than one segment, the direct fallback"""
    m = field["model"][T_HIGH]
    m.check_margins()
    field["model"][T_LOW].check_margins()
    nested = [p for ps in m.pairs.values() for p in ps if p.nested]
    assert {tuple(n & 1 for n in p.phases) for p in nested} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert {n for p in nested for n in p.phases} >= {0, 1, 2}
    # an odd phase followed by another phase (the single-row step), before the second set and behind it
    assert any(p.phases[0] & 1 and p.phases[1] > 0 for p in nested) and any(p.phases[1] & 1 and p.phases[2] > 0 for p in nested)
    # the low threshold walks nested pairs with odd phases too
    low = [p for ps in field["model"][T_LOW].pairs.values() for p in ps if p.nested]
    assert any(p.phases[0] & 1 for p in low) and any(p.phases[1] & 1 for p in low) and any(p.phases[2] & 1 for p in low)
    # seams: a range whose last row is tile row 63 (nothing of it on the next tile), one whose last row is 64, one that begins on 64
    ends63 = ends64 = begins64 = False
    for (b, ty, s), kept in m.kept.items():
        other = {c[0] for c in m.kept.get((b, 1 - ty, s), [])}
        for (lane, rlo, rhi, first, last, L) in kept:
            if ty == 0 and last == 63 and rhi == 64 and lane not in other:
                ends63 = True
            if ty == 1 and last == 0 and rhi == 1:
                ends64 = True
            if ty == 1 and first == 0 and rlo == 0 and lane not in other:
                begins64 = True
    assert ends63 and ends64 and begins64
    # a full 64-row walk next to a component of at most two rows in one nested pair
    assert any(max(r[1] - r[0] for r in p.rows) == 64 and min(r[1] - r[0] for r in p.rows) <= 2 for p in nested)
    # the general walk with more than one segment; the direct fallback
    every = [p for ps in m.pairs.values() for p in ps]
    assert any(p.segments > 1 for p in every) and any(p.direct for p in every)


def test_model_matches_the_kernels_work_counters(cel, field):
    """the host model walks what the device walks: pairs and component-rows per tile (CEL_OPT_TILE_TIMING, third word)"""
    ctx = cel.Context(0)
    for T in (T_HIGH, T_LOW):
        ctx.set_option(cel._lib.CEL_OPT_TILE_TIMING, 1)
        try:
            with tile_parts(cel, ctx, 1), tail_log(ctx, T):
                images = _images(cel, ctx, field)
                images.render(_sources(cel, ctx, field))
                w = images.tile_timing()[:, 2]
        finally:
            ctx.set_option(cel._lib.CEL_OPT_TILE_TIMING, 0)
        for b in range(field["bands"].shape[0]):
            for ty in range(H // TH):
                word = int(w[b * (H // TH) + ty])
                assert ((word >> 12) & 0xfffff, word >> 32) == field["model"][T].counters(b, ty), (T, b, ty)


@pytest.mark.parametrize("T", [T_HIGH, T_LOW])
@pytest.mark.parametrize("parts", [1, 0], ids=["one-wave-per-tile", "default-parts"])
def test_every_pixel_within_the_bound(cel, field, T, parts):
    ctx = cel.Context(0)
    with tile_parts(cel, ctx, parts), tail_log(ctx, T):
        images = _images(cel, ctx, field)
        images.render(_sources(cel, ctx, field))
        lam = images.model_images()
    field["ref"].check(lam, T, "two-row walk, parts %d" % parts)


def test_same_bits_twice_and_incrementally(cel, orc, field):
    """two renders of the field give the same bits; after set_rows moved two galaxies, the incremental render (dirty tiles only)
    equals a full render of the moved catalogue bit for bit, and holds the bound"""
    ctx = cel.Context(0)
    f = field
    with tile_parts(cel, ctx, 1), tail_log(ctx, T_LOW):
        images, again = _images(cel, ctx, f), _images(cel, ctx, f)
        srcs = _sources(cel, ctx, f)
        images.render(srcs)
        first = images.model_images().copy()
        again.render(_sources(cel, ctx, f))
        assert np.array_equal(first, again.model_images())
        images.render(srcs)
        assert np.array_equal(first, images.model_images())
        rows = np.array([0, len(f["typ"]) - 1], np.int32)
        radec2 = f["radec"].copy()
        radec2[rows] += np.array([[1.3e-4, -0.7e-4], [-0.6e-4, 0.9e-4]])
        srcs.set_rows(rows, f["typ"][rows], radec2[rows], f["counts"][rows], f["shape"][rows])
        images.render(srcs)
        assert images.last_render_dirty_tiles() > 0              # the incremental form ran
        moved = dict(f, radec=radec2)
        again.render(_sources(cel, ctx, moved))
        assert again.last_render_dirty_tiles() == -1
        assert np.array_equal(images.model_images(), again.model_images())
        Ref(orc, moved, (T_LOW,)).check(images.model_images(), T_LOW, "incremental")
