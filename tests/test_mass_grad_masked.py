"""The exact conditional's gradient and HMC step on a MASKED image set: CEL_OPT_SAMPLER_MASK = 21, k_mass_grad_masked (k_mass_grad.h),
the resident mode 8 and cel_slice_sample(param = 3) under it, ImageSet.patch_loglik_resident_grad / hmc_step(mask="honour"),
ModelGibbs(mask="honour", mask_engine="device", hmc_conditional="exact").

The scene is tests/test_mass_grad.py's (2 bands on a 96 x 112 frame, seven sources, eleven proposals) with NaN counts written
into band 0 before the split, the split made under CEL_OPT_HONOUR_MASK.  The mask is built from the scene's own boxes:

  (a) the core pixel of the star and of the floored galaxy;
  (b) one whole 32 x 64 chunk of the big galaxy's proposal box (its third chunk: rows y0 .. y0 + 63, columns x0 + 64 .. x0 + 95);
  (c) the row pair either side of that box's chunk seam (box rows 63 and 64) from its second chunk on, and five rows of the
      columns behind its last full 32-column chunk;
  (d) the sharp type-2 source's box (proposal and catalogue row) masked everywhere;
  (e) band 1 without a masked pixel.

  1. slots 1-6: (exact row - reference row) read per band against math.fsum of the derivative stamps over the OBSERVED pixels
     of the proposal's own box; the bar is tests/test_mass_grad.py's (BAR below is the literal of its identity test)
  2. resolving power: the same yardstick summed over EVERY pixel misses by at least 100 x the bar on the sources of (a) and (b)
  3. slots 0 and 7 + b: the row's definition, bit by bit, from stamp_mass under CEL_OPT_HONOUR_MASK; a proposal that fails the
     cover test gives -inf and zeros; a box masked everywhere adds exact zeros
  4. a proposal whose boxes hold no masked pixel, and every proposal in the unmasked band, return the bits of the same records
     on an image set with the NaNs replaced by 0 (the same split: the masked split is that set's, bit for bit)
  5. HMC: hmc_step(conditional="exact", mask="honour") against tests/test_hmc_exact.py's restatement from public calls on its
     scene with a mask of the same kinds; a trajectory off its photon rectangle dies; host engine against device engine through
     ModelGibbs over three updates

MEASURED on the device: worst |rows - observed-pixel fsum| / sum |plane| = 1.96e-12 (bar 1e-10); the all-pixel sum misses by
7.9e7 (star), 1.6e8 (floored galaxy) and 3.6e9 (big galaxy) times the bar in the masked band, by less than 0.02 of it wherever
nothing is masked; the engines' HMC test accepts 33 of 36 updates over 306 gradient evaluations.
"""
import math

import numpy as np
import pytest

import test_hmc_exact as he
import test_mass_grad as tm
from test_mass_grad import B, H, NAMES, P, P_BIG, P_FLOOR, P_MISS, P_SHARP, P_STAR, P_UNCOVERED, W, C_FLOOR, C_SHARP, C_STAR, _six

gpu = pytest.mark.gpu
#: tests/test_mass_grad.py::test_identity_with_the_derivative_stamps holds the unmasked row to 1e-10 x sum |plane|; the literal has
#: no name there, so it is named here and not changed
BAR = 1e-10
MASKED_BAND, CLEAN_BAND = 0, 1


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def _honour(ctx, L):
    import contextlib

    @contextlib.contextmanager
    def cm():
        was = ctx.get_option(L.CEL_OPT_HONOUR_MASK)
        ctx.set_option(L.CEL_OPT_HONOUR_MASK, 1)
        try:
            yield
        finally:
            ctx.set_option(L.CEL_OPT_HONOUR_MASK, was)
    return cm()


def _grow(box, by, Hh, Ww):
    return max(box[0] - by, 0), min(box[1] + by, Hh), max(box[2] - by, 0), min(box[3] + by, Ww)


class MaskedScene(tm.Scene):
    def __init__(self, cel):
        super().__init__(cel)                                    # the unmasked scene and every assertion on its layout
        L = self.L
        cbx, cst = self.iset.source_boxes(self.cat)              # (B, S, 4) = y0, y1, x0, x1
        m = np.zeros((B, H, W), dtype=bool)
        b = MASKED_BAND
        pix = {C_STAR: (31.3, 40.2), C_FLOOR: (88.6, 21.1)}
        self.cores = {}
        for s, (x, y) in pix.items():                            # (a)
            self.cores[s] = (int(math.floor(y)), int(math.floor(x)))
            m[b][self.cores[s]] = True
        y0, y1, x0, x1 = (int(v) for v in self.pboxes[b, P_BIG])
        assert y1 - y0 > 64 and x1 - x0 > 96 and (x1 - x0) % 32
        self.chunk = (y0, y0 + 64, x0 + 64, x0 + 96)             # (b): the box's third chunk (the floored galaxy lies under it)
        m[b, y0:y0 + 64, x0 + 64:x0 + 96] = True
        m[b, y0 + 63:y0 + 65, x0 + 32:x1] = True                 # (c): the seam between the box's row chunks, from its second chunk on
        self.tail = (y0 + 70, y0 + 75, x0 + 32 * ((x1 - x0) // 32), x1)
        assert self.tail[3] > self.tail[2] and self.tail[1] <= y1, (self.tail, y0, y1)
        m[b, self.tail[0]:self.tail[1], self.tail[2]:self.tail[3]] = True
        for bx, st in ((self.pboxes[b, P_SHARP], self.pstatus[b, P_SHARP]), (cbx[b, C_SHARP], cst[b, C_SHARP])):      # (d)
            assert st > 0
            m[b, bx[0]:bx[1], bx[2]:bx[3]] = True
        assert not m[CLEAN_BAND].any()                           # (e)
        self.mask = m
        self.nelec_masked = np.where(m, np.nan, self.nelec)
        self.nelec0 = np.where(m, 0.0, self.nelec)
        # the source of (d) alone has a box masked everywhere; every source keeps the whole of its box in the other band
        for s in range(tm.S - 1):
            bx = cbx[b, s]
            assert (m[b, bx[0]:bx[1], bx[2]:bx[3]].mean() == 1.0) == (s == C_SHARP), s
        self.iset.set_nelec(self.nelec_masked)
        assert list(self.iset.masked) == [int(m[0].sum()), 0]
        self.split(self.iset, self.cat)
        self.sums = self.iset.sample_sums()
        self.has_patch = (self.iset.sample_box_areas() > 0).astype(np.float64)
        self.rects = self.iset.photon_rects()
        assert self.sums[C_SHARP, b] == 0 and self.sums[C_SHARP, CLEAN_BAND] > 0 and self.has_patch[C_SHARP, b] == 1
        assert np.all(self.sums[:tm.C_ONEBAND].sum(axis=1) > 100)
        # the same records on the set with the NaNs replaced by 0: the unmasked library's path
        self.iset0 = cel.ImageSet(self.ctx, self.bands, H, W)
        self.iset0.set_nelec(self.nelec0)
        tm.Scene.split(self, self.iset0, self.cat)
        assert np.array_equal(self.iset0.sample_sums(), self.sums) and np.array_equal(self.iset0.photon_rects(), self.rects)
        # which proposal boxes hold a masked pixel at all
        self.touched = np.zeros((B, P), dtype=bool)
        for bb in range(B):
            for p in range(P):
                if self.pstatus[bb, p] > 0:
                    q = self.pboxes[bb, p]
                    self.touched[bb, p] = m[bb, q[0]:q[1], q[2]:q[3]].any()
        q = self.pboxes[b, P_SHARP]
        assert m[b, q[0]:q[1], q[2]:q[3]].all()
        # the cover test against the masked split's photon rectangles (k_sg_cover's rule on the host)
        self.cov = np.array([self.covered(p) for p in range(P)])
        assert not self.cov[P_MISS] and not self.cov[P_UNCOVERED] and self.cov[[P_STAR, P_FLOOR, P_BIG, P_SHARP]].all() and self.cov.sum() >= 8
        self.covered_rows = [p for p in range(P) if self.cov[p]]

    def split(self, iset, cat):
        with _honour(self.ctx, self.L):
            super().split(iset, cat)

    def rows(self, conditional, prop=None, owner=None, iset=None):
        """the masked set's rows: the exact one under mask="honour", the reference's as it always was (its mode 8 reads no pixel
        outside the patches); iset=: the same call on another image set, without the keyword"""
        prop, owner = self.prop if prop is None else prop, self.owner if owner is None else owner
        if iset is not None:
            return iset.patch_loglik_resident_grad(prop, owner, conditional=conditional)
        return self.iset.patch_loglik_resident_grad(prop, owner, conditional=conditional, mask="honour" if conditional == "exact" else "refuse")

    def observed(self, b, p):
        q = self.pboxes[b, p]
        return ~self.mask[b, q[0]:q[1], q[2]:q[3]]


@pytest.fixture(scope="module")
def scene(cel):
    return MaskedScene(cel)


@pytest.fixture(scope="module")
def dmass(scene):
    """tests/test_mass_grad.py's fixture on the masked set: per band b (d mass_b / d q read off the rows, the rows under 0 and 1)
    with band b's counts alone non-zero"""
    out = []
    for b in range(B):
        prop, c = scene.one_band(b)
        r0, r1 = scene.rows("reference", prop), scene.rows("exact", prop)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = (_six(r1) - _six(r0)) / (-c[:, b])[:, None]
        out.append((d, r0, r1))
    return out


@pytest.fixture(scope="module")
def jac(scene):
    """the derivative stamps of every proposal on its own box, per band (they read no pixel: taken on the NaN-free set)"""
    return [scene.iset0.stamp_jacobians(scene.prop, b, scaled=False)[0] for b in range(B)]


# ---- 1, 2 ------------------------------------------------------------------------------------------------------------------
@gpu
def test_observed_pixel_sum_of_the_derivative_stamps(scene, dmass, jac):
    """d mass_b / d q_i = math.fsum of plane i of the derivative stamps over the OBSERVED pixels of the proposal's own box, to
    BAR x sum |plane| over those pixels; and the all-pixel sum misses by at least 100 x the bar on the sources of (a) and (b)"""
    worst, seen = 0.0, 0
    miss = {}
    for b in range(B):
        d = dmass[b][0]
        for p in scene.covered_rows:
            if scene.has_patch[scene.owner[p], b] == 0:
                continue
            pl = jac[b][p]
            assert pl is not None, (NAMES[p], b)
            obs = scene.observed(b, p)
            assert obs.shape == pl.shape[1:]
            for i in range(1, pl.shape[0]):
                want, mag = math.fsum(pl[i][obs]), math.fsum(np.abs(pl[i][obs]))
                every, mag_every = math.fsum(pl[i].ravel()), math.fsum(np.abs(pl[i]).ravel())
                diff = abs(d[p, i - 1] - want)
                print("OBSERVED band %d %-28s plane %d: rows %.17g stamps %.17g (all pixels %.17g) sum|plane| %.6g ratio %.3g"
                      % (b, NAMES[p], i, d[p, i - 1], want, every, mag, diff / mag if mag > 0 else 0.0))
                assert diff <= BAR * mag, (b, NAMES[p], i, d[p, i - 1], want, mag)
                if mag > 0:
                    worst = max(worst, diff / mag)
                if mag_every > 0:
                    miss[(b, p)] = max(miss.get((b, p), 0.0), abs(d[p, i - 1] - every) / (BAR * mag_every))
                seen += 1
            if pl.shape[0] == 3:
                assert np.all(d[p, 2:] == 0.0)
    assert seen >= 40
    print("observed-pixel sum: worst |difference| / sum |plane| = %.3g; all-pixel sum misses by (x the bar) %s"
          % (worst, {(b, NAMES[p]): "%.3g" % v for (b, p), v in miss.items()}))
    # a kernel that ignores the mask cannot pass
    for p in (P_STAR, P_FLOOR, P_BIG):
        assert scene.touched[MASKED_BAND, p] and miss[(MASKED_BAND, p)] >= 100.0, (NAMES[p], miss[(MASKED_BAND, p)])
    # ... and where nothing is masked the two yardsticks are one
    assert all(v <= 1.0 for (b, p), v in miss.items() if not scene.touched[b, p])


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_row_definition_from_the_observed_mass(scene, dmass):
    sc = scene
    r0, r1 = sc.rows("reference"), sc.rows("exact")
    with _honour(sc.ctx, sc.L):
        mass = sc.iset.stamp_mass(sc.prop)
    full = sc.iset0.stamp_mass(sc.prop)
    # (the observed-mass kernel sums the tile's pixels, the unmasked one inside its walk: the same ~2 000 to 10 000 terms of one sign in
    # another order, n x 2^-53 apart at the most -- 1e-12 holds that with room; the BITS of the observed mass are pinned below)
    assert np.allclose(mass[:, CLEAN_BAND], full[:, CLEAN_BAND], rtol=1e-12, atol=0.0)
    assert mass[P_SHARP, MASKED_BAND] == 0.0 and full[P_SHARP, MASKED_BAND] > 0.5
    for p in (P_STAR, P_FLOOR, P_BIG):
        assert 0.0 < mass[p, MASKED_BAND] < full[p, MASKED_BAND]
    cov = sc.cov
    assert np.array_equal(r0[0], sc.iset.patch_loglik_resident(sc.prop, sc.owner))
    for p in range(P):
        hp = sc.has_patch[sc.owner[p]]
        if not cov[p]:                                           # -inf and zeros
            assert r1[0][p] == -np.inf and np.all(r1[1][p] == 0.0) and np.all(r1[2][p] == 0.0) and np.all(r1[3][p] == 0.0), NAMES[p]
            continue
        acc = 0.0
        for b in range(B):
            acc = acc + (float(sc.pcounts[p, b]) * (float(mass[p, b]) - float(sc.wsum[b]))) * float(hp[b])
        assert r1[0][p] == float(r0[0][p]) + (-acc), (NAMES[p], r1[0][p], r0[0][p], acc)
        for b in range(B):
            assert r1[2][p, b] == float(r0[2][p, b]) + (-(float(mass[p, b]) - float(sc.wsum[b])) * float(hp[b])), (NAMES[p], b)
        ge = _six(r1)[p] - _six(r0)[p]
        parts = sum(_six(dmass[b][2])[p] - _six(dmass[b][1])[p] for b in range(B))
        scale = np.abs(_six(r0)[p]) + np.abs(_six(r1)[p]) + sum(np.abs(_six(dmass[b][1])[p]) + np.abs(_six(dmass[b][2])[p]) for b in range(B))
        assert np.all(np.abs(ge - parts) <= 8 * np.spacing(scale)), (NAMES[p], ge, parts)
    # the box masked everywhere: its band adds exact zeros to slots 1-6 and charges no mass
    d = dmass[MASKED_BAND]
    assert np.array_equal(_six(d[2])[P_SHARP], _six(d[1])[P_SHARP])
    assert d[2][2][P_SHARP, MASKED_BAND] == float(d[1][2][P_SHARP, MASKED_BAND]) + (-(0.0 - float(sc.wsum[MASKED_BAND])))
    assert np.any(_six(dmass[CLEAN_BAND][2])[P_SHARP] != _six(dmass[CLEAN_BAND][1])[P_SHARP])
    # repeated calls: the same bits
    again = sc.rows("exact")
    for a, b in zip(again, r1):
        assert np.array_equal(a, b)
    assert sc.ctx.get_option(sc.L.CEL_OPT_SAMPLER_MASK) == 0 and sc.ctx.get_option(sc.L.CEL_OPT_HONOUR_MASK) == 0


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_unmasked_boxes_return_the_unmasked_bits(scene, dmass):
    sc = scene
    r1, u1 = sc.rows("exact"), sc.rows("exact", iset=sc.iset0)
    clean = [p for p in sc.covered_rows if not sc.touched[:, p].any()]
    dirty = [p for p in sc.covered_rows if sc.touched[:, p].any()]
    print("UNMASKED BITS: proposals without a masked pixel in any box: %s" % [NAMES[p] for p in clean])
    assert len(clean) >= 1 and len(dirty) >= 4
    # slots 1-6 come from k_mass_grad_masked: k_mass_grad's bits where no pixel is masked.  Slots 0 and 7 + b carry the mass, which the
    # observed-mass kernel sums in another order than the unmasked one (test_row_definition_from_the_observed_mass pins their bits
    # to stamp_mass under CEL_OPT_HONOUR_MASK): equal to the rounding of that sum
    assert np.array_equal(_six(r1)[clean], _six(u1)[clean])
    scale = np.abs(sc.pcounts[clean]).sum(axis=1)
    assert np.all(np.abs(r1[0][clean] - u1[0][clean]) <= 1e-12 * scale) and np.allclose(r1[2][clean], u1[2][clean], rtol=0.0, atol=1e-12)
    assert all(np.any(_six(r1)[p] != _six(u1)[p]) for p in (P_STAR, P_FLOOR, P_BIG))
    for a, b in zip(r1, u1):                                      # the uncovered rows are -inf and zeros either way
        assert np.array_equal(a[[P_MISS, P_UNCOVERED]], b[[P_MISS, P_UNCOVERED]])
    # the band without a masked pixel: every proposal
    prop, _ = sc.one_band(CLEAN_BAND)
    assert np.array_equal(_six(dmass[CLEAN_BAND][2]), _six(sc.rows("exact", prop, iset=sc.iset0)))
    # a set without a NaN does not read the option: the same bits with it 0 and 1
    k = sc.iset0.patch_loglik_resident_grad(sc.prop, sc.owner, conditional="exact", mask="honour")
    for a, b in zip(k, u1):
        assert np.array_equal(a, b)


# ---- 5: HMC ----------------------------------------------------------------------------------------------------------------
class MaskedHmc(he.Scene):
    """tests/test_hmc_exact.py's scene with NaN counts in band 0: the edge star's core pixel, the third 32 x 64 chunk and the seam
    rows of the big galaxy's box, and the floored galaxy's box (four pixels of margin: its trajectories stay inside) masked
    everywhere; band 1 without a masked pixel; the split under CEL_OPT_HONOUR_MASK"""

    def __init__(self, cel):
        super().__init__(cel)
        L = self.L
        bx, st = self.iset.source_boxes(self.cat)
        m = np.zeros((B, H, W), dtype=bool)
        m[0, 50, 2] = True                                       # the edge star at (2.3, 50.7)
        y0, y1, x0, x1 = (int(v) for v in bx[0, he.C_GAL])
        assert y1 - y0 > 64 and x1 - x0 >= 96
        m[0, y0:y0 + 64, x0 + 64:x0 + 96] = True
        m[0, y0 + 63:y0 + 65, x0 + 32:x1] = True
        g = _grow(bx[0, he.C_FLOOR], 4, H, W)
        m[0, g[0]:g[1], g[2]:g[3]] = True
        self.mask = m
        self.floor_box = g
        self.iset.set_nelec(np.where(m, np.nan, self.nelec))
        self.ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
        try:
            with _honour(self.ctx, L):
                self.iset.photon_split_resident(self.cat, seed=9)
        finally:
            self.ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
        self.sums = self.iset.sample_sums()
        assert np.all(self.sums[he.RUNNING].sum(axis=1) > 100) and self.sums[he.C_FLOOR, 0] == 0 and self.sums[he.C_NOPATCH].sum() == 0

    def row(self, s, q, phi_max):
        self.one.set(self.typ[s:s + 1], np.array([q[:2]]), self.counts[s:s + 1], np.array([q[2:]]))
        ll, gr, _, gs = self.iset.patch_loglik_resident_grad(self.one, np.array([s], dtype=np.int32), conditional="exact", mask="honour")
        g = [float(gr[0, 0]), float(gr[0, 1])] + ([float(x) for x in gs[0]] if self.typ[s] == 1 else [0.0] * 4)
        pri = 0.0
        if self.typ[s] == 1 and phi_max > 0.0:
            sg = q[3]
            g[3] = g[3] + (2.0 / ((sg * sg) * sg) - 4.0 / sg)
            s2 = sg * sg
            pri = -2.0 * math.log(s2) - 1.0 / s2
        return float(ll[0]) + pri, g


@pytest.fixture(scope="module")
def hmc_scene(cel):
    return MaskedHmc(cel)


@gpu
@pytest.mark.parametrize("L", [1, 3])
def test_hmc_restated_from_public_calls(hmc_scene, L):
    """tests/test_hmc_exact.py::test_restated_from_public_calls on the masked scene: every trajectory, the returned momentum and
    the decision bit for bit, log alpha to its 8 ulp"""
    sc = hmc_scene
    eps, seed = 0.4, 21 + L
    imass = sc.default_imass()
    imass[he.C_FLOOR, 3] *= 1e-4
    p0 = sc.momentum(imass, seed=3 + L)
    sc.reset()
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=he.PHI_MAX, chain_ids=sc.ids, conditional="exact", mask="honour")
    log_u = he._log_u(seed, np.arange(he.S))
    evals = accepted = 0
    for s in he.RUNNING:
        qr, pr, lar, acc, ev, v0, v1 = sc.restated(s, sc.q0()[s], p0[s], imass[s], eps, L, he.PHI_MAX, log_u[s])
        evals += ev
        accepted += int(acc)
        print("RESTATED masked L %d chain %d: log alpha %.17g (device %.17g), log u %.6f, accepted %s, v0 %r v1 %r"
              % (L, s, lar, la[s], log_u[s], acc, v0, v1))
        assert v0 is not None, "the trajectory of chain %d died: choose other inputs" % s
        bar = 8 * np.spacing(max(abs(v0), abs(v1), 1.0))
        assert abs(la[s] - lar) <= bar, (s, la[s], lar, bar)
        assert abs(log_u[s] - lar) > 2 * bar, "the decision lies inside the band: change the seed"
        assert np.array_equal(q[s], np.array(qr)), (s, q[s], qr)
        assert np.array_equal(p[s], np.array(pr)), (s, p[s], pr)
    assert st["steps"] == L and st["evals"] == evals == len(he.RUNNING) * (L + 1) and st["accepted"] == accepted
    # the launch count of the unmasked step: the masked twins replace their launches one for one
    assert st["launches"] - (1 + 1 + 9 * (L + 1) + L + 3 + 2 + 1) in (1, 2), st
    alone = [he.C_T2, he.C_OTHER, he.C_NOPATCH]
    assert np.array_equal(q[alone], sc.q0()[alone]) and np.all(np.isnan(la[alone]))
    assert sc.ctx.get_option(sc.L.CEL_OPT_SAMPLER_MASK) == 0 and sc.ctx.get_option(sc.L.CEL_OPT_HONOUR_MASK) == 0
    assert sc.ctx.get_option(sc.L.CEL_OPT_GRAD_CONDITIONAL) == 0
    # the unmasked mass is another target: the floored galaxy's band 0 charges nothing here
    sc.reset()
    with pytest.raises(ValueError, match="masked"):
        sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=he.PHI_MAX, chain_ids=sc.ids, conditional="exact")
    sc.reset()


@gpu
def test_hmc_trajectory_off_its_photon_rectangle_dies(hmc_scene):
    sc = hmc_scene
    imass, p0 = np.zeros((he.S, 6)), np.zeros((he.S, 6))
    ids = np.full(he.S, -1, dtype=np.int32)
    ids[he.C_STAR] = he.C_STAR
    imass[he.C_STAR, :2] = 1.0
    eps, L = 1.0, 4
    p0[he.C_STAR, 0] = 30.0 * sc.pix_deg / math.cos(math.radians(sc.radec[he.C_STAR, 1]))
    sc.reset()
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, 5, phi_max=he.PHI_MAX, chain_ids=ids, conditional="exact", mask="honour")
    qr, pr, lar, acc, ev, _, _ = sc.restated(he.C_STAR, sc.q0()[he.C_STAR], p0[he.C_STAR], imass[he.C_STAR], eps, L, he.PHI_MAX, 0.0)
    assert lar == -math.inf and ev == 2 and not acc
    assert la[he.C_STAR] == -np.inf and st["evals"] == 2 and st["accepted"] == 0, (la, st)
    assert np.array_equal(q[he.C_STAR], sc.q0()[he.C_STAR]) and np.array_equal(p[he.C_STAR], -p0[he.C_STAR])
    assert np.all(np.isnan(np.delete(la, he.C_STAR)))
    sc.reset()


def _masked_gibbs_pair(cel, mask_kw):
    """tests/test_hmc_exact.py's engines scene (12 sources, seed 23) with NaN counts in band 0: every source's core pixel, the
    columns 40 .. 43 and the rows 63, 64"""
    from desi_mcmc_amd import celeste_mcmc, synth
    Sf = 12
    ctx = cel.Context(0)
    f0 = synth.SyntheticField(ctx, Sf, B, H, W, frac_gal=0.5, seed=23)
    nelec = f0.nelec.copy()
    for x, y in f0.src["pix"]:
        if 0 <= int(y) < H and 0 <= int(x) < W:
            nelec[0, int(y), int(x)] = np.nan
    nelec[0, :, 40:44] = np.nan
    nelec[0, 63:65, :] = np.nan
    flux5 = np.full((Sf, 5), 3.0)
    flux5[:, :B] = f0.src["flux"]
    g = {}
    for e, kw in mask_kw.items():
        imgs = cel.ImageSet(ctx, f0.bands, H, W)
        imgs.set_nelec(nelec)
        gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W, npix_observed=imgs.npix_observed())
        g[e] = celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5, conditional="exact",
                                       hmc_conditional="exact", mask="honour", **kw)
    return ctx, g, Sf


@gpu
def test_hmc_host_engine_against_device_engine(cel):
    L = cel._lib
    ctx, g, Sf = _masked_gibbs_pair(cel, dict(host=dict(engine="host"), auto=dict(engine="auto", mask_engine="device")))
    assert g["auto"]._hmc_engine_on_device() and not g["host"]._hmc_engine_on_device()
    start = np.concatenate([g["auto"].u, g["auto"].shape], axis=1)
    for e in g:
        g[e].resample_photons()
        g[e].resample_fluxes()
    for update in range(3):
        for e in g:
            g[e].resample_hmc()
        for name in ("typ", "u", "fluxes", "shape", "_hmc_p"):
            assert np.array_equal(getattr(g["host"], name), getattr(g["auto"], name)), (update, name)
        assert g["host"].timing["hmc_evals"] == g["auto"].timing["hmc_evals"] > 0
        assert g["host"].timing["hmc_accepted"] == g["auto"].timing["hmc_accepted"]
    t = g["auto"].timing
    print("ENGINES masked: hmc evals %d, accepted %d of %d updates" % (t["hmc_evals"], t["hmc_accepted"], 3 * Sf))
    assert t["hmc_accepted"] > 0 and np.any(np.concatenate([g["auto"].u, g["auto"].shape], axis=1) != start)
    for k in (L.CEL_OPT_GRAD_CONDITIONAL, L.CEL_OPT_SAMPLER_MASK, L.CEL_OPT_HONOUR_MASK):
        assert ctx.get_option(k) == 0
