"""The exact conditional's gradient: CEL_OPT_GRAD_CONDITIONAL = 19, k_mass_grad.h, the resident mode 8 of cel_patch_loglik_multi
under it, ImageSet.patch_loglik_resident_grad(conditional="exact"), ModelGibbs(hmc_conditional="exact").location_loglik_grad.

  0. (no GPU) the boundary: 56 symbols, key 19 in the header and the mirror, ModelGibbs' new keyword, the budget
  1. d mass_b / d q read off the rows against math.fsum of the derivative stamps over the proposal's own box
  2. the same against the explicit mode 10 on all-zero data over the own boxes (device against device)
  3. the row's definition: slot 0 (ModelGibbs.location_loglik's bits), the counts slots, the uncovered proposal, has_patch = 0
  4. key 19 = 0 is a fresh context's bits; repeated calls and both CEL_OPT_KERNEL settings give slots 1.. the same bits
  5. refusals leave the sentinel and the option alone

The scene: 2 bands on a 96 x 112 frame (tests/test_patch_grad.py's frame), a catalogue of seven sources with a resident split made
under CEL_OPT_SPLIT_FULL_BOX, eleven proposals: a star; a star whose box the frame's edge cuts; a type-1 galaxy whose box spans
several 32 x 64 chunks; a galaxy under the sigma floor; a type-2 galaxy; the sharpest galaxy the PSF allows (a type-2 source with
W = 1e-6: every component is a PSF component; k_mass_grad's plain form has ONE path, so this is an ordinary proposal to it); a star
beside the frame with a stamp in one band only (so its source has no sample patch in the other: has_patch = 0); an overlap-test
miss; a proposal of that source moved inward, with a stamp in the band where the source has no patch; a star moved so that its
box no longer covers its photon rectangle; a second proposal of the first star (owner is not the identity).
"""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B = 96, 112, 2
gpu = pytest.mark.gpu
S = 7
C_STAR, C_EDGE, C_BIG, C_FLOOR, C_T2, C_SHARP, C_ONEBAND = range(S)
P_STAR, P_EDGE, P_BIG, P_FLOOR, P_T2, P_SHARP, P_ONEBAND, P_MISS, P_INWARD, P_UNCOVERED, P_STAR2 = range(11)
NAMES = ["star", "edge star", "big galaxy", "floored galaxy", "type-2 galaxy", "sharp type-2", "star with one band", "overlap-test miss",
         "one-band star moved inward", "uncovered star", "second star proposal"]
P = len(NAMES)
COVERED = [p for p in range(P) if p not in (P_MISS, P_UNCOVERED)]


# ---- 0 (no GPU) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import desi_mcmc_amd
    return desi_mcmc_amd


def test_boundary_key_19_and_56_symbols(built):
    from desi_mcmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    assert re.search(r"CEL_OPT_GRAD_CONDITIONAL = 19\b", header) and _lib.CEL_OPT_GRAD_CONDITIONAL == 19
    assert re.search(r"CEL_OPT_SLICE_CONDITIONAL = 18\b", header) and re.search(r"CEL_K_COUNT = 15\b", header)
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    bound = [s[0] for s in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) == 56 and declared == exported == set(bound)
    assert max(_lib.KERNELS.values()) == 14
    # the header states the row, the HMC step's launch count and why the Metropolis test stays exact
    doc = header[header.index("CEL_OPT_GRAD_CONDITIONAL = 19"):header.index("CEL_OPT_TILE_PARTS = 13")]
    assert "v_ref + e" in doc and "FIXED integer box" in doc and "-inf" in doc and "Mode 9, mode 10" in doc
    hmc = header[header.index("param 3: one HMC update"):header.index("int cel_slice_sample(")]
    assert "CEL_OPT_GRAD_CONDITIONAL = 1" in hmc and "9 (L + 1)" in hmc and "volume-preserving" in hmc


class _NoDevice(object):
    """an image set that is never asked anything: ModelGibbs' constructor reads `masked` alone under mask='refuse'"""
    masked = np.zeros(B, dtype=np.int64)
    eps = np.ones(B)
    B = B

    def _refuse_masked(self, who):
        pass


def test_model_gibbs_hmc_conditional_keyword(built):
    from desi_mcmc_amd import celeste_mcmc
    gf = celeste_mcmc.GibbsField(_NoDevice(), list(range(B)), np.ones(B), np.ones(B), H * W)
    args = ([gf], np.zeros(2, dtype=np.int32), np.zeros((2, 2)), np.ones((2, 5)), np.zeros((2, 4)))
    g = celeste_mcmc.ModelGibbs(*args, conditional="exact", hmc_conditional="exact")
    assert g.hmc_conditional == "exact" and g.conditional == "exact"
    assert celeste_mcmc.ModelGibbs(*args, conditional="exact").hmc_conditional is None
    with pytest.raises(ValueError, match="needs conditional='exact'"):
        celeste_mcmc.ModelGibbs(*args, hmc_conditional="exact")
    with pytest.raises(ValueError, match="hmc_conditional"):
        celeste_mcmc.ModelGibbs(*args, conditional="exact", hmc_conditional="reference")


def test_resource_budget_lists_the_kernel(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    k = resource_usage.collect()
    budget = json.load(open(resource_usage.BUDGET))["kernels"]
    assert "k_mass_grad" in k and "k_mass_grad" in budget and "k_mass_grad_apply" in k
    # k_stamp_jac's line: no scratch, no spills, at most 128 VGPRs, four waves
    assert k["k_mass_grad"]["scratch"] == 0 and k["k_mass_grad"]["vgpr_spill"] == 0
    assert k["k_mass_grad"]["vgpr"] <= 128 and k["k_mass_grad"]["occupancy"] >= 4
    assert budget["k_mass_grad"]["min_occupancy"] == 4 and budget["k_mass_grad"]["max_scratch"] == 0
    assert "| `k_mass_grad` |" in resource_usage.table(k)
    assert not [m for m in resource_usage.check(k) if m.startswith("k_mass_grad")]


# ---- the scene ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


class Scene(object):
    def __init__(self, cel):
        from desi_mcmc_amd import synth
        L = cel._lib
        self.cel, self.L = cel, L
        self.ctx = cel.Context(0)
        self.bands = synth.make_bands(H, W, B)
        self.iset = cel.ImageSet(self.ctx, self.bands, H, W)
        self.one = cel.SourceSet(self.ctx, 1, B)
        # a star beside the frame that has a stamp in exactly one band: the first column, going outward, where the bands differ
        x, found = -1.0, None
        while x > -60.0 and found is None:
            u = synth.pixel2equa(self.bands[0], np.array([[x, 50.2]]))
            self.one.set(np.zeros(1, dtype=np.int32), u, np.full((1, B), 5000.0), np.zeros((1, 4)))
            st = self.iset.source_boxes(self.one)[1][:, 0]
            if (st > 0).sum() == 1:
                found = (x, st.copy())
            x -= 0.25
        assert found is not None, "no column beside the frame where one band alone has a stamp"
        self.oneband_x, st = found
        self.band_with, self.band_without = int(np.argmax(st > 0)), int(np.argmin(st > 0))
        pix = np.array([[31.3, 40.2], [2.3, 50.7], [55.4, 47.3], [88.6, 21.1], [22.1, 78.5], [80.3, 75.6], [self.oneband_x, 50.2]])
        self.typ = np.array([0, 0, 1, 1, 2, 2, 0], dtype=np.int32)
        self.shape = np.zeros((S, 4))
        self.shape[C_BIG] = [0.5, 3.0, 30.0, 0.6]
        self.shape[C_FLOOR] = [0.4, 0.02, 40.0, 0.7]           # below k_prep's floor 1/30
        self.shape[C_T2] = [0.35, 1.2, 0.3, 0.9]               # theta, W00, W01, W11
        self.shape[C_SHARP] = [0.5, 1e-6, 0.0, 1e-6]
        self.counts = np.array([[800.0, 1200.0], [6000.0, 9000.0], [40000.0, 50000.0], [7000.0, 5000.0], [15000.0, 11000.0],
                                [9000.0, 8000.0], [4e5, 5e5]])
        self.radec = synth.pixel2equa(self.bands[0], pix)
        ups = self.bands[0][28:32]
        self.pix_deg = math.sqrt(abs(ups[0] * ups[3] - ups[1] * ups[2]))
        self.cat = cel.SourceSet(self.ctx, S, B).set(self.typ, self.radec, self.counts, self.shape)
        self.iset.render(self.cat)
        self.nelec = np.random.RandomState(5).poisson(self.iset.model_images()).astype(np.float64)
        self.iset.set_nelec(self.nelec)
        self.split(self.iset, self.cat)
        self.sums = self.iset.sample_sums()
        self.has_patch = (self.iset.sample_box_areas() > 0).astype(np.float64)
        assert self.has_patch[C_ONEBAND, self.band_with] == 1 and self.has_patch[C_ONEBAND, self.band_without] == 0
        assert np.all(self.has_patch[:C_ONEBAND] == 1) and self.sums[C_ONEBAND, self.band_with] > 0
        self.wsum = np.array([(self.bands[b][3] + self.bands[b][4]) + self.bands[b][5] for b in range(B)])
        # the proposals
        rs = np.random.RandomState(8)
        self.owner = np.array([C_STAR, C_EDGE, C_BIG, C_FLOOR, C_T2, C_SHARP, C_ONEBAND, C_ONEBAND, C_ONEBAND, C_STAR, C_STAR], dtype=np.int32)
        self.ptyp = self.typ[self.owner].copy()
        self.pradec = self.radec[self.owner] + rs.normal(0, 0.05 * self.pix_deg, (P, 2))
        self.pradec[P_ONEBAND] = self.radec[C_ONEBAND]
        self.pradec[P_MISS] = synth.pixel2equa(self.bands[0], np.array([[-60.0, 50.0]]))[0]
        self.pradec[P_INWARD] = synth.pixel2equa(self.bands[0], np.array([[self.oneband_x + 3.0, 50.2]]))[0]
        self.pradec[P_UNCOVERED] = synth.pixel2equa(self.bands[0], np.array([[31.3 + 9.0, 40.2 - 7.0]]))[0]
        self.pshape = self.shape[self.owner].copy()
        self.pshape[P_BIG] = [0.52, 3.1, 31.0, 0.58]
        self.pshape[P_T2] = [0.36, 1.25, 0.28, 0.88]
        self.pcounts = self.counts[self.owner] * rs.uniform(0.9, 1.1, (P, B))
        self.prop = cel.SourceSet(self.ctx, P, B).set(self.ptyp, self.pradec, self.pcounts, self.pshape)
        self.pboxes, self.pstatus = self.iset.source_boxes(self.prop)        # (B, P, 4) = y0, y1, x0, x1; (B, P)
        self.rects = self.iset.photon_rects()
        bx = self.pboxes[:, P_BIG]
        assert np.all(bx[:, 1] - bx[:, 0] > 64) and np.all(bx[:, 3] - bx[:, 2] > 64), bx   # several 32 x 64 chunks, and rows dealt to four parts
        assert np.all(self.pstatus[:, P_MISS] == -1) and np.all(self.pstatus[:, P_INWARD] > 0)
        assert self.pstatus[self.band_without, P_ONEBAND] <= 0 < self.pstatus[self.band_with, P_ONEBAND]
        eb = self.pboxes[0, P_EDGE]
        assert eb[2] == 0 and eb[3] - eb[2] < 2 * (eb[3] - 2)                                # the frame's edge cuts the box

    def split(self, iset, cat):
        was = self.ctx.get_option(self.L.CEL_OPT_SPLIT_FULL_BOX)
        self.ctx.set_option(self.L.CEL_OPT_SPLIT_FULL_BOX, 1)
        try:
            iset.photon_split_resident(cat, seed=9)
        finally:
            self.ctx.set_option(self.L.CEL_OPT_SPLIT_FULL_BOX, was)

    def covered(self, p):
        """k_sg_cover's rule on the host, from public calls"""
        ok = True
        for b in range(B):
            r = self.rects[self.owner[p], b]
            if not (r[1] > r[0] and r[3] > r[2]):
                continue
            q = self.pboxes[b, p]
            ok = ok and self.pstatus[b, p] > 0 and q[0] <= r[0] and q[1] >= r[1] and q[2] <= r[2] and q[3] >= r[3]
        return bool(ok)

    def rows(self, conditional, prop=None, owner=None):
        res = self.iset.patch_loglik_resident_grad(self.prop if prop is None else prop, self.owner if owner is None else owner,
                                                   conditional=conditional)
        return res      # ll[P], g_radec[P,2], g_counts[P,B], g_shape[P,4]

    def one_band(self, b):
        """the proposals with the counts of every band but b set to 0"""
        c = np.zeros((P, B))
        c[:, b] = self.pcounts[:, b]
        return self.cel.SourceSet(self.ctx, P, B).set(self.ptyp, self.pradec, c, self.pshape), c


@pytest.fixture(scope="module")
def scene(cel):
    return Scene(cel)


def _six(res):
    return np.column_stack([res[1], res[3]])


@pytest.fixture(scope="module")
def dmass(scene):
    """per band b: (d mass_b / d q read off the rows, (P, 6); the rows under 0 and 1) with band b's counts alone non-zero:
    (row under 1 - row under 0) = ge = -(counts_b d mass_b / d q) has_patch_b"""
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
    """the derivative stamps of every proposal on its own box, per band (computed once)"""
    return [scene.iset.stamp_jacobians(scene.prop, b, scaled=False)[0] for b in range(B)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_identity_with_the_derivative_stamps(scene, dmass, jac):
    """d mass_b / d q_i = math.fsum of plane i of cel_render_stamps(scaled = 2) over the proposal's own box; bar 1e-10 x sum |plane|
    (tests/test_patch_grad.py's bar for the same identity).  The rows carry g_ref + ge, so reading ge back costs one rounding of
    g_ref, which is counts_b sum r plane with r = z / m: of the bar's own scale x 1e-16 where r is of order one, more where a
    photon sits far out in a small plane.  Worst measured ratio: 7.4e-12 (the sharp type-2 source's theta plane, sum |plane| =
    2.7e-7; every other entry below 2e-15)."""
    worst, seen = 0.0, 0
    for b in range(B):
        d = dmass[b][0]
        for p in COVERED:
            if scene.has_patch[scene.owner[p], b] == 0:
                continue
            pl = jac[b][p]
            assert pl is not None, (NAMES[p], b)
            for i in range(1, pl.shape[0]):
                want, mag = math.fsum(pl[i].ravel()), math.fsum(np.abs(pl[i]).ravel())
                diff = abs(d[p, i - 1] - want)
                print("IDENTITY band %d %-28s plane %d: rows %.17g stamps %.17g sum|plane| %.6g ratio %.3g"
                      % (b, NAMES[p], i, d[p, i - 1], want, mag, diff / mag if mag > 0 else 0.0))
                assert diff <= 1e-10 * mag, (b, NAMES[p], i, d[p, i - 1], want, mag)
                if mag > 0:
                    worst = max(worst, diff / mag)
                seen += 1
            if pl.shape[0] == 3:
                assert np.all(d[p, 2:] == 0.0)                  # a star's shape entries are zeros
    assert seen >= 40
    assert dmass[0][0][P_FLOOR, 3] == 0.0 and dmass[0][0][P_FLOOR, 4] != 0.0       # 0 on sigma under the floor, not on phi
    print("identity with the derivative stamps: worst |difference| / sum |plane| = %.3g" % worst)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_against_mode_10_on_zero_data(scene, dmass, jac):
    """device against device: the explicit mode 10 with all-zero data on the proposals' own boxes returns -counts d mass / d q
    (r = -1 wherever m > 0); the same bar"""
    boxes = np.ascontiguousarray(scene.pboxes.transpose(1, 0, 2))              # (P, B, 4): one patch set per proposal
    boxes = np.where((scene.pstatus.T > 0)[:, :, None], boxes, 0).astype(np.int32)
    patches = [[None if boxes[p, b, 1] <= boxes[p, b, 0] else np.zeros((boxes[p, b, 1] - boxes[p, b, 0], boxes[p, b, 3] - boxes[p, b, 2]))
                for b in range(B)] for p in range(P)]
    worst = 0.0
    for b in range(B):
        prop, c = scene.one_band(b)
        ref = _six(scene.iset.patch_loglik_multi_grad(prop, np.arange(P, dtype=np.int32), boxes, patches, mode=2))
        d = dmass[b][0]
        for p in COVERED:
            if scene.has_patch[scene.owner[p], b] == 0 or jac[b][p] is None:
                continue
            for i in range(jac[b][p].shape[0] - 1):
                mag = math.fsum(np.abs(jac[b][p][i + 1]).ravel())
                diff = abs(d[p, i] - ref[p, i] / -c[p, b])
                assert diff <= 1e-10 * mag, (b, NAMES[p], i, d[p, i], ref[p, i] / -c[p, b], mag)
                if mag > 0:
                    worst = max(worst, diff / mag)
    print("against mode 10 on zero data: worst |difference| / sum |plane| = %.3g" % worst)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_row_definition(scene, dmass):
    sc = scene
    r0, r1 = sc.rows("reference"), sc.rows("exact")
    mass = sc.iset.stamp_mass(sc.prop)
    cov = np.array([sc.covered(p) for p in range(P)])
    assert list(np.nonzero(~cov)[0]) == [P_MISS, P_UNCOVERED]
    assert np.array_equal(r0[0], sc.iset.patch_loglik_resident(sc.prop, sc.owner))
    for p in range(P):
        hp = sc.has_patch[sc.owner[p]]
        if not cov[p]:                                           # -inf and zeros
            assert r1[0][p] == -np.inf and np.all(r1[1][p] == 0.0) and np.all(r1[2][p] == 0.0) and np.all(r1[3][p] == 0.0), NAMES[p]
            continue
        # slot 0: v_ref + e, e in band order from 0.0
        acc = 0.0
        for b in range(B):
            acc = acc + (float(sc.pcounts[p, b]) * (float(mass[p, b]) - float(sc.wsum[b]))) * float(hp[b])
        assert r1[0][p] == float(r0[0][p]) + (-acc), (NAMES[p], r1[0][p], r0[0][p], acc)
        # the counts slots
        for b in range(B):
            assert r1[2][p, b] == float(r0[2][p, b]) + (-(float(mass[p, b]) - float(sc.wsum[b])) * float(hp[b])), (NAMES[p], b)
        # slots 1-6: the bands' one-band ge add up (band order) to the row's ge, to rounding of the row's own entries
        ge = _six(r1)[p] - _six(r0)[p]
        parts = sum(_six(dmass[b][2])[p] - _six(dmass[b][1])[p] for b in range(B))
        scale = np.abs(_six(r0)[p]) + np.abs(_six(r1)[p]) + sum(np.abs(_six(dmass[b][1])[p]) + np.abs(_six(dmass[b][2])[p]) for b in range(B))
        assert np.all(np.abs(ge - parts) <= 8 * np.spacing(scale)), (NAMES[p], ge, parts)
    # has_patch = 0 adds exactly nothing: the inward proposal has a stamp (and a mass) in the band where its source has no patch
    b0 = sc.band_without
    assert mass[P_INWARD, b0] > 0.0 and r1[2][P_INWARD, b0] == r0[2][P_INWARD, b0] == 0.0
    d = dmass[b0]
    assert np.array_equal(_six(d[2])[P_INWARD], _six(d[1])[P_INWARD]) and np.array_equal(_six(d[2])[P_ONEBAND], _six(d[1])[P_ONEBAND])
    assert d[2][0][P_INWARD] == d[1][0][P_INWARD]
    # the exact term moves the gradient where the box cuts the stamp: the edge star's, and the big galaxy's shape
    assert np.any(_six(r1)[P_EDGE] != _six(r0)[P_EDGE]) and np.any(r1[3][P_BIG] != r0[3][P_BIG])


@gpu
def test_slot_0_is_location_loglik(cel, scene):
    """ModelGibbs(conditional="exact").location_loglik against slot 0 of the exact row, and location_loglik_grad under
    hmc_conditional="exact" against the row -- bit for bit; hmc_conditional=None keeps raising"""
    from desi_mcmc_amd import celeste_mcmc
    sc = scene
    sel = [C_STAR, C_EDGE, C_BIG, C_FLOOR, C_ONEBAND]            # (ModelGibbs' catalogue: stars and type-1 galaxies)
    imgs = cel.ImageSet(sc.ctx, sc.bands, H, W)
    imgs.set_nelec(sc.nelec)
    flux5 = np.full((len(sel), 5), 3.0)
    flux5[:, :B] = sc.counts[sel] * sc.bands[None, :, 2] / sc.bands[None, :, 1]
    gf = celeste_mcmc.GibbsField(imgs, list(range(B)), sc.bands[:, 2], sc.bands[:, 1], H * W)
    g = celeste_mcmc.ModelGibbs([gf], sc.typ[sel], sc.radec[sel], flux5, sc.shape[sel], seed=5, conditional="exact", hmc_conditional="exact")
    g.resample_photons()
    idx = np.array([0, 1, 2, 3, 4, 0, 4], dtype=np.int64)
    U = g.u[idx] + np.random.RandomState(3).normal(0, 0.05 * sc.pix_deg, (len(idx), 2))
    U[5] = U[5] + np.array([9.0, -7.0]) * sc.pix_deg            # uncovered
    U[6] = U[6] + np.array([-40.0, 0.0]) * sc.pix_deg           # far beside the frame: an overlap-test miss
    ll = g.location_loglik(idx, U)
    row = gf.iset.patch_loglik_resident_grad(gf.prop, idx.astype(np.int32), conditional="exact")
    assert np.array_equal(ll, row[0]), (ll, row[0])
    assert np.all(np.isfinite(ll[:5])) and ll[5] == -np.inf
    l2, g6 = g.location_loglik_grad(idx, U, shape_grad=True)
    assert np.array_equal(l2, ll) and np.array_equal(g6, _six(row)) and np.all(g6[5] == 0.0)
    plain = celeste_mcmc.ModelGibbs([gf], sc.typ[sel], sc.radec[sel], flux5, sc.shape[sel], seed=5, conditional="exact")
    with pytest.raises(ValueError, match="no analytic derivative"):
        plain.location_loglik_grad(idx, U)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_key_0_bits_repeatability_and_kernel_settings(cel, scene):
    sc, L = scene, scene.L
    assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 0
    r0, r1 = sc.rows("reference"), sc.rows("exact")
    # a context that never heard of the key: the same rows under 0
    ctx2 = cel.Context(0)
    iset2 = cel.ImageSet(ctx2, sc.bands, H, W)
    iset2.set_nelec(sc.nelec)
    cat2 = cel.SourceSet(ctx2, S, B).set(sc.typ, sc.radec, sc.counts, sc.shape)
    ctx2.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    iset2.photon_split_resident(cat2, seed=9)
    ctx2.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
    prop2 = cel.SourceSet(ctx2, P, B).set(sc.ptyp, sc.pradec, sc.pcounts, sc.pshape)
    out = np.zeros(P * (7 + B))
    L.check(L.lib().cel_patch_loglik_multi(iset2._h, prop2._h, sc.owner.ctypes.data_as(L.c_int32_p), S, None, None, None, L.CEL_DEVICE, 8, L.dptr(out)))
    fresh = out.reshape(P, 7 + B)
    assert np.array_equal(fresh[:, 0], r0[0]) and np.array_equal(fresh[:, 1:3], r0[1]) and np.array_equal(fresh[:, 3:7], r0[3])
    assert np.array_equal(fresh[:, 7:], r0[2])
    # modes 9 and 0 do not read the key
    o9, o9b = np.zeros(P * (7 + B)), np.zeros(P * (7 + B))
    sc.ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, 1)            # (the raw key: the mirror would set it itself)
    try:
        L.check(L.lib().cel_patch_loglik_multi(sc.iset._h, sc.prop._h, sc.owner.ctypes.data_as(L.c_int32_p), S, None, None, None, L.CEL_DEVICE, 9, L.dptr(o9)))
        assert np.array_equal(sc.iset.patch_loglik_resident(sc.prop, sc.owner), r0[0])
    finally:
        sc.ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, 0)
    L.check(L.lib().cel_patch_loglik_multi(sc.iset._h, sc.prop._h, sc.owner.ctypes.data_as(L.c_int32_p), S, None, None, None, L.CEL_DEVICE, 9, L.dptr(o9b)))
    assert np.array_equal(o9, o9b)
    # repeated calls and both kernel settings: slots 1.. the same bits (slot 0 carries the value kernels' drop rule)
    before = sc.ctx.get_option(L.CEL_OPT_KERNEL)
    try:
        for kern in ("direct", "recurrence", "recurrence"):
            sc.ctx.set_kernel(kern)
            again = sc.rows("exact")
            for a, b in zip(again[1:], r1[1:]):
                assert np.array_equal(a, b), kern
            assert np.array_equal(np.isinf(again[0]), np.isinf(r1[0]))
    finally:
        sc.ctx.set_option(L.CEL_OPT_KERNEL, before)
    assert np.array_equal(sc.rows("exact")[0], r1[0])
    assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 0    # the mirror restored the caller's value


@gpu
def test_photon_route_takes_the_same_exact_term(scene):
    """under CEL_OPT_PHOTON_LISTS + 4 the reference part is summed at the photon lists; ge is added to it just the same"""
    sc, L = scene, scene.L
    was = sc.ctx.get_option(L.CEL_OPT_PHOTON_LISTS)
    r0d, r1d = sc.rows("reference"), sc.rows("exact")
    try:
        sc.ctx.set_option(L.CEL_OPT_PHOTON_LISTS, was + 4)
        r0, r1 = sc.rows("reference"), sc.rows("exact")
    finally:
        sc.ctx.set_option(L.CEL_OPT_PHOTON_LISTS, was)
    assert np.array_equal(r1[0], r1d[0])
    for f in (_six, lambda r: r[2]):                             # slots 1-6, then the counts slots
        a, b = f(r1) - f(r0), f(r1d) - f(r0d)
        scale = np.abs(f(r0)) + np.abs(f(r1))
        assert np.all(np.abs(a - b) <= 4 * np.spacing(scale))
    assert np.all(_six(r1)[P_UNCOVERED] == 0.0) and r1[0][P_UNCOVERED] == -np.inf


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_sentinel_and_the_option(cel, scene):
    sc, L = scene, scene.L
    n = P * (7 + B)
    sent = np.full(n + 3, -7.25)

    def raw(iset, prop, owner, NB):
        return L.lib().cel_patch_loglik_multi(iset._h, prop._h, owner.ctypes.data_as(L.c_int32_p), NB, None, None, None, L.CEL_DEVICE, 8, L.dptr(sent))

    def refused(rc, word):
        assert rc == L.CEL_ERR_INVALID and np.all(sent == -7.25)
        assert word in L.lib().cel_last_error().decode("utf-8", "replace")

    # the value 2 (and anything else): refused, the stored value unchanged
    for start in (0.0, 1.0):
        sc.ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, start)
        for bad in (2.0, -1.0, 0.5, float("nan")):
            assert L.lib().cel_ctx_set_option(sc.ctx._h, L.CEL_OPT_GRAD_CONDITIONAL, bad) == L.CEL_ERR_INVALID
            assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == start
    sc.ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, 1)
    try:
        # a masked set (its split is gone with the new pixels: the mask is named first)
        ne = sc.nelec.copy()
        ne[0, 5, 5] = np.nan
        masked = cel.ImageSet(sc.ctx, sc.bands, H, W)
        masked.set_nelec(ne)
        refused(raw(masked, sc.prop, sc.owner, S), "mask")
        # no resident split of this catalogue
        bare = cel.ImageSet(sc.ctx, sc.bands, H, W)
        bare.set_nelec(sc.nelec)
        refused(raw(bare, sc.prop, sc.owner, S), "resident photon split")
        refused(raw(sc.iset, sc.prop, np.minimum(sc.owner, S - 2).astype(np.int32), S - 1), "resident photon split")
        # a row window (with a split of its own)
        win = cel.ImageSet(sc.ctx, sc.bands, 64, W)
        win.set_window(16, H)
        win.set_nelec(np.ascontiguousarray(sc.nelec[:, 16:80, :]))
        sc.split(win, sc.cat)
        refused(raw(win, sc.prop, sc.owner, S), "row window")
        assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 1
        # ... and the call itself works under the raw key
        assert raw(sc.iset, sc.prop, sc.owner, S) == L.CEL_OK and np.all(sent[n:] == -7.25)
        assert np.array_equal(sent[:n].reshape(P, 7 + B)[:, 0], sc.rows("exact")[0])
        assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 1            # the mirror restored the caller's 1
    finally:
        sc.ctx.set_option(L.CEL_OPT_GRAD_CONDITIONAL, 0)
    # the mirror restores the option when the call fails
    with pytest.raises(ValueError):
        bare.patch_loglik_resident_grad(sc.prop, sc.owner, conditional="exact")
    assert sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 0
    with pytest.raises(ValueError):
        sc.iset.patch_loglik_resident_grad(sc.prop, sc.owner, conditional="both")
    with pytest.raises(ValueError):
        sc.iset.patch_loglik_resident_grad(sc.prop, sc.owner, isolated=True, conditional="exact")
