"""Every WCS-consuming kernel under a rotated, sheared, per-band WCS with CRPIX off the frame (tests/_general_wcs.py).

CPU (unmarked):
  1. the oracle against tests/golden/general_wcs.npz -- the reference's own run under this WCS -- at test_oracle.py's tolerances
  2. the host mirror (FitsImage, gen_galaxy_transformation) against the same fixture
  3. resolving power: five ablations of the yardstick's WCS arithmetic each move an expected value of a GPU assertion below by
     at least 100 times the tolerance it is compared at

GPU (marked), at the tolerances of the diagonal-WCS tests they restate:
  a. k_prep: boxes and status exact, star and galaxy stamps (RT_STAMP), the 14-source field (RT_LAM, RT_LL; both kernels, T = 0
     and the default)
  b. star-only kernels: CEL_OPT_STAR_TILES 1 (k_small_stars), 2 (k_render_stars) and the general kernel against the oracle
  c. k_grad_chain: test_loglik_grad.py's restatement (1e-8) and central differences (1e-6) on its scene under this WCS
  d. k_stamp_jac: test_stamp_jacobians.py's Richardson differences (1e-7) and its identity with cel_loglik_grad (1e-10)
  e. k_patch_grad_chain: test_patch_grad.py's identity (1e-10) and Richardson differences of the oracle's value (1e-6), modes 8-10
  f. row strips tile the frame (test_hip_parity.py's body and bounds)
  g. the device slice samplers: test_slice_sample_contract.py's scene A under this WCS, cel_slice_locations and one set each of
     cel_slice_sample's locations and shapes, chain by chain against the oracle's slicesample on the device's own scorer

Measured resolving power (part 3; |expected with the fault - expected| / tolerance, the largest entry of the named assertion;
test_ablations_are_visible prints them):
    (i)   ups_inv transposed            1.15e11   star stamps against the fixture (test a, RT_STAMP 1e-10)
    (ii)  band 0's WCS for every band   1.2e11    star stamps against the fixture, bands 1 and 2 (test a, 1e-10)
    (iii) location-through-CD dropped   204       g_radec against the restatement (test c, 1e-8) -- on test c's catalogue with the
                                                  oracle's lambda and Poisson draw in place of the device's; 21 at dec 63.44,
                                                  which is why CRVAL's declination is 87
    (iv)  cos(dec) / cos(phi_1) = 1     7.24e9    galaxy stamps against the fixture (test a, 1e-10)
    (v)   CD's off-diagonals zeroed     3.48e58   galaxy stamps against the fixture (test a, 1e-10)

Result on the device: every test passes at the unchanged tolerances; no device or host fault was found.  Test f: the strips are
the frame's rows within test_row_strips_tile_the_frame's bounds (1e-12 at T = 32, RT_LAM at the default), not bit for bit -- a
window's positions are window-relative, under this WCS as under the diagonal one.
"""
import numpy as np
import pytest

import _general_wcs as gw
from conftest import load_golden, tail_log, unpack_ragged

gpu = pytest.mark.gpu
H, W, NB = gw.FIX_H, gw.FIX_W, gw.FIX_B
RTOL = 1e-10                                               # test_oracle.py's


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def fix(orc):
    g = load_golden("general_wcs.npz")
    assert (int(g["H"]), int(g["W"]), len(g["eps"])) == (H, W, NB)
    return g, orc.pack_bands(g)


def _star_patches(g):
    return unpack_ragged(g["st_flat"], g["st_offs"], g["st_shapes"])


def _gal_patches(g):
    return unpack_ragged(g["ga_flat"], g["ga_offs"], g["ga_shapes"])


def _field_counts(g):
    return g["f_flux"] / g["calib"][None, :] * g["kappa"][None, :]          # celeste.py:80-81, 94


# ---- 1. the oracle against the reference under rotation ----------------------------------------------------------------------
def test_general_bands_are_the_fixtures_records(fix):
    """general_bands(H, W, B) holds the WCS the reference was handed, bit for bit, and synth.make_bands' other fields"""
    from desi_mcmc_amd import synth
    g, B = fix
    mine, plain = gw.general_bands(H, W, NB), synth.make_bands(H, W, NB)
    assert np.array_equal(mine[:, 24:32], B[:, 24:32])
    np.testing.assert_allclose(mine[:, 32:36], B[:, 32:36], rtol=1e-14)
    assert np.array_equal(mine[:, :24], plain[:, :24]) and np.array_equal(mine[:, 36], plain[:, 36])
    np.testing.assert_allclose(mine[:, :24], B[:, :24], rtol=1e-15)
    for b in range(NB):
        ups = B[b, 28:32].reshape(2, 2)
        assert np.all(np.abs(ups) > 2e-5) and np.linalg.det(ups) < 0          # no zero entry; a parity flip
        assert np.any(B[b, 24:26] < 0) or B[b, 25] > H                         # CRPIX off the frame
    assert len({tuple(B[b, 24:36]) for b in range(NB)}) == NB                 # no two bands share a WCS


def test_oracle_wcs_under_rotation(fix, orc):
    g, B = fix
    for b in range(NB):
        for p, e, pb, cd in zip(g["w_pix"], g["w_equa"][b], g["w_pix_back"][b], g["w_cd"][b]):
            np.testing.assert_allclose(orc.pixel2equa(B[b], p), e, rtol=1e-15)
            np.testing.assert_allclose(orc.equa2pixel(B[b], e), pb, rtol=1e-12, atol=1e-10)
            np.testing.assert_allclose(orc.cd_at_pixel(B[b], p[0], p[1]), cd, rtol=1e-9, atol=1e-18)
        for p, row in zip(g["t_pix"], g["t_tinv"][b]):
            cd = orc.cd_at_pixel(B[b], p[0], p[1])
            for th, tinv in zip(g["t_shapes"], row):
                np.testing.assert_allclose(orc.galaxy_tinv(th[1], th[3], th[2], cd), tinv, rtol=1e-9)
    # the samples see what a diagonal WCS hides: cos(dec) / cos(phi_1) off 1 by more than 1e-4 somewhere, off-diagonals of CD
    r = g["w_cd"][0][:, 0, 0] / g["ups"][0][0, 0]
    assert np.max(np.abs(r - 1.0)) > 1e-4 and np.all(np.abs(g["w_cd"][:, :, 0, 1]) > 2e-5)


def test_oracle_star_stamps_under_rotation(fix, orc):
    g, B = fix
    patches, st = _star_patches(g), int(g["st_stride"])
    seen = {"none": 0, "empty": 0, "cut": 0, "whole": 0}
    for i, (b, si, none, box) in enumerate(zip(g["st_band"], g["st_idx"], g["st_none"], g["st_box"])):
        u = g["s_u"][si]
        patch, yl, xl = orc.source_patch(B[b], H, W, 0, u)
        ok, v, obox = orc.star_box(B[b], H, W, u)
        if none:
            seen["none"] += 1
            assert not ok and patch is None
            continue
        assert ok
        assert (yl[0], yl[1], xl[0], xl[1]) == tuple(int(t) for t in box), (i, box)
        if patches[i].size == 0:
            seen["empty"] += 1
            assert patch is None
            continue
        seen["cut" if (box[0] == 0 or box[2] == 0 or box[1] == H or box[3] == W) else "whole"] += 1
        np.testing.assert_allclose(patch[::st, ::st], patches[i], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(patch.sum(), g["st_sum"][i], rtol=RTOL)
    assert all(v > 0 for v in seen.values()), seen
    # one star lies on different sides of the overlap test in different bands: only its own band's WCS says which
    per_star = g["st_none"].reshape(NB, -1)
    assert np.any(per_star.min(axis=0) != per_star.max(axis=0))


def test_oracle_galaxy_stamps_under_rotation(fix, orc):
    g, B = fix
    patches, st = _gal_patches(g), int(g["ga_stride"])
    for i, (b, gi) in enumerate(zip(g["ga_band"], g["ga_idx"])):
        th, u = g["g_th"][gi], g["g_u"][gi]
        _, _, _, pxy, tinv = orc.galaxy_table(B[b], th, u)
        np.testing.assert_allclose(pxy, g["ga_pxy"][i], rtol=1e-12)
        np.testing.assert_allclose(tinv, g["ga_tinv"][i], rtol=1e-9)
        patch, yl, xl = orc.source_patch(B[b], H, W, 1, u, th)
        assert (yl[0], yl[1], xl[0], xl[1]) == tuple(int(t) for t in g["ga_box"][i]), (i, g["ga_box"][i])
        np.testing.assert_allclose(patch.sum(), g["ga_sum"][i], rtol=1e-10)
        np.testing.assert_allclose(patch[::st, ::st], patches[i], rtol=RTOL, atol=1e-300)
    assert g["g_th"][3, 1] < 1.0 / 30 and g["g_th"][4, 3] < 0.2               # the floored and the thin galaxy are there


def test_oracle_mixed_field_under_rotation(fix, orc):
    g, B = fix
    st = int(g["f_stride"])
    counts, nelec = _field_counts(g), g["f_nelec"].astype(np.float64)
    lam, ll, _ = orc.render_field(B, H, W, g["f_is_gal"], g["f_radec"], counts, g["f_shape"], nelec)
    np.testing.assert_allclose(lam[:, ::st, ::st], g["f_lam"], rtol=RTOL)
    np.testing.assert_allclose(ll, g["f_ll_band"], rtol=1e-12)
    for b in range(NB):
        for s in range(len(counts)):
            _, yl, xl = orc.source_patch(B[b], H, W, g["f_is_gal"][s], g["f_radec"][s], g["f_shape"][s])
            assert (yl[0], yl[1], xl[0], xl[1]) == tuple(g["f_box"][b, s]), (b, s)
    stars = g["f_is_gal"] == 0
    n = int(stars.sum())
    lam, ll, _ = orc.render_field(B, H, W, np.zeros(n, np.int32), g["f_radec"][stars], counts[stars], np.zeros((n, 4)), nelec)
    np.testing.assert_allclose(lam[:, ::st, ::st], g["f_star_lam"], rtol=RTOL)
    np.testing.assert_allclose(ll, g["f_star_ll"], rtol=1e-12)


# ---- 2. the host mirror ---------------------------------------------------------------------------------------------------------
def _fits_images(g, nelec=None):
    from desi_mcmc_amd.fits_image import FitsImage
    return [FitsImage.from_record("ugriz"[b], g, b, np.zeros((H, W)) if nelec is None else nelec[b]) for b in range(NB)]


def test_host_mirror_under_rotation(fix):
    from desi_mcmc_amd import celeste_galaxy_conditionals as gal
    g, B = fix
    for b, im in enumerate(_fits_images(g)):
        np.testing.assert_allclose(im.R, g["R"][b], rtol=1e-13)
        np.testing.assert_allclose(im.Ups_n_inv, g["ups_inv"][b], rtol=1e-14)
        np.testing.assert_allclose(im.band_record(), B[b], rtol=1e-13)
        for p, e, pb, cd in zip(g["w_pix"], g["w_equa"][b], g["w_pix_back"][b], g["w_cd"][b]):
            np.testing.assert_allclose(im.pixel2equa(p), e, rtol=1e-15)
            np.testing.assert_allclose(im.equa2pixel(e), pb, rtol=1e-12, atol=1e-10)
            np.testing.assert_allclose(im.cd_at_pixel(p[0], p[1]), cd, rtol=1e-9, atol=1e-18)
        for p, row in zip(g["t_pix"], g["t_tinv"][b]):
            for th, tinv in zip(g["t_shapes"], row):
                np.testing.assert_allclose(gal.gen_galaxy_transformation(th[1], th[3], th[2], im.cd_at_pixel(p[0], p[1])), tinv, rtol=1e-9)
        for i in np.nonzero(g["ga_band"] == b)[0]:
            th, u = g["g_th"][g["ga_idx"][i]], g["g_u"][g["ga_idx"][i]]
            _, _, _, pxy = gal.galaxy_mixture(th, u, im)
            np.testing.assert_allclose(pxy, g["ga_pxy"][i], rtol=1e-12)


# ---- 3. resolving power -----------------------------------------------------------------------------------------------------------
def _stamp_ratio(g, B, orc, kind, ablate, bands_checked=range(NB)):
    """the stamp assertions of test a: for every fixture patch of `kind` ("star" | "galaxy") the yardstick's expected stamp
    with and without the ablation.  -> (worst |plain - fixture| / |fixture|, largest |ablated - plain| / (RT_STAMP |fixture|))"""
    from test_hip_parity import RT_STAMP
    if kind == "star":
        patches, st = _star_patches(g), int(g["st_stride"])
        rows = [(i, int(b), 0, g["s_u"][si], np.zeros(4), g["st_box"][i]) for i, (b, si) in enumerate(zip(g["st_band"], g["st_idx"]))
                if patches[i].size]
    else:
        patches, st = _gal_patches(g), int(g["ga_stride"])
        rows = [(i, int(b), 1, g["g_u"][gi], g["g_th"][gi], g["ga_box"][i]) for i, (b, gi) in enumerate(zip(g["ga_band"], g["ga_idx"]))]
    own, moved = 0.0, 0.0
    for i, b, typ, u, th, box in rows:
        if b not in bands_checked:
            continue
        want = patches[i]
        plain = gw.unit_patch(gw.components(B, b, typ, u, th, orc), box)[::st, ::st]
        abl = gw.unit_patch(gw.components(B, b, typ, u, th, orc, ablate), box)[::st, ::st]
        own = max(own, np.max(np.abs(plain - want) / want))
        moved = max(moved, np.max(np.abs(abl - plain) / (RT_STAMP * want)))
    return own, moved


@pytest.fixture(scope="module")
def grad_proxy(orc):
    """test c's catalogue (test_loglik_grad._catalogue on general_bands: the same sources at the same places) with lambda and a
    Poisson draw from the oracle in place of the device's, its two type-2 sources left out: per source and band the box and
    d ll / d (px, py, W00, W01, W11) from test_loglik_grad's seven sums"""
    import test_loglik_grad as tlg
    bands = gw.general_bands(tlg.H, tlg.W, tlg.B)
    ob = bands.copy()
    ob[:, 36] = [orc.band_radius(ob[b]) for b in range(tlg.B)]
    cat, rs = tlg._catalogue(bands)
    keep = np.nonzero(cat["typ"] != 2)[0]
    typ, radec, counts, shape = cat["typ"][keep], cat["radec"][keep], cat["counts"][keep], cat["shape"][keep]
    S = len(keep)
    from desi_mcmc_amd import synth
    radec_t = synth.pixel2equa(bands[0], cat["pix"] + rs.normal(0, 0.3, (len(cat["typ"]), 2)))[keep]
    counts_t = (cat["counts"] * rs.uniform(0.95, 1.05, cat["counts"].shape))[keep]
    lam_t, _, _ = orc.render_field(ob, tlg.H, tlg.W, typ, radec_t, counts_t, shape)
    nelec = rs.poisson(lam_t).astype(np.float64)
    lam, _, _ = orc.render_field(ob, tlg.H, tlg.W, typ, radec, counts, shape)
    r = nelec / lam - 1.0
    dv = np.zeros((S, tlg.B, 5))
    for s in range(S):
        for b in range(tlg.B):
            patch, yl, xl = orc.source_patch(ob[b], tlg.H, tlg.W, typ[s], radec[s], shape[s])
            if patch is None:
                continue
            bx = (yl[0], yl[1], xl[0], xl[1])
            q = tlg._seven(gw.components(ob, b, typ[s], radec[s], shape[s], orc), bx, r[b, bx[0]:bx[1], bx[2]:bx[3]])
            dv[s, b] = counts[s, b] * np.array([q[1], q[2], q[3], 2.0 * q[4], q[5]])
    return dict(tlg=tlg, ob=ob, typ=typ, radec=radec, shape=shape, dv=dv, S=S)


def _g_radec(p, orc, ablate=(), oracle_map=False):
    """g_radec of the proxy scene: sum over bands of J dv, J from the switched yardstick (or, oracle_map, from the oracle's own
    parameter map as test_loglik_grad._restated_grad takes it)"""
    tlg = p["tlg"]
    g = np.zeros((p["S"], 2))
    for s in range(p["S"]):
        for b in range(tlg.B):
            if oracle_map:
                J = np.zeros((2, 5))
                for i in range(2):
                    e = np.zeros(2); e[i] = 1e-6
                    J[i] = (tlg._param_map(p["ob"][b], p["typ"][s], p["radec"][s] + e, p["shape"][s], orc) -
                            tlg._param_map(p["ob"][b], p["typ"][s], p["radec"][s] - e, p["shape"][s], orc)) / 2e-6
            else:
                J = gw.param_jacobian(p["ob"], b, p["typ"][s], p["radec"][s], p["shape"][s], orc, ablate)
            g[s] += J @ p["dv"][s, b]
    return g


def _close_ratio(abl, plain, rtol):
    """test_loglik_grad._close's bar per entry: max(rtol |want|, rtol max |column|); -> the largest |abl - plain| / bar"""
    bar = np.maximum(rtol * np.abs(plain), rtol * np.max(np.abs(plain), axis=0, keepdims=True))
    return float(np.max(np.abs(abl - plain) / bar))


def test_the_switched_yardstick_is_the_oracle_when_nothing_is_switched(fix, orc, grad_proxy):
    """the numpy copy that carries the switches is a copy: its stamps are the fixture's at RT_STAMP, its parameter map is the
    oracle's, and its g_radec is the one test_loglik_grad's own restatement forms"""
    from test_hip_parity import RT_STAMP
    g, B = fix
    for kind in ("star", "galaxy"):
        own, moved = _stamp_ratio(g, B, orc, kind, ())
        assert own <= RT_STAMP and moved == 0.0, (kind, own)
    for b in range(NB):
        for gi in range(len(g["g_th"])):
            _, _, _, pxy, tinv = orc.galaxy_table(B[b], g["g_th"][gi], g["g_u"][gi])
            Wm = tinv @ tinv.T
            np.testing.assert_allclose(gw.param_map(B, b, 1, g["g_u"][gi], g["g_th"][gi], orc),
                                       [pxy[0], pxy[1], Wm[0, 0], Wm[0, 1], Wm[1, 1]], rtol=1e-12)
    a, o = _g_radec(grad_proxy, orc), _g_radec(grad_proxy, orc, oracle_map=True)
    assert _close_ratio(a, o, 1e-8) <= 0.1


def test_ablations_are_visible(fix, orc, grad_proxy):
    """each fault the GPU tests are for moves an expected value of a named GPU assertion by >= 100 x that assertion's tolerance
    on at least one entry it checks (the measured ratios: this module's docstring)"""
    g, B = fix
    ratios = {}
    # (i), (ii): test a, star stamps against the fixture's patches (RT_STAMP); (ii) shows in bands 1 and 2 only
    ratios["ups_inv_T"] = _stamp_ratio(g, B, orc, "star", ("ups_inv_T",))[1]
    ratios["band0_wcs"] = _stamp_ratio(g, B, orc, "star", ("band0_wcs",), bands_checked=(1, 2))[1]
    assert _stamp_ratio(g, B, orc, "star", ("band0_wcs",), bands_checked=(0,))[1] == 0.0
    # (iii): test c, g_radec against test_loglik_grad's restatement (1e-8 per entry, floor 1e-8 of the column's largest)
    plain = _g_radec(grad_proxy, orc)
    dropped = _g_radec(grad_proxy, orc, ("no_cd_term",))
    gal = grad_proxy["typ"] == 1
    assert np.array_equal(dropped[~gal], plain[~gal])
    ratios["no_cd_term"] = _close_ratio(dropped, plain, 1e-8)
    # (iv), (v): test a, galaxy stamps against the fixture's patches (RT_STAMP)
    ratios["cosd_cphi_1"] = _stamp_ratio(g, B, orc, "galaxy", ("cosd_cphi_1",))[1]
    ratios["cd_diagonal"] = _stamp_ratio(g, B, orc, "galaxy", ("cd_diagonal",))[1]
    print("resolving power, |expected with the fault - expected| / tolerance: " + ", ".join("%s %.3g" % kv for kv in ratios.items()))
    assert set(ratios) == set(gw.ABLATIONS)
    for name, ratio in ratios.items():
        assert ratio >= 100.0, (name, ratio)


# ==== GPU ===========================================================================================================================
@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(cel):
    return cel.Context(0)


def _expected_status(none, size):
    return -1 if none else (1 if size else 0)


# ---- a. k_prep ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_star_boxes_and_stamps_match_the_reference(cel, ctx, fix):
    """cel_stamp_boxes / cel_source_boxes / cel_render_stamps for the fixture's stars: status and boxes exact, stamps at
    test_hip_parity.py's RT_STAMP"""
    from test_hip_parity import RT_STAMP
    g, B = fix
    S = len(g["s_u"])
    patches, st = _star_patches(g), int(g["st_stride"])
    iset = cel.ImageSet(ctx, B, H, W)
    sset = cel.SourceSet(ctx, S, NB).set(np.zeros(S, np.int32), g["s_u"], np.ones((S, NB)), np.zeros((S, 4)))
    all_boxes, all_status = iset.source_boxes(sset)
    for b in range(NB):
        boxes, status = iset.stamp_boxes(sset, b)
        got, boxes2 = iset.stamps(sset, b)
        assert np.array_equal(boxes, all_boxes[b]) and np.array_equal(status, all_status[b]) and np.array_equal(boxes, boxes2)
        for s in range(S):
            i = b * S + s
            assert (g["st_band"][i], g["st_idx"][i]) == (b, s)
            assert status[s] == _expected_status(g["st_none"][i], patches[i].size), (b, s, status[s])
            if status[s] <= 0:
                assert got[s] is None
                continue
            assert tuple(boxes[s]) == tuple(int(t) for t in g["st_box"][i]), (b, s)
            np.testing.assert_allclose(got[s][::st, ::st], patches[i], rtol=RT_STAMP, atol=1e-300)
            np.testing.assert_allclose(got[s].sum(), g["st_sum"][i], rtol=RT_STAMP)


@gpu
def test_galaxy_boxes_and_stamps_match_the_reference(cel, ctx, fix):
    from test_hip_parity import RT_STAMP
    g, B = fix
    S = len(g["g_u"])
    patches, st = _gal_patches(g), int(g["ga_stride"])
    iset = cel.ImageSet(ctx, B, H, W)
    sset = cel.SourceSet(ctx, S, NB).set(np.ones(S, np.int32), g["g_u"], np.ones((S, NB)), g["g_th"])
    all_boxes, all_status = iset.source_boxes(sset)
    for b in range(NB):
        boxes, status = iset.stamp_boxes(sset, b)
        got, _ = iset.stamps(sset, b)
        assert np.array_equal(boxes, all_boxes[b]) and np.array_equal(status, all_status[b])
        for s in range(S):
            i = b * S + s
            assert (g["ga_band"][i], g["ga_idx"][i]) == (b, s) and status[s] == 1
            assert tuple(boxes[s]) == tuple(int(t) for t in g["ga_box"][i]), (b, s)
            np.testing.assert_allclose(got[s].sum(), g["ga_sum"][i], rtol=1e-10)
            np.testing.assert_allclose(got[s][::st, ::st], patches[i], rtol=RT_STAMP, atol=1e-300)


@gpu
@pytest.mark.parametrize("kernel,tail", [("direct", 0.0), ("direct", "default"), ("recurrence", 0.0), ("recurrence", "default")])
def test_mixed_field_matches_the_reference(cel, ctx, fix, kernel, tail):
    """the 14-source field: model image (RT_LAM), per-band log-likelihood (RT_LL), every source's box and status"""
    from test_hip_parity import RT_LAM, RT_LL
    g, B = fix
    st = int(g["f_stride"])
    S = len(g["f_is_gal"])
    ctx.set_kernel(kernel)
    ctx.set_tail_log(tail)
    try:
        iset = cel.ImageSet(ctx, B, H, W, nelec=g["f_nelec"].astype(np.float64))
        sset = cel.SourceSet(ctx, S, NB).set(g["f_is_gal"], g["f_radec"], _field_counts(g), g["f_shape"])
        ll, llb = iset.render(sset, loglik=True)
        np.testing.assert_allclose(iset.model_images()[:, ::st, ::st], g["f_lam"], rtol=RT_LAM)
        np.testing.assert_allclose(llb, g["f_ll_band"], rtol=RT_LL)
        np.testing.assert_allclose(ll, g["f_ll_band"].sum(), rtol=RT_LL)
        boxes, status = iset.source_boxes(sset)
        for b in range(NB):
            for s in range(S):
                y0, y1, x0, x1 = g["f_box"][b, s]
                assert status[b, s] == (1 if (y1 > y0 and x1 > x0) else 0), (b, s)
                if status[b, s] > 0:
                    assert tuple(boxes[b, s]) == (y0, y1, x0, x1), (b, s)
    finally:
        ctx.set_kernel("recurrence")
        ctx.set_tail_log("default")


# ---- b. the star-only kernels ----------------------------------------------------------------------------------------------------
@gpu
def test_star_kernels_agree_with_the_oracle_and_each_other(cel, ctx, fix, orc):
    """the fixture's stars and 40 more through CEL_OPT_STAR_TILES = 1 (k_small_stars: its own prep_pixel / prep_star_box),
    2 (k_render_stars) and 0 (the general kernel): each against the oracle at test_hip_parity.py's star-field tolerances
    (RT_LAM_STRICT, RT_LL), the three sets of boxes and status equal"""
    from test_hip_parity import RT_LAM_STRICT, RT_LL
    L = cel._lib
    g, B = fix
    rs = np.random.RandomState(61)
    more = np.array([orc.pixel2equa(B[0], p) for p in np.column_stack([rs.uniform(-30, W + 30, 40), rs.uniform(-30, H + 30, 40)])])
    radec = np.vstack([g["s_u"], more])
    S = len(radec)
    typ = np.zeros(S, np.int32)
    counts = np.exp(rs.uniform(np.log(50.0), np.log(5e4), size=(S, NB)))
    o_lam, _, _ = orc.render_field(B, H, W, typ, radec, counts, np.zeros((S, 4)))
    nelec = rs.poisson(o_lam).astype(np.float64)
    o_lam, o_ll, o_st = orc.render_field(B, H, W, typ, radec, counts, np.zeros((S, 4)), nelec)
    seen = {}
    try:
        for mode, slot in ((0, "render"), (1, "small_stars"), (2, "render_stars")):
            ctx.set_option(L.CEL_OPT_STAR_TILES, mode)
            iset = cel.ImageSet(ctx, B, H, W, nelec=nelec)
            sset = cel.SourceSet(ctx, S, NB).set(typ, radec, counts)
            ctx.profile(True)
            ll, llb = iset.render(sset, loglik=True)
            ran = {k: ctx.profile_get(k)[1] for k in ("render", "small_stars", "render_stars")}
            ctx.profile(False)
            assert ran == {k: int(k == slot) for k in ran}, (mode, ran)
            np.testing.assert_allclose(iset.model_images(), o_lam, rtol=RT_LAM_STRICT)
            np.testing.assert_allclose(llb, o_ll, rtol=RT_LL)
            assert iset.stats()["n_srcpix"] == o_st["n_srcpix"]
            seen[mode] = iset.source_boxes(sset)
    finally:
        ctx.profile(False)
        ctx.set_option(L.CEL_OPT_STAR_TILES, 1)
    for mode in (1, 2):
        assert np.array_equal(seen[mode][0], seen[0][0]) and np.array_equal(seen[mode][1], seen[0][1]), mode
    assert {-1, 0, 1} <= set(np.unique(seen[0][1]))                 # misses, empty boxes and stamps are all there


# ---- c. k_grad_chain ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grad_scene(cel, ctx):
    import test_loglik_grad as tlg
    return tlg._scene(cel, ctx, bands=gw.general_bands(tlg.H, tlg.W, tlg.B))


@gpu
def test_grad_restatement_under_the_general_wcs(ctx, grad_scene, orc):
    """test_loglik_grad.py's test_grad_matches_numpy_restatement (1e-8) on its scene under the general WCS"""
    import test_loglik_grad as tlg
    assert np.all(grad_scene["typ"][:3] == [1, 2, 2]) and grad_scene["shape"][0, 1] < 1.0 / 30
    tlg.test_grad_matches_numpy_restatement(ctx, grad_scene, orc)


@gpu
def test_grad_central_differences_under_the_general_wcs(ctx, cel, grad_scene, orc):
    """test_loglik_grad.py's test_grad_central_differences (1e-6)"""
    import test_loglik_grad as tlg
    tlg.test_grad_central_differences(ctx, cel, grad_scene, orc)


# ---- d. k_stamp_jac ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jac_scene(cel, ctx):
    import test_stamp_jacobians as sj
    scene = sj._scene(cel, ctx, bands=gw.general_bands(sj.H, sj.W, sj.B))
    return scene, sj._jac(ctx, scene)


@gpu
def test_planes_contract_to_loglik_grad_under_the_general_wcs(jac_scene):
    """k_stamp_jac.h's chain rule against k_grad.h's: test_stamp_jacobians.py's identity (1e-10 sum |r plane|)"""
    import test_stamp_jacobians as sj
    sj.test_planes_contract_to_loglik_grad(*jac_scene)


@gpu
@pytest.mark.parametrize("b", range(3))
def test_planes_against_central_differences_under_the_general_wcs(jac_scene, orc, b):
    """every derivative plane (ra, dec; a galaxy's four shape coordinates) against test_stamp_jacobians.py's Richardson
    differences of the oracle's stamp, its bound 1e-7 max |plane|"""
    import test_stamp_jacobians as sj
    sj.test_planes_against_central_differences(jac_scene[0], jac_scene[1], orc, b)


# ---- e. k_patch_grad_chain ---------------------------------------------------------------------------------------------------------
PG_NAMES = ["star", "edge star", "galaxy", "floored galaxy", "type-2 galaxy", "edge galaxy"]


def _patch_scene(orc):
    """test_patch_grad.py's frame (96 x 112, 2 bands) under the general WCS: four interior proposals -- a star, a type-1 galaxy
    on an 81 x 89 patch, a galaxy under the sigma floor (index 3, as test_patch_grad.py's LEFT_TO_TEST_1 names it), a type-2
    galaxy -- and two cut by the frame's edge, a star on the left and a galaxy on the right; patches imposed per set, z a
    Poisson draw from the proposal's own model (+ eps in mode 1)"""
    import test_patch_grad as tpg
    from desi_mcmc_amd import synth
    bands = gw.general_bands(tpg.H, tpg.W, tpg.B)
    ob = bands.copy()
    ob[:, 36] = [orc.band_radius(bands[b]) for b in range(tpg.B)]
    boxes = np.zeros((4, tpg.B, 4), dtype=np.int32)
    boxes[0] = [[34, 47, 20, 42], [30, 50, 20, 43]]
    boxes[1] = [[7, 88, 11, 100], [7, 88, 11, 100]]
    boxes[2] = [[40, 61, 0, 12], [41, 60, 0, 11]]
    boxes[3] = [[45, 75, 92, 112], [44, 76, 90, 112]]
    pix = np.array([[31.3, 40.2], [2.3, 50.7], [55.4, 47.3], [30.6, 41.1], [32.1, 39.5], [108.0, 60.0]])
    typ = np.array([0, 0, 1, 1, 2, 1], dtype=np.int32)
    shape = np.zeros((6, 4))
    shape[2] = [0.5, 3.0, 30.0, 0.6]
    shape[3] = [0.4, 0.02, 40.0, 0.7]
    shape[4] = [0.35, 1.2, 0.3, 0.9]
    shape[5] = [0.6, 1.0, 120.0, 0.5]
    owner = np.array([0, 2, 1, 0, 0, 3], dtype=np.int32)
    counts = np.array([[8000.0, 12000.0], [6000.0, 9000.0], [40000.0, 50000.0], [7000.0, 5000.0], [15000.0, 11000.0], [9000.0, 14000.0]])
    radec = synth.pixel2equa(bands[0], pix)
    assert tpg.P_FLOOR == 3 and shape[tpg.P_FLOOR, 1] < 1.0 / 30
    rs = np.random.RandomState(11)
    z = {}
    for mode in (0, 1, 2):
        for p in range(6):
            for b in range(tpg.B):
                m = counts[p, b] * tpg._unit(tpg._comps(ob[b], typ[p], radec[p], shape[p], orc), boxes[owner[p], b])
                z[mode, p, b] = rs.poisson(m + (ob[b, 0] if mode == 1 else 0.0)).astype(np.float64)
    return dict(bands=bands, ob=ob, boxes=boxes, typ=typ, shape=shape, owner=owner, counts=counts, radec=radec, z=z, P=6, names=PG_NAMES)


@pytest.fixture(scope="module")
def patch_scene(orc):
    return _patch_scene(orc)


@pytest.fixture(scope="module")
def patch_fd(orc, patch_scene):
    import test_patch_grad as tpg
    return tpg._fd_pairs(orc, patch_scene)


def test_patch_scene_quotients_agree(patch_scene, patch_fd):
    """before any GPU run, as test_patch_grad.py's test_the_yardsticks_own_quotients_agree: the oracle's quotients at h and
    h / 2 agree within a tenth of the 1e-6 bar for every entry compared"""
    import test_patch_grad as tpg
    for mode in (0, 1, 2):
        q1, q2 = patch_fd[mode]
        top = np.max(np.abs((4.0 * q2 - q1) / 3.0), axis=0)
        assert np.all(top > 0)
        for p in range(patch_scene["P"]):
            for col in range(6 + tpg.B):
                if tpg._compared(p, col):
                    assert abs(q1[p, col] - q2[p, col]) <= 1e-7 * top[col], (mode, PG_NAMES[p], tpg.COORDS[col], q1[p, col], q2[p, col])


@pytest.fixture(scope="module")
def patch_dev(cel, ctx, patch_scene):
    import test_patch_grad as tpg
    sc = patch_scene
    iset = cel.ImageSet(ctx, sc["bands"], tpg.H, tpg.W)
    prop = cel.SourceSet(ctx, sc["P"], tpg.B).set(sc["typ"], sc["radec"], sc["counts"], sc["shape"])
    out = {}
    for mode in (0, 1, 2):
        own, boxes, patches = tpg._batch(sc, mode)
        out[mode] = iset.patch_loglik_multi_grad(prop, own, boxes, patches, mode=mode)
    return dict(iset=iset, prop=prop, out=out)


@gpu
def test_patch_grad_identity_under_the_general_wcs(patch_scene, patch_dev):
    """k_patch_grad.h's chain rule against k_stamp_jac.h's planes contracted on the host: test_patch_grad.py's identity, modes
    8, 9 and 10, bar 1e-10 sum |r plane|"""
    import test_patch_grad as tpg
    tpg.test_identity_with_the_derivative_stamps(patch_scene, patch_dev)


@gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_patch_grad_central_differences_under_the_general_wcs(patch_scene, patch_dev, patch_fd, mode):
    """every entry against (4 fd_{h/2} - fd_h) / 3 of the oracle's value as test_patch_grad.py forms it; its bar, 1e-6 x the
    column's largest |entry| over the batch"""
    import test_patch_grad as tpg
    q1, q2 = patch_fd[mode]
    rich = (4.0 * q2 - q1) / 3.0
    got = tpg._flat(patch_dev["out"][mode])
    top = np.max(np.abs(rich), axis=0)
    worst, over = 0.0, []
    for p in range(patch_scene["P"]):
        for col in range(6 + tpg.B):
            if not tpg._compared(p, col):
                continue
            d = abs(got[p, col] - rich[p, col]) / top[col]
            worst = max(worst, d)
            if not d <= 1e-6:
                over.append((PG_NAMES[p], tpg.COORDS[col], got[p, col], rich[p, col], d))
    print("mode %d: worst |entry - fd| / column max = %.3g" % (8 + mode, worst))
    assert not over, over
    stars = patch_scene["typ"] == 0
    assert np.all(got[stars, 2:6] == 0.0) and np.all(got[:, :2] != 0.0)


@gpu
def test_patch_loglik_values_under_the_general_wcs(patch_scene, patch_dev, orc):
    """slot 0 of the same calls, the plain conditional log-likelihoods of the stars and type-1 galaxies (the per-source kernels
    place a source themselves): against the oracle's patch_loglik at test_hip_parity.py's test_fuzz_patch_loglik_vs_oracle bounds"""
    import test_patch_grad as tpg
    from test_hip_parity import RT_LL
    sc = patch_scene
    for mode in (0, 1):
        for p in np.nonzero(sc["typ"] != 2)[0]:
            args = [(sc["ob"][b], tpg.H, tpg.W, sc["typ"][p], sc["radec"][p], sc["shape"][p], sc["counts"][p, b], sc["boxes"][sc["owner"][p], b],
                     sc["z"][mode, p, b]) for b in range(tpg.B)]
            want = sum(orc.patch_loglik(*a, mode) for a in args)
            tol = RT_LL * abs(want)
            if mode == 0:
                t = np.array([orc.patch_loglik_terms(*a) for a in args])
                tol = RT_LL * t[:, 1].sum() + 8 * np.finfo(float).eps * t[:, 2].sum() + t[:, 3].sum()
            got = patch_dev["out"][mode][0][p]
            assert abs(got - want) <= tol, (mode, PG_NAMES[p], got, want, tol)


# ---- f. row strips -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("world,tail", [(2, "default"), (2, "strict"), (3, "default"), (3, "strict")])
def test_row_strips_tile_the_frame_under_the_general_wcs(cel, ctx, fix, world, tail):
    """the 14-source field cut into 2 and 3 row windows (cel_images_set_window): test_hip_parity.py's
    test_row_strips_tile_the_frame body and bounds (1e-12 at T = 32, where only the row origin of the arithmetic moves; RT_LAM
    at the shipping threshold, where a strip that starts off a tile row drops other components)"""
    import types
    from test_hip_parity import RT_LAM, _row_strips_body
    g, B = fix
    S = len(g["f_is_gal"])
    nelec = g["f_nelec"].astype(np.float64)
    f = types.SimpleNamespace(bands=B, nelec=nelec, images=cel.ImageSet(ctx, B, H, W, nelec=nelec),
                              sources=cel.SourceSet(ctx, S, NB).set(g["f_is_gal"], g["f_radec"], _field_counts(g), g["f_shape"]))
    from desi_mcmc_amd import dist
    with tail_log(ctx, tail):
        _row_strips_body(cel, ctx, f, H, W, world, 0.5, 1e-12 if tail == "strict" else RT_LAM)
        lam, same = f.images.model_images(), []
        for r in range(world):                                        # (a figure, not a bound: which strips are the frame's bits)
            y0, y1 = dist.strip_rows(H, world, r)
            strip = cel.ImageSet(ctx, B, y1 - y0, W)
            strip.set_window(y0, H)
            strip.render(f.sources)
            same.append(bool(np.array_equal(strip.model_images(), lam[:, y0:y1])))
    print("world %d, %s: strips bit-equal to the frame's rows: %s" % (world, tail, same))


# ---- g. the slice samplers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slice_scene(cel):
    import test_slice_sample_contract as ssc
    return ssc.Scene(cel, bands=gw.general_bands(128, 128, 3))


@gpu
def test_slice_locations_follow_the_oracle_under_the_general_wcs(slice_scene):
    """cel_slice_locations (k_slice.h places every proposal itself, named in (ra, dec)) on test_slice_sample_contract.py's
    scene A under the general WCS: every chain's `u` and `llh` the oracle's, bit for bit, as test_the_location_engines_agree
    holds them on the diagonal WCS"""
    import test_slice_sample_contract as ssc
    sc = slice_scene
    assert sc.has_patch.sum() >= ssc.S // 2
    seed = ssc.SEEDS[0]
    ids = ssc.chain_ids(seed)
    want = sc.oracle(0, ids, seed, sigma=1e-3, step_out=False)
    sc.reset()
    sc.split()
    sc.check(sc.f.images.slice_locations(sc.f.sources, 1e-3, seed, chain_ids=ids), want, 0, ("slice_locations", seed))
    sc.check(sc.device(0, ids, seed, sigma=1e-3, step_out=False, resplit=True), want, 0, ("slice_sample", seed))


@gpu
@pytest.mark.parametrize("param,name", [(0, "narrow"), (1, "compwise")])
def test_slice_sample_follows_the_oracle_under_the_general_wcs(slice_scene, param, name):
    """cel_slice_sample (k_slice_gen.h): one doubling set of the locations and one of the shapes from
    test_slice_sample_contract.py, one seed, with that module's coverage requirements"""
    import test_slice_sample_contract as ssc
    opts, kinds = (ssc.SHAPE_SETS if param else ssc.LOCATION_SETS)[name]
    ssc.run_sets(slice_scene, param, name, opts, kinds, seeds=ssc.SEEDS[:1])
