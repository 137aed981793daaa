"""The Gibbs sweep on MASKED images (CEL_OPT_HONOUR_MASK, ModelGibbs(mask="honour")).

A NaN count marks a pixel that was not observed.  With the option on
  * the photon split gives such a pixel no photons, no share of the sky sum and no random numbers -- it is, bit for bit, the
    split of the set whose masked counts were replaced by 0 (the fill identity; the Philox streams are keyed by pixel and source);
  * cel_stamp_mass* returns the unit stamp summed over the UNMASKED pixels of a source's own box (k_stamp_mass_masked), checked
    against the oracle's patches and against cel_estep_stats' mass at the suite's 1e-10 stamp tolerance;
  * the flux step runs on those sums and masses, the sky step counts unmasked pixels;
  * ModelGibbs(conditional="exact", mask="honour") is the calibrated sweep (the exact rank statistic of tests/test_calibration.py),
    and fails that calibration by many orders when the masses are the unmasked ones.
With the option off (the default) every call behaves as before.  The frame is frame A of tests/test_masked_pixels.py
(200 x 150, 2 bands, 24 sources) with its mask: a whole column, both sides of every tile seam, the frame corners, a ragged last
tile row and column, one whole 32 x 64 tile, source centres, 1 % of the rest, five half-masked boxes and one box masked everywhere."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, tail_log
from test_masked_pixels import HA, WA, BA, EMPTY_TILE, SPARSE_TILE
from test_masked_pixels import frame_a_catalogue, mask_pattern, sparse_mask, draw_counts, _estep_mask, _fits_images
from test_calibration import chi2_pvalue, K_DRAWS, THIN, FLUX_A, FLUX_B, EPS_A, EPS_B, CELL

gpu = pytest.mark.gpu
SEED = 31


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(cel):
    return cel.Context(0)          # a context of this module's own: the option never leaks into the suite's default context


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def frame(cel, ctx):
    """frame A with the E-step test's mask (five half-masked boxes, source 12's box masked in band 0)"""
    f = frame_a_catalogue()
    f["nelec"] = draw_counts(cel, ctx, f["bands"], HA, WA, f["typ"], f["pix"], f["counts"], f["shape"], 21)
    gal = int(np.nonzero(f["typ"] == 1)[0][4])
    mask = np.zeros((BA, HA, WA), bool)
    mask[0] = mask_pattern(HA, WA, f["pix"][:6], f["pix"][gal], EMPTY_TILE, SPARSE_TILE, 5)
    mask[1] = sparse_mask(HA, WA, 6)
    f["mask"] = mask
    probe = cel.ImageSet(ctx, f["bands"], HA, WA)
    boxes, status = probe.source_boxes(_sources(cel, ctx, f))
    probe.close()
    assert np.all(status > 0)
    f["boxes"] = boxes
    f["mask"], f["half"], f["gone"] = _estep_mask(f)
    return f


def _sources(cel, ctx, f):
    return cel.SourceSet(ctx, f["S"], BA).set(f["typ"], f["radec"], f["counts"], f["shape"])


class _option(object):
    """CEL_OPT_HONOUR_MASK (or another key) set for a block and put back behind it"""

    def __init__(self, ctx, key, value):
        self.ctx, self.key, self.value = ctx, key, value

    def __enter__(self):
        self.was = self.ctx.get_option(self.key)
        self.ctx.set_option(self.key, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.key, self.was)


def _honour(cel, ctx, on=1):
    return _option(ctx, cel._lib.CEL_OPT_HONOUR_MASK, on)


def _resident(cel, ctx, f, iset, seed=SEED):
    """one resident split of the frame's catalogue (after a render of it: the state in which the split's mass short cut applies)
    and everything the sweep reads from it"""
    srcs = _sources(cel, ctx, f)
    iset.render(srcs, loglik=True)
    noise = iset.photon_split_resident(srcs, seed)
    boxes, offs, data = iset.fetch_samples()
    out = dict(noise=noise, boxes=boxes, offs=offs, data=data.copy(), sums=iset.sample_sums(), rects=iset.photon_rects(),
               areas=iset.sample_box_areas(), ready=iset.stamp_mass_ready(srcs))
    return out, srcs


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


# ---- 8. CPU: the constant, the symbol count --------------------------------------------------------------------------------------
def test_the_option_is_declared_bound_and_adds_no_symbol():
    import subprocess
    import __graft_entry__ as ge
    ge.build()
    from desi_mcmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    keys = dict((k, int(v)) for k, v in re.findall(r"^\s*(CEL_OPT_\w+) = (\d+)\b", header, flags=re.M))
    assert keys["CEL_OPT_HONOUR_MASK"] == 17 == _lib.CEL_OPT_HONOUR_MASK
    assert sorted(keys.values()) == list(range(1, 18))                      # 17 was free: every key once
    for k, v in keys.items():
        assert getattr(_lib, k) == v, k
    blob = open(_lib.LIB_PATH, "rb").read()                                    # the library knows the key by its name
    assert b"CEL_OPT_HONOUR_MASK must be 0 or 1" in blob
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    bound = [s[0] for s in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) == 56 and declared == exported == set(bound)


def test_honour_needs_the_exact_conditional_and_the_host_engine():
    """both refusals come before any device call"""
    import __graft_entry__ as ge
    ge.build()
    from desi_mcmc_amd import celeste_mcmc
    with pytest.raises(ValueError, match="exact"):
        celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)), mask="honour")
    with pytest.raises(ValueError, match="host"):
        celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)), mask="honour",
                                conditional="exact", engine="device")
    with pytest.raises(ValueError, match="mask"):
        celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)), mask="ignore")


# ---- 1. the option off: today's refusals; on, an unmasked set is untouched -------------------------------------------------------
@gpu
def test_option_off_refuses_and_option_on_leaves_an_unmasked_set_alone(cel, ctx, frame):
    L = cel._lib
    f = frame
    assert ctx.get_option(L.CEL_OPT_HONOUR_MASK) == 0
    with pytest.raises(Exception):
        ctx.set_option(L.CEL_OPT_HONOUR_MASK, 2)
    srcs = _sources(cel, ctx, f)
    mset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(f["mask"], np.nan, f["nelec"]))
    letters, cal, kap = [0, 1], f["bands"][:, 2], f["bands"][:, 1]
    noise = np.zeros(BA)
    for call in (lambda: mset.photon_split(srcs, 3), lambda: mset.photon_split_resident(srcs, 3)):
        with pytest.raises(L.MaskedImagesError, match="does not honour a mask"):
            call()
    assert L.lib().cel_photon_split(mset._h, srcs._h, C.c_uint64(3), None, None, L.CEL_DEVICE, L.dptr(noise)) == L.CEL_ERR_INVALID
    assert b"cel_photon_split: the image set holds" in L.lib().cel_last_error()
    with pytest.raises(ValueError, match="cel_flux_conditionals: the image set holds"):      # (the library's own refusal)
        mset.flux_conditionals(srcs, 1, 5.0, 0.005, letters, cal, kap)
    with _honour(cel, ctx):                  # what stays refused whatever the option says
        for call in (lambda: mset.slice_locations(srcs, 1e-3, 1), lambda: mset.slice_sample(srcs, 0, 1e-3, 1),
                     lambda: mset.patch_loglik_resident(srcs, np.arange(f["S"]), isolated=True)):
            with pytest.raises(ValueError, match="masked"):
                call()
    assert ctx.get_option(L.CEL_OPT_HONOUR_MASK) == 0
    mset.close()
    # a set without a NaN: the same bits with the option on and off
    got = {}
    for on in (0, 1):
        with _honour(cel, ctx, on):
            iset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=f["nelec"])
            r, srcs = _resident(cel, ctx, f, iset)
            r["mass"] = iset.stamp_mass(srcs)
            iset.stamp_mass_begin(srcs)
            r["mass_be"] = iset.stamp_mass_end()
            r["flux"], r["act"] = iset.flux_conditionals(srcs, 9, 5.0, 0.005, letters, cal, kap)
            patches, _, r["noise_c"] = iset.photon_split(_sources(cel, ctx, f), SEED)
            r["caller"] = np.concatenate([p.ravel() for row in patches for p in row])
            iset.close()
            got[on] = r
    assert got[0]["ready"] is True and got[1]["ready"] is True
    _same(got[0], got[1], ["noise", "data", "sums", "rects", "areas", "mass", "mass_be", "flux", "act", "noise_c", "caller"])


# ---- 2. the split's fill identity -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("full_box", [0, 1], ids=["strict", "full-box"])
@pytest.mark.parametrize("kernel", ["recurrence", "direct"])
def test_split_fill_identity(cel, ctx, frame, kernel, full_box):
    """the split of the masked set is, bit for bit, the split of the set with 0 counts at the masked pixels (which may take the
    16-bit photons-left plane: the identity crosses instantiations on purpose) -- every patch, the noise sums, the photon sums,
    rectangles and patch areas, resident and caller-buffer forms; no photon at a masked pixel; photons conserved per band"""
    L = cel._lib
    f = frame
    mask = f["mask"]
    observed = np.where(mask, 0.0, f["nelec"])
    ctx.set_kernel(kernel)
    try:
        with _option(ctx, L.CEL_OPT_SPLIT_FULL_BOX, full_box):
            zset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=observed)
            want, srcs = _resident(cel, ctx, f, zset)
            wp, wboxes, wnoise = zset.photon_split(srcs, SEED)
            zset.close()
            with _honour(cel, ctx):
                mset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, np.nan, f["nelec"]))
                assert np.array_equal(mset.masked, mask.sum(axis=(1, 2)))
                got, srcs = _resident(cel, ctx, f, mset)
                gp, gboxes, gnoise = mset.photon_split(srcs, SEED)
                mset.close()
    finally:
        ctx.set_kernel("recurrence")
    assert got["ready"] is False                                              # no mass short cut on a masked set
    _same(got, want, ["noise", "boxes", "offs", "data", "sums", "rects", "areas"])
    assert np.array_equal(gnoise, wnoise) and np.array_equal(gboxes, wboxes)
    tot = np.zeros(BA)
    for s in range(f["S"]):
        for b in range(BA):
            y0, y1, x0, x1 = got["boxes"][s, b]
            assert np.array_equal(gp[b][s], wp[b][s])                         # the caller-buffer form
            p = got["data"][got["offs"][s * BA + b]:got["offs"][s * BA + b + 1]].reshape(y1 - y0, x1 - x0)
            assert np.all(p[mask[b, y0:y1, x0:x1]] == 0) and np.all(gp[b][s][mask[b, y0:y1, x0:x1]] == 0)
            assert p.sum() == got["sums"][s, b]
            tot[b] += p.sum()
    assert got["data"].sum() > 1e5 and np.all(np.isfinite(got["noise"]))
    for b in range(BA):                                                       # Poisson integers: exact
        assert got["noise"][b] + tot[b] == observed[b].sum(), b
        assert gnoise[b] + sum(gp[b][s].sum() for s in range(f["S"])) == observed[b].sum(), b


@gpu
@pytest.mark.parametrize("kernel", ["recurrence", "direct"])
def test_a_band_masked_everywhere_holds_nothing(cel, ctx, frame, kernel):
    f = frame
    mask = f["mask"].copy()
    mask[1] = True
    ctx.set_kernel(kernel)
    try:
        with _honour(cel, ctx):
            mset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, np.nan, f["nelec"]))
            got, srcs = _resident(cel, ctx, f, mset)
            mass = mset.stamp_mass(srcs)
            mset.close()
    finally:
        ctx.set_kernel("recurrence")
    assert got["noise"][1] == 0.0 and np.all(got["sums"][:, 1] == 0.0) and np.all(got["rects"][:, 1] == 0)
    assert got["noise"][0] > 0 and got["sums"][:, 0].sum() > 1e4
    # band 0 is untouched by band 1's mask.  (Its own mask leaves some sources next to nothing -- the half-masked boxes and the
    # box masked everywhere cover their neighbours: by the oracle's patches 14 sources keep more than half their mass, 7 less than
    # 3 % -- so photons are asked of the sources that kept a third of theirs: at least 300 x 0.3 expected)
    assert np.all(mass[:, 1] == 0.0) and mass[f["gone"], 0] == 0.0 and np.all(mass[:, 0] >= 0.0)
    kept = mass[:, 0] > 0.3
    assert kept.sum() >= 12 and np.all(got["sums"][kept, 0] > 0)


# ---- 3. the observed stamp mass ------------------------------------------------------------------------------------------------
@gpu
def test_observed_mass_against_the_oracle_and_the_estep(cel, ctx, orc, frame):
    f = frame
    mask, half, gone = f["mask"], f["half"], f["gone"]
    S = f["S"]
    srcs = _sources(cel, ctx, f)
    # a second mask that leaves most boxes whole: column 40 of band 0, one pixel of band 1
    thin = np.zeros_like(mask)
    thin[0, :, 40] = True
    thin[1, 0, 0] = True
    with tail_log(ctx, "strict"):
        mset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, np.nan, f["nelec"]))
        tset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(thin, np.nan, f["nelec"]))
        full = mset.stamp_mass(srcs)                          # the option off: the unmasked kernel, on the same records
        assert np.array_equal(full, tset.stamp_mass(srcs))
        with _honour(cel, ctx):
            ms = mset.stamp_mass(srcs)
            again = mset.stamp_mass(srcs)
            mset.stamp_mass_begin(srcs)
            ms_be = mset.stamp_mass_end()
            ms_thin = tset.stamp_mass(srcs)
        _, ms_e, _ = mset.estep_stats(srcs)
        ob = f["bands"].copy()
        for b in range(BA):
            ob[b, 36] = orc.checked_radius(ob[b], mset.band(b)[36])
        mset.close()
        tset.close()
    assert np.array_equal(ms, again) and np.array_equal(ms, ms_be)             # the same bits: run to run, and begin / end
    boxes = f["boxes"]
    ny, nx = boxes[..., 1] - boxes[..., 0], boxes[..., 3] - boxes[..., 2]
    assert np.any((nx > 32) & (ny > 64) & (f["typ"][None, :] == 1))             # a galaxy box of several chunks, both ways
    want = np.zeros((S, BA))
    for s in range(S):
        for b in range(BA):
            patch, (y0, y1), (x0, x1) = orc.source_patch(ob[b], HA, WA, f["typ"][s], f["radec"][s], f["shape"][s])
            assert np.array_equal(boxes[b, s], [y0, y1, x0, x1])
            want[s, b] = math.fsum(patch[~mask[b, y0:y1, x0:x1]])
    print("observed mass: max |library - oracle| / mass = %.3g; against the E-step's: %.3g" % (
        np.max(np.abs(ms - want) / np.maximum(want, 1e-300)), np.max(np.abs(ms - ms_e) / np.maximum(want, 1e-300))))
    assert np.all(np.abs(ms - want) <= 1e-10 * want)
    assert np.all(np.abs(ms - ms_e) <= 1e-10 * want)
    frac = 1.0 - ms[:, 0] / full[:, 0]
    assert all(0.2 <= frac[s] <= 0.6 for s in half), frac[half]
    assert ms[gone, 0] == 0.0 and ms[gone, 1] > 0.5
    # boxes without a masked pixel: the unmasked kernel's value (another order of summation: 1e-13, not the same bits)
    clean = np.array([[not thin[b, boxes[b, s, 0]:boxes[b, s, 1], boxes[b, s, 2]:boxes[b, s, 3]].any() for b in range(BA)] for s in range(S)])
    assert clean[:, 0].sum() >= 5 and clean[:, 1].sum() >= 20 and (~clean[:, 0]).sum() >= 5
    assert np.all(np.abs(ms_thin - full)[clean] <= 1e-13 * full[clean])
    assert np.all(ms_thin[~clean] <= full[~clean]) and np.sum(ms_thin[:, 0] < (1 - 1e-3) * full[:, 0]) >= 5
    # (the oracle's patches: column 40 holds 0.4-8.6 % of seven boxes' mass, less than 1e-4 of most others')


# ---- 4. the flux step -------------------------------------------------------------------------------------------------------------
def _chain(cel, ctx, f, mask, seed=5, **kw):
    from desi_mcmc_amd import celeste_mcmc
    iset = cel.ImageSet(ctx, f["bands"], HA, WA, nelec=np.where(mask, np.nan, f["nelec"]))
    cal, kap = f["bands"][:, 2], f["bands"][:, 1]
    flux5 = np.full((f["S"], 5), 3.0)
    flux5[:, :BA] = f["counts"] * cal[None, :] / kap[None, :]
    gf = celeste_mcmc.GibbsField(iset, list(range(BA)), cal, kap, HA * WA, npix_observed=iset.npix_observed())
    g = celeste_mcmc.ModelGibbs([gf], f["typ"], f["radec"], flux5, f["shape"], seed=seed, conditional="exact", mask="honour", **kw)
    return g, gf, flux5


@gpu
def test_device_flux_step_is_the_host_flux_step_on_a_masked_set(cel, ctx, frame):
    """cel_flux_conditionals with the option on against the host form of the flux step (sums and masses read back, fluxes formed
    in numpy: what ModelGibbs(conditional="exact") runs), bit for bit; a source masked in every band draws from its prior"""
    L = cel._lib
    f = frame
    mask = f["mask"].copy()
    gone = f["gone"]
    y0, y1, x0, x1 = f["boxes"][1, gone]
    mask[1, y0:y1, x0:x1] = True                               # source 12's box: masked in both bands
    g, gf, flux5 = _chain(cel, ctx, f, mask)
    g.resample_photons()
    assert ctx.get_option(L.CEL_OPT_HONOUR_MASK) == 0 and ctx.get_option(L.CEL_OPT_SPLIT_FULL_BOX) == 0      # both put back
    assert not g._device_flux_applies() and g.active.all()
    host = g.resample_fluxes().copy()
    seed = g.step_seed("flux")
    with _honour(cel, ctx):
        mass = gf.iset.stamp_mass(gf.sset)
        new, act = gf.iset.flux_conditionals(gf.sset, seed, g.flux_a_0, g.flux_b_0, gf.band_index, gf.calib, gf.kappa)
    assert act.all() and np.array_equal(new, host)
    assert np.all(gf.sums[gone] == 0.0) and np.all(mass[gone] == 0.0)
    prior = ctx.gamma_streams(np.full(f["S"] * 5, g.flux_a_0), seed).reshape(f["S"], 5) * (1.0 / g.flux_b_0)
    assert np.array_equal(new[gone], prior[gone]) and np.all(new[gone] > 0)      # Gamma(a0, b0): no photons, no mass
    seen = mass > 0.3                                                            # (a source with mass in a band is charged it)
    assert seen.sum() >= 24 and np.all(new[:, :BA][seen] != prior[:, :BA][seen])
    gf.iset.close()


# ---- 5. the sky step -------------------------------------------------------------------------------------------------------------
@gpu
def test_sky_step_counts_the_observed_pixels(cel, ctx, frame):
    f = frame
    g, gf, _ = _chain(cel, ctx, f, f["mask"], seed=7)
    assert np.array_equal(gf.npix_observed, HA * WA - f["mask"].sum(axis=(1, 2))) and gf.npix_observed[0] < HA * WA - 2000
    noise = np.array([41234.0, 39877.0])
    g.noise_sums = [noise]
    g._resample_sky()
    want = np.random.RandomState(7).gamma(gf.a_0 + noise, 1.0 / (gf.b_0 + gf.npix_observed))
    assert np.array_equal(gf.epsilon, want) and np.array_equal(gf.iset.eps, want)
    assert not np.array_equal(want, np.random.RandomState(7).gamma(gf.a_0 + noise, 1.0 / (gf.b_0 + HA * WA)))
    gf.iset.close()


# ---- 6. ModelGibbs ---------------------------------------------------------------------------------------------------------------
@gpu
def test_model_gibbs_sweeps_masked_fits_images(cel, frame):
    from desi_mcmc_amd import celeste_mcmc
    L = cel._lib
    f = frame
    mask = f["mask"]
    iv = np.where(mask, 0.0, 1.0)
    cal, kap = f["bands"][:, 2], f["bands"][:, 1]
    flux = f["counts"] * cal[None, :] / kap[None, :]
    params = []
    for s in range(f["S"]):
        fl = np.full(5, 3.0)
        fl[:BA] = flux[s]
        th = f["shape"][s]
        kw = dict(theta=th[0], sigma=th[1], phi=th[2], rho=th[3]) if f["typ"][s] == 1 else {}
        params.append(cel.SrcParams(u=f["radec"][s], a=int(f["typ"][s]), fluxes=fl, **kw))

    def images():
        return [dict(zip("ug", _fits_images(f["bands"], f["nelec"], HA, WA, iv)))]

    with pytest.raises(L.MaskedImagesError):
        celeste_mcmc.ModelGibbs.from_images(images(), params, seed=1)
    with pytest.raises(ValueError, match="exact"):
        celeste_mcmc.ModelGibbs.from_images(images(), params, seed=1, mask="honour")
    with pytest.raises(ValueError, match="host"):
        celeste_mcmc.ModelGibbs.from_images(images(), params, seed=1, mask="honour", conditional="exact", engine="device")
    runs = []
    for k in range(2):
        g = celeste_mcmc.ModelGibbs.from_images(images(), params, seed=3, mask="honour", conditional="exact")
        gf = g.fields[0]
        assert np.array_equal(gf.npix_observed, HA * WA - mask.sum(axis=(1, 2)))
        trace = []
        for sweep in range(3):
            g.resample_photons()
            boxes, offs, data = gf.iset.fetch_samples()
            for s in range(g.S):
                for b in range(BA):
                    y0, y1, x0, x1 = boxes[s, b]
                    p = data[offs[s * BA + b]:offs[s * BA + b + 1]].reshape(y1 - y0, x1 - x0)
                    assert np.all(p[mask[b, y0:y1, x0:x1]] == 0), (sweep, s, b)
            assert data.sum() > 1e5
            g.resample_fluxes()
            g.resample_locations()
            g.merge_ranks()
            g.sweeps += 1
            trace.append(g.log_likelihood())
            assert np.all(np.isfinite(g.u)) and np.all(np.isfinite(g.fluxes)) and np.all(g.fluxes > 0) and np.all(np.isfinite(gf.epsilon))
            assert np.isfinite(trace[-1])
        assert gf.iset.ctx.get_option(L.CEL_OPT_HONOUR_MASK) == 0
        assert np.abs(g.u - f["radec"]).max() > 0
        runs.append((g.u.copy(), g.fluxes.copy(), gf.epsilon.copy(), np.array(trace)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 7. calibration --------------------------------------------------------------------------------------------------------------
def make_masked_scene(cel, ctx, rep, NCELL=5):
    """theta* ~ prior, a mask, and data ~ model(theta*) with NaN written at the mask.  The scene is test_calibration.make_scene's
    (RandomState(9000 + rep)); the mask is RandomState(77000 + rep)'s: 1 % of all pixels in every band plus, per band and per
    scene, a segment 2 columns wide and 24 rows tall centred on the scene centre's row at x = round(cx + U(-5, 5))"""
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(9000 + rep)
    H = W = max(CELL * NCELL, 320)
    B = 5
    bands = synth.make_bands(H, W, B)
    eps = rs.gamma(EPS_A, 1.0 / EPS_B, B)
    bands[:, 0] = eps
    cy, cx = np.meshgrid(np.arange(NCELL), np.arange(NCELL), indexing="ij")
    centres = np.column_stack([cx.ravel() * CELL + CELL / 2.0, cy.ravel() * CELL + CELL / 2.0])
    nper = rs.choice([1, 2, 3], centres.shape[0], p=[0.4, 0.4, 0.2])
    pix = np.concatenate([c[None, :] + rs.uniform(-6.0, 6.0, (n, 2)) for c, n in zip(centres, nper)])
    S = pix.shape[0]
    typ = (rs.rand(S) < 0.4).astype(np.int32)
    shape = np.column_stack([rs.uniform(0.1, 0.9, S), np.exp(rs.uniform(np.log(0.4), np.log(1.2), S)), rs.uniform(0, 180, S),
                             rs.uniform(0.3, 0.95, S)])
    shape[typ == 0] = 0.0
    flux = rs.gamma(FLUX_A, 1.0 / FLUX_B, (S, 5))
    radec = synth.pixel2equa(bands[0], pix)
    counts = flux / bands[None, :, 2] * bands[None, :, 1]
    iset = cel.ImageSet(ctx, bands, H, W)
    sset = cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape)
    iset.render(sset, loglik=False)
    nelec = rs.poisson(iset.model_images()).astype(np.float64)
    rm = np.random.RandomState(77000 + rep)
    mask = rm.rand(B, H, W) < 0.01
    for b in range(B):
        for c in centres:
            x = int(round(c[0] + rm.uniform(-5.0, 5.0)))
            y = int(c[1])
            mask[b, y - 12:y + 12, x:x + 2] = True
    iset.set_nelec(np.where(mask, np.nan, nelec))
    # how much of its stamp each (source, band) loses: the library's own two mass calls
    full = iset.stamp_mass(sset)
    with _honour(cel, ctx):
        seen = iset.stamp_mass(sset)
    return dict(bands=bands, iset=iset, typ=typ, radec=radec, flux=flux, shape=shape, H=H, W=W, B=B, S=S, pix=pix, mask=mask,
                lost=1.0 - seen / full)


def _charge_unmasked_masses(cel, iset):
    """the control: every mass the sweep reads from this image set is the UNMASKED one (the option off around the mass calls; a
    queued call is collected and answered by the unmasked kernel for the same sources)"""
    K = cel._lib.CEL_OPT_HONOUR_MASK
    real_mass, real_begin, real_end = iset.stamp_mass, iset.stamp_mass_begin, iset.stamp_mass_end
    pending = []

    def unmasked(sources):
        with _option(iset.ctx, K, 0):
            return real_mass(sources)

    def begin(sources):
        pending[:] = [sources]
        return real_begin(sources)

    def end():
        real_end()
        return unmasked(pending[0])
    iset.stamp_mass, iset.stamp_mass_begin, iset.stamp_mass_end = unmasked, begin, end


def run_masked_replicate(cel, ctx, rep, chain_seed, J, ncell=5, control=False):
    """test_calibration.run_replicate on a masked scene: conditional="exact", the host engine, no shape step, mask="honour"
    -> (location ranks (S, 2), flux ranks (S, 5), the (S, B) share of its stamp each source loses to the mask)"""
    from desi_mcmc_amd import celeste_mcmc
    sc = make_masked_scene(cel, ctx, rep, ncell)
    if control:
        _charge_unmasked_masses(cel, sc["iset"])

    def chain():
        gf = celeste_mcmc.GibbsField(sc["iset"], list(range(sc["B"])), sc["bands"][:, 2], sc["bands"][:, 1], sc["H"] * sc["W"],
                                     a_0=EPS_A, b_0=EPS_B, npix_observed=sc["iset"].npix_observed())
        for b in range(sc["B"]):
            sc["iset"].set_epsilon(b, sc["bands"][b, 0])
        return celeste_mcmc.ModelGibbs([gf], sc["typ"], sc["radec"], sc["flux"], sc["shape"], seed=chain_seed, flux_a_0=FLUX_A,
                                       flux_b_0=FLUX_B, engine="host", conditional="exact", mask="honour")
    du, df = [], []
    g = chain()
    for k in range((K_DRAWS - J) * THIN):
        g.sweep()
        g.log_likelihood()
        assert g.active.all()
        if k % THIN == THIN - 1:
            du.append(g.u.copy())
            df.append(g.fluxes.copy())
    if K_DRAWS - J > 0:
        assert (np.abs(du[-1] - sc["radec"]).max(axis=1) > 0).mean() > 0.99
    g = chain()
    g.seed = chain_seed + 7919
    g._split_photons()
    for k in range(J * THIN):
        g.sweep_reversed()
        if k % THIN == THIN - 1:
            du.append(g.u.copy())
            df.append(g.fluxes.copy())
    du, df = np.array(du), np.array(df)
    assert du.shape[0] == K_DRAWS
    sc["iset"].close()
    return (du < sc["radec"][None]).sum(axis=0), (df < sc["flux"][None]).sum(axis=0), sc["lost"]


def masked_pooled_ranks(cel, ctx, control=False):
    parts = [run_masked_replicate(cel, ctx, rep, chain_seed=rep, J=rep % (K_DRAWS + 1), control=control) for rep in range(K_DRAWS + 1)]
    ru, rf, lost = (np.concatenate(p) for p in zip(*parts))
    per_rep = [float((p[2].max(axis=1) >= 0.1).mean()) for p in parts]
    return ru, rf, lost, per_rep


@gpu
def test_masked_sweep_leaves_the_posterior_invariant(cel, ctx):
    """The calibration of tests/test_calibration.py (its docstring explains the exact rank statistic) on masked scenes: 8
    replicates of 320 x 320 x 5 bands, ~45 sources each, 1 % of the pixels masked plus a 2 x 24 segment through every scene in
    every band -- most sources lose 10-50 % of their stamp mass in some band (asserted: the masks must bite).  The sweep with
    mask="honour" passes at the existing threshold; the same sweep charged the UNMASKED masses fails by many orders.
    Measured on an MI355X (8 replicates, 364 sources): p(location x) = 0.18, p(location y) = 0.31, p(flux) = 0.94; the control
    p(flux) = 0 (below the smallest double), p(location x) = 1e-183, p(location y) = 2e-52."""
    ru, rf, lost, per_rep = masked_pooled_ranks(cel, ctx)
    pairs = float((lost >= 0.1).mean())
    print("masked scenes: %d sources; per replicate the share losing >= 10 %% in some band: %s; pooled share of (source, band) "
          "pairs: %.3f; largest loss %.3f" % (ru.shape[0], np.round(per_rep, 3).tolist(), pairs, lost.max()))
    assert min(per_rep) >= 0.8 and pairs >= 0.4 and lost.max() < 1.0
    out = {}
    for name, r in (("location x", ru[:, 0]), ("location y", ru[:, 1]), ("flux", rf)):
        stat, p, counts = chi2_pvalue(r, K_DRAWS)
        out[name] = (round(stat, 2), p, counts.astype(int).tolist())
    print("SBC ranks on masked scenes (host engine, exact conditional, %d sources in %d replicates): %s" % (ru.shape[0], K_DRAWS + 1, out))
    for name, (stat, p, counts) in out.items():
        assert p > 1e-3 / 3, (name, stat, p, counts)
    # the control: every mass the sweep reads is the UNMASKED one
    ru, rf, _, _ = masked_pooled_ranks(cel, ctx, control=True)
    p_flux = chi2_pvalue(rf, K_DRAWS)[1]
    print("the unmasked masses in the masked sweep: p(flux) = %.3g, p(location x, y) = %.3g, %.3g" % (
        p_flux, chi2_pvalue(ru[:, 0], K_DRAWS)[1], chi2_pvalue(ru[:, 1], K_DRAWS)[1]))
    assert p_flux < 1e-8
