"""CPU-only checks of the masked-pixel plumbing: FitsImage's invvar / mask_invvar / observed, the binding of
cel_images_mask_info and the new profile slot, the host-side refusals.  No compute call reaches a device here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import desi_mcmc_amd
    return desi_mcmc_amd


def _image(built, nelec, **kw):
    from desi_mcmc_amd import synth
    from desi_mcmc_amd.fits_image import FitsImage
    r = synth.make_bands(nelec.shape[0], nelec.shape[1], 1)[0]
    return FitsImage("r", nelec, epsilon=r[0], kappa=r[1], calib=r[2], weights=r[3:6], means=r[6:12].reshape(3, 2),
                     covars=r[12:24].reshape(3, 2, 2), rho_n=r[24:26], phi_n=r[26:28], Ups_n=r[28:32].reshape(2, 2), **kw)


def _counts():
    rs = np.random.RandomState(2)
    nelec = rs.poisson(200.0, (12, 17)).astype(np.float64)
    nelec[3, 4] = -2.0                                            # a negative count is data
    iv = rs.uniform(0.5, 2.0, nelec.shape)
    iv[rs.rand(*nelec.shape) < 0.1] = 0.0
    iv[3, 5] = 0.0
    return nelec, iv


def test_observed_is_nan_exactly_where_invvar_is_zero(built):
    nelec, iv = _counts()
    im = _image(built, nelec, invvar=iv, mask_invvar=True)
    obs = im.observed
    assert np.array_equal(np.isnan(obs), iv == 0) and (iv == 0).sum() > 5
    assert np.array_equal(obs[iv != 0], nelec[iv != 0]) and obs[3, 4] == -2.0
    assert im.n_masked == (iv == 0).sum()
    assert im.invvar is iv                                        # kept as given
    assert np.array_equal(im.nelec, nelec)                        # nelec itself is untouched
    assert im.observed is obs and not obs.flags.writeable


def test_default_construction_ignores_invvar(built):
    nelec, iv = _counts()
    im = _image(built, nelec)
    assert im.invvar is None and im.mask_invvar is False and im.observed is im.nelec and im.n_masked == 0
    im = _image(built, nelec, invvar=iv)                          # invvar alone: stored, not applied (celeste.py:237-240)
    assert im.invvar is iv and im.observed is im.nelec and im.n_masked == 0
    with pytest.raises(ValueError):
        _image(built, nelec, mask_invvar=True)                    # nothing to mask by
    with pytest.raises(ValueError):
        _image(built, nelec, invvar=iv[:5], mask_invvar=True)


def test_from_record_passes_both_through(built):
    from desi_mcmc_amd import synth
    from desi_mcmc_amd.fits_image import FitsImage
    nelec, iv = _counts()
    r = synth.make_bands(12, 17, 2)
    rec = dict(eps=r[:, 0], kappa=r[:, 1], calib=r[:, 2], weights=r[:, 3:6], means=r[:, 6:12].reshape(2, 3, 2),
               covars=r[:, 12:24].reshape(2, 3, 2, 2), rho=r[:, 24:26], phi=r[:, 26:28], ups=r[:, 28:32].reshape(2, 2, 2))
    im = FitsImage.from_record("g", rec, 1, nelec, invvar=iv, mask_invvar=True)
    assert im.invvar is iv and im.mask_invvar and np.array_equal(np.isnan(im.observed), iv == 0)
    im = FitsImage.from_record("g", rec, 1, nelec)
    assert im.invvar is None and im.observed is im.nelec


def test_mask_info_is_bound_as_declared(built):
    from desi_mcmc_amd import _lib
    assert _lib.KERNELS["masked_ll"] == 14
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    assert re.search(r"^int cel_images_mask_info\(cel_images \*img, int64_t \*masked[^)]*\);", header, flags=re.M)
    assert re.search(r"CEL_K_MASKED_LL = 14,", header) and re.search(r"CEL_K_COUNT = 15\b", header)
    row = [s for s in _lib.SYMBOLS if s[0] == "cel_images_mask_info"]
    assert row == [("cel_images_mask_info", C.c_int, [C.c_void_p, _lib.c_int64_p])]
    fn = _lib.lib().cel_images_mask_info
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, _lib.c_int64_p]
    # one more entry point than before, and the three lists of them stay equal: the header's, the library's, the binding's
    import subprocess
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    bound = [s[0] for s in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) == 56 and declared == exported == set(bound)
    # null arguments are refused like everywhere else (no device needed)
    assert fn(None, None) == _lib.CEL_ERR_INVALID
    assert issubclass(_lib.MaskedImagesError, _lib.CelesteHipError) and issubclass(_lib.MaskedImagesError, ValueError)


def test_host_refusals_come_before_any_device_call(built):
    """Field.resample_photons and ModelGibbs.from_images look at the FitsImages alone: they raise on a machine without a GPU"""
    from desi_mcmc_amd import _lib, celeste_mcmc, models
    nelec, iv = _counts()
    im = _image(built, nelec, invvar=iv, mask_invvar=True)
    eps = im.epsilon
    with pytest.raises(ValueError, match="masked"):
        models.Field({"r": im}).resample_photons([])
    with pytest.raises(_lib.CelesteHipError, match="masked"):
        celeste_mcmc.ModelGibbs.from_images([{"r": im}], [])
    del eps
