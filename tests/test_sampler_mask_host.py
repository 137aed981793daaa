"""CPU-only checks of CEL_OPT_SAMPLER_MASK = 21 (the device samplers of the exact conditional on a masked image set): the key in the
header and the binding, the entry points unchanged, ModelGibbs(mask_engine=) and the refusals it leaves standing.  No compute call
reaches a device here."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import desi_mcmc_amd
    return desi_mcmc_amd


def _empty():
    return [], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4))


def test_the_key_is_21_and_no_entry_point_was_added(built):
    from desi_mcmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    assert re.search(r"CEL_OPT_SAMPLER_MASK = 21\b", header) and _lib.CEL_OPT_SAMPLER_MASK == 21
    assert re.search(r"CEL_K_COUNT = 15\b", header)
    # the paragraph names what it admits and what stays refused
    doc = header[header.index("CEL_OPT_SAMPLER_MASK = 21"):header.index("CEL_OPT_SLICE_CONDITIONAL = 18")]
    for word in ("CEL_OPT_HONOUR_MASK = 1", "k_stamp_mass_masked", "k_mass_grad_masked", "cel_slice_locations", "isolated", "row window",
                 "reference's conditional", "CEL_ERR_INVALID"):
        assert word in doc, word
    # the keys are distinct in the binding
    keys = [v for k, v in vars(_lib).items() if k.startswith("CEL_OPT_")]
    assert len(keys) == len(set(keys))
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    bound = [s[0] for s in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) == 56 and declared == exported == set(bound)
    # the two kernels are in the library's device code
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"k_mass_grad_masked" in blob and b"k_stamp_mass_masked" in blob


def test_mask_engine_opens_the_device_engine_and_nothing_else(built):
    from desi_mcmc_amd import celeste_mcmc
    G = celeste_mcmc.ModelGibbs
    g = G(*_empty(), mask="honour", conditional="exact", engine="device", mask_engine="device")
    assert g.mask_engine == "device" and g._exact_on_device() is True and g._sampler_mask() == "honour"
    g.fields = [None]
    assert g._device_engine_applies() is True
    g = G(*_empty(), mask="honour", conditional="exact", engine="auto", mask_engine="device",
          slice_args=dict(step_out=False, sigma=1e-3), hmc_conditional="exact")
    g.fields = [None]
    assert g._device_engine_applies() is True and g._shape_engine_on_device() is True
    assert g._type_engine_on_device() is True and g._hmc_engine_on_device() is True
    g.fields = [None, None]                                         # several fields keep the host engine
    assert g._device_engine_applies() is False and g._type_engine_on_device() is False and g._hmc_engine_on_device() is False
    # the default: every path and every refusal as before
    with pytest.raises(ValueError, match="host"):
        G(*_empty(), mask="honour", conditional="exact", engine="device")
    with pytest.raises(ValueError, match="host"):
        G(*_empty(), mask="honour", conditional="exact", engine="device", mask_engine="host")
    h = G(*_empty(), mask="honour", conditional="exact", hmc_conditional="exact")
    h.fields = [None]
    assert h.mask_engine == "host" and h._exact_on_device() is False
    assert h._type_engine_on_device() is False and h._hmc_engine_on_device() is False and h._shape_engine_on_device() is False
    # the reference's HMC step charges no observed mass: it stays on the host engine's refusal
    r = G(*_empty(), mask="honour", conditional="exact", mask_engine="device")
    r.fields = [None]
    assert r._hmc_engine_on_device() is False
    # an unmasked sweep does not read it
    u = G(*_empty(), conditional="exact", mask_engine="device")
    assert u._sampler_mask() == "refuse" and u._exact_on_device() is True
    with pytest.raises(ValueError, match="mask_engine"):
        G(*_empty(), mask="honour", conditional="exact", mask_engine="gpu")
    with pytest.raises(ValueError, match="mask_engine"):
        G(*_empty(), mask_engine="gpu")
    with pytest.raises(ValueError, match="exact"):
        G(*_empty(), mask="honour", mask_engine="device")            # the reference's conditional stays refused
    with pytest.raises(ValueError, match="mask_engine"):
        G.from_images([], [], mask="honour", conditional="exact", mask_engine="gpu")


def test_the_wrappers_check_mask_before_any_device_call(built):
    """mask= is validated by the ImageSet wrappers on the host: an unknown value raises without a handle being touched"""
    from desi_mcmc_amd import field
    im = object.__new__(field.ImageSet)
    for who in ("slice_sample", "type_move", "hmc_step", "patch_loglik_resident_grad"):
        with pytest.raises(ValueError, match="mask must be"):
            im._sampler_mask(who, "ignore", "exact")
