"""ctypes binding of libceleste_hip.so (the C ABI declared in include/celeste_hip.h).

There is no fallback: if the HIP library is missing or no GPU is visible, every entry point
raises.  Nothing here imports torch or the oracle.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CEL_HIP_LIBRARY: another build of the same sources (tools: the -DCEL_ABLATE library, occupancy experiments); never a fallback
LIB_PATH = os.environ.get("CEL_HIP_LIBRARY") or os.path.join(_HERE, "libceleste_hip.so")

CEL_OK, CEL_ERR_INVALID, CEL_ERR_HIP, CEL_ERR_NOMEM, CEL_ERR_NO_DEVICE = 0, 1, 2, 3, 4
CEL_HOST, CEL_DEVICE = 0, 1
CEL_RENDER_LOGLIK, CEL_RENDER_NO_STORE = 1, 2
#: cel_patch_loglik[_multi]: mode = CEL_PLL_GRAD + m (m = 0, 1, 2) is the gradient form of mode m; ll_out holds P * (7 + B) doubles
CEL_PLL_GRAD = 8
#: k_patch_grad_nz.h (the resident gradient at the photon lists, CEL_OPT_PHOTON_LISTS = 4 / 5): the photons of a trip, and the
#: longest list that one block takes whole (a longer one is dealt to four blocks, trip by trip)
PGNZ_TRIP, PGNZ_DEAL_PHOTONS = 128, 512
#: cel_slice_sample: param = CEL_SLICE_MOMENTS runs no sampler; stats receives the S * B * 6 int64 moments of the resident split
#: (ImageSet.photon_moments; k_moments.h).  A patch of more than CEL_MOMENTS_SPLIT_PIXELS pixels is dealt to four blocks
CEL_SLICE_MOMENTS, CEL_MOMENTS_SPLIT_PIXELS = 10, 4096
CEL_OPT_KERNEL, CEL_OPT_TAIL_LOG, CEL_OPT_PROFILE, CEL_OPT_TILE_ORDER, CEL_OPT_TILE_ROWS = 1, 2, 3, 4, 5
CEL_OPT_TILE_TIMING, CEL_OPT_TILE_LAYOUT, CEL_OPT_DEBUG, CEL_OPT_PHOTON_LISTS, CEL_OPT_STAR_TILES, CEL_OPT_SPLIT_REUSE = 6, 7, 8, 9, 10, 11
CEL_OPT_TAIL_LOG_SOURCE, CEL_OPT_TILE_PARTS, CEL_OPT_INCREMENTAL, CEL_OPT_SPLIT_FULL_BOX, CEL_OPT_SLICE_FUSE = 12, 13, 14, 15, 16
#: 1 = on a masked image set the photon split, the stamp masses and the flux step honour the mask (0, the default: they refuse it)
CEL_OPT_HONOUR_MASK = 17
#: what cel_slice_sample scores: 0 the reference's conditional (default), 1 the exact one (ImageSet.slice_sample(conditional=))
CEL_OPT_SLICE_CONDITIONAL = 18
#: which conditional the resident gradient (cel_patch_loglik_multi's resident mode 8) and the HMC step (cel_slice_sample, param 3)
#: differentiate: 0 the reference's (default), 1 the exact one (ImageSet.patch_loglik_resident_grad / hmc_step(conditional=))
CEL_OPT_GRAD_CONDITIONAL = 19
#: 1 (default): renders that prepare no source load every record's mixture components from a cache built once per record
#: generation (k_comps, counted under KERNELS["gmm"]; k_render_hwc) -- the same bits as the plain kernel's; 0 = never
CEL_OPT_COMP_CACHE = 20
#: 1 (with CEL_OPT_HONOUR_MASK = 1): the device samplers of the exact conditional (cel_slice_sample under CEL_OPT_SLICE_CONDITIONAL /
#: CEL_OPT_GRAD_CONDITIONAL = 1) and the exact resident mode 8 accept a masked image set and charge the OBSERVED stamp mass and its
#: derivative (ImageSet.slice_sample / type_move / hmc_step / patch_loglik_resident_grad(mask="honour")); 0 (default): they refuse it
CEL_OPT_SAMPLER_MASK = 21
#: CEL_OPT_TAIL_LOG presets.  32 (the default): a skipped component is below eps * e^-32 on its tile, model pixels
#: agree with the reference to ~1e-13, which is what the parity tests assert (1e-10).  20: the documented fast
#: preset for callers that need only north_star's 1e-6 -- a skipped component is below eps * 2e-9, the sum of
#: all skips on a pixel stays below ~1e-7 of lambda (tests/test_hip_parity.py::test_tail_log_fast_preset...).
#: Round 4: the FIELD RENDER's default is 24 (a skipped component is below eps * 4e-11; the benchmark field's log-likelihood
#: keeps all 16 digits and every pixel stays within 1e-10 of the oracle: tests/test_hip_parity.py::test_config3_full_vs_oracle),
#: the per-source kernels keep 32 (CEL_OPT_TAIL_LOG_SOURCE reads / sets theirs alone).  TAIL_LOG_STRICT = 32 for both: the
#: strict variants of the parity tests (conftest.tail_log); the suite itself runs at these shipping defaults.
TAIL_LOG_DEFAULT, TAIL_LOG_STRICT, TAIL_LOG_FAST = 24.0, 32.0, 20.0
KERNELS = {"prep": 0, "bin": 1, "render": 2, "reduce": 3, "stamps": 4, "gmm": 5, "patch_ll": 6, "split": 7, "mass": 8, "estep": 9, "render_stars": 10, "small_stars": 11, "totals": 12, "grad": 13, "masked_ll": 14}
BAND_DOUBLES = 37
MAX_BANDS = 16

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_void_pp = C.POINTER(C.c_void_p)

# every symbol include/celeste_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("cel_abi_version", C.c_int, []),
    ("cel_last_error", C.c_char_p, []),
    ("cel_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("cel_ctx_create", C.c_int, [C.c_int, C.c_void_p, c_void_pp]),
    ("cel_ctx_destroy", C.c_int, [C.c_void_p]),
    ("cel_ctx_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("cel_ctx_synchronize", C.c_int, [C.c_void_p]),
    ("cel_ctx_set_option", C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    ("cel_ctx_get_option", C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    ("cel_images_create", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, c_void_pp]),
    ("cel_images_destroy", C.c_int, [C.c_void_p]),
    ("cel_images_set_nelec", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("cel_images_mask_info", C.c_int, [C.c_void_p, c_int64_p]),
    ("cel_images_set_epsilon", C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    ("cel_images_set_window", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("cel_images_set_noise_rows", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("cel_images_get_band", C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    ("cel_images_get_lambda", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("cel_images_device_ptrs", C.c_int, [C.c_void_p, c_void_pp, c_void_pp]),
    ("cel_images_loglik_device", C.c_int, [C.c_void_p, c_void_pp]),
    ("cel_sources_create", C.c_int, [C.c_void_p, C.c_int64, C.c_int, c_void_pp]),
    ("cel_sources_destroy", C.c_int, [C.c_void_p]),
    ("cel_sources_set", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("cel_sources_set_rows", C.c_int, [C.c_void_p, C.c_int64, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    ("cel_sources_get", C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    ("cel_render_field", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_double_p, c_double_p]),
    ("cel_field_stats", C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("cel_gamma_streams", C.c_int, [C.c_void_p, C.c_int64, c_double_p, C.c_uint64, c_double_p]),
    ("cel_flux_conditionals", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, c_int32_p, c_double_p, c_double_p,
                                        c_double_p, c_int32_p]),
    ("cel_debug_split_rates", C.c_int, [C.c_void_p, c_double_p]),
    ("cel_debug_tile_timing", C.c_int, [C.c_void_p, C.c_void_p, c_int64_p]),
    ("cel_debug_last_render", C.c_int, [C.c_void_p, c_int64_p]),
    ("cel_stamp_boxes", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_int32_p, c_int32_p]),
    ("cel_render_stamps", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, c_int32_p, c_int64_p, C.c_void_p, C.c_int]),
    ("cel_patch_loglik", C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, c_int64_p, C.c_void_p, C.c_int, C.c_int, c_double_p]),
    ("cel_patch_loglik_multi", C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, C.c_int64, c_int32_p, c_int64_p, C.c_void_p,
                                          C.c_int, C.c_int, c_double_p]),
    ("cel_stamp_mass", C.c_int, [C.c_void_p, C.c_void_p, c_double_p]),
    ("cel_stamp_mass_ready", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    ("cel_stamp_mass_begin", C.c_int, [C.c_void_p, C.c_void_p]),
    ("cel_stamp_mass_end", C.c_int, [C.c_void_p, c_double_p]),
    ("cel_slice_locations", C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, C.c_double, C.c_uint64, C.c_int, c_double_p,
                                      c_double_p, c_int64_p]),
    ("cel_slice_sample", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, c_int32_p, c_double_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_uint64, C.c_int, c_double_p, c_double_p, c_int64_p]),
    ("cel_source_boxes", C.c_int, [C.c_void_p, C.c_void_p, c_int32_p, c_int32_p]),
    ("cel_photon_split", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, c_int64_p, C.c_void_p, C.c_int, c_double_p]),
    ("cel_samples_info", C.c_int, [C.c_void_p, c_int64_p, c_int64_p]),
    ("cel_samples_fetch", C.c_int, [C.c_void_p, c_int32_p, c_int64_p, C.c_void_p, c_double_p]),
    ("cel_samples_photon_rects", C.c_int, [C.c_void_p, c_int32_p]),
    ("cel_debug_binomial", C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_uint64, C.c_int64, c_int64_p]),
    ("cel_estep_stats", C.c_int, [C.c_void_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("cel_loglik_grad", C.c_int, [C.c_void_p, C.c_void_p, c_double_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("cel_gmm_like_2d", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, c_double_p, c_double_p, c_double_p, C.c_int,
                                  C.c_void_p, C.c_int]),
    ("cel_mog_loglike", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, c_double_p, c_double_p, c_double_p, C.c_int,
                                  C.c_void_p, C.c_int]),
    ("cel_galaxy_mixture_params", C.c_int, [C.c_void_p, C.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                            c_double_p, C.c_int, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p,
                                            c_double_p]),
    ("cel_bounding_radius", C.c_int, [c_double_p, c_double_p, c_double_p, C.c_int, C.c_double, c_double_p, c_double_p]),
    ("cel_profile_reset", C.c_int, [C.c_void_p]),
    ("cel_profile_get", C.c_int, [C.c_void_p, C.c_int, c_double_p, c_int64_p]),
]


class CelesteHipError(RuntimeError):
    pass


class MaskedImagesError(CelesteHipError, ValueError):
    """a call that has not been taught about masked pixels (NaN counts, cel_images_set_nelec) was handed a masked image set:
    the library's refusal (CEL_ERR_INVALID, hence a ValueError) raised by the Python layer before any device call"""


_lib = None


def lib():
    """Load the HIP library.  Loud failure when it has not been built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CelesteHipError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C desi-mcmc_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)   # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        if L.cel_abi_version() != 1:
            raise CelesteHipError("ABI version mismatch")
        _lib = L
    return _lib


def check(status):
    if status == CEL_OK:
        return
    msg = lib().cel_last_error().decode("utf-8", "replace")
    if status == CEL_ERR_INVALID:
        raise ValueError(msg)               # gmm_like_fast.pyx:146-149 raises ValueError
    if status == CEL_ERR_NOMEM:
        raise MemoryError(msg)
    raise CelesteHipError(msg)


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def device_count():
    n = C.c_int(0)
    check(lib().cel_device_count(C.byref(n)))
    return n.value
