/*
 * celeste_hip.h -- C ABI of the MI355X (gfx950) render + Poisson log-likelihood path.
 *
 * The reference (HIPS/DESI-MCMC, CelestePy) has no FFI layer for this path: the boundary
 * is the module-function API of CelestePy/celeste.py and celeste_galaxy_conditionals.py,
 * plus one native seam (CelestePy/util/like/__init__.py:5-14, which swaps the Cython
 * gmm_like_2d in for the numpy gmm_prob).  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference root).  The Python mirror in
 * desi-mcmc_amd/ binds exactly these symbols with ctypes; INTEGRATION.md shows the stub a
 * CelestePy maintainer would add.
 *
 * Conventions
 *   - plain C: pointers and sizes only; no C++/torch/numpy types cross this boundary;
 *   - every function returns a cel_status; nothing throws across the ABI;
 *     cel_last_error() gives the message of the calling thread's last failure;
 *   - all arithmetic and all image / parameter buffers are IEEE fp64, images row-major [y][x];
 *   - `mem` says where a caller buffer lives: CEL_HOST (pageable or pinned host memory) or
 *     CEL_DEVICE (a HIP device pointer on the context's device, e.g. torch.Tensor.data_ptr());
 *   - device memory for images, sources, bins and partial sums is owned by the library;
 *   - work is enqueued on the context's HIP stream; calls that return values to the host
 *     synchronise that stream, the *_async forms do not;
 *   - threads: a context and the objects created on it belong to one host thread at a time; different contexts may be
 *     driven from different threads at once (tools/dbg/two_threads.py: results equal to the threads run alone);
 *   - there is NO CPU fallback: without a HIP device cel_ctx_create fails with
 *     CEL_ERR_NO_DEVICE.
 */
#ifndef CELESTE_HIP_H
#define CELESTE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CEL_ABI_VERSION 1

typedef enum {
    CEL_OK = 0,
    CEL_ERR_INVALID = 1,   /* bad argument / shape mismatch: the Python mirror raises ValueError
                              (gmm_like_fast.pyx:146-149) */
    CEL_ERR_HIP = 2,       /* a HIP runtime call failed */
    CEL_ERR_NOMEM = 3,
    CEL_ERR_NO_DEVICE = 4  /* no usable gfx950 device */
} cel_status;

enum { CEL_HOST = 0, CEL_DEVICE = 1 };

/* cel_render_field flags */
enum {
    CEL_RENDER_LOGLIK = 1,   /* also reduce sum(nelec*log(lambda) - lambda) per band */
    CEL_RENDER_NO_STORE = 2  /* do not write the model images (log-lik only)        */
};

/* cel_ctx_set_option keys */
enum {
    CEL_OPT_KERNEL = 1,    /* 0 = direct exp per Gaussian-pixel, 1 = row-recurrence (default).
                              Selects the form of every evaluating kernel: field render, stamps,
                              conditional log-likelihoods, photon split, E-step reductions        */
    CEL_OPT_TAIL_LOG = 2,  /* T >= 0: a mixture component is skipped on an image tile when its
                              contribution stays below eps * e^-T everywhere on the part of the
                              tile its source covers (eps = the band's sky level, so the bound is
                              relative to lambda >= eps).  0 = never skip.
                              |d lambda| / lambda <= n_skipped * e^-T: the field render's default is
                              T = 24 (n * 3.8e-11: three orders inside the 1e-6 parity bar for a
                              thousand skips on one pixel; measured on the benchmark field: every
                              pixel within 1e-10 of the oracle, the log-likelihood unchanged in all 16
                              digits, the kernel 13 % shorter than at 32).
                              The per-source kernels whose output has no sky in it (stamps, the
                              conditional log-likelihood, the E-step sums, the photon split's stamps)
                              use T against the source's own smallest value on the tile instead of
                              eps -- the relative error of every pixel stays below n_components * e^-T
                              -- and default to T = 32.  Setting the option sets BOTH thresholds; NaN
                              restores the two defaults; cel_ctx_get_option returns the render's
                              (the per-source kernels': CEL_OPT_TAIL_LOG_SOURCE).  CEL_TAIL_LOG in the
                              environment, when inside [0, 300], is the initial value of both       */
    CEL_OPT_TAIL_LOG_SOURCE = 12, /* the per-source kernels' threshold alone (set / get; NaN: its default, 32) */
    CEL_OPT_INCREMENTAL = 14, /* 1 (default): a cel_render_field whose image set still holds the model image, tile lists and Poisson
                               partials of an earlier state of the SAME catalogue, from which at most 64 rows were changed by
                               cel_sources_set_rows since, renders only the tiles those rows' old and new boxes touch -- each
                               from its complete source list, so every pixel and the log-likelihood are the full render's bit
                               for bit (source preparation and binning still run in full).  The reference's single-source moves
                               (util/infer/mcmc_transitions.py:37-152) evaluate the whole likelihood after changing one source.
                               A render after cel_sources_set, or with nothing changed, renders every tile.  A render of a
                               catalogue that has not changed since this image set's last render of it (a new sky level or new
                               pixels in between, a log-likelihood after a plain render) prepares no source again: the records
                               and tile lists on the device are this catalogue's.  0 = always every tile, always prepared and binned */
    /* component cache: */ CEL_OPT_COMP_CACHE = 20,  /* 1 (default): a general cel_render_field that prepares no source (see CEL_OPT_INCREMENTAL: the records
                               on the device are this catalogue's) builds every record's mixture components once -- k_comps, timed
                               under CEL_K_GMM -- and this and the following such renders load them per tile entry instead of
                               computing them (k_render_hwc; the one-block form of the 32 x 64 layout: CEL_OPT_TILE_PARTS = 1 or a
                               frame of more than 3 072 tiles).  The rows hold what the plain kernel computes, bit for bit, so
                               pixels and log-likelihoods are the same bits either way; 2 520 bytes per (band, source).  A render
                               that prepares its sources takes the plain kernel.  0 = always the plain kernel */
    CEL_OPT_SPLIT_FULL_BOX = 15, /* 0 (default): the photon split gives a source photons only STRICTLY inside its box on the low side, as
                               the reference does (celeste_sample_sources.pyx:50-51: the first row and column of every sample patch
                               stay 0) -- although the renderer adds the source on its whole box (celeste.py:217-219).  1 = on the
                               whole box: the split of the model the renderer draws from, which the exact conditionals of
                               ModelGibbs(conditional="exact") need (DESIGN Q20: with the reference's rule a big galaxy's first box
                               row and column -- up to 10^-4 of its photons -- are modelled but never attributed).  The stamp-mass
                               short cut of CEL_OPT_SPLIT_REUSE = 2 is not taken then */
    CEL_OPT_SLICE_FUSE = 16, /* 0 (default): a round of cel_slice_locations is three launches (likelihoods, chain step).  N > 1: a round
                                of at most N likelihood blocks is ONE launch when every patch of the call is scored at its photons --
                                the block that finishes a chain's last job of the round consumes the chain's log-likelihoods, names
                                its next point and writes that point's records; 1: every round.  The chains are the same bit for
                                bit either way.  Measured in round 6: no gain at any N, hence off */
    CEL_OPT_HONOUR_MASK = 17, /* 0 (default): the calls of the Gibbs sweep refuse a MASKED image set (NaN counts, cel_images_set_nelec)
                                 as before.  1: on a masked set cel_photon_split (resident and caller-buffer forms, both kernels)
                                 gives a masked pixel no photons -- every patch value there is 0, it adds nothing to the noise
                                 sum whether or not a box covers it, and it draws no random numbers (the twins k_photon_split_hw_masked
                                 / k_photon_split_masked; everything at observed pixels is the split of the set with 0 counts at the
                                 masked pixels, bit for bit); cel_stamp_mass / _begin / _end return the unit stamp summed over the
                                 UNMASKED pixels of the source's box (k_stamp_mass_masked: cel_estep_stats' `mass`), the stamp-mass
                                 short cut of CEL_OPT_SPLIT_REUSE = 2 is not taken and cel_stamp_mass_ready answers 0; and
                                 cel_flux_conditionals runs on those sums and masses (a source masked in every band draws from its
                                 prior).  On a set without a NaN the option changes nothing: the same kernels, launches and bits.
                                 cel_slice_locations, cel_slice_sample and the isolated forms of cel_patch_loglik[_multi] refuse a
                                 masked set whatever this option says (the device samplers of the exact conditional: CEL_OPT_SAMPLER_MASK) */
    /* samplers on a masked set: */ CEL_OPT_SAMPLER_MASK = 21, /* 0 (default): every device sampler and the exact resident gradient refuse a MASKED
                                 image set, as before.  1, together with CEL_OPT_HONOUR_MASK = 1: a masked set is accepted by exactly
                                 these calls, each under the exact conditional alone --
                                   cel_slice_sample, params 0, 1, 2 under CEL_OPT_SLICE_CONDITIONAL = 1: the per-round mass launch is the
                                     OBSERVED-mass kernel (k_stamp_mass_masked: the unit stamp over the unmasked pixels of the proposal's
                                     own box, bit for bit what cel_stamp_mass returns under CEL_OPT_HONOUR_MASK) on the same job list;
                                     the cover test, the likelihood launches and the launch count in `stats` are untouched (the masked
                                     split places no photon at a masked pixel);
                                   cel_slice_sample, param 3 and cel_patch_loglik_multi's resident mode 8, both under the
                                     exact gradient's key (CEL_OPT_GRAD_CONDITIONAL = 1): e and slots 7 + b come from the observed mass, slots 1-6 from its
                                     derivative (k_mass_grad_masked: k_mass_grad's sum over the observed pixels of the box alone; a pixel
                                     whose count is NaN is skipped before any arithmetic, so a box without a masked pixel gives
                                     k_mass_grad's bits and a box masked everywhere exact zeros).
                                 Still refused, in the words they always had: cel_slice_locations, the isolated forms, a row window
                                 and the reference's conditional (it charges the sum of the PSF weights, which is wrong beside a mask).
                                 On a set without a NaN the option changes nothing: the same kernels, launches and bits.  It only
                                 stores; cel_images_set_nelec drops the split a new mask invalidates.  Any other value:
                                 CEL_ERR_INVALID, the stored value unchanged */
    /* exact conditional: */ CEL_OPT_SLICE_CONDITIONAL = 18, /* what cel_slice_sample scores.  0 (default): the reference's conditional, as before: the same
                                 kernels, launches and bits.  1: the EXACT conditional of ModelGibbs(conditional="exact") (DESIGN Q20):
                                 a proposal of a chain with expected photons c_b scores  prior + (sum_b mode-0 likelihood + e),
                                 e = -sum_b (c_b * (mass_b - sum of the band's PSF weights)) * [the source has a sample patch in b],
                                 mass_b = the proposal's unit stamp summed over its OWN box (cel_stamp_mass's kernel), and -inf -- never
                                 rendered, counted in `evals` -- where in a band that holds a photon of the source the proposal has no
                                 stamp or its box does not contain the source's photon rectangle (cel_samples_photon_rects).  Per round
                                 the proposals' records are written WITH their boxes, then k_sg_cover, the likelihoods, the masses,
                                 k_sg_exact_terms; no further host synchronisation.  It applies to cel_slice_sample ALONE:
                                 cel_slice_locations does not read it and keeps its code, launches and bits -- the location step under
                                 the exact conditional is cel_slice_sample(param 0, dirs = NULL, step_out = 0).  Under 1 a masked set is
                                 refused as under 0 (unless CEL_OPT_SAMPLER_MASK admits it), and so is an image set with a row window (cel_images_set_window: the cover test
                                 is not window-relative).  Any other value: CEL_ERR_INVALID */
    /* exact gradient: */ CEL_OPT_GRAD_CONDITIONAL = 19, /* which conditional the RESIDENT GRADIENT differentiates.  0 (default): the reference's, as
                                 before: the same kernels, launches and bits, and every refusal of the exact conditional stands.  1: the
                                 EXACT conditional of ModelGibbs(conditional="exact") (the option above describes it), value and gradient.
                                 Exactly two calls read it.
                                 (a) cel_patch_loglik_multi's RESIDENT mode 8 (boxes = offsets = data = NULL, mode = 8).  The row of
                                 proposal p with owner s, v_ref / g_ref being the row under 0:
                                   slot 0      v_ref + e,  e = -sum_b (counts[p][b] * (mass_b - wsum_b)) * has_patch(s, b), added in band order
                                               from 0.0 without FMA contraction (k_sg_exact_terms), mass_b the mass kernel's value on the
                                               proposal's own box
                                   slots 1-6   g_ref[i] + ge[i],  ge[i] = -sum_b (counts[p][b] * d mass_b / d q_i) * has_patch(s, b), same order;
                                               the derivative is taken at the proposal's FIXED integer box (the box moves in jumps: between
                                               two jumps the sum's limits are constants), in cel_loglik_grad's units and conventions
                                   slot 7 + b  the reference's entry + -(mass_b - wsum_b) * has_patch(s, b)
                                 A proposal that fails the cover test (k_sg_cover's rule, see the option above) has slot 0 = -inf and
                                 slots 1 .. = 0; its jobs retire at their first instructions.  d mass_b / d q comes from k_mass_grad.h: the
                                 plain form -- every component at every pixel of the box, nothing dropped, neither CEL_OPT_TAIL_LOG_SOURCE
                                 nor CEL_OPT_KERNEL read, the same bits on every call -- followed by the gradient form's chain rule.
                                 The call then has the exact slice engine's preconditions: a masked set (unless CEL_OPT_SAMPLER_MASK admits it), a row window and a missing
                                 resident split are refused before any launch, ll_out untouched.  Mode 9, mode 10, explicit patches
                                 and cel_patch_loglik do not read the key.
                                 (b) cel_slice_sample(param = 3): the HMC step's v and g are the exact ones above (see there);
                                 CEL_OPT_SLICE_CONDITIONAL is not read by param 3 then.
                                 Any other value: CEL_ERR_INVALID, the stored value unchanged */
    CEL_OPT_TILE_PARTS = 13, /* how many one-wave blocks share a render tile of the general 32 x 64 kernel.  0 (default) = by
                               the frame's size: 4 for at most 512 tiles, 2 for at most 3 072, else 1 -- a frame of few tiles
                               (one rank's row strip of a field cut 8 ways, a 51 x 51 real field) finishes when its heaviest
                               tile does; with PARTS blocks per tile each takes every PARTS-th source of the tile's list and the
                               last to finish adds their accumulators in part order.  1 / 2 / 4 = always that many.  Values
                               agree to rounding between settings and are reproducible bit for bit under each */
    CEL_OPT_PROFILE = 3,   /* 1 = bracket every kernel launch with HIP events; 2 = the evaluating kernels only (render,
                              conditional likelihoods, split, mass, E-step: not the prep / binning / reduction launches
                              around a render -- an event pair costs the host ~10 us per launch); 3 = as 2 on a SAMPLE of
                              the launches, every fourth of a kernel (for steps of a few tens of microseconds)     */
    CEL_OPT_TILE_ORDER = 4,/* launch order of the render tiles; never changes results.  0 = index order,
                              1 (default) = heaviest first by the durations the tiles had in the previous
                              render of the same number of sources (the binning pass's estimate when there
                              is none), 2 = heaviest first by the estimate only                         */
    CEL_OPT_TILE_ROWS = 5, /* rows per render tile, 32 (default) or 64; read by cel_images_create  */
    CEL_OPT_TILE_TIMING = 6,/* diagnostic: 1 = k_render stamps every tile's start/end wall clock   */
    CEL_OPT_TILE_LAYOUT = 7,/* render tile geometry, read by cel_images_create:
                               0 = 64 columns x TILE_ROWS rows, one lane per column;
                               1 (default) = 32 columns x 64 rows, two component groups per column;
                               2 = 16 columns x 128 rows, four component groups per column (fewer
                               recurrence seeds, more per-tile set-up: measured 4 % slower than 1
                               on the benchmark field, kept for fields of tall narrow boxes)      */
    CEL_OPT_PHOTON_LISTS = 9, /* how the conditional likelihoods read a device-resident photon split: 0 (default) = per
                               patch, at the pixels that hold a photon or densely, whichever the layout pass estimates
                               cheaper; 1 = every patch at its photons; 2 = never (no lists are built).  The values
                               agree to rounding; set it before cel_photon_split.  4 and 5 = as 0 / as 1 for the value, AND
                               the resident gradient (cel_patch_loglik_multi's resident mode 8, cel_slice_sample's param 3)
                               sums at the photon lists (k_patch_grad_nz.h) instead of over the patches: the same terms in
                               another order, equal to rounding.  That bit is read when a gradient is launched; without
                               lists (a split made under 2) the dense kernel runs.  3, 6 and anything else is refused */
    CEL_OPT_STAR_TILES = 10,/* which kernel renders the field of a catalogue WITHOUT galaxies (known when the types
                               came from host memory): 0 = the general one (k_render_hw); 1 (default) = k_render_stars
                               -- the same 32 x 64 tiles taken in two column halves, 8 KB of accumulator instead of 16,
                               three waves per SIMD instead of two -- when the frame has more than 2048 tiles (the
                               general kernel's wave slots; fewer do not fill the extra waves), and for a catalogue of at
                               most 4096 stars on at most 2048 tiles (BASELINE configs[1]) ONE launch that prepares,
                               bins, renders and reduces (k_small_stars: every quarter of a tile's columns a wave of
                               its own, no tile lists); 2 = k_render_stars at any size; 3 = rule 1 without the
                               one-launch path.  Tile layout 1 and the row-recurrence only.  The two kernels add a pixel's stars in different orders: values
                               agree to rounding (1e-15), and which one runs depends on the call's inputs only */
    CEL_OPT_SPLIT_REUSE = 11,/* what a resident cel_photon_split takes from work already done.  1 = its totals image (every
                               pixel's rate under the split's strict boxes): when the model image of exactly these sources and
                               sky levels is on the device -- the chain's trace render came last -- it is formed from that image
                               by subtracting the sources' first box row and column (k_strict_totals: 0.35 ms instead of a
                               1.3 ms render at configs[4]).  The two agree to ~1e-10 of a pixel's rate on those pixels
                               (exactly elsewhere): equal in distribution, not photon for photon.  2 (default) = that, and the
                               two kernels also add up every unit stamp they evaluate, so that a cel_stamp_mass[_begin] of the
                               same catalogue right after the split reads the masses off those sums instead of evaluating
                               every stamp again (1.7 ms at configs[4]); galaxies fainter than a sixteenth of a sky pixel (counts <
                               eps / 16; stars: eps / 1024) still go through the mass kernel, and so does a stamp over the frame's
                               edge that leaves less than that ON the frame (counts * mass).  The sums carry the split's drop rule:
                               masses agree with the mass kernel's to 1e-11 eps / counts at most for a galaxy, 1.5e-13 eps / counts for
                               a star (measured; 1e-14 for a bright source): 1.6e-10 at the thresholds.  0 = totals always rendered from scratch, masses
                               always by the mass kernel */
    CEL_OPT_DEBUG = 8       /* diagnostics.  The shipped library accepts two result-preserving bits: 64 = the E-step
                               takes its per-source form, 128 = CEL_OPT_TILE_TIMING's third word carries the
                               row-waste counters of tools/row_waste.py.  The timing-only ABLATION bits (render:
                               1 = skip the star walk, 2 = the star seeds + walk, 4 = the epilogue's log, 8 =
                               everything after the tile header, 16 = the epilogue's global loads / stores, 32 =
                               every source; photon split: 1 = no draws, 2 = every draw 1, 4 = no stamp walk) exist
                               only in a -DCEL_ABLATE build (`make -C desi-mcmc_amd/csrc ablate`, loaded by
                               tools/ablate_render.py); the shipped library refuses them: CEL_ERR_INVALID */
};

/* kernels reported by cel_profile_get */
enum {
    CEL_K_PREP = 0, CEL_K_BIN = 1, CEL_K_RENDER = 2, CEL_K_REDUCE = 3, CEL_K_STAMPS = 4,
    CEL_K_GMM = 5,          /* the mixture builders: cel_mog_loglike, cel_galaxy_mixture_params, and k_comps (CEL_OPT_COMP_CACHE) */
    CEL_K_PATCH_LL = 6,     /* k_patch_ll[_hw]: cel_patch_loglik[_multi] and every round of cel_slice_locations */
    CEL_K_SPLIT = 7,        /* k_photon_split[_hw] */
    CEL_K_MASS = 8,         /* cel_stamp_mass */
    CEL_K_ESTEP = 9,        /* cel_estep_stats */
    CEL_K_RENDER_STARS = 10,/* k_render_stars: the field render of a catalogue without galaxies (CEL_OPT_STAR_TILES) */
    CEL_K_SMALL_STARS = 11,/* k_small_stars: a small star field's whole step in one launch (CEL_OPT_STAR_TILES = 1) */
    CEL_K_TOTALS = 12,     /* k_strict_totals: the photon split's totals image from the model image on the device (CEL_OPT_SPLIT_REUSE) */
    CEL_K_GRAD = 13,       /* k_grad_src + k_grad_chain: cel_loglik_grad */
    CEL_K_MASKED_LL = 14,  /* k_masked_ll: the Poisson term of a masked image set, a pass of its own behind the render */
    CEL_K_COUNT = 15
};

typedef struct cel_ctx cel_ctx;
typedef struct cel_images cel_images;
typedef struct cel_sources cel_sources;

/* One band image's parameters = the FitsImage fields the path reads
 * (CelestePy/fits_image.py:85-155).  37 doubles, no padding. */
typedef struct {
    double eps;        /* epsilon = SKY*GAIN                     fits_image.py:113 */
    double kappa;      /* GAIN                                   fits_image.py:112 */
    double calib;      /* CALIB, nmgy per count                  fits_image.py:116 */
    double w[3];       /* PSF mixture weights                    fits_image.py:129 */
    double mu[6];      /* PSF means, (x,y) per component         fits_image.py:130 */
    double cov[12];    /* PSF covariances, 2x2 per component     fits_image.py:135-137 */
    double rho[2];     /* CRPIX - 1                              fits_image.py:99  */
    double phi[2];     /* CRVAL                                  fits_image.py:100 */
    double ups[4];     /* CD matrix                              fits_image.py:101 */
    double ups_inv[4]; /* inv(CD)                                fits_image.py:103 */
    double R;          /* star bounding radius (error 1e-3)      fits_image.py:151-155;
                          <= 0: computed by the library with cel_bounding_radius */
} cel_band;

/* ---- library / context ------------------------------------------------------------- */
int cel_abi_version(void);
const char *cel_last_error(void);
int cel_device_count(int *n);

/* device: HIP ordinal.  stream: a hipStream_t to enqueue on (NULL = the library creates one). */
int cel_ctx_create(int device, void *stream, cel_ctx **out);
/* fails with CEL_ERR_INVALID (and destroys nothing) while image sets or source sets created on the context are alive: their own
 * destructors use the context's stream */
int cel_ctx_destroy(cel_ctx *ctx);
int cel_ctx_set_stream(cel_ctx *ctx, void *stream);
int cel_ctx_synchronize(cel_ctx *ctx);
int cel_ctx_set_option(cel_ctx *ctx, int key, double value);
int cel_ctx_get_option(cel_ctx *ctx, int key, double *value);

/* ---- images: B bands of one H x W field -------------------------------------------- */
/* Replaces constructing B FitsImage objects (fits_image.py:48-155) as far as the path reads them. */
int cel_images_create(cel_ctx *ctx, int B, int H, int W, const cel_band *bands, cel_images **out);
int cel_images_destroy(cel_images *img);
/* nelec: B*H*W observed electron counts, FitsImage.nelec (fits_image.py:86-93); stays on device.  The call also reduces the
 * image's range on the device (one pass, synchronous): images within 0 ... 65 535 let cel_photon_split keep its photons-left
 * plane in 16 bits (a seventh wave per CU); any other image takes the 32-bit instantiation, with the same draws.
 * MASKED PIXELS.  A NaN count marks a pixel that was not observed (FitsImage.invvar == 0: a saturated core, a cosmic-ray hit,
 * an interpolated column); a negative count is data.  The mask belongs to its band and there is no second plane: the NaNs in
 * the device's nelec ARE the mask, so row windows and cel_images_device_ptrs carry it.  The same pass counts them per band
 * (cel_images_mask_info); an image set with at least one is a MASKED set until the next cel_images_set_nelec.  On a masked
 * set a masked pixel contributes to no sum of cel_render_field's log-likelihood, cel_loglik_grad and cel_estep_stats (see
 * there); the calls that have not been taught about a mask -- cel_photon_split, the isolated forms of cel_patch_loglik[_multi]
 * and, for want of a split, cel_flux_conditionals and cel_slice_* -- refuse a masked set with CEL_ERR_INVALID before they
 * launch anything.  Everything that does not read nelec (stamps, boxes, masses, the mode 4 planes, which carry their own NaN
 * mask) is unchanged, and a set without a NaN takes exactly the code it took before there was a mask.
 * THE RESIDENT SPLIT.  New pixels drop the resident photon split, which was drawn from the old ones: after this call
 * cel_samples_info reports S = 0, cel_stamp_mass_ready answers 0, and cel_flux_conditionals, cel_slice_locations, cel_slice_sample,
 * the resident forms of cel_patch_loglik_multi, cel_samples_fetch, cel_samples_photon_rects and cel_slice_sample's moments (param 10) fail with CEL_ERR_INVALID, naming
 * the missing split, until the next resident cel_photon_split (on a masked set the masked refusal above comes first).  Pixels
 * written in place through cel_images_device_ptrs are the caller's business, as that call says. */
int cel_images_set_nelec(cel_images *img, const double *nelec, int mem);
/* masked[b] = the number of NaN (masked) pixels of band b that the last cel_images_set_nelec found (0 before the first) */
int cel_images_mask_info(cel_images *img, int64_t *masked /* B */);
/* Gibbs resamples the sky level (models.py:156-160) */
int cel_images_set_epsilon(cel_images *img, int band, double eps);
/* Declare that this image set holds rows [y0, y0 + H) of a full_H-row frame (row-strip partition
 * of one field across GPUs).  Source boxes and the overlap test are formed against
 * the full frame (celeste.py:130-140) and then cut to the window, so the strips tile the frame's
 * model image exactly.  WCS (rho) stays that of the full frame.
 * ANOTHER window than the set has drops what was cut to the old one: records, boxes, tile lists, the model image, and the
 * RESIDENT SPLIT, whose patches are boxes of the old window -- cel_samples_info reports S = 0, cel_stamp_mass_ready answers 0,
 * the calls that need the split fail with CEL_ERR_INVALID naming the missing split (as after cel_images_set_nelec) and a pending
 * cel_stamp_mass_begin is refused by its _end, until the next resident cel_photon_split.  Set the window when the set is
 * created, before the first split.  The same (y0, full_H) again changes nothing and drops nothing. */
int cel_images_set_window(cel_images *img, int y0, int full_H);
/* The rows [y0, y1) of THIS image set (window-relative) that it OWNS; default: every row.  cel_photon_split's noise sums count
 * the left-over photons of these rows only, and cel_render_field's log-likelihood adds the Poisson terms of these rows only
 * (they must then begin and end on render-tile rows, 64 in the default layout; the model image is rendered on every row).  One Gibbs chain partitioned over GPUs by row strips ("the photon split ... uses the same spatial
 * partition"): a rank's image set holds its strip plus a halo as tall as its own sources' boxes reach, so that their sample
 * patches are complete; the sky photons of the halo rows belong to the neighbours' sums (Field.resample_photons,
 * CelestePy/models.py:155-160, needs the frame's total: the ranks all-reduce their strips' sums). */
int cel_images_set_noise_rows(cel_images *img, int y0, int y1);
int cel_images_get_band(cel_images *img, int band, cel_band *out);
/* copy the last rendered model images (B*H*W) out */
int cel_images_get_lambda(cel_images *img, double *out, int mem);
/* raw device pointers of the library-owned B*H*W buffers (for zero-copy consumers).  Asking for `nelec` tells the library that
 * the caller may write the observed image in place: it stops assuming the range cel_images_set_nelec found (the photon split's
 * 16-bit photons-left plane) until the next cel_images_set_nelec, and from then on keeps no per-tile Poisson sums between
 * renders (CEL_OPT_INCREMENTAL renders every tile when a log-likelihood is asked for).  nelec = NULL asks for neither.
 * The mask state (cel_images_set_nelec) is taken when cel_images_set_nelec runs: a caller who writes pixels through this pointer
 * must neither create nor remove NaNs.  A resident photon split stays the split of the pixels it was drawn from: handing the
 * address out drops none (the library cannot know when the caller writes), and cel_images_set_nelec is how a caller announces
 * new pixels */
int cel_images_device_ptrs(cel_images *img, void **nelec, void **lambda);
/* device pointer of the B per-band log-likelihoods of the LAST render with CEL_RENDER_LOGLIK (doubles, valid until the next
 * render, photon split or E-step call on this image set -- they reduce into the same buffer; the stream has been synchronised
 * when the render returned): what a multi-GPU caller hands to
 * its all-reduce without a trip through host memory (the one collective of the path). */
int cel_images_loglik_device(cel_images *img, void **ll_band);

/* ---- sources ------------------------------------------------------------------------ */
/* Replaces a python list of SrcParams (celeste_src.py:57-94) as far as the path reads them:
 *   type[s]   0 star, 1 galaxy (SrcParams.a);
 *             2 = a galaxy on the older per-profile route, gen_galaxy_prof_psf_image
 *             (celeste_galaxy_conditionals.py:134-182): shape[s] = theta, W00, W01, W11 with
 *             W = R R^T as the caller formed it (:151, R from the constant img.Ups_n, :33);
 *             theta = 1 / 0 is the 'exp' / 'dev' profile alone; its box is the int() box of
 *             :166-167 from the bounding radius (ERROR 1e-5) of the components that carry weight
 *   radec[s]  (ra, dec) degrees (SrcParams.u)
 *   counts[s*B + b] expected photons of source s in band b -- the multiplier that
 *             gen_src_image applies (celeste.py:35-62; the caller picks the flux convention)
 *   shape[s]  theta, sigma (arcsec), phi (DEGREES, celeste_galaxy_conditionals.py:97), rho */
int cel_sources_create(cel_ctx *ctx, int64_t capacity, int B, cel_sources **out);
int cel_sources_destroy(cel_sources *src);
int cel_sources_set(cel_sources *src, int64_t S, const int32_t *type, const double *radec,
                    const double *counts, const double *shape, int mem);
/* Replace n rows of the catalogue (host arrays, packed row-major as above; idx[i] = the row that packed row i goes to).
 * What a caller that changed ONE source between two evaluations uploads -- the slice steps and RJ moves of
 * CelestePy/util/infer/mcmc_transitions.py:37-152 call celeste_likelihood(list of SrcParams) after every such change. */
int cel_sources_set_rows(cel_sources *src, int64_t n, const int32_t *idx, const int32_t *type, const double *radec,
                         const double *counts, const double *shape);
/* The catalogue as the device holds it now, to host arrays laid out as cel_sources_set takes them (any may be NULL).  The
 * device samplers rewrite it in place -- cel_flux_conditionals the counts of the sources that have a patch, the slice samplers
 * the locations and shapes -- and this reads back what they left. */
int cel_sources_get(cel_sources *src, int32_t *type, double *radec, double *counts, double *shape);

/* ---- the hot path --------------------------------------------------------------------- */
/* gen_model_image (celeste.py:203-219) for every band + celeste_likelihood /
 * celeste_likelihood_multi_image (celeste.py:237-252), fused.  Galaxies are accumulated by
 * their own patches (models.py:88-108 semantics).
 *   lambda[b] = eps_b + sum_s counts[s][b] * unit_stamp(s, b)     (kept on device)
 *   ll_band[b] = sum_{y,x} nelec*log(lambda) - lambda              (host, B doubles, may be NULL)
 *   ll_total   = sum_b ll_band[b]                                  (host, may be NULL)
 * Synchronises the stream when ll_band or ll_total is non-NULL.
 * On a MASKED image set (a NaN in nelec, cel_images_set_nelec) the model image is unchanged, bit for bit, and
 *   ll_band[b] = sum over the UNMASKED pixels of nelec*log(lambda) - lambda   (a band masked everywhere: 0)
 * formed by a pass of its own behind the render (CEL_K_MASKED_LL); cel_images_loglik_device holds the same values.  That pass
 * reads the stored image: CEL_RENDER_NO_STORE with CEL_RENDER_LOGLIK stores the image anyway on a masked set, and
 * CEL_OPT_INCREMENTAL renders the dirty tiles' pixels only but forms every tile's Poisson partial again.  Either way the
 * values are those of a full, storing render, bit for bit. */
int cel_render_field(cel_images *img, cel_sources *src, int flags, double *ll_band, double *ll_total);
/* work counters of the last cel_render_field: n_srcpix = sum of box areas (source-pixel
 * evaluations), n_gauss = sum of K*area, n_tile_entries = length of the tile lists */
int cel_field_stats(cel_images *img, double *n_srcpix, double *n_gauss, double *n_tile_entries);
/* diagnostic (CEL_OPT_TILE_TIMING): per render TILE i in [band][tile row][tile column] order -- whatever position the tile
 * order gave its block in the launch -- out[3i] = start, out[3i+1] = end (100 MHz wall clock ticks), out[3i+2] = packed work
 * counters (32x64 / 16x128 layouts: list length | pairs of groups << 12 | kept component-rows << 32; 64x32 layout:
 * (tile index << 32) | list length).  out == NULL: only *n_tiles is returned.  Never enabled in a timed run. */
/* the totals image the last cel_photon_split on the recurrence kernels drew from (every pixel's rate under the split's
 * strict boxes), B*H*W doubles to host memory: what the tests compare between the two ways of forming it (CEL_OPT_SPLIT_REUSE) */
int cel_debug_split_rates(cel_images *img, double *out);
int cel_debug_tile_timing(cel_images *img, uint64_t *out, int64_t *n_tiles);
/* diagnostic: how the last cel_render_field of this image set rendered -- *dirty_tiles = -1: every tile; >= 0: incrementally
 * (CEL_OPT_INCREMENTAL), that many tiles: those touched by the boxes of the rows cel_sources_set_rows changed since the
 * image set's previous render of the same catalogue.  What the tests use to know which path ran; replaces nothing in the
 * reference (its gen_model_image re-renders every source on every call, CelestePy/celeste.py:203-219). */
int cel_debug_last_render(cel_images *img, int64_t *dirty_tiles);

/* ---- stamps --------------------------------------------------------------------------- */
/* gen_point_source_psf_image (celeste.py:114-176) / gen_galaxy_psf_image
 * (celeste_galaxy_conditionals.py:185-214) for every source of `src` in one band.
 * Step 1: boxes[s*4..] = y0, y1, x0, x1 and status[s]: 1 = has a stamp, 0 = the box is empty,
 *         -1 = the reference's overlap test fails and it returns (None, None, None)
 *         (celeste.py:130-135) whatever limits the caller imposes.  Host arrays.
 * Step 2: the caller sizes a packed buffer (offsets[s+1]-offsets[s] = box area, or the area of
 *         the caller-imposed box in boxes_in) and the stamps are written into it, row-major.
 *   scaled: 0 = unit flux, 1 = multiplied by counts[s][band] (gen_src_image_with_fluxes,
 *           celeste.py:84-96)
 *           2, 3 = DERIVATIVE STAMPS of the unit (2) / counts-scaled (3) stamp: the slot of a source holds several planes of
 *           the box's size, packed row-major one after another, and offsets[s+1]-offsets[s] = planes * area (checked before
 *           anything is launched or written, as mode 4 of cel_patch_loglik checks its two planes):
 *             plane 0     the stamp itself
 *             plane 1, 2  d / d ra, d / d dec, per degree
 *             plane 3-6   galaxies only: d / d of the four shape coordinates cel_sources_set takes -- theta, sigma
 *                         [arcsec], phi [degrees], rho for type 1; theta, W00, W01, W11 for type 2
 *           so a star's slot holds 3 planes and a galaxy's 7.  Units and conventions are cel_loglik_grad's: the integer box
 *           is held fixed; ra / dec act through equa2pixel and, for type 1, through cd_at_pixel's cos(dec) term in W;
 *           d / d sigma is 0 where the floor max(1/30, sigma) holds; d / d theta keeps both profiles.  Contracted with
 *           r = nelec / lambda - 1 over the boxes and summed over the bands, the scaled = 3 planes are cel_loglik_grad's
 *           g_radec / g_shape and plane 0 of scaled = 2 is g_counts.  Nothing is dropped: every component is evaluated at
 *           every pixel of the box and CEL_OPT_TAIL_LOG[_SOURCE] is not read (a derivative can vanish where the value does
 *           not, so a rule relative to the pixel's value bounds nothing); CEL_OPT_KERNEL 0 and 1 take the same kernel
 *           (k_stamp_jac.h) and give the same bits.  A source without a stamp has its whole slot, every plane, zero-filled.
 *           Any other value is CEL_ERR_INVALID.  (Before the derivative stamps every non-zero value meant "scaled"; that
 *           was never documented, and only 0 and 1 keep their meaning.)
 *   boxes_in: NULL = each source's own box; else S*4 caller limits (xlim/ylim arguments of
 *           celeste.py:145-152); a source with an empty box is skipped. */
int cel_stamp_boxes(cel_images *img, cel_sources *src, int band, int32_t *boxes, int32_t *status);
int cel_render_stamps(cel_images *img, cel_sources *src, int band, int scaled, const int32_t *boxes_in,
                      const int64_t *offsets, double *out, int mem);

/* ---- per-source conditional log-likelihoods --------------------------------------------- */
/* Source.log_likelihood (CelestePy/sources.py:134-183) and Source.log_likelihood_isolated
 * (:188-237) for a batch of P parameter proposals of ONE source -- what slice sampling / HMC
 * call 10-50 times per source per sweep (sources.py:308-319).
 *   src      P proposals (type, radec, counts[B], shape), usually one coordinate varied
 *   boxes    B*4 ints: the fixed limits y0,y1,x0,x1 of the source's sample patch per band
 *            (samp_img.y0/y1/x0/x1); an empty box = no sample image in that band
 *   offsets  B+1: packed position of each band's patch data; offsets[b+1]-offsets[b] = box area
 *   data     patch values, row-major per band: photons attributed to the source (mode 0) or
 *            the observed nelec patch (mode 1); `mem` says host or device
 *   mode 0   ll = sum_b [ sum_{m>0} log(m) z - counts_b sum(psf weights_b) ],  m = counts_b * stamp
 *            (a star failing the overlap test contributes -counts_b sum(weights_b), :160-163)
 *   mode 1   ll = sum_b [ sum log(m + eps_b) z - sum (m + eps_b) ]
 *   mode 2   ll = sum_b [ sum_{m>0} log(m) z - sum m ]   -- galaxy_source_like
 *            (celeste_galaxy_conditionals.py:15-42) on given limits
 *   mode 4   ll = sum_b [ sum_{z unmasked, m+bg>0} log(m + bg) z - (m + bg) ]   -- poisson_loglike of the observed box
 *            against background + model, the image_like closure of the star <-> galaxy move
 *            (CelestePy/sources.py:6-12,277-291).  Each band's patch data is TWO planes, z then bg
 *            (offsets[b+1]-offsets[b] = 2 x box area); a NaN z marks a masked pixel (invvar == 0); negative counts are data
 *   ll_out   P doubles (host)
 *
 *   mode 8 + m, m in {0, 1, 2}  -- CEL_PLL_GRAD = 8, a value of `mode` and no enumerator: THE GRADIENT FORM of mode m.  Boxes,
 *            offsets (ONE plane per band, as in
 *            mode m: offsets sized for 7 + B planes are refused), data, mem, owner, NB and the resident form (m = 0 or 1)
 *            keep their meaning; ONLY THE SIZE OF ll_out CHANGES:
 *   ll_out   P * (7 + B) doubles (host).  Per proposal p, at ll_out + p * (7 + B):
 *              0        the value the same call with mode = m returns, bit for bit (that path is run)
 *              1, 2     d / d ra, d / d dec, per degree
 *              3 .. 6   type 1: d / d (theta, sigma [arcsec], phi [degrees], rho); type 2: d / d (theta, W00, W01, W11);
 *                       stars: zeros
 *              7 + b    d / d counts[p][b]
 *            Slots 1 .. 6 are summed over the bands in band order.  The gradient is that of the value documented for mode m
 *            on the FIXED patch limits (no integer box of the source enters).  With u the unit stamp, m(pix) = counts_b u(pix)
 *            and dq = d u / d q, a location or shape entry is sum_b counts_b sum_pix r dq and the counts entry sum_pix r u, with
 *              m = 0:  r = z / m where m > 0, else 0; the counts entry gets a further - sum(psf weights_b)
 *              m = 1:  r = z / (m + eps_b) - 1
 *              m = 2:  r = z / m - 1 where m > 0, else 0
 *            (a pixel with m == 0 adds nothing: no 0 / 0, every output finite whenever the value is).  Conventions are
 *            cel_loglik_grad's: ra / dec act through equa2pixel and, for type 1, through cd_at_pixel's cos(dec) term in W;
 *            d / d sigma is 0 where the floor max(1/30, sigma) holds; d / d theta keeps both profiles.  A band with an empty
 *            patch contributes nothing; a source whose own box is empty still renders its kind, and its derivatives, on the
 *            imposed limits; an overlap-test miss contributes only - sum(psf weights_b) to its counts entry for m = 0 and
 *            renders as a star for m = 1, 2, as the value does.
 *            Slot 0 and slots 1 .. differ by the drop rule: slot 0 carries whatever rule mode m applies under
 *            CEL_OPT_TAIL_LOG[_SOURCE] and CEL_OPT_KERNEL; the gradient kernel (k_patch_grad.h) reads neither option, drops
 *            nothing (every component at every pixel) and gives the same bits under CEL_OPT_KERNEL 0 and 1 and on every call.
 *            Refused with CEL_ERR_INVALID before anything is launched or written: whatever mode m refuses for the same
 *            arguments; 8 + 3, 8 + 4 and any other value; an image set with a row window (cel_images_set_window), as
 *            cel_loglik_grad refuses it.  The launches are timed under CEL_K_PATCH_LL.
 *            Under CEL_OPT_PHOTON_LISTS = 4 or 5 cel_patch_loglik_multi's RESIDENT mode 8 takes slots 1 .. at the split's photon
 *            lists (k_patch_grad_nz.h: the same sums in another order, nothing dropped, the same bits under CEL_OPT_KERNEL 0 and 1
 *            and on every call); explicit patches, modes 9 and 10 and cel_patch_loglik keep the dense kernel. */
int cel_patch_loglik(cel_images *img, cel_sources *src, const int32_t *boxes, const int64_t *offsets,
                     const double *data, int mem, int mode, double *ll_out);
/* The same for proposals of MANY sources in one launch (a whole sweep of per-source updates):
 * NB patch sets (boxes NB*B*4, offsets NB*B+1, index set*B + band) and owner[p] = the patch set
 * proposal p is scored on (the source it is a proposal for).
 * RESIDENT form: boxes = offsets = data = NULL and NB = the S of the last resident
 * cel_photon_split: mode 0 scores against that split's device-resident sample patches, mode 1
 * against the observed image on the same boxes -- nothing crosses PCIe but the proposals. */
int cel_patch_loglik_multi(cel_images *img, cel_sources *src, const int32_t *owner, int64_t NB,
                           const int32_t *boxes, const int64_t *offsets, const double *data, int mem, int mode,
                           double *ll_out);

/* n standard Gamma(a[i]) variates, element i from its own counter-based streams keyed by (seed, i): the flux conditionals'
 * draws of Source.resample_fluxes (CelestePy/sources.py:341-345) for a whole catalogue (celeste_mcmc.gamma_by_stream is the
 * host form: the same streams and decisions, values equal to rounding).  Host arrays. */
int cel_gamma_streams(cel_ctx *ctx, int64_t n, const double *a, uint64_t seed, double *out);
/* Sum of every source's UNIT stamp over its own box, in every band: mass[s*B + b] -- what
 * Source.resample_fluxes multiplies by kappa/calib for the rate of its Gamma conditional
 * (CelestePy/sources.py:336-339) and celeste_em's sum_fs (celeste_em.py:89).  0 without a stamp.  Host output.
 * Right after a resident cel_photon_split of the same catalogue that took its totals from the model image on the device
 * (CEL_OPT_SPLIT_REUSE = 2) the values are read off the sums that split made (see the option); cel_stamp_mass_ready says
 * whether this call would: a caller that could also ask for a part of the catalogue only (a rank of a dealt chain) then asks
 * for the whole, which costs nothing and gives every rank the numbers the single-rank chain has.  The sums carry the drop rule of
 * the split that made them: they serve while the per-source threshold (CEL_OPT_TAIL_LOG / CEL_OPT_TAIL_LOG_SOURCE) is the one
 * that split ran at; under another one cel_stamp_mass_ready answers 0 and cel_stamp_mass / _begin run the mass kernel. */
int cel_stamp_mass(cel_images *img, cel_sources *src, double *mass);
int cel_stamp_mass_ready(cel_images *img, cel_sources *src, int *ready);
/* The same in two halves: _begin queues the kernel and returns, _end waits and copies the S*B values out -- so that the host
 * can draw its Gamma variates while the device sums the stamps (the flux step of a Gibbs sweep) without a second thread.
 * Between the two, calls that touch neither the catalogue, the source records nor the photon split may run on this context
 * (cel_gamma_streams, cel_samples_fetch, cel_images_set_epsilon: what ModelGibbs does there); _end fails with
 * CEL_ERR_INVALID when the source records or the photon split were rebuilt in between -- by a device sampler, by a render or a
 * stamp call of another catalogue or generation, by any cel_photon_split -- whether or not _begin took the split's short cut. */
int cel_stamp_mass_begin(cel_images *img, cel_sources *src);
int cel_stamp_mass_end(cel_images *img, double *mass);
/* Source.resample_fluxes (CelestePy/sources.py:321-349) for every source of a catalogue whose resident photon split is on the
 * device, without a host round trip (round 6): element (s, L) of flux_new[S][5] (L = band letter u g r i z) =
 *     Gamma(a0 + photons of s in the images of letter L) / (b0 + sum over those images of mass(s, image) * kappa / calib),
 * the Gamma variate from element s * 5 + L's own streams (cel_gamma_streams' sampler), the masses cel_stamp_mass's (short cut
 * and leftovers alike), every operation in the order celeste_mcmc.ModelGibbs.resample_fluxes takes on the host: the same bits.
 * band_letter[b] in 0..4 names image b's letter; calib / kappa per image.  active[s] = 1 when the source has a sample patch in
 * some image: only those sources' expected counts (flux / calib * kappa) are rewritten in the catalogue's device array -- the
 * caller keeps the old flux of the others, as the reference leaves a source without a patch alone (sources.py:243). */
int cel_flux_conditionals(cel_images *img, cel_sources *src, uint64_t seed, double a0, double b0, const int32_t *band_letter,
                          const double *calib, const double *kappa, double *flux_new, int32_t *active);

/* Source.resample_location (CelestePy/sources.py:308-319) for EVERY source of `src` at once: slicesample
 * (CelestePy/util/infer/slicesample.py:89-227) with the options of that call -- component-wise, no stepping
 * out, interval width sigma (degrees) -- run as a lock-step state machine on the device against the
 * resident photon split of exactly these sources (cel_photon_split with offsets = NULL): every round each
 * unfinished chain's next point is scored by the conditional-likelihood kernel (mode 0 of
 * cel_patch_loglik_multi, resident form) and the chains advance; rounds are queued four at a time and
 * four counters (chains running, error bits, evaluations, rounds that had work) cross PCIe per batch.
 * A source without any sample patch is left where it is, and so is one with chain_ids[s] < 0 (when ONE
 * chain is dealt over several GPUs each rank updates only its own sources and the ranks exchange the
 * new locations afterwards).  Random numbers: one SplitMix64 stream per
 * chain keyed by (seed, chain_ids[s] or s), in the reference's draw order -- the same streams and
 * arithmetic as the host engine of the Python mirror (util/infer/slicesample.py), chain for chain.
 *   radec_out  S*2 (host, may be NULL): the new locations; they also REPLACE src's locations on the device
 *   llh_out    S (host, may be NULL): log-likelihood at the new location (NaN for a source left alone)
 *   stats      4 (host, may be NULL): rounds, likelihood evaluations, the ALGORITHMIC HBM bytes those evaluations
 *              read (per evaluation and band: 4 B per pixel of the photon rectangle it walks + one 128-B
 *              record), conditional-likelihood launches */
int cel_slice_locations(cel_images *img, cel_sources *src, const int32_t *chain_ids, double sigma, uint64_t seed,
                        int max_rounds, double *radec_out, double *llh_out, int64_t *stats);

/* slicesample (CelestePy/util/infer/slicesample.py:89-227) with the options cel_slice_locations does not run -- random
 * directions and stepping out by doubling with the `acceptable` test -- over every source's location (param 0: D = 2) or
 * every GALAXY's shape (param 1: D = 4: theta, sigma, phi, rho; the call of CelestePy/celeste_mcmc.py:229-239,
 * slice_sample_skew), as a lock-step state machine on the device against the resident photon split of exactly these
 * sources.  Every round each unfinished chain's next one or two points are scored (mode 0 of cel_patch_loglik_multi,
 * resident form) and the chains advance.  Same per-chain SplitMix64 streams, draw order and arithmetic as the host engine
 * of the Python mirror (util/infer/slicesample.py), chain for chain.
 *   dirs       S*numdir*D (host): the chains' random unit directions, drawn by the caller (the mirror draws them from each
 *              chain's normal stream); NULL = component-wise, the axes in each chain's own random order (numdir ignored)
 *   step_out   0 = none, 1 = doubling (at most max_steps_out doublings per direction)
 *   phi_max    param 1: log-prior galaxy_shape_prior_constrained (celeste_galaxy_conditionals.py:268-275) with this bound on
 *              phi is added to the conditional likelihood; a point outside its support scores -inf and is never rendered.
 *              <= 0: no prior.  (Any other prior: the host engine.)
 *   chain_ids  as cel_slice_locations; a star is left alone under param 1
 *   x_out      S*D (host, may be NULL): the new states; they also REPLACE src's on the device.  llh_out, stats: as
 *              cel_slice_locations (stats[2] = 0)
 * CEL_OPT_SLICE_CONDITIONAL = 1: the exact conditional in place of the reference's (see the option).
 *
 * param 2: the star <-> galaxy move (Source.resample_type, CelestePy/sources.py:247-306) for every source at once: ONE
 * Metropolis-Hastings proposal per chain against the resident split -- given the photon split a source's conditional involves
 * no other source, so all sources move in one call, exactly.  A chain's current row and the row with the type flipped are
 * scored as params 0 and 1 score a slot (the bands' mode-0 values added in band order from 0.0, plus the exact conditional's
 * term and cover test under CEL_OPT_SLICE_CONDITIONAL = 1);  log alpha = (score(proposal) - score(current)) + h,  accepted
 * iff log(u) < log alpha with u the FIRST uniform of the chain's SplitMix64 stream keyed by (seed, chain id).  The arguments
 * are re-read:
 *   dirs       S*5 (host, required; numdir must be 1): per chain (theta, sigma, phi, rho, h).  The shape is the galaxy proposed
 *              for a chain that is a star now (ignored for a galaxy: its proposal is the star at the same location with the
 *              same expected counts); a shape outside theta in (0,1), sigma > 0, rho in (0,1) is never rendered and is
 *              rejected, and counts as an evaluation.  h is the caller's term of the log acceptance ratio of the move the chain
 *              would make -- prior odds, proposal densities, Jacobian: everything that is not the likelihood (the reference's
 *              proposal_fun seam).  It must be finite for every chain with chain_ids[s] >= 0 (CEL_ERR_INVALID otherwise,
 *              before any launch)
 *   chain_ids  as above; a source without a sample patch in any band and a source of type 2 are left alone too: their rows
 *              stay bit for bit
 *   step_out, max_steps_out, phi_max, max_rounds: not read; sigma: not read, but must be > 0
 *   x_out      S*5 (host, may be NULL): the new type as a double, then the new shape.  An accepted row REPLACES src's type and
 *              shape on the device (a galaxy turned star keeps its shape row's bits); locations and counts are untouched
 *   llh_out    S (host, may be NULL): log alpha, NaN for a chain left alone
 *   stats      {1, scored slots (two per running chain), accepted moves, likelihood launches}
 * A proposal the cover test refuses scores -inf and is rejected.  A running chain whose CURRENT row scores -inf (it cannot
 * after a full-box split) stays where it is and the call returns CEL_ERR_INVALID behind the other chains' moves.  The same
 * refusals as params 0 and 1: a masked set, no resident split of these sources, under the exact conditional a row window.
 *
 * param 3: one HMC update (hmc_sample_galaxy_params, CelestePy/celeste_mcmc.py:281-331: util/infer/hmc.py's leapfrog with
 * num_iter = 1) of every source's location and shape at once, q = (ra, dec, theta, sigma, phi, rho) with ra and dec in degrees;
 * a star moves in (ra, dec) only.  The counts are held fixed: their conditional is a Gamma, which cel_flux_conditionals samples
 * exactly -- HMC on it would be strictly worse.  The target v(q) is the score params 0-2 form under the reference's conditional
 * (the bands' resident mode-0 values added in band order from 0.0, a band's parts first; for a galaxy under phi_max > 0 plus
 * the log-prior of param 1); its gradient g(q) is slots 1-6 of cel_patch_loglik_multi's mode-8 row of the proposal, the prior's
 * derivative 2 / sigma^3 - 4 / sigma added to the sigma entry; a star's entries 2-5 are 0.  Every chain's whole trajectory is
 * queued on the stream, the gradients never leave the device, and there is one readback at the end:
 *     p = p0 + (0.5 eps) g(q0)
 *     for l in 0 .. L-1:   q = q + (eps imass) p;   p = p + (l == L-1 ? 0.5 eps : eps) g(q)
 *     K(p) = 0.5 sum_i imass_i (p_i p_i)                  (added in coordinate order from 0.0)
 *     log alpha = (v(qL) - v(q0)) + (K(p0) - K(pL));      accepted iff log(u) < log alpha
 * with u the FIRST uniform of the chain's SplitMix64 stream keyed by (seed, chain id), as param 2 forms it.  Support: theta in
 * (0,1), sigma > 0, rho in (0,1) always, phi in (0, phi_max) when phi_max > 0.  A trajectory with a position outside the support,
 * or a position or gradient entry that is not finite, is dead: it is never rendered again and is rejected with log alpha = -inf.
 * The arguments are re-read:
 *   dirs       S*12 (host, required; numdir must be 12): per chain the momentum p0[6], then the inverse mass imass[6] (>= 0 and
 *              finite; 0 freezes that coordinate).  A star's entries 2-5 are ignored.  A p0 that is not finite, or an imass
 *              that is negative or not finite, in an entry that a star or galaxy with chain_ids[s] >= 0 reads gives
 *              CEL_ERR_INVALID before any launch
 *   sigma      the step size eps > 0;  max_rounds: the leapfrog steps L, 1 <= L <= 1024;  phi_max: as param 1
 *   chain_ids  as above; a source without a sample patch in any band and a source of type 2 are left alone too: their rows
 *              stay bit for bit
 *   step_out, max_steps_out: not read
 *   x_out      S*12 (host, may be NULL): the new q, then the momentum to carry on with: pL on accept, -p0 on reject (the
 *              reference's negate, accept, negate); a chain left alone: its row and its p0.  An accepted row REPLACES src's
 *              location and (a galaxy's) shape on the device; types and counts are untouched
 *   llh_out    S (host, may be NULL): log alpha, NaN for a chain left alone
 *   stats      {L, gradient evaluations (L + 1 per chain that runs to the end), accepted updates, launches}
 * A running chain whose CURRENT row scores -inf stays where it is and the call returns CEL_ERR_INVALID behind the other chains'
 * moves.  Refused before any launch, the outputs untouched: what params 0-2 refuse; an image set with a row window (the gradient
 * form refuses it); CEL_OPT_SLICE_CONDITIONAL = 1 (the exact conditional's stamp-mass term has no analytic derivative yet).
 * Under CEL_OPT_PHOTON_LISTS = 4 or 5 the L + 1 gradients are taken at the split's photon lists, as the resident mode 8 takes them
 * then: g(q) is still that call's row bit for bit, and the launch count does not change.
 * CEL_OPT_GRAD_CONDITIONAL = 1: v and g are the EXACT conditional's -- v = prior + (the mode-0 values + e), g = slots 1-6 of the
 * resident mode-8 row under that option, bit for bit.  Each of the L + 1 gradient evaluations writes the proposals' records WITH
 * their boxes, then runs the cover test (k_sg_cover + k_hmc_cover), the likelihood gradient by whichever route
 * CEL_OPT_PHOTON_LISTS selects, the mass kernel, k_mass_grad, the chain rule on its sums and k_mass_grad_apply.  A trajectory that
 * reaches a point whose box does not cover the source's photons is dead (owner = -1, log alpha = -inf), exactly like one that
 * leaves the support; the evaluation that found it is counted.  The two slots scored at the end get their cover test and their e.
 * A chain whose CURRENT row already fails the cover test does not run: it is reported as a chain left alone (its row, its p0,
 * log alpha NaN, no evaluation).  The force is a function of q alone, so the leapfrog with this piecewise force is still a
 * reversible, volume-preserving map and the Metropolis test keeps the update exact across the jumps of v at a change of the
 * integer box.  No further host synchronisation.  Launches (stats[3]), with J = 1 under CEL_OPT_KERNEL = 1 (the job lists) else 0
 * and V = the value launches of the two scored slots (1 or 2):
 *     reference's conditional:  1 + J + 3 (L + 1) + L + 2 + V + 1
 *     exact conditional:        1 + J + 9 (L + 1) + L + 3 + V + 2 + 1
 * Refused as under 0, and a masked set, a row window and a missing split as params 0-2 refuse them.
 *
 * param CEL_SLICE_MOMENTS (10 = 8 + 2, as mode 8 + m of cel_patch_loglik is the gradient of mode m): no sampler runs -- the
 * STATISTIC a data-driven proposal of the type move (param 2) conditions on, the moments of every source's photons in the
 * resident photon split, reduced on the device (k_moments.h; celeste_mcmc.MomentProposal).  It enters as a new value of an
 * existing argument, as the type move and the HMC step did: no new symbol.  Per (source, band),
 *   stats[(s*B+b)*6 ..] = N, Sx, Sy, Sxx, Sxy, Syy = sum over the patch's pixels of z, z dx, z dy, z dx dx, z dx dy, z dy dy,
 * z the photons the split gave s at that pixel, dx = x - x0, dy = y - y0 from the low corner of the patch's box as
 * cel_samples_fetch reports it.  All zeros without a patch.  int64, EXACT (integer sums, any order) while they fit.
 *   stats    S*B*6 int64 (host), S from cel_samples_info -- NOT the four counters of the other params
 *   src      the catalogue of the split, or NULL (the split's own S is taken); every other argument is ignored and may be 0 / NULL
 * RANGE.  Every sum must stay below 2^63: sum over a patch of z d^2 < 2^63.  With int32 samples and boxes of at most 2^12 pixels
 * a side one pixel's term is below 2^31 * 2^24 = 2^55, so 2^8 such pixels fit whatever they hold -- and a patch whose photons
 * number below 2^39 fits whatever its pixels.  Not checked on the device.
 * ROUTES.  Where the split's photon lists stand, a patch is summed at its list or over its dense pixels as the conditional
 * likelihoods read it (CEL_OPT_PHOTON_LISTS, CEL_OPT_KERNEL); the integers are the same.  A patch of more than
 * CEL_MOMENTS_SPLIT_PIXELS pixels is dealt to several blocks that add with 64-bit integer atomics: invisible in the result.
 * STATE.  Reads the split and writes only `stats`: no cached state of the set changes, the catalogue is not touched, and a call
 * between a split and a sampler, the flux step or a resident likelihood leaves their results bit for bit.
 * Fails with CEL_ERR_INVALID, before any launch and with `stats` untouched, when the set holds no resident photon split of these
 * sources (none yet, or dropped by cel_images_set_nelec or a new window).  A masked set and a row window are NOT refused here: a
 * masked set holds a split only while CEL_OPT_HONOUR_MASK is on; that split puts no photon on a masked pixel, so none
 * contributes.  Every other value of param outside 0-3 is refused. */
enum {
    CEL_SLICE_MOMENTS = 10,
    CEL_MOMENTS_SPLIT_PIXELS = 4096
};
int cel_slice_sample(cel_images *img, cel_sources *src, int param, const int32_t *chain_ids, const double *dirs, int numdir,
                     int step_out, int max_steps_out, double sigma, double phi_max, uint64_t seed, int max_rounds,
                     double *x_out, double *llh_out, int64_t *stats);

/* ---- photon split (Gibbs step) ------------------------------------------------------------ */
/* boxes[(b*S+s)*4..] = y0,y1,x0,x1 and status[b*S+s] (as cel_stamp_boxes) for every band at once */
int cel_source_boxes(cel_images *img, cel_sources *src, int32_t *boxes, int32_t *status);
/* sample_source_counts / sample_multinomial (CelestePy/celeste_sample_sources.pyx:61-156) for every
 * band image: each pixel's nelec photons are split among the sources whose patch strictly contains
 * the pixel (:50-51) and the sky, by conditional binomials in source order, sky last.
 *   offsets  S*B+1: packed position of the sample patch of (source s, band b) at index s*B+b (the
 *            patch-set layout of cel_patch_loglik_multi); offsets[i+1]-offsets[i] = that box's area
 *            (cel_source_boxes), 0 without a patch.
 *            NULL = RESIDENT form: the library lays the patches out itself and keeps them in
 *            device memory for cel_patch_loglik_multi / cel_samples_fetch; samp is ignored
 *   samp     packed sample patches (doubles holding integers, as NativePatch.data), zeroed here
 *   noise    B doubles (host): photons attributed to the sky, the reference's noise_sum
 * Random numbers: Philox4x32-10 keyed by (seed; band, pixel, source) -- a result depends only on
 * the seed and the inputs.  The reference's randomkit stream cannot be reproduced on a GPU:
 * parity with it is statistical. */
int cel_photon_split(cel_images *img, cel_sources *src, uint64_t seed, const int64_t *offsets, double *samp,
                     int mem, double *noise);

/* the resident split's bookkeeping: number of sources and of packed patch values */
int cel_samples_info(cel_images *img, int64_t *S, int64_t *total);
/* copy out what the resident split holds; every output may be NULL:
 *   boxes S*B*4 (y0,y1,x0,x1 at s*B+b), offsets S*B+1, data (offsets[S*B] doubles),
 *   sums S*B = photons attributed to source s in band b (the flux Gibbs step's statistic,
 *   sources.py:327-345), reduced on the device */
int cel_samples_fetch(cel_images *img, int32_t *boxes, int64_t *offsets, double *data, double *sums);
/* where the resident split put each source's photons: rects S*B*4 (y0,y1,x0,x1 at s*B+b), the smallest rectangle of the
 * patch of (s, b) that holds every pixel with a photon, all zeros when the patch holds none.  A proposal for source s has
 * a non-zero conditional probability only if its own box covers that rectangle: the model draws a source's photons on its
 * box and nowhere else (celeste.py:217-219 adds the patch at its limits; sources.py:134-183 scores the fixed data patch
 * whatever the proposal's limits -- ModelGibbs(conditional="exact") applies the rule, DESIGN Q20). */
int cel_samples_photon_rects(cel_images *img, int32_t *rects);
/* diagnostic: N independent Binomial(n, p) variates from the split's sampler (stream i = draw i) */
int cel_debug_binomial(cel_ctx *ctx, int64_t n, double p, uint64_t seed, int64_t N, int64_t *out);

/* ---- E-step sufficient statistics -------------------------------------------------------- */
/* What celeste_em (CelestePy/celeste_em.py:38-91) reduces gen_src_prob_layers
 * (celeste.py:222-234) to, without building the (S+1) x H x W responsibility tensor:
 *   xtilde[s*B+b] = sum_pixels nelec * F_s / lambda     (celeste_em.py:85)
 *   mass[s*B+b]   = sum_pixels unit stamp of s in band b (celeste_em.py:89, before the min(1, .))
 *   noise[b]      = sum_pixels nelec * eps / lambda      (celeste_em.py:62, before the / size)
 * Renders lambda for `src` first.  Host outputs; any of them may be NULL.
 * On a MASKED image set (a NaN in nelec, cel_images_set_nelec) xtilde and noise run over the unmasked pixels, and
 *   mass[s*B+b] = sum of the unit stamp over the UNMASKED pixels of the box
 * -- the denominator the M-step needs: the light of s that the image could have recorded (0 for a box masked everywhere). */
int cel_estep_stats(cel_images *img, cel_sources *src, double *xtilde, double *mass, double *noise);

/* ---- gradient of the field log-likelihood ------------------------------------------------------ */
/* For the catalogue in `src` and the image set `img`:
 *     ll = sum_b sum_p  nelec log(lambda) - lambda,    lambda_b(p) = eps_b + sum_s counts[s][b] unit_stamp(s, b)(p)
 * The gradient is taken with every source's integer box held fixed (the box the render uses): lambda is piecewise smooth in
 * the parameters and the boxes are where it is not.  Outputs (any may be NULL) are the partial derivatives of ll with
 * respect to what cel_sources_set takes, in its units, summed over the bands:
 *   g_radec[s*2 + i]   d ll / d ra, d ll / d dec, per degree (the mean through equa2pixel and, for galaxies, W through
 *                      cd_at_pixel's cos(dec) term, Q9)
 *   g_counts[s*B + b]  d ll / d counts[s][b]
 *   g_shape[s*4 + i]   type 1: d ll / d (theta, sigma [arcsec], phi [degrees], rho); 0 for sigma where k_prep's floor
 *                      max(1/30, sigma) holds.  Type 2: d ll / d (theta, W00, W01, W11).  Stars: zeros.
 * ll_total (host, may be NULL) is the value cel_render_field(CEL_RENDER_LOGLIK) returns for the same call, bit for bit.
 * Renders lambda for `src` first, as cel_estep_stats does.  g_* follow `mem` (CEL_DEVICE: device pointers, e.g. an
 * optimiser's state); the stream is synchronised before the call returns.  Sums run in a fixed order (no atomics): two calls
 * give the same bits.  Drop rule and its error bound: desi-mcmc_amd/csrc/k_grad.h (per-source threshold
 * CEL_OPT_TAIL_LOG_SOURCE; the gradient's relative error stays below ~K T_k e^-T, 4e-11 at the default T = 32).  At the
 * shipping defaults the render's T = 24 moves every r(p) = nelec / lambda - 1 by at most n e^-24 nelec / lambda as well: every
 * entry then stays within 1e-7 of the largest |entry| of its column of the gradient with nothing dropped (T = 0).
 * CEL_ERR_INVALID without cel_images_set_nelec and on an image set with a row window (cel_images_set_window): partitioned
 * (strip / windowed) gradients are not provided.
 * On a MASKED image set (a NaN in nelec, cel_images_set_nelec) r(p) = nelec / lambda - 1 at the unmasked pixels and 0 at the
 * masked ones; ll_total is cel_render_field's masked value, bit for bit. */
int cel_loglik_grad(cel_images *img, cel_sources *src, double *ll_total, double *g_radec, double *g_counts, double *g_shape,
                    int mem);

/* ---- generic evaluator ------------------------------------------------------------------ */
/* gmm_like_2d (util/like/gmm_like_fast.pyx:130-176; wrapper util/like/__init__.py:7-11):
 * probs[n] = sum_k ws[k] N(x[n]; mus[k], sigs[k]).  x: N*2, mus: K*2, sigs: K*4 covariances.
 * x and probs follow `mem`; ws/mus/sigs are host arrays. */
int cel_gmm_like_2d(cel_ctx *ctx, const double *x, int64_t N, const double *ws, const double *mus,
                    const double *sigs, int K, double *probs, int mem);

/* mog_loglike (util/dists/mog.py:5-21), the log-domain evaluator MixtureOfGaussians.logpdf /
 * evaluate_grid (:58-60, :102-112) and gen_point_source_psf_image (celeste.py:158) call:
 *   out[n] = logsumexp_k( -(x_n - mu_k)^T icov_k (x_n - mu_k) / 2 + logw[k] )
 * logw[k] = -log(2 pi) - log(dets[k]) / 2 + log(pis[k]), formed by the caller as the reference forms
 * it (a weight <= 0 gives NaN / -inf there; NaN propagates to every output).
 * x and out follow `mem`; means (K*2), icovs (K*4), logw (K) are host arrays. */
int cel_mog_loglike(cel_ctx *ctx, const double *x, int64_t N, const double *means, const double *icovs,
                    const double *logw, int K, double *out, int mem);

/* gen_galaxy_prof_psf_mixture_params (CelestePy/celeste_fast.pyx:100-140), for N sources sharing the
 * PSF and profile arrays: the convolved component tables, PSF-major (index k * J + j):
 *   weights[n][k*J+j] = image_ws[k] * amp[j]
 *   means  [n][k*J+j] = v_s[n] + image_means[k]
 *   covars [n][k*J+j] = image_covars[k] + sigs[j] * W[n]
 * W: N*4 (= R R^T), v_s: N*2, image_*: the PSF (K_psf components), amp/sigs: the profile (J).
 * gen_galaxy_psf_mixture_params (:29-94) is the same call with amp = [thetas[0] * exp_amp,
 * thetas[1] * dev_amp] and sigs = [exp_sigs, dev_sigs].  Host arrays in and out; built on the device. */
int cel_galaxy_mixture_params(cel_ctx *ctx, int64_t N, const double *W, const double *v_s, const double *image_ws,
                              const double *image_means, const double *image_covars, int K_psf, const double *amp,
                              const double *sigs, int J, double *weights, double *means, double *covars);

/* calc_bounding_radius (util/bound/bounding_box.py:9-31); host arithmetic, no device needed */
int cel_bounding_radius(const double *w, const double *mu, const double *cov, int K, double error,
                        const double *center, double *out);

/* ---- measurement -------------------------------------------------------------------------- */
/* With CEL_OPT_PROFILE = 1 (2: see the option) every launch of kernel `k` is bracketed by HIP events on the
 * context's stream; cel_profile_get synchronises and returns the mean duration. */
int cel_profile_reset(cel_ctx *ctx);
int cel_profile_get(cel_ctx *ctx, int kernel, double *mean_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* CELESTE_HIP_H */
