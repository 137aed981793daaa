"""What the calls LEAVE BEHIND: a random walk over everything that shares one image set and one catalogue, device samplers, masked
pixels and the resident photon split included (tests/_state_walk.py).

The library keeps about ten "whose state is this" stamps between calls (recs_gen, lists_gen, lambda_gen, partials_gen, massfx_gen,
mass_gen, samp_S / ssum_valid; on the catalogue gen, full_gen, row_gen[], n_gal, h_type) and every short cut trusts them: the
dirty-tile render, the split's totals from the resident model image, stamp masses read off the split's sums, the star-only
kernels, cel_stamp_mass_end.  The walkers of tests/test_stress.py predate every call that rewrites the catalogue ON THE DEVICE
(cel_flux_conditionals, cel_slice_locations, cel_slice_sample params 0 / 1 / 2) and everything that changes what an image set is
(masks, CEL_OPT_HONOUR_MASK, CEL_OPT_SPLIT_FULL_BOX, the exact conditional, cel_images_set_nelec between the three kinds of
pixels).  Here they are walked: after every call that returns numbers the live pair is compared, bit for bit, with fresh objects
that reach the same inputs the documented way and have no memory.

What the walk and its construction found, fixed in the same change and scripted in test_named_transitions:
  * cel_images_set_nelec left the resident split of the OLD pixels in place (flux step, slice samplers, resident patch
    log-likelihoods and cel_samples_fetch went on answering from it): new pixels now drop the split;
  * cel_stamp_mass_end handed out whatever waited in the context's scratch slot when a device sampler (or a photon split, which
    takes the same slot) had run since _begin on a catalogue without the split's stamp sums: it now refuses, as the header says;
  * the stamp-mass short cut vouched for a source by its counts alone: a galaxy of 1 900 photons hanging over the frame's edge,
    1.2e-5 of its light on the frame, came out 1.7e-9 off the mass kernel (bound 1e-9): it now vouches by counts * mass.

That the file can fail: libraries with ONE stamp broken each fail it -- no generation bump in cel_flux_conditionals or in the
type move, n_gal left stale by the type move, lambda_gen kept by cel_images_set_epsilon, cel_images_set_nelec keeping the split,
cel_stamp_mass_end without its check -- while test_stress.py, test_hip_parity.py and test_type_move.py pass on the first, second and
fifth of them (the table is in the message of the change that added this file).

The stamps' only writers are the events of csrc/field_state.h (DESIGN.md section 4b names, per event and product, the test that
would notice its loss); the two the walk cannot reach -- a new window under cached products (in the walk the window only frames a
refusal) and the observed pixels' address handed out -- are scripted in test_named_transitions (8., 9.).

Timings, measured on the MI355X: a walk of 250 steps takes 0.5 - 1.6 s (the first of a session 3.2 s with the library's load and
the scene's draw), test_named_transitions 0.3 - 0.4 s, the whole file 4.5 s.
"""
import numpy as np
import pytest

import _state_walk as sw

gpu = pytest.mark.gpu
#: the walks: (seed, flavour), and their length (0.5 - 1.6 s per walk on the MI355X: no need to halve it)
STEPS = 250
WALKS = [(1, "gibbs"), (2, "gibbs"), (1, "edits"), (2, "edits")]


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def test_generator_meets_its_coverage():
    """ops() alone, for the seeds and step counts the GPU walks use: every operation at least 3 times, every named pattern and
    every documented refusal at least once, no _end without its _begin, and the same sequence for the same seed -- the walks'
    coverage assertions are met by construction"""
    for seed, flavour in WALKS:
        seq = sw.ops(seed, STEPS, flavour)
        assert STEPS <= len(seq) < STEPS + 12
        assert seq == sw.ops(seed, STEPS, flavour)
        count, refused, pat, paired = sw.coverage(seq)
        assert paired
        assert min(count.values()) >= 3, {k: v for k, v in count.items() if v < 3}
        assert min(refused.values()) >= 1, refused
        assert min(pat.values()) >= 1, pat
        assert all(op["op"] in sw.OPERATIONS or op["op"] in ("window_on", "window_off") for op in seq)
    a, b = sw.ops(1, STEPS, "gibbs"), sw.ops(1, STEPS, "edits")
    heavy = lambda seq: sum(op["op"] in sw.SAMPLERS + sw.EXACT for op in seq) / float(sum(op["op"] in sw.SET_ROWS + ("render", "render_noll") for op in seq))
    assert heavy(a) > 2 * heavy(b)                              # (the flavours are different walks)


@gpu
@pytest.mark.parametrize("seed,flavour", WALKS)
def test_walk(cel, seed, flavour):
    """STEPS random operations on one live pair, every returned number equal to the replay's; then the coverage, counted on the
    live pair: conditions, not measurements"""
    w = sw.Walker(cel)
    try:
        w.walk(sw.ops(seed, STEPS, flavour))
    finally:
        print("walk %s/%d: %d operations; %s; refused %s" % (flavour, seed, len(w.log), w.seen, w.refused))
    assert w.seen["dirty_after_pattern"] >= 1, (w.seen, "no dirty-tile render behind device sampler -> full render -> set_rows")
    assert w.seen["ready1"] >= 1 and w.seen["ready0"] >= 1, w.seen
    assert min(w.count.values()) >= 3, {k: v for k, v in w.count.items() if v < 3}
    assert min(w.refused.values()) >= 1, w.refused
    w.close()


def _op(name, seed, expect=None, **kw):
    return dict(op=name, seed=seed, expect=expect, **kw)


@gpu
def test_named_transitions(cel):
    """the transitions a walk must not be left to find by luck, on the walk's scene and with the walk's replay recipes"""
    # 0. (found by the walk) stamps that hang over the frame's edge: the split's sums vouch for a mass by the light ON THE FRAME, so
    #    the short cut and the mass kernel agree to 1e-9 of a mass of 1e-5 as well
    from desi_mcmc_amd import synth
    w = sw.Walker(cel)
    gal, star = np.arange(26, 38), np.arange(6, 12)
    w.cur[3][gal] = [0.75, 0.41, 47.6, 0.51]                         # (the walk's case: a compact galaxy of 330 and 1 900 photons)
    w.cur[2][gal] = [334.5, 1908.8]
    rows = np.concatenate([gal, star])
    w.cur[1][rows] = synth.pixel2equa(w.sc["bands"][0], np.tile([80.0, 96.0], (rows.size, 1)))
    w.ss.set(*w.cur)
    boxes, _ = w.im.source_boxes(w.ss)                                # (B, S, 4) = y0, y1, x0, x1
    half = 0.5 * (boxes[1, rows, 3] - boxes[1, rows, 2])
    on = np.concatenate([2.5 + 0.5 * np.arange(gal.size), 2.0 + np.arange(star.size)])     # columns of the half box left on the frame
    w.cur[1][rows] = synth.pixel2equa(w.sc["bands"][0], np.column_stack([on - half, np.linspace(20.0, 170.0, rows.size)]))
    w.ss.set(*w.cur)
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 2), _op("mass", 3), _op("flux", 4)])
    assert w.seen["ready1"] == 1
    w.close()

    # 1., 2. split -> device sampler -> set_rows of one row -> render: incremental only if legal, and equal either way
    for k, sampler in enumerate(("flux", "slice_locations", "slice_sample1", "type_move")):
        w = sw.Walker(cel)
        w.walk([_op("render", 1, loglik=True), _op("split_traced", 10 + k), _op("mass", 5), _op(sampler, 20 + k), _op("mass", 6)])
        assert w.seen["ready1"] == 1 and w.seen["ready0"] == 1, sampler        # (the split's stamp sums are not the rewritten catalogue's)
        w.walk([_op("set_rows_1", 30 + k), _op("render", 2, loglik=True)])
        assert w.im.last_render_dirty_tiles() == -1, sampler       # (no render of the sampler's catalogue came before: every tile)
        w.walk([_op(sampler, 40 + k), _op("render", 3, loglik=True), _op("set_rows_1", 50 + k), _op("render", 4, loglik=True)])
        assert w.im.last_render_dirty_tiles() >= 0 and w.seen["dirty_after_pattern"] == 1, sampler
        w.close()

    # 3. stars only: the type move makes galaxies where the host's types say there are none, and takes them away again
    w = sw.Walker(cel, stars_only=True)
    n = w.n
    assert not np.any(w.cur[0])
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 5)])
    w.ctx.profile(True)
    w.run(_op("render", 2, loglik=True))
    assert w.ctx.profile_get("small_stars")[1] + w.ctx.profile_get("render_stars")[1] >= 1      # (a star-only kernel is this scene's)
    for seed in range(60, 70):
        w.run(_op("type_move", seed, h=np.full(n, 50.0)))
        if np.any(w.ss.get()[0] == 1):
            break
    assert np.any(w.cur[0] == 1), "no star was accepted as a galaxy under h = +50"
    w.ctx.profile(True)
    w.run(_op("render", 3, loglik=True))                            # equal to a fresh render of the catalogue read back ...
    assert w.ctx.profile_get("small_stars")[1] + w.ctx.profile_get("render_stars")[1] == 0 and w.ctx.profile_get("render")[1] >= 1
    w.run(_op("estep", 4))
    w.run(_op("mass", 5))
    for seed in range(70, 90):                                      # (h is the term of the move a chain WOULD make: back for the galaxies only)
        w.run(_op("type_move", seed, h=np.where(w.cur[0] == 1, 50.0, -50.0)))
        if not np.any(w.ss.get()[0]):
            break
    assert not np.any(w.cur[0]), "a galaxy stayed under h = +50 for the move back"
    w.ctx.profile(False)
    w.run(_op("render", 6, loglik=True))                            # ... and of an all-star catalogue set from host memory
    w.run(_op("split_traced", 7))
    w.run(_op("flux", 8))
    w.close()

    # 4. new pixels drop the resident split: every call that needs it names the missing split (a masked set: the mask first)
    w = sw.Walker(cel)
    w.options(dict(honour=1.0))
    calls = {
        "flux": lambda: w.im.flux_conditionals(w.ss, 1, 5.0, 0.005, w.letters, w.calib, w.kappa),
        "slice_locations": lambda: w.im.slice_locations(w.ss, sw.SIGMA_LOC, 1),
        "slice_sample0": lambda: w.im.slice_sample(w.ss, 0, sw.SIGMA_LOC, 1, step_out=False),
        "slice_sample1": lambda: w.im.slice_sample(w.ss, 1, sw.SIGMA_SHAPE, 1),
        "type_move": lambda: w.im.type_move(w.ss, np.tile([0.5, 1.0, 30.0, 0.5], (w.n, 1)), np.zeros(w.n), 1),
        "pll": lambda: w.im.patch_loglik_resident(w.ss, np.arange(w.n, dtype=np.int32)),
        "pll_isolated": lambda: w.im.patch_loglik_resident(w.ss, np.arange(w.n, dtype=np.int32), isolated=True),
        "sample_sums": lambda: w.im.sample_sums(),
        "fetch_samples": lambda: w.im.fetch_samples(),
        "photon_rects": lambda: w.im.photon_rects(),
    }
    for kind in (1, 2, 0):
        w.walk([_op("render", 1, loglik=True), _op("split_traced", 3), _op("mass", 4)])
        assert w.samples_info(w.im)[0] == w.n
        assert w.im.stamp_mass_ready(w.ss) == (w.kind != 2)         # (a masked set under CEL_OPT_HONOUR_MASK takes no short cut)
        w.run(_op("set_nelec", 5, kind=kind))
        assert w.samples_info(w.im) == (0, 0) and not w.im.stamp_mass_ready(w.ss)
        for name, call in calls.items():
            masked_first = kind == 2 and name in ("slice_locations", "slice_sample0", "slice_sample1", "type_move", "pll_isolated")
            with pytest.raises(ValueError, match="masked" if masked_first else "resident photon split"):
                call()
        w.same("catalogue behind the refusals", w.ss.get(), tuple(w.cur))
        w.walk([_op("mass", 6), _op("render", 7, loglik=True), _op("split_traced", 8), _op("flux", 9), _op("mass", 10), _op("pll", 11)])
        if kind != 2:
            w.walk([_op("slice_locations", 12), _op("type_move", 13), _op("render", 14, loglik=True)])
    w.close()

    # 5. a refused call between two accepted ones changes nothing
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 2), _op("mass", 3)])
    assert w.im.stamp_mass_ready(w.ss)
    with pytest.raises(ValueError, match="finite"):
        w.im.type_move(w.ss, np.tile([0.5, 1.0, 30.0, 0.5], (w.n, 1)), np.full(w.n, np.nan), 4)
    assert w.im.stamp_mass_ready(w.ss)
    w.walk([_op("mass", 5), _op("window_on", 6), _op("exact_type_move", 7, expect="window"), _op("window_off", 8), _op("flux", 9)])
    w.walk([_op("set_nelec", 10, kind=2), _op("opt_honour_mask", 11, value=1), _op("render", 12, loglik=True), _op("split_traced", 13), _op("flux", 14),
            _op("opt_honour_mask", 15, value=0), _op("flux", 16, expect="masked_unhonoured"), _op("split_cold", 17, expect="masked_unhonoured"),
            _op("slice_locations", 18, expect="masked_sampler"), _op("opt_honour_mask", 19, value=1), _op("flux", 20), _op("mass", 21)])
    w.close()

    # 6. (found by the walk) cel_stamp_mass_end behind a device sampler or a photon split refuses -- with and without the split's
    #    stamp sums, where the pending values wait in a scratch slot that the calls in between take
    w = sw.Walker(cel)
    w.walk([_op("set_rows_1", 1), _op("split_cold", 2), _op("mass_begin", 3), _op("slice_locations", 4), _op("mass_end", 5, expect="end_rebuilt")])
    w.walk([_op("render", 6, loglik=True), _op("split_traced", 7), _op("mass_begin", 8), _op("type_move", 9), _op("mass_end", 10, expect="end_rebuilt")])
    w.walk([_op("mass_begin", 11), _op("render", 12, loglik=True), _op("split_traced", 13), _op("mass_end", 14, expect="end_rebuilt")])
    w.walk([_op("mass_begin", 13), _op("set_epsilon", 14), _op("mass_end", 15), _op("mass", 16)])
    w.close()

    # 7. a new sky level under a model image that is on the device: the dirty-tile render without a log-likelihood (which the
    #    Poisson partials do not stop) and the split's totals must not take the old image
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("set_epsilon", 2), _op("set_rows_1", 3), _op("render_noll", 4)])
    w.walk([_op("render", 5, loglik=True), _op("set_epsilon", 6), _op("split_cold", 7), _op("flux", 8), _op("render", 9, loglik=True)])
    w.close()

    # 8. a new window cuts the boxes anew: the host's boxes, the split's stamp sums and (with the records of the same catalogue
    #    written again, and row stamps to go by) the model image and tile lists of the old window must not be taken
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 2), _op("mass", 3)])
    old = w.im.source_boxes(w.ss)
    assert w.im.stamp_mass_ready(w.ss)
    w.run(_op("window_on", 4))
    rim, rss = w.fresh(w.cur)
    rim.set_window(32, sw.H + 64)
    assert not w.im.stamp_mass_ready(w.ss)
    new = w.im.source_boxes(w.ss)
    assert not np.array_equal(new[0], old[0])
    w.same("boxes behind a new window", new, rim.source_boxes(rss))
    w.same("masses behind a new window", w.im.stamp_mass(w.ss), rim.stamp_mass(rss))
    w.run(_op("set_rows_1", 5))
    rss.set(*w.cur)
    out = w.im.render(w.ss, loglik=True)
    assert w.im.last_render_dirty_tiles() == -1
    w.same("render behind a new window: log-likelihood", out, rim.render(rss, loglik=True))
    w.same("render behind a new window: model images", w.im.model_images(), rim.model_images())
    rim.close()
    w.close()

    # 9. the observed pixels' address handed out: the caller writes them when it likes, and no tile's Poisson partial outlives it
    import ctypes as C
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("set_rows_1", 2), _op("render", 3, loglik=True)])
    assert w.im.last_render_dirty_tiles() >= 0                      # (the dirty-tile render is this set's, until ...)
    pixels = np.ascontiguousarray(w.sc["nelec"][0] + 1.0)
    hip = C.CDLL(cel._lib.LIB_PATH)                                 # (dlsym through the library finds the HIP runtime IT is linked to)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(w.im.device_ptrs()[0], pixels.ctypes.data, pixels.nbytes, 1) == 0
    w.run(_op("set_rows_1", 4))
    out = w.im.render(w.ss, loglik=True)
    assert w.im.last_render_dirty_tiles() == -1
    rim = cel.ImageSet(w.ctx, w.bands(w.eps), sw.H, sw.W, nelec=pixels)
    w.same("render behind the caller's own pixels", out, rim.render(cel.SourceSet(w.ctx, w.n, sw.B).set(*w.cur), loglik=True))
    rim.close()
    w.close()
