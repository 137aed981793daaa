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
would notice its loss).

The inputs every cached product depends on are walked as well ("strips", "options" and the stars_only scene's "stars"; the replay
rule is in tests/_state_walk.py): the row window (window_to), the owned rows (noise_rows), the context options that change
results (opt_tail: both thresholds; opt_kernel) and those that must not (opt_tile_order, opt_tile_parts, opt_slice_fuse,
opt_star_tiles), and the observed pixels' address handed out with the same pixels written back through it (hand_out).  What was
decided with them, fixed in the same change and scripted in test_named_transitions (10. - 15.):
  * a new window left the resident split of the OLD window's boxes in place (cel_slice_locations scored new records against old
    patches): cel_images_set_window with another window now drops the split, the window it already has drops nothing (10.);
  * the split took its totals from the model image on the device whatever threshold that image was rendered at: model_current
    now asks (11.);
  * the stamp-mass short cut read the split's stamp sums whatever per-source threshold they were formed at (6.9e-2 off at
    T = 8 against the default): sums_of now asks (12.);
  * CEL_OPT_KERNEL needs no stamp (13.), cel_images_set_noise_rows drops nothing (14.), cel_images_device_ptrs keeps the split (15.).
Found by the new walks' first run, in the TEST: the short cut's bound of 1e-9 is the shipping per-source threshold's; under a
coarser one it scales with the dropped terms' ceiling (Walker.third_mass).  No mismatch of the library's beyond the decided cases.

That these can fail: libraries with ONE comparison removed each -- model_current without the threshold: 11. (the split's noise
sums, 834 727 against 834 749 photons) and the walks strips/1, options/1 and stars/1 (pattern_tail_split: totals 1e-8 off);
sums_of without it: 12. (stamp_mass_ready stays 1).  The window's fix is shown on the CPU alone (tests/host/field_state_events.cpp:
without the drop, the new_window row and the pending-mass block fail): a library without it would score against patches of
another window.

Timings, measured on the MI355X: a walk of 250 steps takes 0.5 - 1.5 s for "gibbs" and "edits" (the first of a session more, with
the library's load and the scene's draw), 0.3 - 0.4 s for "strips" and "options" (below the earlier walks' range, not above it: fewer of
their steps are device samplers), 0.15 s for "stars" (12 sources); test_named_transitions 0.6 s (0.3 s
before 10. - 15.); the whole file 5.5 s (4.4 s before).
"""
import numpy as np
import pytest

import _state_walk as sw

gpu = pytest.mark.gpu
#: the walks: (seed, flavour), and their length (0.5 - 1.6 s per walk on the MI355X: no need to halve it)
STEPS = 250
WALKS = [(1, "gibbs"), (2, "gibbs"), (1, "edits"), (2, "edits"), (1, "strips"), (1, "options")]
STAR_WALKS = [(1, "stars")]             # the stars_only scene (12 stars): CEL_OPT_STAR_TILES and the star-only kernels


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


def test_generator_meets_its_coverage():
    """ops() alone, for the seeds and step counts the GPU walks use: every operation at least 3 times, every named pattern and
    every documented refusal at least once, no _end without its _begin, and the same sequence for the same seed -- the walks'
    coverage assertions are met by construction"""
    for seed, flavour in WALKS + STAR_WALKS:
        seq = sw.ops(seed, STEPS, flavour)
        assert STEPS <= len(seq) < STEPS + 12
        assert seq == sw.ops(seed, STEPS, flavour)
        count, refused, pat, paired = sw.coverage(seq, flavour)
        assert paired
        assert set(count) == set(sw.required(flavour))
        assert min(count.values()) >= 3, {k: v for k, v in count.items() if v < 3}
        if flavour in ("gibbs", "edits"):
            assert min(refused.values()) >= 1, refused
            assert min(pat.values()) >= 1, pat
        elif flavour != "stars":            # (the inputs' walks owe the refusals that an input causes; no masked pixels, no window on the stars' walk)
            assert refused["window"] >= 1 and refused["no_split"] >= 2, refused
            assert min(pat.values()) >= 1, pat
        assert all(op["op"] in sw.OPERATIONS + ("opt_star_tiles",) for op in seq)
        if flavour in ("strips", "options"):
            # strips: every window and every choice of owned rows; options: every threshold, both variants, every value of the result-preserving options
            seen = lambda name, key: set(tuple(op[key]) if isinstance(op[key], (tuple, list)) else op[key] for op in seq if op["op"] == name)
            if flavour == "strips":
                assert seen("window_to", "window") == set(sw.WINDOWS) and seen("noise_rows", "rows") == set(sw.NOISE_ROWS)
            else:
                assert seen("opt_tail", "value") == set(sw.TAILS) and seen("opt_kernel", "value") == {0, 1}
                assert seen("opt_tile_parts", "value") == {0, 1, 2, 4} and seen("opt_slice_fuse", "value") == {0, 2} and seen("opt_tile_order", "value") == {0, 1, 2}
        if flavour == "stars":
            assert set(op["value"] for op in seq if op["op"] == "opt_star_tiles") == {0, 1, 2}
    a, b = sw.ops(1, STEPS, "gibbs"), sw.ops(1, STEPS, "edits")
    heavy = lambda seq: sum(op["op"] in sw.SAMPLERS + sw.EXACT for op in seq) / float(sum(op["op"] in sw.SET_ROWS + ("render", "render_noll") for op in seq))
    assert heavy(a) > 2 * heavy(b)                              # (the flavours are different walks)
    share = lambda seq, names: sum(op["op"] in names for op in seq) / float(len(seq))
    c, d = sw.ops(1, STEPS, "strips"), sw.ops(1, STEPS, "options")
    assert share(c, ("window_to", "noise_rows")) > 2 * share(d, ("window_to", "noise_rows"))
    assert share(d, ("opt_tail", "opt_kernel", "opt_tile_order", "opt_tile_parts", "opt_slice_fuse")) > \
        1.5 * share(c, ("opt_tail", "opt_kernel", "opt_tile_order", "opt_tile_parts", "opt_slice_fuse"))        # (both owe three of each)


@gpu
@pytest.mark.parametrize("seed,flavour", WALKS)
def test_walk(cel, seed, flavour):
    """STEPS random operations on one live pair, every returned number equal to the replay's; then the coverage, counted on the
    live pair: conditions, not measurements"""
    w = sw.Walker(cel, required=sw.required(flavour))
    try:
        w.walk(sw.ops(seed, STEPS, flavour))
    finally:
        print("walk %s/%d: %d operations; %s; refused %s" % (flavour, seed, len(w.log), w.seen, w.refused))
    assert w.seen["dirty_after_pattern"] >= 1, (w.seen, "no dirty-tile render behind device sampler -> full render -> set_rows")
    assert w.seen["ready1"] >= 1 and w.seen["ready0"] >= 1, w.seen
    assert min(w.count.values()) >= 3, {k: v for k, v in w.count.items() if v < 3}
    assert min(w.refused[k] for k in (sw.REFUSALS if flavour in ("gibbs", "edits") else ("window", "no_split"))) >= 1, w.refused
    w.close()


@gpu
@pytest.mark.parametrize("seed,flavour", STAR_WALKS)
def test_walk_stars(cel, seed, flavour):
    """the same on the stars_only scene: a catalogue without galaxies stays one (no type move, no star <-> galaxy edit), so the
    one-launch render of a small star field, the star-tile kernel and the general kernel take turns under CEL_OPT_STAR_TILES"""
    w = sw.Walker(cel, stars_only=True, required=sw.required(flavour))
    try:
        w.walk(sw.ops(seed, STEPS, flavour))
    finally:
        print("walk %s/%d: %d operations; %s; refused %s" % (flavour, seed, len(w.log), w.seen, w.refused))
    assert not np.any(w.cur[0])
    assert w.seen["ready1"] >= 1 and w.seen["ready0"] >= 1 and w.seen["full"] >= 1 and w.seen["dirty"] >= 1, w.seen
    assert min(w.count.values()) >= 3, {k: v for k, v in w.count.items() if v < 3}
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
    w.walk([_op("mass", 5), _op("window_to", 6, window=(32, sw.H + 64)), _op("exact_type_move", 7, expect="window"),
            _op("window_to", 8, window=(0, sw.H)), _op("flux", 9, expect="no_split")])     # (the window took the split with it: 10.)
    w.walk([_op("render", 9, loglik=True), _op("split_traced", 9), _op("flux", 9)])
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
    w.run(_op("window_to", 4, window=(32, sw.H + 64)))
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

    # 10. a new window drops the resident split: its patches are boxes of the OLD window.  Every call that needs a split names
    #     the missing one, a pending cel_stamp_mass_begin is refused like one behind a rebuilt catalogue, the catalogue is
    #     untouched; then everything equals a fresh windowed pair.  The window it already has drops nothing
    w = sw.Walker(cel)
    win = (32, sw.H + 64)
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 2), _op("mass", 3)])
    assert w.seen["ready1"] == 1 and w.samples_info(w.im)[0] == w.n
    w.run(_op("mass_begin", 4))
    w.run(_op("window_to", 5, window=win))
    assert w.samples_info(w.im) == (0, 0) and not w.im.stamp_mass_ready(w.ss)
    for name, call in calls.items():
        with pytest.raises(ValueError, match="resident photon split"):
            call()
    with pytest.raises(ValueError, match="rebuilt since"):          # (mass.intact: the records _begin summed are nobody's)
        w.im.stamp_mass_end()
    w.same("catalogue behind a new window", w.ss.get(), tuple(w.cur))
    w.walk([_op("render", 6, loglik=True), _op("split_traced", 7), _op("flux", 8), _op("slice_locations", 9), _op("mass", 10)])
    info = w.samples_info(w.im)
    assert info[0] == w.n
    w.run(_op("window_to", 11, window=win))                         # the same window again: a no-op
    assert w.samples_info(w.im) == info
    w.walk([_op("flux", 12), _op("pll", 13), _op("window_to", 14, window=(0, sw.H)), _op("window_to", 15, window=(0, sw.H)),
            _op("pll", 16, expect="no_split")])
    w.close()

    # 11. a model image of the coarse threshold, then the strict one, then the split: its totals, sums and draws are those of a
    #     pair that never saw the coarse threshold.  With its image at another threshold the split is "cold" by the documented rule
    #     (split_cold: bit for bit against a fresh strict pair's cold split); against a fresh strict pair's render + split the
    #     totals are the same image under CEL_OPT_SPLIT_FULL_BOX (bit for bit) and agree to the 1e-10 the header gives for the
    #     two forms of the strict totals otherwise (1e-9 asserted: tools/dbg/reuse_stress.py's figure)
    for reuse, full in ((1, 0), (2, 0), (2, 1)):
        w = sw.Walker(cel)
        w.options(dict(reuse=float(reuse), full=float(full)))
        w.walk([_op("opt_tail", 1, value="all8"), _op("render", 2, loglik=True)])
        coarse = w.im.model_images()
        w.walk([_op("opt_tail", 3, value="strict"), _op("split_cold", 4)])
        rim, rss = w.fresh(w.cur)
        rim.render(rss, loglik=True)
        strict = rim.model_images()
        rim.photon_split_resident(rss, 4)
        gap = np.max(np.abs(w.im.split_rates() - rim.split_rates()) / rim.split_rates())
        stale = np.max(np.abs(coarse - strict) / strict)
        print("11. reuse %d full %d: totals against a strict render + split %.3e relative; the T = 8 image against the strict one %.3e" % (reuse, full, gap, stale))
        if full:
            w.same("totals, sums and draws behind a threshold change (full boxes)", (w.im.split_rates(), w.im.sample_sums(), w.im.fetch_samples()),
                   (rim.split_rates(), rim.sample_sums(), rim.fetch_samples()))
        assert gap <= 1e-9
        assert stale > 1e-6                                         # (non-vacuity, on fresh values alone: the stale image is far off)
        rim.close()
        w.walk([_op("flux", 5), _op("mass", 6)])
        w.close()

    # 12. the split's stamp sums of one per-source threshold are not the masses of another: the short cut steps aside
    w = sw.Walker(cel)
    w.walk([_op("opt_tail", 1, value="source8"), _op("render", 2, loglik=True), _op("split_traced", 3)])
    assert w.im.stamp_mass_ready(w.ss)
    coarse = w.im.stamp_mass(w.ss)                                  # (the short cut, at T = 8)
    w.options(dict(tail_T=32.0))                                    # the per-source threshold back to its default
    assert not w.im.stamp_mass_ready(w.ss)
    rim, rss = w.fresh(w.cur)
    want = rim.stamp_mass(rss)                                      # (the mass kernel: this pair never had a split)
    rim.close()
    w.same("stamp_mass behind a threshold change", w.im.stamp_mass(w.ss), want)
    w.im.stamp_mass_begin(w.ss)
    w.same("stamp_mass_begin / _end behind a threshold change", w.im.stamp_mass_end(), want)
    w.run(_op("mass", 4))
    assert w.seen["ready0"] == 1 and w.seen["ready1"] == 0
    off = np.max(np.abs(coarse - want) / np.maximum(want, 1e-300))
    print("12. the T = 8 short-cut masses against the mass kernel's: %.3e relative" % off)
    assert off > 1e-6
    w.options(dict(tail_T=8.0))                                     # ... and back at the split's threshold the sums serve again
    assert w.im.stamp_mass_ready(w.ss)
    w.same("the short cut at the split's own threshold", w.im.stamp_mass(w.ss), coarse)
    w.close()

    # 13. the kernel variant between a product and its reader.  A render by the direct kernels vouches for no model image
    #     (render_succeeded: `vouches` needs the recurrence), the dirty-tile render and the split's totals from the image are the
    #     recurrence's alone, records and tile lists do not depend on the variant: nothing has to remember it
    w = sw.Walker(cel)
    dirty = lambda: w.im.last_render_dirty_tiles()
    w.walk([_op("opt_kernel", 1, value=0), _op("render", 2, loglik=True), _op("opt_kernel", 3, value=1), _op("set_rows_1", 4), _op("render", 5, loglik=True)])
    assert dirty() == -1                                            # (direct -> recurrence: no image to start from)
    w.walk([_op("set_rows_1", 6), _op("render_noll", 7)])
    assert dirty() >= 0                                             # (the recurrence's own image: legal)
    w.walk([_op("opt_kernel", 8, value=0), _op("set_rows_1", 9), _op("render", 10, loglik=True)])
    assert dirty() == -1                                            # (recurrence -> direct: the direct kernels render every tile)
    w.walk([_op("set_rows_1", 11), _op("render_noll", 12)])
    assert dirty() == -1
    w.walk([_op("opt_kernel", 13, value=1), _op("set_rows_1", 14), _op("render_noll", 15)])
    assert dirty() == -1
    w.walk([_op("opt_kernel", 16, value=0), _op("render", 17, loglik=True), _op("opt_kernel", 18, value=1), _op("split_cold", 19), _op("flux", 20),
            _op("mass", 21), _op("render", 22, loglik=True), _op("opt_kernel", 23, value=0)])

    def direct_split(im, ss):
        noise = im.photon_split_resident(ss, 24)
        return dict(noise=noise, sums=im.sample_sums(), samples=im.fetch_samples(), info=w.samples_info(im))
    a = w.outcome(lambda: direct_split(w.im, w.ss))                 # the recurrence's image on the device, the direct split
    rim, rss = w.fresh(w.cur)
    b = w.outcome(lambda: direct_split(rim, rss))
    assert a[0] == "ok" and b[0] == "ok", (a, b)
    w.same("the direct split behind a recurrence render", a[1], b[1])
    rim.close()
    w.close()

    # 14. other owned rows under the per-tile Poisson partials: the reduce takes the owned tile rows of THIS render, so the dirty
    #     tiles' render is legal and equal; the split's noise sums are a product of their time
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("noise_rows", 2, rows=(64, 128)), _op("set_rows_1", 3), _op("render", 4, loglik=True)])
    assert dirty() >= 0
    noise = w.im.photon_split_resident(w.ss, 5)
    rim, rss = w.fresh(w.cur)
    rim.render(rss, loglik=True)
    w.same("noise sums of the owned rows", noise, rim.photon_split_resident(rss, 5))
    rim.close()
    w.run(_op("noise_rows", 6, rows=(0, sw.H)))
    kept = np.zeros(sw.B)
    hip = C.CDLL(cel._lib.LIB_PATH)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(kept.ctypes.data, w.im.loglik_device_ptr(), kept.nbytes, 2) == 0
    w.same("the split's noise sums behind other owned rows", kept, noise)
    w.walk([_op("render", 7, loglik=True), _op("split_traced", 8)])
    whole = np.zeros(sw.B)
    assert hip.hipMemcpy(whole.ctypes.data, w.im.loglik_device_ptr(), whole.nbytes, 2) == 0
    assert np.all(whole > noise)                                    # (non-vacuity: three tile rows hold more sky photons than one)
    w.close()

    # 15. the observed pixels' address handed out keeps the resident split: it stays the split of the pixels it was drawn from
    #     (the library cannot know when the caller writes); cel_images_set_nelec is how a caller announces new pixels
    w = sw.Walker(cel)
    w.walk([_op("render", 1, loglik=True), _op("split_traced", 2)])
    info = w.samples_info(w.im)
    w.write_pixels(pixels)                                          # (9.'s pixels: every count one more)
    assert w.samples_info(w.im) == info
    rim, rss = w.with_split()                                       # a replay that split on the old pixels
    w.same("sample_sums behind foreign pixels", w.im.sample_sums(), rim.sample_sums())
    rim.close()
    w.walk([_op("flux", 3), _op("mass", 4)])
    w.im.set_nelec(pixels)
    assert w.samples_info(w.im) == (0, 0) and not w.im.stamp_mass_ready(w.ss)
    with pytest.raises(ValueError, match="resident photon split"):
        calls["flux"]()
    w.close()
