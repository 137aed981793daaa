"""ImageSet.photon_moments (cel_slice_sample with param = CEL_SLICE_MOMENTS, k_moments.h): the moments of every source's photons in the resident split.

The contract is integer equality.  For every (source, band) the six int64 sums N, Sx, Sy, Sxx, Sxy, Syy must equal, with
np.array_equal, the same sums formed in int64 numpy from what cel_samples_fetch hands out (boxes, offsets, data), dx and dy
counted from the low corner of the fetched box; a row without a patch is six zeros.  The kernel has two routes (the photon
lists, the dense patches) and deals a job of more than CEL_MOMENTS_SPLIT_PIXELS pixels to several blocks that add with integer
atomics: every test holds all of them to the same integers.

1. scene A, the slice contract's (SyntheticField(ctx, 24, 3, 128, 128, frac_gal=0.5), full-box resident split) plus one source
   off the frame, under CEL_OPT_PHOTON_LISTS = 0, 1, 2 (what the suite sets for the resident likelihoods) x CEL_OPT_KERNEL = 0, 1.
2. scene B, a 256 x 256 frame of hand-placed sources (boxes from the CPU oracle's rule, asserted on the fetched boxes): a
   149-pixel galaxy box (wider and taller than 64, dealt), a galaxy whose three bands' boxes are 63^2, 64^2 (= the threshold:
   whole) and 65^2 (dealt), a star cut to ONE column by the left edge, stars cut by each edge and by a corner, a source off the
   frame; and the same frame dark but for the LAST pixel of one patch.
3. a masked set under CEL_OPT_HONOUR_MASK = 1.
4. refusals (no split; a split of another catalogue; a split dropped by set_nelec, by another window) and the state: a call between a split and a sampler or
   the flux step changes none of their bits.
"""
import os
import re

import numpy as np
import pytest

import desi_mcmc_amd  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def split_pixels():
    """CEL_MOMENTS_SPLIT_PIXELS of include/celeste_hip.h"""
    with open(os.path.join(ROOT, "include", "celeste_hip.h")) as fh:
        return int(re.search(r"^\s*CEL_MOMENTS_SPLIT_PIXELS\s*=\s*(\d+)", fh.read(), flags=re.M).group(1))


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(cel):
    return cel.default_context(0)


class options(object):
    """context options set for a block and put back behind it"""

    def __init__(self, ctx, **kv):
        from desi_mcmc_amd import _lib
        self.ctx, self.kv = ctx, [(getattr(_lib, "CEL_OPT_" + k), v) for k, v in kv.items()]

    def __enter__(self):
        self.was = [(k, self.ctx.get_option(k)) for k, _ in self.kv]
        for k, v in self.kv:
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in reversed(self.was):
            self.ctx.set_option(k, v)


def reference_moments(iset):
    """the six sums in int64 numpy from cel_samples_fetch's boxes, offsets and data -> (S, B, 6), and the boxes"""
    boxes, offs, data = iset.fetch_samples()
    S, B = boxes.shape[:2]
    assert np.array_equal(data, np.rint(data)) and np.all(np.abs(data) < 2.0 ** 31)
    z_all = data.astype(np.int64)
    out = np.zeros((S, B, 6), dtype=np.int64)
    for s in range(S):
        for b in range(B):
            y0, y1, x0, x1 = (int(v) for v in boxes[s, b])
            i = s * B + b
            n = int(offs[i + 1] - offs[i])
            assert n == max(y1 - y0, 0) * max(x1 - x0, 0)
            if n == 0:
                continue
            z = z_all[offs[i]:offs[i + 1]].reshape(y1 - y0, x1 - x0)
            dy, dx = np.meshgrid(np.arange(y1 - y0, dtype=np.int64), np.arange(x1 - x0, dtype=np.int64), indexing="ij")
            out[s, b] = [z.sum(), (z * dx).sum(), (z * dy).sum(), (z * dx * dx).sum(), (z * dx * dy).sum(), (z * dy * dy).sum()]
    return out, boxes


def check_equal(iset):
    ref, boxes = reference_moments(iset)
    got = iset.photon_moments()
    assert got.dtype == np.int64 and got.shape == ref.shape
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:8]
    return got, boxes


def with_off_frame(src, bands):
    """the catalogue plus one star 100 px left of the frame: the reference's overlap test fails, it gets no patch"""
    from desi_mcmc_amd import synth
    far = synth.pixel2equa(bands[0], np.array([[-100.0, 40.0]]))
    return dict(type=np.append(src["type"], 0).astype(np.int32), radec=np.vstack([src["radec"], far]),
                counts=np.vstack([src["counts"], src["counts"][:1] * 0 + 5000.0]), shape=np.vstack([src["shape"], np.zeros((1, 4))]))


# ---- 1. scene A under every route ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_a(cel, ctx):
    from desi_mcmc_amd import synth
    f = synth.SyntheticField(ctx, 24, 3, 128, 128, frac_gal=0.5)
    src = with_off_frame(f.src, f.bands)
    sset = cel.SourceSet(ctx, 25, 3).set(src["type"], src["radec"], src["counts"], src["shape"])
    return f, src, sset


@gpu
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("lists", [0, 1, 2])
def test_moments_equal_the_fetched_patches_sums_under_every_route(scene_a, ctx, lists, kernel):
    f, src, sset = scene_a
    with options(ctx, SPLIT_FULL_BOX=1, PHOTON_LISTS=lists, KERNEL=kernel):
        f.images.photon_split_resident(sset, seed=5)
        got, boxes = check_equal(f.images)
    areas = (boxes[..., 1] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 2])
    assert np.all(areas[24] == 0) and np.all(got[24] == 0)                 # the source off the frame: no patch, six zeros
    assert np.all(got[areas == 0] == 0)
    assert np.array_equal(got[..., 0], f.images.sample_sums().astype(np.int64))
    assert (got[:24, :, 0] > 0).sum() > 60 and (got[..., 4] > 0).sum() > 60    # a scene with photons and second moments to sum


# ---- 2. scene B: shapes where it can go wrong ----------------------------------------------------------------------------------
HB = WB = 256
#            x       y      type  flux(nmgy)   shape
PLACED = [(128.3, 127.6, 1, 400., (0.5, 2.0, 30., 0.9)),        # 0  a box of ~149 px: wider and taller than 64, dealt
          (60.3, 190.6, 1, 200., (0.5, 0.5, 30., 0.3)),         # 1  boxes of 64^2, 65^2, 63^2: either side of the threshold
          (-20.9, 128.4, 0, 2e5, None),                         # 2  cut to ONE column by the left edge (bands 0 and 2)
          (5.2, 60.7, 0, 50., None),                            # 3  left edge
          (251.4, 90.2, 0, 50., None),                          # 4  right edge
          (150.6, 4.1, 0, 50., None),                           # 5  low rows
          (190.3, 252.8, 0, 50., None),                         # 6  high rows
          (3.4, 2.7, 0, 80., None),                             # 7  a corner
          (215.5, 40.5, 0, 30., None),                          # 8  a whole star box (the last-pixel case)
          (-100.0, 40.0, 0, 50., None)]                         # 9  off the frame: no patch


@pytest.fixture(scope="module")
def scene_b(cel, ctx):
    from desi_mcmc_amd import synth
    bands = synth.make_bands(HB, WB, 3)
    pix = np.array([[p[0], p[1]] for p in PLACED])
    typ = np.array([p[2] for p in PLACED], dtype=np.int32)
    flux = np.array([[p[3]] * 3 for p in PLACED])
    shape = np.array([p[4] if p[4] else (0., 0., 0., 0.) for p in PLACED])
    counts = flux / bands[None, :, 2] * bands[None, :, 1]
    iset = cel.ImageSet(ctx, bands, HB, WB)
    sset = cel.SourceSet(ctx, len(PLACED), 3).set(typ, synth.pixel2equa(bands[0], pix), counts, shape)
    iset.render(sset, loglik=False)
    nelec = np.random.RandomState(7).poisson(iset.model_images()).astype(np.float64)
    iset.set_nelec(nelec)
    return dict(iset=iset, sset=sset, nelec=nelec, bands=bands)


@gpu
@pytest.mark.parametrize("lists", [1, 2])
def test_hand_placed_patches_on_either_side_of_the_dealing_threshold(scene_b, ctx, lists):
    iset, sset = scene_b["iset"], scene_b["sset"]
    T = split_pixels()
    with options(ctx, SPLIT_FULL_BOX=1, PHOTON_LISTS=lists):
        iset.set_nelec(scene_b["nelec"])
        iset.photon_split_resident(sset, seed=3)
        got, boxes = check_equal(iset)
    ny, nx = boxes[..., 1] - boxes[..., 0], boxes[..., 3] - boxes[..., 2]
    area = ny.astype(np.int64) * nx
    print("box sides (ny, nx) per source and band:", [[(int(a), int(b)) for a, b in zip(r, c)] for r, c in zip(ny, nx)])
    print("photons per source and band:", got[..., 0].tolist())
    # the scene is what the docstring says it is
    assert np.all((nx[0] > 64) & (ny[0] > 64)) and np.all(area[0] > T) and np.all(got[0, :, 0] > 0)
    assert np.any(area[1] > T) and np.any((area[1] <= T) & (area[1] > 0.9 * T)) and np.all(got[1, :, 0] > 0)   # either side
    assert np.any((nx[2] == 1) & (ny[2] > 1)) and got[2][nx[2] == 1][:, 0].sum() > 0                            # one column, lit
    assert np.all(boxes[3, :, 2] == 0) and np.all(boxes[4, :, 3] == WB) and np.all(boxes[5, :, 0] == 0) and np.all(boxes[6, :, 1] == HB)
    assert np.all(boxes[7, :, 0] == 0) and np.all(boxes[7, :, 2] == 0) and np.all(area[7] > 0)
    assert np.all(got[3:9, :, 0] > 0)
    assert np.all(area[9] == 0) and np.all(got[9] == 0)


@gpu
@pytest.mark.parametrize("lists", [1, 2])
def test_a_patch_whose_only_photon_sits_in_its_last_pixel(scene_b, ctx, lists):
    iset, sset = scene_b["iset"], scene_b["sset"]
    s = 8
    boxes, status = iset.source_boxes(sset)                      # (B, S, 4) = y0, y1, x0, x1
    assert np.all(status[:, s] > 0)
    nelec = np.zeros((3, HB, WB))
    for b in range(3):
        nelec[b, boxes[b, s, 1] - 1, boxes[b, s, 3] - 1] = 1000.0
    eps = list(iset.eps[:3])
    try:
        with options(ctx, SPLIT_FULL_BOX=1, PHOTON_LISTS=lists):
            iset.set_nelec(nelec)
            for b in range(3):
                iset.set_epsilon(b, 1e-12)                       # (the sky takes none of them)
            iset.photon_split_resident(sset, seed=4)
            got, sb = check_equal(iset)
    finally:
        for b in range(3):
            iset.set_epsilon(b, eps[b])
    for b in range(3):
        y0, y1, x0, x1 = (int(v) for v in sb[s, b])
        assert (y0, y1, x0, x1) == tuple(int(v) for v in boxes[b, s])
        dx, dy = x1 - x0 - 1, y1 - y0 - 1
        N = int(got[s, b, 0])
        assert N > 0 and list(got[s, b]) == [N, N * dx, N * dy, N * dx * dx, N * dx * dy, N * dy * dy]


# ---- 3. a masked set -----------------------------------------------------------------------------------------------------------
@gpu
def test_masked_set_under_honour_mask(cel, ctx, scene_a):
    f, src, sset = scene_a
    mask = np.zeros((3, 128, 128), dtype=bool)
    rs = np.random.RandomState(11)
    mask[0, :, 40:44] = True                                     # bad columns, a block, scattered pixels
    mask[1, 60:90, 20:70] = True
    mask[2] = rs.rand(128, 128) < 0.05
    pix = np.floor(f.src["pix"]).astype(int)
    for s in range(6):                                           # and the core pixel of six sources in every band
        mask[:, min(pix[s, 1], 127), min(pix[s, 0], 127)] = True
    mset = cel.ImageSet(ctx, f.bands, 128, 128, nelec=np.where(mask, np.nan, f.nelec))
    assert int(mset.masked.sum()) == int(mask.sum())
    with pytest.raises(Exception):                               # a masked set holds no split while the option is off ...
        mset.photon_split_resident(sset, seed=5)
    with pytest.raises(ValueError, match="resident photon split"):
        mset.photon_moments()                                    # ... so the moments refuse it
    with options(ctx, SPLIT_FULL_BOX=1, HONOUR_MASK=1):
        mset.photon_split_resident(sset, seed=5)
        got, boxes = check_equal(mset)
        sums = mset.sample_sums()
        _, offs, data = mset.fetch_samples()
    assert np.array_equal(got[..., 0], sums.astype(np.int64)) and got[..., 0].sum() > 0
    # no contribution from a masked pixel: the moments of the patches with their masked pixels struck out are the same
    S, B = boxes.shape[:2]
    struck, hit = np.zeros_like(got), 0
    for s in range(S):
        for b in range(B):
            y0, y1, x0, x1 = (int(v) for v in boxes[s, b])
            if y1 <= y0 or x1 <= x0:
                continue
            i = s * B + b
            z = data[offs[i]:offs[i + 1]].astype(np.int64).reshape(y1 - y0, x1 - x0)
            m = mask[b, y0:y1, x0:x1]
            hit += int(m.sum())
            assert not np.any(z[m])
            z = np.where(m, 0, z)
            dy, dx = np.meshgrid(np.arange(y1 - y0, dtype=np.int64), np.arange(x1 - x0, dtype=np.int64), indexing="ij")
            struck[s, b] = [z.sum(), (z * dx).sum(), (z * dy).sum(), (z * dx * dx).sum(), (z * dx * dy).sum(), (z * dy * dy).sum()]
    assert hit > 1000 and np.array_equal(got, struck)
    mset.close()


# ---- 4. state and refusals -----------------------------------------------------------------------------------------------------
def raw_moments(iset, srcs, out):
    """cel_slice_sample(param = CEL_SLICE_MOMENTS) as a C caller makes it; srcs None: no catalogue named"""
    import ctypes as C
    from desi_mcmc_amd import _lib as L
    return L.lib().cel_slice_sample(iset._h, None if srcs is None else srcs._h, L.CEL_SLICE_MOMENTS, None, None, 0, 0, 0, 0.0, 0.0,
                                    C.c_uint64(0), 0, None, None, None if out is None else out.ctypes.data_as(L.c_int64_p))


def refused_untouched(iset, cel, srcs=None):
    """the raw call on a sentinel-filled array, with and without the catalogue named: CEL_ERR_INVALID in the resident-split words
    (need_resident_split's own when a catalogue is named), the array as it was"""
    from desi_mcmc_amd import _lib as L
    out = np.full((25, iset.B, 6), -7, dtype=np.int64)
    for s in (None, srcs):
        with pytest.raises(ValueError, match="needs a resident photon split"):
            L.check(raw_moments(iset, s, out))
        assert np.all(out == -7)
    with pytest.raises(ValueError, match="resident photon split"):
        iset.photon_moments()


@gpu
def test_refuses_without_a_resident_split(cel, ctx, scene_a):
    from desi_mcmc_amd import _lib as L
    f, src, sset = scene_a
    iset = cel.ImageSet(ctx, f.bands, 128, 128, nelec=f.nelec)
    refused_untouched(iset, cel, sset)                           # no split yet
    iset.photon_split_resident(sset, seed=5)
    named = np.zeros((25, 3, 6), dtype=np.int64)
    L.check(raw_moments(iset, sset, named))
    assert named[..., 0].sum() > 0 and np.array_equal(named, iset.photon_moments())      # the catalogue named or not: the same
    fewer = cel.SourceSet(ctx, 24, 3).set(src["type"][:24], src["radec"][:24], src["counts"][:24], src["shape"][:24])
    sent = np.full((25, 3, 6), -7, dtype=np.int64)
    with pytest.raises(ValueError, match="of these 24 sources"):     # a split of another catalogue is not this one's
        L.check(raw_moments(iset, fewer, sent))
    assert raw_moments(iset, sset, None) == L.CEL_ERR_INVALID and np.all(sent == -7)
    iset.set_nelec(f.nelec)                                      # new pixels drop the split
    refused_untouched(iset, cel, sset)
    iset.photon_split_resident(sset, seed=5)
    assert iset.photon_moments()[..., 0].sum() > 0
    iset.set_window(32, 128 + 64)                                # another window drops it
    refused_untouched(iset, cel, sset)
    iset.close()


@gpu
def test_a_moments_call_changes_nothing_a_sampler_or_the_flux_step_returns(cel, ctx, scene_a):
    f, src, sset = scene_a
    S = 25
    shapes = np.tile(np.array([0.4, 1.1, 50., 0.6]), (S, 1))
    h = np.zeros(S)
    letter, calib, kappa = np.arange(3, dtype=np.int32), f.bands[:, 2].copy(), f.bands[:, 1].copy()

    def run(step, with_moments):
        sset.set(src["type"], src["radec"], src["counts"], src["shape"])
        f.images.set_nelec(f.nelec)
        f.images.photon_split_resident(sset, seed=5)
        mom = f.images.photon_moments() if with_moments else None
        if step == "slice":
            x, llh, st = f.images.slice_sample(sset, 0, 1e-3, 11)
            out = (x, llh, st["evals"])
        elif step == "type":
            typ, shp, la, st = f.images.type_move(sset, shapes, h, 12)
            out = (typ, shp, la, st["evals"], st["accepted"])
        else:
            out = f.images.flux_conditionals(sset, 13, 5.0, 0.005, letter, calib, kappa)
        return out + tuple(sset.get()), mom

    first = None
    for step in ("slice", "type", "flux"):
        run(step, False)                                         # (so that both runs compared follow the same kind of call)
        plain, _ = run(step, False)
        between, mom = run(step, True)
        assert len(plain) == len(between)
        for a, b in zip(plain, between):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), step
        first = mom if first is None else first
        assert np.array_equal(mom, first)                        # and the same split gives the same moments every time


# ---- CPU: no new entry point, the constants ----------------------------------------------------------------------------------------
def test_the_moments_add_no_symbol_and_the_constants_agree():
    """the moments enter as a new value of cel_slice_sample's param (as the type move and the HMC step did): the boundary keeps its
    entry points, the header and the binding name the same two numbers, and the kernel's threshold is the header's"""
    from desi_mcmc_amd import _lib
    names = [s[0] for s in _lib.SYMBOLS]
    assert "cel_samples_moments" not in names and "cel_slice_sample" in names
    with open(os.path.join(ROOT, "include", "celeste_hip.h")) as fh:
        header = fh.read()
    assert "cel_samples_moments" not in header
    assert int(re.search(r"^\s*CEL_SLICE_MOMENTS\s*=\s*(\d+)", header, flags=re.M).group(1)) == _lib.CEL_SLICE_MOMENTS == 10
    assert split_pixels() == _lib.CEL_MOMENTS_SPLIT_PIXELS == 4096
    with open(os.path.join(ROOT, "desi-mcmc_amd", "csrc", "k_moments.h")) as fh:
        assert "#define MOM_SPLIT_PIXELS CEL_MOMENTS_SPLIT_PIXELS" in fh.read()
