"""Lock-step HMC on location and shape for every source, on the device: cel_slice_sample(param = 3), k_hmc.h,
ImageSet.hmc_step, ModelGibbs.resample_hmc.

  1. restated from public calls: a per-chain leapfrog on Python floats, gradients from patch_loglik_resident_grad and values from
     patch_loglik_resident (one proposal per call) -- q, the returned momentum and the decision bit for bit, log alpha to 8 ulp
  2. host engine against device engine through ModelGibbs, three sweep(hmc=True)
  3. contract: frozen coordinates, chains left alone, the reject rule, the catalogue follows, stats
  4. support: a galaxy at rho = 0.999 pushed outward
  5. refusals, each with sentinel-filled outputs intact
  6. reversibility on the device
  7. law: one star against a fixed split

The scene: 2 bands on a 96 x 112 frame (tests/test_patch_grad.py's frame and shapes), seven chains: a star (faint: tests 6 and 7
move it by pixels), a star cut by the frame's edge, a type-1 galaxy, a type-1 galaxy under the sigma floor, a type-2 source, a
star whose chain id is negative, a star beside the frame that has no patch.  The data is a Poisson draw from the scene's model
image; the split is the full-box resident split (CEL_OPT_SPLIT_FULL_BOX = 1) of seed 9.
"""
import ctypes as C
import math

import numpy as np
import pytest

H, W, B = 96, 112, 2
gpu = pytest.mark.gpu
C_STAR, C_EDGE, C_GAL, C_FLOOR, C_T2, C_OTHER, C_NOPATCH = range(7)
S = 7
RUNNING = [C_STAR, C_EDGE, C_GAL, C_FLOOR]
PHI_MAX = 180.0


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
        pix = np.array([[31.3, 40.2], [2.3, 50.7], [55.4, 47.3], [88.6, 21.1], [22.1, 78.5], [92.3, 74.6], [-60.0, 50.0]])
        self.typ = np.array([0, 0, 1, 1, 2, 0, 0], dtype=np.int32)
        self.shape = np.zeros((S, 4))
        self.shape[C_GAL] = [0.5, 3.0, 30.0, 0.6]
        self.shape[C_FLOOR] = [0.4, 0.02, 40.0, 0.7]           # below k_prep's floor 1/30
        self.shape[C_T2] = [0.35, 1.2, 0.3, 0.9]               # theta, W00, W01, W11
        self.counts = np.array([[120.0, 160.0], [6000.0, 9000.0], [40000.0, 50000.0], [7000.0, 5000.0], [15000.0, 11000.0],
                                [5000.0, 7000.0], [9000.0, 8000.0]])
        self.radec = synth.pixel2equa(self.bands[0], pix)
        self.iset = cel.ImageSet(self.ctx, self.bands, H, W)
        self.cat = cel.SourceSet(self.ctx, S, B)
        self.reset()
        self.iset.render(self.cat)
        self.nelec = np.random.RandomState(5).poisson(self.iset.model_images()).astype(np.float64)
        self.iset.set_nelec(self.nelec)
        self.split(self.iset)
        self.sums = self.iset.sample_sums()
        assert np.all(self.sums[RUNNING].sum(axis=1) > 100) and self.sums[C_NOPATCH].sum() == 0
        assert np.all(self.iset.sample_box_areas()[C_NOPATCH] == 0)
        self.ids = np.arange(S, dtype=np.int32)
        self.ids[C_OTHER] = -1
        ups = self.bands[0][28:32]
        self.pix_deg = math.sqrt(abs(ups[0] * ups[3] - ups[1] * ups[2]))
        self.one = cel.SourceSet(self.ctx, 1, B)

    def split(self, iset):
        was = self.ctx.get_option(self.L.CEL_OPT_SPLIT_FULL_BOX)
        self.ctx.set_option(self.L.CEL_OPT_SPLIT_FULL_BOX, 1)
        try:
            iset.photon_split_resident(self.cat, seed=9)
        finally:
            self.ctx.set_option(self.L.CEL_OPT_SPLIT_FULL_BOX, was)

    def reset(self, radec=None, shape=None):
        """the catalogue back at the scene's rows (the split stays: it is of these S sources)"""
        self.cat.set(self.typ, self.radec if radec is None else radec, self.counts, self.shape if shape is None else shape)

    def q0(self):
        return np.concatenate([self.radec, self.shape], axis=1)

    def default_imass(self):
        """the library's scale-free start (ModelGibbs.hmc_default_imass)"""
        N = np.maximum(self.sums.sum(axis=1), 1.0)
        im = np.empty((S, 6))
        im[:, :2] = (self.pix_deg ** 2 / N)[:, None]
        im[:, 2:] = (1.0 / N)[:, None]
        return im

    def momentum(self, imass, seed):
        z = np.random.RandomState(seed).randn(S, 6)
        return np.where(imass > 0, z / np.sqrt(np.where(imass > 0, imass, 1.0)), 0.0)

    # -- the public calls, one proposal at a time
    def value(self, s, q, phi_max):
        self.one.set(self.typ[s:s + 1], np.array([q[:2]]), self.counts[s:s + 1], np.array([q[2:]]))
        v = float(self.iset.patch_loglik_resident(self.one, np.array([s], dtype=np.int32))[0])
        pri = 0.0
        if self.typ[s] == 1 and phi_max > 0.0:
            s2 = q[3] * q[3]
            pri = -2.0 * math.log(s2) - 1.0 / s2
        return v + pri

    def gradient(self, s, q, phi_max):
        self.one.set(self.typ[s:s + 1], np.array([q[:2]]), self.counts[s:s + 1], np.array([q[2:]]))
        _, gr, _, gs = self.iset.patch_loglik_resident_grad(self.one, np.array([s], dtype=np.int32))
        g = [float(gr[0, 0]), float(gr[0, 1])] + ([float(x) for x in gs[0]] if self.typ[s] == 1 else [0.0] * 4)
        if self.typ[s] == 1 and phi_max > 0.0:
            sg = q[3]
            g[3] = g[3] + (2.0 / ((sg * sg) * sg) - 4.0 / sg)
        return g

    def inside(self, s, q, phi_max):
        if not all(math.isfinite(x) for x in (q if self.typ[s] == 1 else q[:2])):
            return False
        if self.typ[s] != 1:
            return True
        ok = 0.0 < q[2] < 1.0 and q[3] > 0.0 and 0.0 < q[5] < 1.0
        return ok and (not phi_max > 0.0 or 0.0 < q[4] < phi_max)

    def restated(self, s, q0, p0, im, eps, L, phi_max, log_u):
        """header comment of param 3 on Python floats -> (q, p, log alpha, accepted, evaluations, v0, v1)"""
        nd = 6 if self.typ[s] == 1 else 2
        q = [float(x) for x in q0]
        p = [float(p0[i]) if i < nd else 0.0 for i in range(6)]
        im = [float(im[i]) if i < nd else 0.0 for i in range(6)]
        pstart = list(p)

        def kin(x):
            acc = 0.0
            for i in range(6):
                acc = acc + im[i] * (x[i] * x[i])
            return 0.5 * acc

        evals, dead = 0, False
        for l in range(L + 1):
            g = self.gradient(s, q, phi_max)
            evals += 1
            if not all(math.isfinite(x) for x in g):
                dead = True
                break
            h = 0.5 * eps if l in (0, L) else eps
            for i in range(nd):
                p[i] = p[i] + h * g[i]
            if l < L:
                for i in range(nd):
                    q[i] = q[i] + (eps * im[i]) * p[i]
                if not self.inside(s, q, phi_max):
                    dead = True
                    break
        q0 = [float(x) for x in q0]
        if dead:
            return q0, [-x for x in pstart], -math.inf, False, evals, None, None
        v0, v1 = self.value(s, q0, phi_max), self.value(s, q, phi_max)
        la = (v1 - v0) + (kin(pstart) - kin(p))
        if log_u < la:
            return q, p, la, True, evals, v0, v1
        return q0, [-x for x in pstart], la, False, evals, v0, v1


@pytest.fixture(scope="module")
def scene(cel):
    return Scene(cel)


def _log_u(seed, ids):
    from desi_mcmc_amd.util.infer.slicesample import ChainStreams
    return np.log(ChainStreams(seed, ids).uniform(np.arange(len(ids))))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("phi_max", [PHI_MAX, 0.0])
def test_restated_from_public_calls(scene, L, phi_max):
    _restated_step(scene, L, phi_max)


@gpu
def test_the_direct_kernel_backs_the_step(scene):
    """1., CEL_OPT_KERNEL = 0: no block lists, k_patch_ll<int> over all 2 S B jobs of q0 / qL; the restatement is taken under the
    same option, so the bar stands"""
    L = scene.L
    before = scene.ctx.get_option(L.CEL_OPT_KERNEL)
    scene.ctx.set_kernel("direct")
    try:
        _restated_step(scene, 1, PHI_MAX)
    finally:
        scene.ctx.set_option(L.CEL_OPT_KERNEL, before)


def _restated_step(sc, L, phi_max):
    eps, seed = 0.4, 21 + L
    imass = sc.default_imass()
    imass[C_FLOOR, 3] *= 1e-4                 # (the prior's wall at sigma = 0.02 is steep: keep the trajectory inside the support)
    p0 = sc.momentum(imass, seed=3 + L)
    sc.reset()
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=phi_max, chain_ids=sc.ids)
    log_u = _log_u(seed, np.arange(S))
    evals = accepted = 0
    for s in RUNNING:
        qr, pr, lar, acc, ev, v0, v1 = sc.restated(s, sc.q0()[s], p0[s], imass[s], eps, L, phi_max, log_u[s])
        evals += ev
        accepted += int(acc)
        print("RESTATED L %d phi_max %g chain %d: log alpha %.17g (device %.17g), log u %.6f, accepted %s, v0 %r v1 %r"
              % (L, phi_max, s, lar, la[s], log_u[s], acc, v0, v1))
        assert v0 is not None, "the trajectory of chain %d died: choose other inputs" % s
        bar = 8 * np.spacing(max(abs(v0), abs(v1), 1.0))
        assert abs(la[s] - lar) <= bar, (s, la[s], lar, bar)
        assert abs(log_u[s] - lar) > 2 * bar, "the decision lies inside the band: change the seed"
        assert np.array_equal(q[s], np.array(qr)), (s, q[s], qr)
        assert np.array_equal(p[s], np.array(pr)), (s, p[s], pr)
        assert acc == bool(not np.array_equal(q[s], sc.q0()[s]))
    assert st["steps"] == L and st["evals"] == evals == len(RUNNING) * (L + 1) and st["accepted"] == accepted


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_host_engine_against_device_engine(cel):
    from desi_mcmc_amd import celeste_mcmc, synth
    Sf = 12
    ctx = cel.Context(0)
    f0 = synth.SyntheticField(ctx, Sf, B, H, W, frac_gal=0.5, seed=23)
    flux5 = np.full((Sf, 5), 3.0)
    flux5[:, :B] = f0.src["flux"]
    g = {}
    for e in ("host", "auto"):
        imgs = cel.ImageSet(ctx, f0.bands, H, W)
        imgs.set_nelec(f0.nelec)
        gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W)
        g[e] = celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5, engine=e)
    assert g["auto"]._hmc_engine_on_device() and not g["host"]._hmc_engine_on_device()
    start = np.concatenate([g["auto"].u, g["auto"].shape], axis=1)
    for sweep in range(3):
        for e in g:
            g[e].sweep(hmc=True)
        for name in ("typ", "u", "fluxes", "shape", "_hmc_p"):
            assert np.array_equal(getattr(g["host"], name), getattr(g["auto"], name)), (sweep, name)
        assert g["host"].timing["hmc_evals"] == g["auto"].timing["hmc_evals"] > 0
        assert g["host"].timing["hmc_accepted"] == g["auto"].timing["hmc_accepted"]
    t = g["auto"].timing
    print("ENGINES: hmc evals %d, accepted %d of %d updates" % (t["hmc_evals"], t["hmc_accepted"], 3 * Sf))
    assert t["hmc_accepted"] > 0 and np.any(np.concatenate([g["auto"].u, g["auto"].shape], axis=1) != start)
    assert np.any(g["auto"]._hmc_p != 0.0) and np.all(g["auto"]._hmc_p[g["auto"].typ == 0, 2:] == 0.0)
    # without the flag the chain is that of a run that never mentions it
    plain = {}
    for k in ("plain", "off"):
        imgs = cel.ImageSet(ctx, f0.bands, H, W)
        imgs.set_nelec(f0.nelec)
        gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W)
        plain[k] = celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5)
    plain["plain"].sweep()
    plain["off"].sweep(hmc=False)
    for name in ("u", "fluxes", "shape"):
        assert np.array_equal(getattr(plain["plain"], name), getattr(plain["off"], name))
    with pytest.raises(ValueError, match="exact"):
        celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5, conditional="exact").resample_hmc()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_contract(scene):
    sc = scene
    L, seed = 3, 31
    imass = sc.default_imass()
    imass[C_FLOOR, 3] *= 1e-4
    imass[C_GAL, 4] = 0.0                     # the galaxy's phi is frozen
    imass[C_EDGE, 1] = 0.0                    # ... and the edge star's dec
    p0 = sc.momentum(imass, seed=7)
    p0[C_GAL, 4] = 0.7                        # (a frozen coordinate's momentum is still kicked; its position is not)
    p0[[C_T2, C_OTHER, C_NOPATCH]] = np.random.RandomState(1).randn(3, 6)
    q0 = sc.q0()
    alone = [C_T2, C_OTHER, C_NOPATCH]
    # a small step: every running chain accepts (log alpha ~ 0); then a huge one: the stars are rejected
    for eps, want in ((0.02, True), (40.0, False)):
        sc.reset()
        q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=PHI_MAX, chain_ids=sc.ids)
        print("CONTRACT eps %g: log alpha %s, stats %s" % (eps, la, st))
        acc = np.array([not np.array_equal(q[s], q0[s]) for s in range(S)])
        assert np.array_equal(q[alone], q0[alone]) and np.array_equal(p[alone], p0[alone]) and np.all(np.isnan(la[alone]))
        assert np.array_equal(q[[C_STAR, C_EDGE], 2:], q0[[C_STAR, C_EDGE], 2:])              # a star's shape row
        assert q[C_GAL, 4] == q0[C_GAL, 4] and q[C_EDGE, 1] == q0[C_EDGE, 1]                # frozen coordinates
        if want:
            assert np.all(np.isfinite(la[RUNNING])) and acc[RUNNING].all() and np.all(np.abs(la[RUNNING]) < 0.5)
            assert np.all(q[C_GAL, [0, 1, 2, 3, 5]] != q0[C_GAL, [0, 1, 2, 3, 5]]) and q[C_EDGE, 0] != q0[C_EDGE, 0]
            assert st["evals"] == len(RUNNING) * (L + 1)
        else:
            assert not acc[C_STAR] and not acc[C_EDGE]
        for s in RUNNING:
            if not acc[s]:                                                                    # the reject rule
                keep = 6 if sc.typ[s] == 1 else 2
                assert np.array_equal(q[s], q0[s]) and np.array_equal(p[s, :keep], -p0[s, :keep]) and np.all(p[s, keep:] == 0.0)
        assert st["steps"] == L and st["accepted"] == int(acc.sum()) and st["launches"] >= 4 * (L + 1) + 4
        # the catalogue on the device holds the returned rows
        own = np.arange(S, dtype=np.int32)
        after = sc.iset.patch_loglik_resident(sc.cat, own)
        fresh = sc.cel.SourceSet(sc.ctx, S, B).set(sc.typ, q[:, :2], sc.counts, q[:, 2:])
        assert np.array_equal(after, sc.iset.patch_loglik_resident(fresh, own))
        if want:
            sc.reset()
            assert not np.array_equal(after[RUNNING], sc.iset.patch_loglik_resident(sc.cat, own)[RUNNING])
    sc.reset()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_support(scene):
    sc = scene
    shape = sc.shape.copy()
    shape[C_GAL, 3] = 0.999
    sc.reset(shape=shape)
    imass, p0 = np.zeros((S, 6)), np.zeros((S, 6))
    imass[C_GAL, 5], p0[C_GAL, 5] = 1.0, 1000.0              # the first drift: rho = 0.999 + 1e-3 (1000 + 5e-4 g) > 1
    ids = np.full(S, -1, dtype=np.int32)
    ids[C_GAL] = C_GAL
    L = 4
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, 1e-3, L, 5, phi_max=PHI_MAX, chain_ids=ids)
    assert la[C_GAL] == -np.inf and np.array_equal(q[C_GAL, 2:], shape[C_GAL]) and np.array_equal(q[C_GAL, :2], sc.radec[C_GAL])
    assert np.array_equal(p[C_GAL], -p0[C_GAL])
    assert st["evals"] == 1 and st["accepted"] == 0, st                                      # its evaluations stopped
    assert np.all(np.isnan(np.delete(la, C_GAL)))
    # inward it runs to the end
    p0[C_GAL, 5] = -1000.0
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, 1e-6, L, 5, phi_max=PHI_MAX, chain_ids=ids)
    assert np.isfinite(la[C_GAL]) and st["evals"] == L + 1
    sc.reset()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _raw(sc, iset, param, dirs, numdir, x, la, stats, sigma=0.1, rounds=2, ids=None, srcs=None):
    L = sc.L
    return L.lib().cel_slice_sample(iset._h, (sc.cat if srcs is None else srcs)._h, param,
                                    None if ids is None else ids.ctypes.data_as(L.c_int32_p),
                                    None if dirs is None else L.dptr(dirs), numdir, 0, 0, float(sigma), PHI_MAX, C.c_uint64(1), rounds,
                                    L.dptr(x), L.dptr(la), stats.ctypes.data_as(L.c_int64_p))


@gpu
def test_refusals(scene):
    sc = scene
    L = sc.L
    sc.reset()
    imass = sc.default_imass()
    dirs = np.ascontiguousarray(np.concatenate([sc.momentum(imass, 2), imass], axis=1))
    x, la, stats = np.full(S * 12 + 3, -7.25), np.full(S + 3, -7.25), np.full(4, -7, dtype=np.int64)
    before = sc.iset.patch_loglik_resident(sc.cat, np.arange(S, dtype=np.int32))

    def last_error():
        return L.lib().cel_last_error().decode("utf-8", "replace")

    def refused(rc, word=None):
        assert rc == L.CEL_ERR_INVALID and np.all(x == -7.25) and np.all(la == -7.25) and np.all(stats == -7)
        if word:
            assert word in last_error(), last_error()

    refused(_raw(sc, sc.iset, 3, None, 12, x, la, stats), "param")
    refused(_raw(sc, sc.iset, 3, dirs, 11, x, la, stats), "numdir = 12")
    # the existing type-move test's call: rows of 5, numdir = 1, an x_out of S * 5 doubles
    x5 = np.full(S * 5, -7.25)
    d5 = np.ascontiguousarray(dirs[:, :5])
    assert _raw(sc, sc.iset, 3, d5, 1, x5, la, stats) == L.CEL_ERR_INVALID and "param" in last_error() and np.all(x5 == -7.25)
    refused(L.CEL_ERR_INVALID)
    refused(_raw(sc, sc.iset, 4, dirs, 12, x, la, stats), "param must be")
    refused(_raw(sc, sc.iset, -1, dirs, 12, x, la, stats), "param must be")
    refused(_raw(sc, sc.iset, 3, dirs, 12, x, la, stats, sigma=0.0), "sigma")
    refused(_raw(sc, sc.iset, 3, dirs, 12, x, la, stats, rounds=0))
    refused(_raw(sc, sc.iset, 3, dirs, 12, x, la, stats, rounds=1025), "1024")
    for col, bad in ((1, np.nan), (0, np.inf), (6, -1e-9), (7, np.inf), (9, np.nan)):
        d = dirs.copy()
        d[C_GAL, col] = bad
        refused(_raw(sc, sc.iset, 3, d, 12, x, la, stats), "chain %d" % C_GAL)
    # ... but not in a chain that does not run, nor in a star's entries 2-5
    d = dirs.copy()
    d[C_OTHER, 0] = np.nan
    d[C_T2, 8] = -1.0
    d[C_STAR, 3] = np.nan
    d[C_STAR, 10] = -1.0
    xo, lo, so = np.zeros(S * 12), np.zeros(S), np.zeros(4, dtype=np.int64)
    assert _raw(sc, sc.iset, 3, d, 12, xo, lo, so, sigma=1e-3, ids=sc.ids) == L.CEL_OK
    assert np.all(np.isfinite(lo[RUNNING])) and np.all(np.isfinite(xo.reshape(S, 12)[RUNNING]))
    sc.reset()
    # the exact conditional: refused in the words of location_loglik_grad's; the option is the caller's to restore
    was = sc.ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL)
    sc.ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 1)
    try:
        refused(_raw(sc, sc.iset, 3, dirs, 12, x, la, stats), "stamp-mass term has no analytic derivative yet")
        with pytest.raises(ValueError, match="no analytic derivative"):
            sc.iset.hmc_step(sc.cat, dirs[:, :6], dirs[:, 6:], 0.1, 2, 1)
        assert sc.ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 1
    finally:
        sc.ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, was)
    # no resident split of these sources
    bare = sc.cel.ImageSet(sc.ctx, sc.bands, H, W)
    bare.set_nelec(sc.nelec)
    refused(_raw(sc, bare, 3, dirs, 12, x, la, stats), "resident photon split")
    fewer = sc.cel.SourceSet(sc.ctx, S - 1, B).set(sc.typ[:-1], sc.radec[:-1], sc.counts[:-1], sc.shape[:-1])
    refused(_raw(sc, sc.iset, 3, np.ascontiguousarray(dirs[:-1]), 12, x, la, stats, srcs=fewer), "resident photon split")
    # a masked set
    ne = sc.nelec.copy()
    ne[0, 5, 5] = np.nan
    masked = sc.cel.ImageSet(sc.ctx, sc.bands, H, W)
    masked.set_nelec(ne)
    refused(_raw(sc, masked, 3, dirs, 12, x, la, stats), "mask")
    # a row window (with a split of its own: only the window is at stake)
    win = sc.cel.ImageSet(sc.ctx, sc.bands, 64, W)
    win.set_window(16, H)
    win.set_nelec(np.ascontiguousarray(sc.nelec[:, 16:80, :]))
    sc.split(win)
    refused(_raw(sc, win, 3, dirs, 12, x, la, stats), "row window")
    with pytest.raises(ValueError):
        sc.iset.hmc_step(sc.cat, dirs[:, :5], dirs[:, 6:], 0.1, 2, 1)
    # nothing moved the catalogue
    assert np.array_equal(before, sc.iset.patch_loglik_resident(sc.cat, np.arange(S, dtype=np.int32)))


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
def _star_scale(sc):
    """(inverse mass, widths) of the faint star's location from the curvature of its conditional: central differences of
    the analytic gradient half a pixel apart"""
    h = 0.5 * sc.pix_deg
    q = list(sc.q0()[C_STAR])
    w = []
    for i in range(2):
        a, b = list(q), list(q)
        a[i] += h
        b[i] -= h
        c = -(sc.gradient(C_STAR, a, 0.0)[i] - sc.gradient(C_STAR, b, 0.0)[i]) / (2 * h)
        assert c > 0
        w.append(1.0 / math.sqrt(c))
    return np.array(w) ** 2, np.array(w)


@gpu
def test_reversibility_on_the_device(scene):
    """An accepted update that carries the faint star about three pixels in ra and in dec (twelve steps of 0.075 in units of its
    oscillation: ra is 253 degrees, one ulp is 2.8e-14 degrees, and 1e-9 of a three-pixel journey is twelve of them), then the
    call from (q1, -p1)"""
    sc = scene
    var, width = _star_scale(sc)
    eps, L = 0.075, 12
    ids = np.full(S, -1, dtype=np.int32)
    ids[C_STAR] = C_STAR
    imass, p0 = np.zeros((S, 6)), np.zeros((S, 6))
    imass[C_STAR, :2] = var                                      # unit frequency in both coordinates
    travel = 3.0 * sc.pix_deg * np.array([1.0 / math.cos(math.radians(sc.radec[C_STAR, 1])), -1.0])
    p0[C_STAR, :2] = travel / (var * math.sin(eps * L))
    sc.reset()
    q0 = sc.q0()[C_STAR]

    def accepted_call(p):
        for seed in range(1, 65):                                # a seed that accepts: a rejected call leaves the catalogue where it was
            q, pn, la, st = sc.iset.hmc_step(sc.cat, p, imass, eps, L, seed, phi_max=PHI_MAX, chain_ids=ids)
            if st["accepted"] == 1:
                return q[C_STAR], pn[C_STAR], la[C_STAR], seed
        raise AssertionError("no seed in 1..64 accepts (log alpha %g)" % la[C_STAR])

    q1, p1, la1, seed1 = accepted_call(p0)
    pb = np.zeros((S, 6))
    pb[C_STAR] = -p1
    q2, p2, la2, seed2 = accepted_call(pb)
    dist = np.abs(q1[:2] - q0[:2])
    miss = np.abs(q2[:2] - q0[:2])
    print("REVERSIBILITY on the device: travelled %s deg (%s px), log alpha %.4f there (seed %d) and %.4f back (seed %d); "
          "returned within %s of the distance (%s ulp)" % (dist, dist / sc.pix_deg, la1, seed1, la2, seed2, miss / dist,
                                                            miss / np.spacing(np.abs(q0[:2]))))
    assert np.all(dist > sc.pix_deg)
    assert np.all(miss <= 1e-9 * dist), (miss, dist)
    assert np.allclose(-p2[:2], p0[C_STAR, :2], rtol=1e-6)
    sc.reset()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_law_of_one_star(scene):
    """400 updates (L = 3, full refresh, the scale-free default's eps and inverse mass) of the faint star against the fixed
    split: the means of ra and dec against those of exp(v) by quadrature on a 41 x 41 grid of +-6 posterior widths"""
    sc = scene
    _, width = _star_scale(sc)
    # quadrature: one call scores the grid
    ax = np.linspace(-6.0, 6.0, 41)
    R, Dc = np.meshgrid(sc.radec[C_STAR, 0] + ax * width[0], sc.radec[C_STAR, 1] + ax * width[1], indexing="ij")
    n = R.size
    grid = sc.cel.SourceSet(sc.ctx, n, B).set(np.zeros(n, dtype=np.int32), np.column_stack([R.ravel(), Dc.ravel()]),
                                             np.tile(sc.counts[C_STAR], (n, 1)), np.zeros((n, 4)))
    v = sc.iset.patch_loglik_resident(grid, np.full(n, C_STAR, dtype=np.int32)).reshape(41, 41)
    wgt = np.exp(v - v.max())
    wgt /= wgt.sum()
    assert wgt[0].max() < 1e-6 and wgt[-1].max() < 1e-6 and wgt[:, 0].max() < 1e-6 and wgt[:, -1].max() < 1e-6
    mean = np.array([(wgt * R).sum(), (wgt * Dc).sum()])
    sd = np.sqrt(np.array([(wgt * (R - mean[0]) ** 2).sum(), (wgt * (Dc - mean[1]) ** 2).sum()]))
    # the chain
    N, NB, L, eps = 400, 20, 3, 0.5
    imass = np.zeros((S, 6))
    imass[C_STAR, :2] = sc.default_imass()[C_STAR, :2]
    ids = np.full(S, -1, dtype=np.int32)
    ids[C_STAR] = C_STAR
    rs = np.random.RandomState(12)
    sc.reset()
    xs, accepted = np.empty((N, 2)), 0
    for k in range(N):
        p0 = np.zeros((S, 6))
        p0[C_STAR, :2] = rs.randn(2) / np.sqrt(imass[C_STAR, :2])
        q, _, _, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, 1000 + k, phi_max=PHI_MAX, chain_ids=ids)
        accepted += st["accepted"]
        xs[k] = q[C_STAR, :2]
    rate = accepted / N
    bm = xs.reshape(NB, N // NB, 2).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / math.sqrt(NB)
    z = (xs.mean(axis=0) - mean) / se
    print("LAW: acceptance %.3f at eps %g; posterior sd %s deg (%s px); chain mean - quadrature mean = %s se (se %s deg); "
          "chain sd / posterior sd %s" % (rate, eps, sd, sd / sc.pix_deg, z, se, xs.std(axis=0) / sd))
    assert rate > 0.5
    assert np.all(np.abs(z) <= 5.0), z
    sc.reset()
