"""The HMC step with its gradients at the photon lists: CEL_OPT_PHOTON_LISTS = 5 under cel_slice_sample(param = 3),
ModelGibbs(grad_route="photons").

  1. every trajectory restated from public calls made under the same option value -- q, the returned momentum and the decision bit
     for bit, log alpha to 8 ulp, the launch count that of the dense route
  2. host engine against device engine through ModelGibbs(grad_route="photons"), three sweep(hmc=True) on 12 sources
  3. reversibility on the device
  4. grad_route validation; conditional="exact" still raises

The law is not tested again: the route changes rounding, not the target, and 1 and 2 tie it to the host engine that
tests/test_hmc_host.py holds to its law.

The scene and the helpers are those of tests/test_hmc.py, restated: 2 bands on a 96 x 112 frame, seven chains -- a faint star, a
star cut by the frame's edge, a type-1 galaxy, a type-1 galaxy under the sigma floor, a type-2 source, a star whose chain id is
negative (its gradient jobs have an owner of -1), a star beside the frame that has no patch.  The data is a Poisson draw from the
scene's model image; the split is the full-box resident split of seed 9, made under CEL_OPT_PHOTON_LISTS = 5.
"""
import math

import numpy as np
import pytest

H, W, B = 96, 112, 2
gpu = pytest.mark.gpu
C_STAR, C_EDGE, C_GAL, C_FLOOR, C_T2, C_OTHER, C_NOPATCH = range(7)
S = 7
RUNNING = [C_STAR, C_EDGE, C_GAL, C_FLOOR]
PHI_MAX = 180.0
ROUTE = 5                       # every patch's value at its photons, and the resident gradient too


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
        self.ctx.set_option(L.CEL_OPT_PHOTON_LISTS, ROUTE)
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
        was = self.ctx.get_option(L.CEL_OPT_SPLIT_FULL_BOX)
        self.ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
        try:
            self.iset.photon_split_resident(self.cat, seed=9)
        finally:
            self.ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, was)
        self.sums = self.iset.sample_sums()
        # every running chain has photons, in every band
        assert np.all(self.sums[RUNNING] > 20) and self.sums[C_NOPATCH].sum() == 0
        self.ids = np.arange(S, dtype=np.int32)
        self.ids[C_OTHER] = -1
        ups = self.bands[0][28:32]
        self.pix_deg = math.sqrt(abs(ups[0] * ups[3] - ups[1] * ups[2]))
        self.one = cel.SourceSet(self.ctx, 1, B)

    def option(self, v):
        self.ctx.set_option(self.L.CEL_OPT_PHOTON_LISTS, v)

    def reset(self):
        """the catalogue back at the scene's rows (the split stays: it is of these S sources)"""
        self.cat.set(self.typ, self.radec, self.counts, self.shape)

    def q0(self):
        return np.concatenate([self.radec, self.shape], axis=1)

    def default_imass(self):
        N = np.maximum(self.sums.sum(axis=1), 1.0)
        im = np.empty((S, 6))
        im[:, :2] = (self.pix_deg ** 2 / N)[:, None]
        im[:, 2:] = (1.0 / N)[:, None]
        return im

    def momentum(self, imass, seed):
        z = np.random.RandomState(seed).randn(S, 6)
        return np.where(imass > 0, z / np.sqrt(np.where(imass > 0, imass, 1.0)), 0.0)

    # -- the public calls, one proposal at a time, under whatever option value stands
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
        """the header's comment of param 3 on Python floats -> (q, p, log alpha, accepted, evaluations, v0, v1)"""
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
def test_restated_from_public_calls_at_the_photons(scene, L, phi_max):
    sc = scene
    eps, seed = 0.4, 21 + L
    imass = sc.default_imass()
    imass[C_FLOOR, 3] *= 1e-4                 # (the prior's wall at sigma = 0.02 is steep: keep the trajectory inside the support)
    p0 = sc.momentum(imass, seed=3 + L)
    # the dense route's call first: its launch count, and rows that are not this route's bits
    sc.option(1)
    sc.reset()
    qd, pd, lad, std = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=phi_max, chain_ids=sc.ids)
    sc.option(ROUTE)
    sc.reset()
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=phi_max, chain_ids=sc.ids)
    assert st["launches"] == std["launches"] and 4 * L + 9 <= st["launches"] <= 4 * L + 10, (st, std)
    assert not np.array_equal(p[RUNNING], pd[RUNNING]), "the two routes returned the same bits: the list kernel did not run"
    log_u = _log_u(seed, np.arange(S))
    evals = accepted = 0
    for s in RUNNING:
        qr, pr, lar, acc, ev, v0, v1 = sc.restated(s, sc.q0()[s], p0[s], imass[s], eps, L, phi_max, log_u[s])
        evals += ev
        accepted += int(acc)
        print("RESTATED at the photons L %d phi_max %g chain %d: log alpha %.17g (device %.17g), log u %.6f, accepted %s"
              % (L, phi_max, s, lar, la[s], log_u[s], acc))
        assert v0 is not None, "the trajectory of chain %d died: choose other inputs" % s
        bar = 8 * np.spacing(max(abs(v0), abs(v1), 1.0))
        assert abs(la[s] - lar) <= bar, (s, la[s], lar, bar)
        assert abs(log_u[s] - lar) > 2 * bar, "the decision lies inside the band: change the seed"
        assert np.array_equal(q[s], np.array(qr)), (s, q[s], qr)
        assert np.array_equal(p[s], np.array(pr)), (s, p[s], pr)
        assert acc == bool(not np.array_equal(q[s], sc.q0()[s]))
    assert st["steps"] == L and st["evals"] == evals == len(RUNNING) * (L + 1) and st["accepted"] == accepted
    # the chains left alone (one of them with an owner of -1 in every gradient launch) left nothing non-finite behind
    alone = [C_T2, C_OTHER, C_NOPATCH]
    assert np.all(np.isfinite(q[RUNNING])) and np.all(np.isfinite(p[RUNNING])) and np.all(np.isfinite(la[RUNNING]))
    assert np.array_equal(q[alone], sc.q0()[alone]) and np.array_equal(p[alone], p0[alone]) and np.all(np.isnan(la[alone]))
    sc.reset()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_host_engine_against_device_engine_at_the_photons(cel):
    from desi_mcmc_amd import _lib as L, celeste_mcmc, synth
    Sf = 12
    ctx = cel.Context(0)
    f0 = synth.SyntheticField(ctx, Sf, B, H, W, frac_gal=0.5, seed=23)
    flux5 = np.full((Sf, 5), 3.0)
    flux5[:, :B] = f0.src["flux"]
    g = {}
    for e, route in (("host", "photons"), ("auto", "photons"), ("dense", "dense")):
        imgs = cel.ImageSet(ctx, f0.bands, H, W)
        imgs.set_nelec(f0.nelec)
        gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W)
        g[e] = celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5,
                                       engine="auto" if e == "dense" else e, grad_route=route)
    assert g["auto"]._hmc_engine_on_device() and not g["host"]._hmc_engine_on_device()
    for sweep in range(3):
        for e in g:
            g[e].sweep(hmc=True)
            assert ctx.get_option(L.CEL_OPT_PHOTON_LISTS) == 0        # what the caller had is restored
        for name in ("typ", "u", "fluxes", "shape", "_hmc_p"):
            assert np.array_equal(getattr(g["host"], name), getattr(g["auto"], name)), (sweep, name)
        assert g["host"].timing["hmc_evals"] == g["auto"].timing["hmc_evals"] > 0
        assert g["host"].timing["hmc_accepted"] == g["auto"].timing["hmc_accepted"]
    t = g["auto"].timing
    print("ENGINES at the photons: hmc evals %d, accepted %d of %d updates" % (t["hmc_evals"], t["hmc_accepted"], 3 * Sf))
    assert t["hmc_accepted"] > 0
    # the route was taken: the dense run's momenta are not these bits
    assert not np.array_equal(g["dense"]._hmc_p, g["auto"]._hmc_p)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_reversibility_on_the_device_at_the_photons(scene):
    """tests/test_hmc.py's journey: an accepted update that carries the faint star about three pixels in ra and in dec (twelve
    steps of 0.075 in units of its oscillation), then the call from (q1, -p1): back at q0 within 1e-9 of the distance"""
    sc = scene
    sc.option(ROUTE)
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
    var = np.array(w) ** 2
    eps, L = 0.075, 12
    ids = np.full(S, -1, dtype=np.int32)
    ids[C_STAR] = C_STAR
    imass, p0 = np.zeros((S, 6)), np.zeros((S, 6))
    imass[C_STAR, :2] = var
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
    print("REVERSIBILITY at the photons: travelled %s px, log alpha %.4f there (seed %d) and %.4f back (seed %d); returned within "
          "%s of the distance" % (dist / sc.pix_deg, la1, seed1, la2, seed2, miss / dist))
    assert np.all(dist > sc.pix_deg)
    assert np.all(miss <= 1e-9 * dist), (miss, dist)
    assert np.allclose(-p2[:2], p0[C_STAR, :2], rtol=1e-6)
    sc.reset()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_grad_route_is_validated(cel):
    from desi_mcmc_amd import celeste_mcmc, synth
    ctx = cel.Context(0)
    f0 = synth.SyntheticField(ctx, 4, B, H, W, frac_gal=0.5, seed=3)
    flux5 = np.full((4, 5), 3.0)
    flux5[:, :B] = f0.src["flux"]
    imgs = cel.ImageSet(ctx, f0.bands, H, W)
    imgs.set_nelec(f0.nelec)
    gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W)
    args = ([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"])
    assert celeste_mcmc.ModelGibbs(*args).grad_route == "dense"
    assert celeste_mcmc.ModelGibbs(*args, grad_route="photons").grad_route == "photons"
    for bad in ("lists", "Photons", "", None, 5):
        with pytest.raises(ValueError, match="grad_route"):
            celeste_mcmc.ModelGibbs(*args, grad_route=bad)
    exact = celeste_mcmc.ModelGibbs(*args, conditional="exact", grad_route="photons")
    with pytest.raises(ValueError, match="exact"):
        exact.resample_hmc()
    with pytest.raises(ValueError, match="exact"):
        exact.location_loglik_grad(np.arange(2), f0.src["radec"][:2])
