"""HMC under the exact conditional: cel_slice_sample(param = 3) under CEL_OPT_GRAD_CONDITIONAL = 1, ImageSet.hmc_step(conditional=
"exact"), ModelGibbs(conditional="exact", hmc_conditional="exact").resample_hmc / sweep(hmc=True).

  1. every running chain's trajectory restated on Python floats from one-proposal patch_loglik_resident_grad(conditional="exact")
     calls: q, the returned momentum and the decision bit for bit, log alpha to tests/test_hmc.py's 8 ulp; L = 1 and 3, with and
     without the prior, under both gradient routes
  2. a trajectory pushed off its photon rectangle dies at that evaluation; a chain whose current row is uncovered is left alone
  3. host engine against device engine through ModelGibbs over three sweep(hmc=True), both grad_route settings
  4. reversibility on the device from (q1, -p1)
  5. law: 400 updates of the faint star against the fixed split, against quadrature of the exact target
  6. the reference conditional's step keeps its bits, and key 18 is not read under key 19 = 1

The scene is tests/test_hmc.py's: 2 bands on a 96 x 112 frame, seven chains (a faint star, a star cut by the frame's edge, a type-1
galaxy, a type-1 galaxy under the sigma floor, a type-2 source, a star whose chain id is negative, a star beside the frame without
a patch), the full-box resident split of seed 9.
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
        self.shape[C_FLOOR] = [0.4, 0.02, 40.0, 0.7]
        self.shape[C_T2] = [0.35, 1.2, 0.3, 0.9]
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
        assert np.all(self.sums[RUNNING].sum(axis=1) > 100) and self.sums[C_NOPATCH].sum() == 0
        self.ids = np.arange(S, dtype=np.int32)
        self.ids[C_OTHER] = -1
        ups = self.bands[0][28:32]
        self.pix_deg = math.sqrt(abs(ups[0] * ups[3] - ups[1] * ups[2]))
        self.one = cel.SourceSet(self.ctx, 1, B)

    def reset(self, radec=None, shape=None):
        self.cat.set(self.typ, self.radec if radec is None else radec, self.counts, self.shape if shape is None else shape)

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

    def route(self, photons):
        """CEL_OPT_PHOTON_LISTS + 4 around a block (the gradient at the photon lists), restored behind it"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            was = self.ctx.get_option(self.L.CEL_OPT_PHOTON_LISTS)
            try:
                if photons:
                    self.ctx.set_option(self.L.CEL_OPT_PHOTON_LISTS, was + 4)
                yield
            finally:
                self.ctx.set_option(self.L.CEL_OPT_PHOTON_LISTS, was)
        return cm()

    # -- the public call, one proposal at a time: the exact row
    def row(self, s, q, phi_max):
        """-> (v, g): slot 0 of the exact row + the prior, slots 1-6 + the prior's derivative"""
        self.one.set(self.typ[s:s + 1], np.array([q[:2]]), self.counts[s:s + 1], np.array([q[2:]]))
        ll, gr, _, gs = self.iset.patch_loglik_resident_grad(self.one, np.array([s], dtype=np.int32), conditional="exact")
        g = [float(gr[0, 0]), float(gr[0, 1])] + ([float(x) for x in gs[0]] if self.typ[s] == 1 else [0.0] * 4)
        pri = 0.0
        if self.typ[s] == 1 and phi_max > 0.0:
            sg = q[3]
            g[3] = g[3] + (2.0 / ((sg * sg) * sg) - 4.0 / sg)
            s2 = sg * sg
            pri = -2.0 * math.log(s2) - 1.0 / s2
        return float(ll[0]) + pri, g

    def inside(self, s, q, phi_max):
        if not all(math.isfinite(x) for x in (q if self.typ[s] == 1 else q[:2])):
            return False
        if self.typ[s] != 1:
            return True
        ok = 0.0 < q[2] < 1.0 and q[3] > 0.0 and 0.0 < q[5] < 1.0
        return ok and (not phi_max > 0.0 or 0.0 < q[4] < phi_max)

    def restated(self, s, q0, p0, im, eps, L, phi_max, log_u):
        """the header's param 3 under CEL_OPT_GRAD_CONDITIONAL = 1 on Python floats
        -> (q, p, log alpha, accepted, evaluations, v0, v1); evaluations = None: the chain is left alone (its row is uncovered)"""
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
            v, g = self.row(s, q, phi_max)
            if l == 0 and v == -math.inf:
                return [float(x) for x in q0], pstart, math.nan, False, None, None, None
            evals += 1
            if v == -math.inf or not all(math.isfinite(x) for x in g):
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
        v0, v1 = self.row(s, q0, phi_max)[0], self.row(s, q, phi_max)[0]
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
@pytest.mark.parametrize("photons", [False, True])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("phi_max", [PHI_MAX, 0.0])
def test_restated_from_public_calls(scene, L, phi_max, photons):
    sc = scene
    eps, seed = 0.4, 21 + L
    imass = sc.default_imass()
    imass[C_FLOOR, 3] *= 1e-4                 # (the prior's wall at sigma = 0.02 is steep: keep the trajectory inside the support)
    p0 = sc.momentum(imass, seed=3 + L)
    sc.reset()
    with sc.route(photons):
        q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, seed, phi_max=phi_max, chain_ids=sc.ids, conditional="exact")
        log_u = _log_u(seed, np.arange(S))
        evals = accepted = 0
        for s in RUNNING:
            qr, pr, lar, acc, ev, v0, v1 = sc.restated(s, sc.q0()[s], p0[s], imass[s], eps, L, phi_max, log_u[s])
            evals += ev
            accepted += int(acc)
            print("RESTATED exact L %d phi_max %g photons %s chain %d: log alpha %.17g (device %.17g), log u %.6f, accepted %s, v0 %r v1 %r"
                  % (L, phi_max, photons, s, lar, la[s], log_u[s], acc, v0, v1))
            assert v0 is not None, "the trajectory of chain %d died: choose other inputs" % s
            bar = 8 * np.spacing(max(abs(v0), abs(v1), 1.0))
            assert abs(la[s] - lar) <= bar, (s, la[s], lar, bar)
            assert abs(log_u[s] - lar) > 2 * bar, "the decision lies inside the band: change the seed"
            assert np.array_equal(q[s], np.array(qr)), (s, q[s], qr)
            assert np.array_equal(p[s], np.array(pr)), (s, p[s], pr)
            assert acc == bool(not np.array_equal(q[s], sc.q0()[s]))
    assert st["steps"] == L and st["evals"] == evals == len(RUNNING) * (L + 1) and st["accepted"] == accepted
    # the launch count the header states: 1 + J + 9 (L + 1) + L + 3 + V + 2 + 1 with J = 1 and V = 1 or 2
    assert st["launches"] - (1 + 1 + 9 * (L + 1) + L + 3 + 2 + 1) in (1, 2), st
    alone = [C_T2, C_OTHER, C_NOPATCH]
    assert np.array_equal(q[alone], sc.q0()[alone]) and np.all(np.isnan(la[alone]))
    sc.reset()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_trajectory_off_its_photon_rectangle_dies(scene):
    """the faint star thrown 30 px per leapfrog step: the first drift carries its box off its photons, the evaluation there is
    counted and is its last; the restated trajectory agrees.  Then the same chain started from an uncovered row: left alone."""
    sc = scene
    imass, p0 = np.zeros((S, 6)), np.zeros((S, 6))
    ids = np.full(S, -1, dtype=np.int32)
    ids[C_STAR] = C_STAR
    imass[C_STAR, :2] = 1.0
    eps, L = 1.0, 4
    p0[C_STAR, 0] = 30.0 * sc.pix_deg / math.cos(math.radians(sc.radec[C_STAR, 1]))
    sc.reset()
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, 5, phi_max=PHI_MAX, chain_ids=ids, conditional="exact")
    qr, pr, lar, acc, ev, _, _ = sc.restated(C_STAR, sc.q0()[C_STAR], p0[C_STAR], imass[C_STAR], eps, L, PHI_MAX, 0.0)
    assert lar == -math.inf and ev == 2 and not acc
    assert la[C_STAR] == -np.inf and st["evals"] == 2 and st["accepted"] == 0, (la, st)
    assert np.array_equal(q[C_STAR], sc.q0()[C_STAR]) and np.array_equal(p[C_STAR], -p0[C_STAR])
    assert np.all(np.isnan(np.delete(la, C_STAR)))
    # under the reference's conditional the same call runs to the end: there is no cover test there
    sc.reset()
    _, _, la_ref, st_ref = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, 5, phi_max=PHI_MAX, chain_ids=ids)
    assert st_ref["evals"] == L + 1 and not np.isnan(la_ref[C_STAR])
    # the catalogue's own row uncovered: the chain does not run
    moved = sc.radec.copy()
    moved[C_STAR, 0] += p0[C_STAR, 0]
    sc.reset(radec=moved)
    p0[C_STAR, 0] = 1e-3 * sc.pix_deg
    q, p, la, st = sc.iset.hmc_step(sc.cat, p0, imass, 1e-3, L, 5, phi_max=PHI_MAX, chain_ids=ids, conditional="exact")
    assert np.isnan(la[C_STAR]) and st["evals"] == 0 and st["accepted"] == 0
    assert np.array_equal(q[C_STAR, :2], moved[C_STAR]) and np.array_equal(p[C_STAR], p0[C_STAR])
    sc.reset()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("grad_route", ["dense", "photons"])
def test_host_engine_against_device_engine(cel, grad_route):
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
        g[e] = celeste_mcmc.ModelGibbs([gf], f0.src["type"], f0.src["radec"], flux5, f0.src["shape"], seed=5, engine=e,
                                       conditional="exact", hmc_conditional="exact", grad_route=grad_route)
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
    print("ENGINES exact (%s): hmc evals %d, accepted %d of %d updates" % (grad_route, t["hmc_evals"], t["hmc_accepted"], 3 * Sf))
    assert t["hmc_accepted"] > 0 and np.any(np.concatenate([g["auto"].u, g["auto"].shape], axis=1) != start)
    assert ctx.get_option(cel._lib.CEL_OPT_GRAD_CONDITIONAL) == 0 and ctx.get_option(cel._lib.CEL_OPT_PHOTON_LISTS) in (0, 1)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _star_scale(sc):
    """(inverse mass, widths) of the faint star's location from the curvature of its exact conditional: central differences
    of the analytic gradient half a pixel apart"""
    h = 0.5 * sc.pix_deg
    q = list(sc.q0()[C_STAR])
    w = []
    for i in range(2):
        a, b = list(q), list(q)
        a[i] += h
        b[i] -= h
        c = -(sc.row(C_STAR, a, 0.0)[1][i] - sc.row(C_STAR, b, 0.0)[1][i]) / (2 * h)
        assert c > 0
        w.append(1.0 / math.sqrt(c))
    return np.array(w) ** 2, np.array(w)


@gpu
def test_reversibility_on_the_device(scene):
    """tests/test_hmc.py's journey (twelve steps of 0.075 that carry the faint star about three pixels in ra and in dec, across
    several changes of its integer box) under the exact conditional, then the call from (q1, -p1): the force is a function of q
    alone, so the leapfrog retraces itself; the same bar, 1e-9 of the distance"""
    sc = scene
    var, width = _star_scale(sc)
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
        for seed in range(1, 65):
            q, pn, la, st = sc.iset.hmc_step(sc.cat, p, imass, eps, L, seed, phi_max=PHI_MAX, chain_ids=ids, conditional="exact")
            if st["accepted"] == 1:
                return q[C_STAR], pn[C_STAR], la[C_STAR], seed
        raise AssertionError("no seed in 1..64 accepts (log alpha %g)" % la[C_STAR])

    q1, p1, la1, seed1 = accepted_call(p0)
    boxes = [tuple(sc.iset.source_boxes(sc.one.set(sc.typ[:1], np.array([x[:2]]), sc.counts[:1], np.zeros((1, 4))))[0][0, 0]) for x in (q0, q1)]
    pb = np.zeros((S, 6))
    pb[C_STAR] = -p1
    q2, p2, la2, seed2 = accepted_call(pb)
    dist = np.abs(q1[:2] - q0[:2])
    miss = np.abs(q2[:2] - q0[:2])
    print("REVERSIBILITY exact: travelled %s px, boxes %s -> %s, log alpha %.4f there (seed %d) and %.4f back (seed %d); returned "
          "within %s of the distance (%s ulp)" % (dist / sc.pix_deg, boxes[0], boxes[1], la1, seed1, la2, seed2, miss / dist,
                                                  miss / np.spacing(np.abs(q0[:2]))))
    assert boxes[0] != boxes[1]                                  # the journey crossed a jump of the integer box
    assert np.all(dist > sc.pix_deg)
    assert np.all(miss <= 1e-9 * dist), (miss, dist)
    assert np.allclose(-p2[:2], p0[C_STAR, :2], rtol=1e-6)
    sc.reset()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_law_of_one_star(scene):
    """400 updates (L = 3, full refresh, the scale-free default's eps and inverse mass) of the faint star against the fixed split,
    under the exact conditional: the means and standard deviations of ra and dec against those of exp(v) by quadrature.
    The grid: 161 x 161 over +-6 posterior widths, 0.075 widths (about 0.007 px) apart, scored by slot 0 of the exact row, which
    carries the jumps of v where the integer box changes (and -inf where the box leaves a photon out): a jump is placed to within
    half a cell, so the quadrature's error is below 0.04 widths x the density at the jump x the jump's relative size.
    Bars: tests/test_hmc.py's 5 batch-means standard errors on the means; on chain sd / posterior sd the window [0.7, 1.4]: twenty
    batch means of twenty updates carry the sd to a relative standard error of about 1 / sqrt(2 ESS) <= 0.08 for an effective
    sample of 80 or more of the 400 updates (acceptance above one half, full momentum refresh), five of which are 0.4."""
    sc = scene
    _, width = _star_scale(sc)
    ng = 161
    ax = np.linspace(-6.0, 6.0, ng)
    R, Dc = np.meshgrid(sc.radec[C_STAR, 0] + ax * width[0], sc.radec[C_STAR, 1] + ax * width[1], indexing="ij")
    n = R.size
    grid = sc.cel.SourceSet(sc.ctx, n, B).set(np.zeros(n, dtype=np.int32), np.column_stack([R.ravel(), Dc.ravel()]),
                                             np.tile(sc.counts[C_STAR], (n, 1)), np.zeros((n, 4)))
    own = np.full(n, C_STAR, dtype=np.int32)
    v = sc.iset.patch_loglik_resident_grad(grid, own, conditional="exact")[0].reshape(ng, ng)
    vref = sc.iset.patch_loglik_resident(grid, own).reshape(ng, ng)
    wgt = np.exp(v - v.max())
    wgt /= wgt.sum()
    assert wgt[0].max() < 1e-6 and wgt[-1].max() < 1e-6 and wgt[:, 0].max() < 1e-6 and wgt[:, -1].max() < 1e-6
    mean = np.array([(wgt * R).sum(), (wgt * Dc).sum()])
    sd = np.sqrt(np.array([(wgt * (R - mean[0]) ** 2).sum(), (wgt * (Dc - mean[1]) ** 2).sum()]))
    print("LAW exact: the exact term over the grid: min %.4g max %.4g nats, -inf at %d of %d points"
          % (np.min((v - vref)[np.isfinite(v)]), np.max((v - vref)[np.isfinite(v)]), int(np.sum(~np.isfinite(v))), n))
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
        q, _, _, st = sc.iset.hmc_step(sc.cat, p0, imass, eps, L, 1000 + k, phi_max=PHI_MAX, chain_ids=ids, conditional="exact")
        accepted += st["accepted"]
        xs[k] = q[C_STAR, :2]
    rate = accepted / N
    bm = xs.reshape(NB, N // NB, 2).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / math.sqrt(NB)
    z = (xs.mean(axis=0) - mean) / se
    ratio = xs.std(axis=0) / sd
    print("LAW exact: acceptance %.3f at eps %g; posterior sd %s px; chain mean - quadrature mean = %s se; chain sd / posterior sd %s"
          % (rate, eps, sd / sc.pix_deg, z, ratio))
    assert rate > 0.5
    assert np.all(np.abs(z) <= 5.0), z
    assert np.all((ratio >= 0.7) & (ratio <= 1.4)), ratio
    sc.reset()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_reference_step_keeps_its_bits_and_key_18_is_not_read(cel, scene):
    sc, L = scene, scene.L
    imass = sc.default_imass()
    imass[C_FLOOR, 3] *= 1e-4
    p0 = sc.momentum(imass, seed=4)

    def step(iset, cat, **kw):
        cat.set(sc.typ, sc.radec, sc.counts, sc.shape)
        return iset.hmc_step(cat, p0, imass, 0.4, 3, 77, phi_max=PHI_MAX, chain_ids=sc.ids, **kw)

    ref = step(sc.iset, sc.cat)
    exact = step(sc.iset, sc.cat, conditional="exact")
    # a context that never heard of the key gives the reference step's bits
    ctx2 = cel.Context(0)
    iset2 = cel.ImageSet(ctx2, sc.bands, H, W)
    iset2.set_nelec(sc.nelec)
    cat2 = cel.SourceSet(ctx2, S, B).set(sc.typ, sc.radec, sc.counts, sc.shape)
    ctx2.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    iset2.photon_split_resident(cat2, seed=9)
    ctx2.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
    fresh = step(iset2, cat2)
    for a, b in zip(ref[:3], fresh[:3]):
        assert np.array_equal(a, b, equal_nan=True)
    assert ref[3] == fresh[3]
    assert not np.array_equal(ref[2][RUNNING], exact[2][RUNNING])            # the exact target is another target
    assert exact[3]["launches"] > ref[3]["launches"]
    # under key 19 = 1 key 18 is not read; the mirror restores both
    sc.ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 1)
    try:
        again = step(sc.iset, sc.cat, conditional="exact")
        for a, b in zip(exact[:3], again[:3]):
            assert np.array_equal(a, b, equal_nan=True)
        with pytest.raises(ValueError, match="no analytic derivative"):
            step(sc.iset, sc.cat)
        assert sc.ctx.get_option(L.CEL_OPT_SLICE_CONDITIONAL) == 1 and sc.ctx.get_option(L.CEL_OPT_GRAD_CONDITIONAL) == 0
    finally:
        sc.ctx.set_option(L.CEL_OPT_SLICE_CONDITIONAL, 0)
    with pytest.raises(ValueError):
        step(sc.iset, sc.cat, conditional="both")
    sc.reset()
