"""The photon split's draws against the exact multinomial law, draw by draw.

cel_photon_split splits each pixel's photons among the sources whose box strictly contains it and the sky,
z ~ Multinomial(trunc(nelec); F_1, ..., F_k, eps), as conditional binomials (k_split.h).  The reference's random stream cannot
be reproduced, so the contract is the law.  Here it is computed on the host, independently of the library: F_s = counts *
unit stamp from the oracle (first box row and column zeroed under the strict rule), and at every covered pixel, walking the
sources in ascending index with the kernel's own z,

    n_s = trunc(nelec) - sum_{j<s} z_j,        p_s = F_s / (eps + sum_{j>=s} F_j).

Under a correct kernel every draw is Binomial(n_s, p_s) given the ones before it: that is the multinomial, whatever order
the kernel draws in (its tile lists hold a tile's stars before its galaxies) and however it is built.  The draws are sorted
into classes by the regime the kernel takes (the first decision on a 16-bit word that eight rows of a column share,
inversion, flipped inversion, BTPE, more than 65 535 photons) and each class is held to three z-scores (the count of z > 0,
sum z, sum (z - n p)^2) and, where it has the mass, a randomized-PIT chi^2.  Pair statistics on the indicator residuals
e = 1{z > 0} - q catch draws that share randomness (rows of one Philox group, neighbouring columns, consecutive sources at one
pixel, consecutive seeds): every marginal can be exact while the draws are not independent.

Seeds are fixed, so the outcome is deterministic.  The statistics' own calibration (numpy's exact sampler passes, a sampler
that reuses its randomness fails) needs no GPU; every other test is marked gpu.
"""
import copy

import numpy as np
import pytest

H = W = 256
NB = 3
S = 60
SKY_BAND = 1                 # this band's sky is SKY_LOW: bright pixels reach p > 1/2 with a tiny 1 - p
SKY_LOW = 1e-3
FIELD_SEED = 11
BRIGHT_PEAK = 5e5            # the bright variant's largest rate: the 32-bit photons-left plane, n > 65 535, large-n BTPE
Z_MAX = 5.0
PIT_P_MIN = 1e-6
PIT_BINS = 20
MIN_VAR = 30.0               # a z-score is held to Z_MAX once its variance reaches this (below it a few events decide)

# "word": p <= 1/2 and n p < 1 -- the first test on the shared word decides, split by decade of n p; "inv": inversion,
# 1 <= n min(p, 1-p) <= 30; "btpe": above 30; "flip": p > 1/2 (the sampler draws n - Binomial(n, 1 - p))
CLASSES = (["word np<1e-6"] + ["word np 1e%d..1e%d" % (d, d + 1) for d in range(-6, 0)] +
           ["flip n(1-p)<1", "inv p<=.5", "inv flip", "btpe p<=.5", "btpe flip", "n>65535"])
C_WORD0, C_FLIP_TINY, C_INV, C_INV_FLIP, C_BTPE, C_BTPE_FLIP, C_BIG = 0, 7, 8, 9, 10, 11, 12
NCLASS = len(CLASSES)
PAIRS = ("rows y, y+2j of one group", "adjacent columns", "consecutive sources", "seeds k, k+1")

# (form, statistic) -> (value, held to the bound), printed at the end of the module (pytest -s)
REPORT = {}


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


# ---------------------------------------------------------------------------------------------------------------------
# the field and the exact law
class SplitField(object):
    """NB bands of H x W, S stars and galaxies from desi_mcmc_amd.synth, the oracle's unit stamps, nelec ~ Poisson(lambda)"""

    def __init__(self, orc, bright=False):
        from desi_mcmc_amd import synth
        bands = synth.make_bands(H, W, NB)
        bands[SKY_BAND, 0] = SKY_LOW
        self.lib_bands = bands.copy()                # radius 0: the library derives its own (checked against the oracle's)
        bands[:, 36] = [orc.band_radius(b) for b in bands]
        self.bands = bands
        src = synth.make_sources(S, H, W, bands, frac_gal=0.5, seed=FIELD_SEED)
        self.typ, self.radec, self.shape = src["type"], src["radec"], src["shape"]
        self.units = [[None] * S for _ in range(NB)]
        for b in range(NB):
            for s in range(S):
                p, (y0, y1), (x0, x1) = orc.source_patch(bands[b], H, W, self.typ[s], self.radec[s], self.shape[s])
                if p is not None:
                    self.units[b][s] = ((y0, y1, x0, x1), p)
        self.counts = src["counts"].copy()
        if bright:
            self.counts *= BRIGHT_PEAK / float((self.rate() - bands[:, 0, None, None]).max())
        self.lam = self.rate()
        self.nelec = np.random.RandomState(FIELD_SEED + 1).poisson(self.lam).astype(np.float64)

    def rate(self):
        lam = np.repeat(self.bands[:, 0], H * W).reshape(NB, H, W)
        for b in range(NB):
            for s in range(S):
                if self.units[b][s] is not None:
                    (y0, y1, x0, x1), u = self.units[b][s]
                    lam[b, y0:y1, x0:x1] += self.counts[s, b] * u
        return lam


class Chains(object):
    """Every draw of a split of `fld` as the law sees it, sorted by (pixel, source): the static part (p, 1 - p, the pixel's
    trunc(nelec), where the draw sits in the concatenated patches) and the static pairs.  strict: a source takes part only
    strictly inside its box on the low side (the reference's rule); False: on its whole box (CEL_OPT_SPLIT_FULL_BOX)."""

    def __init__(self, fld, strict=True):
        k = 1 if strict else 0
        pix, src, F, fpos, border = [], [], [], [], []
        self.patches, self.covered = [], np.zeros((NB, H, W), bool)
        pos = 0
        for b in range(NB):
            for s in range(S):
                if fld.units[b][s] is None:
                    continue
                (y0, y1, x0, x1), u = fld.units[b][s]
                ny, nx = u.shape
                self.patches.append((b, s, y0, x0, ny, nx, pos))
                self.covered[b, y0 + k:y1, x0 + k:x1] = True
                yy, xx = np.mgrid[k:ny, k:nx]
                pix.append(((b * H + y0 + yy) * W + x0 + xx).ravel())
                src.append(np.full(yy.size, s))
                F.append((fld.counts[s, b] * u[k:, k:]).ravel())
                fpos.append((pos + yy * nx + xx).ravel())
                if strict:
                    border.append(pos + np.r_[np.arange(nx), np.arange(1, ny) * nx])
                pos += ny * nx
        self.size = pos
        pix, src, F, fpos = (np.concatenate(a) for a in (pix, src, F, fpos))
        self.border = np.concatenate(border) if border else np.zeros(0, np.int64)
        o = np.lexsort((src, pix))
        self.pix, self.src, F, self.fpos = pix[o], src[o], F[o], fpos[o]
        N = self.pix.size
        first = np.r_[True, self.pix[1:] != self.pix[:-1]]
        self.gstart = np.maximum.accumulate(np.where(first, np.arange(N), 0))       # the pixel's first draw
        self.rank = np.arange(N) - self.gstart
        has_next = np.r_[self.pix[1:] == self.pix[:-1], False]
        after = np.zeros(N)                                                           # F summed over the later sources
        for r in range(int(self.rank.max()) - 1, -1, -1):
            i = np.nonzero((self.rank == r) & has_next)[0]
            after[i] = after[i + 1] + F[i + 1]
        eps = fld.bands[self.pix // (H * W), 0]
        self.p = F / (eps + F + after)
        self.r = (eps + after) / (eps + F + after)                                     # 1 - p without the cancellation
        self.set_nelec(fld.nelec)
        # static pairs, as indices into the sorted draws
        inv = np.full(pos, -1, np.int64)
        inv[self.fpos] = np.arange(N)
        rows, cols = [], []
        for (b, s, y0, x0, ny, nx, off) in self.patches:
            idx = inv[off:off + ny * nx].reshape(ny, nx)
            for j in range(1, 8):
                if ny <= 2 * j:
                    break
                y = y0 + np.arange(ny - 2 * j)
                same = (y & ~14) == ((y + 2 * j) & ~14)          # full-frame rows of one Philox group
                a, c = idx[:-2 * j][same], idx[2 * j:][same]
                ok = (a >= 0) & (c >= 0)
                rows.append(np.stack([a[ok], c[ok]]))
            a, c = idx[:, :-1], idx[:, 1:]
            ok = (a >= 0) & (c >= 0)
            cols.append(np.stack([a[ok], c[ok]]))
        nxt = np.nonzero(has_next)[0]
        self.pairs = [np.concatenate(rows, axis=1), np.concatenate(cols, axis=1), np.stack([nxt, nxt + 1])]

    def set_nelec(self, nelec):
        self.nelec = nelec
        self.nt = np.trunc(nelec.ravel()[self.pix]).astype(np.int64)

    def with_nelec(self, nelec):
        out = copy.copy(self)
        out.set_nelec(nelec)
        return out

    def gather(self, patches):
        """the split's patches -> one array in this object's concatenation order"""
        return np.concatenate([patches[b][s].ravel() for (b, s, _, _, _, _, _) in self.patches])

    def noise(self, z, rows=(0, H)):
        """each band's sky photons by the rule: nelec over the pixels nobody covers, trunc(nelec) - sum_s z_s over the rest"""
        taken = np.bincount(self.pix, weights=z, minlength=NB * H * W).reshape(NB, H, W)
        v = np.where(self.covered, np.trunc(self.nelec) - taken, self.nelec)
        return v[:, rows[0]:rows[1]].sum(axis=(1, 2))


class Law(object):
    """the statistics of the splits of one form, accumulated seed by seed"""

    def __init__(self, chains, name):
        self.c, self.name = chains, name
        self.acc = np.zeros((9, NCLASS))          # count obs / exp / var, sum obs / exp / var, square obs / exp / var
        self.npop = np.zeros(NCLASS, np.int64)
        self.pair = np.zeros((len(PAIRS), 2))     # sum e_i e_j, sum v_i v_j
        self.pit = {}                              # class -> PIT histogram
        self.prev = None
        self.u_rng = np.random.RandomState(2024)  # the randomized PIT's extra uniform
        self.seeds = 0

    def add(self, zflat):
        """one split (its patches concatenated in the chains' order) -> its draws in the chains' sorted order"""
        c = self.c
        # exact: non-negative integers, nothing on a box's first row or column (strict rule), nothing where the pixel has
        # no photon left, never more than it has left (so sum_s z_s <= trunc(nelec))
        assert np.all(zflat >= 0) and np.all(zflat == np.floor(zflat)), self.name
        assert np.all(zflat[c.border] == 0), "%s: a photon on the first row or column of a box" % self.name
        z = zflat[c.fpos].astype(np.int64)
        before = np.cumsum(z) - z
        n = c.nt - (before - before[c.gstart])
        act = (n > 0) & (c.p > 0)
        assert np.all(z[~act] == 0), "%s: a photon drawn at a pixel with none left" % self.name
        assert np.all(z <= np.maximum(n, 0)), "%s: more photons drawn than the pixel had left" % self.name
        nf, p, r = n.astype(np.float64), c.p, c.r
        flip = p > 0.5
        mu = np.where(act, nf * p, 1e-300)
        q = np.where(act, -np.expm1(nf * np.where(flip, np.log(r), np.log1p(-p))), 0.0)
        m = nf * np.minimum(p, r)
        dec = np.clip(np.floor(np.log10(mu)), -7, -1).astype(np.int64) + 7               # word decade: 0 (< 1e-6) .. 6
        cls = np.where(flip, np.where(m < 1, C_FLIP_TINY, np.where(m <= 30, C_INV_FLIP, C_BTPE_FLIP)),
                       np.where(mu < 1, C_WORD0 + dec, np.where(m <= 30, C_INV, C_BTPE)))
        cls = np.where(act, cls, NCLASS)
        big = act & (n > 65535)
        var = nf * p * r
        hit = (z > 0).astype(np.float64)
        for j, (o, e, v) in enumerate(((hit, q, q * (1 - q)), (z, mu, var),
                                       ((z - mu) ** 2, var, var * (1.0 + (2.0 * nf - 6.0) * p * r)))):
            for k, w in enumerate((o, e, v)):
                w = np.where(act, w, 0.0)
                self.acc[3 * j + k, :C_BIG] += np.bincount(cls, weights=w, minlength=NCLASS + 1)[:C_BIG]
                self.acc[3 * j + k, C_BIG] += np.sum(w[big])
        self.npop[:C_BIG] += np.bincount(cls, minlength=NCLASS + 1)[:C_BIG]
        self.npop[C_BIG] += int(big.sum())
        # randomized PIT (a flipped draw through n - z ~ Binomial(n, 1 - p): the same uniform law, 1 - p unrounded)
        if self.seeds == 0:
            for k in range(NCLASS):
                sel = big if k == C_BIG else (cls == k)
                if sel.sum() >= 100 and np.median(mu[sel]) >= 0.3:
                    self.pit[k] = np.zeros(PIT_BINS)
        if self.pit:
            from scipy import stats
            for k in sorted(self.pit):
                sel = big if k == C_BIG else (cls == k)
                zz, nn, fl = z[sel], n[sel], flip[sel]
                y = np.where(fl, nn - zz, zz)
                pp = np.where(fl, r[sel], p[sel])
                u = stats.binom.cdf(y - 1, nn, pp) + self.u_rng.uniform(size=y.size) * stats.binom.pmf(y, nn, pp)
                self.pit[k] += np.bincount(np.clip((u * PIT_BINS).astype(np.int64), 0, PIT_BINS - 1), minlength=PIT_BINS)
        # pairs on the indicator residuals (an inactive draw: q = 0, e = 0)
        e, v = hit - q, q * (1 - q)
        for j, (a, b) in enumerate(c.pairs):
            self.pair[j] += (np.sum(e[a] * e[b]), np.sum(v[a] * v[b]))
        if self.prev is not None:
            self.pair[3] += (np.sum(e * self.prev[0]), np.sum(v * self.prev[1]))
        self.prev = (e, v)
        self.seeds += 1
        return z

    def results(self):
        """-> [(statistic, value, held to the bound)]: z-scores, and the PIT chi^2's p-values"""
        from scipy import stats
        out = []
        for k in range(NCLASS):
            for j, what in enumerate(("count z>0", "sum z", "sum (z-np)^2")):
                o, e, v = self.acc[3 * j:3 * j + 3, k]
                out.append(("%s: %s" % (CLASSES[k], what), (o - e) / np.sqrt(v) if v > 0 else 0.0, bool(v >= MIN_VAR)))
        for k in sorted(self.pit):
            h = self.pit[k]
            E = h.sum() / PIT_BINS
            out.append(("%s: PIT p" % CLASSES[k], float(stats.chi2.sf(((h - E) ** 2 / E).sum(), PIT_BINS - 1)),
                        bool(E >= 50)))
        for j, what in enumerate(PAIRS):
            num, den = self.pair[j]
            out.append(("pairs: %s" % what, num / np.sqrt(den) if den > 0 else 0.0, bool(den >= MIN_VAR)))
        return out

    def check(self):
        res = self.results()
        for name, val, held in res:
            REPORT[(self.name, name)] = (val, held)
        bad = [(n_, v) for n_, v, held in res if held and (v < PIT_P_MIN if n_.endswith("PIT p") else abs(v) > Z_MAX)]
        assert not bad, "%s: %s" % (self.name, bad)
        return dict((n_, (v, held)) for n_, v, held in res)


def exact_draws(chains, rng):
    """a split drawn by numpy's exact conditional-binomial chain, concatenated like the library's patches"""
    c = chains
    N = c.pix.size
    z = np.zeros(N, np.int64)
    left = c.nt.copy()
    for k in range(int(c.rank.max()) + 1):
        i = np.nonzero(c.rank == k)[0]
        n = np.maximum(left[i], 0)
        z[i] = rng.binomial(n, c.p[i])
        j = i + 1
        ok = j < N
        ok[ok] = c.rank[j[ok]] == k + 1
        left[j[ok]] = n[ok] - z[i[ok]]
    zflat = np.zeros(c.size)
    zflat[c.fpos] = z
    return zflat


@pytest.fixture(scope="module")
def field(orc):
    return SplitField(orc)


@pytest.fixture(scope="module")
def chains(field):
    return {True: Chains(field), False: Chains(field, strict=False)}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\nsplit law statistics (z-score, or the PIT chi^2's p-value; * = held to the bound):")
        for (form, name) in sorted(REPORT):
            v, held = REPORT[(form, name)]
            print("  %-14s %-44s %11.4g %s" % (form, name, v, "*" if held else ""))


def test_statistics_calibrated_on_an_exact_sampler(field, chains):
    """(no GPU) numpy's exact conditional-binomial sampler meets every bound on the field's chains, and a sampler that hands
    seed k + 1 the draws of seed k fails the seeds pair statistic: the bounds are neither too tight nor blind"""
    law = Law(chains[True], "numpy")
    for k in range(20):
        law.add(exact_draws(chains[True], np.random.RandomState(500 + k)))
    res = law.check()
    assert sum(held for _, held in res.values()) >= 30, res
    stale = Law(chains[True], "stale")
    zf = exact_draws(chains[True], np.random.RandomState(77))
    for k in range(3):
        stale.add(zf)
    zs = stale.results()[-1]
    assert zs[0] == "pairs: seeds k, k+1" and zs[1] > 50, zs


# ---------------------------------------------------------------------------------------------------------------------
# the library's split, in each of its forms
SEED0 = 7000
# The default form takes 400 seeds: the tail classes (n p < 1e-4) gather a few hundred expected photons per 100 seeds, and
# the first uniform of a queued draw started one 2^-16 step low (q too small by 2^-16 / (n p) there) moves them by 3.7 sigma
# per 100 seeds -- by more than Z_MAX only from ~200 seeds on.
FORMS = (("default", 400),       # a render, then the split on the totals k_strict_totals forms from its model image
         ("reuse0", 30),         # CEL_OPT_SPLIT_REUSE = 0: the totals from a strict render of their own
         ("direct", 30),         # set_kernel("direct"): k_photon_split
         ("plane32", 30),        # the 32-bit photons-left plane (the caller holds the image's address)
         ("full_box", 30))       # CEL_OPT_SPLIT_FULL_BOX = 1: whole boxes, the totals are the model image itself
# the classes every form of the field must bring to the bound: the statistic whose variance must reach MIN_VAR
FIELD_HOLDS = ([("count z>0", C_WORD0 + d) for d in range(3, 7)] +
               [("sum z", k) for k in (C_FLIP_TINY, C_INV, C_INV_FLIP, C_BTPE, C_BTPE_FLIP)])
BRIGHT_HOLDS = [("sum z", k) for k in (C_BTPE, C_BTPE_FLIP, C_BIG)]


def open_form(cel, orc, fld, form, nelec=None):
    """-> (ctx, images, sources) of a fresh context set up for `form`"""
    L = cel._lib
    ctx = cel.Context(0)
    if form == "direct":
        ctx.set_kernel("direct")
    if form == "reuse0":
        ctx.set_option(L.CEL_OPT_SPLIT_REUSE, 0)
    if form == "full_box":
        ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    images = cel.ImageSet(ctx, fld.lib_bands, H, W, nelec=fld.nelec if nelec is None else nelec)
    for b in range(NB):
        assert orc.checked_radius(fld.lib_bands[b], images.band(b)[36]) == fld.bands[b, 36]
    sources = cel.SourceSet(ctx, S, NB).set(fld.typ, fld.radec, fld.counts, fld.shape)
    if form == "plane32":
        images.device_ptrs()
    if form in ("default", "plane32", "full_box"):
        images.render(sources)
    return ctx, images, sources


def run_splits(fld, chains, images, sources, law, seeds, rows=(0, H)):
    """split once per seed; the boxes are the oracle's, the draws go to `law`, the noise sums are the rule's"""
    tol = 1e-12 * np.abs(chains.nelec).sum(axis=(1, 2))
    for seed in seeds:
        patches, boxes, noise = images.photon_split(sources, seed)
        if law.seeds == 0:
            for b in range(NB):
                for s in range(S):
                    u = fld.units[b][s]
                    assert (patches[b][s] is None) == (u is None), (b, s)
                    assert u is None or tuple(boxes[b, s]) == u[0], (b, s, boxes[b, s], u[0])
        z = law.add(chains.gather(patches))
        ref = chains.noise(z, rows)
        assert np.all(np.abs(noise - ref) <= tol), (law.name, seed, noise, ref)


def assert_holds(law, holds):
    """the field reaches every regime it is meant to: each listed statistic has the variance to be held to the bound"""
    res = dict((n_, held) for n_, _, held in law.results())
    missing = [(CLASSES[k], what, int(law.npop[k])) for what, k in holds if not res["%s: %s" % (CLASSES[k], what)]]
    assert not missing, "%s: classes below the population the bound needs: %s" % (law.name, missing)


@pytest.mark.gpu
@pytest.mark.parametrize("form,nseeds", FORMS, ids=[f for f, _ in FORMS])
def test_split_draws_follow_the_law(cel, orc, field, chains, form, nseeds):
    ch = chains[form != "full_box"]
    ctx, images, sources = open_form(cel, orc, field, form)
    law = Law(ch, form)
    ctx.profile(True)
    try:
        run_splits(field, ch, images, sources, law, range(SEED0, SEED0 + nseeds))
        n_totals = ctx.profile_get("totals")[1]
    finally:
        ctx.profile(False)
    # the default and the 32-bit forms take their totals from the render's image; the others never
    assert n_totals == (nseeds if form in ("default", "plane32") else 0), (form, n_totals)
    assert_holds(law, FIELD_HOLDS)
    law.check()


@pytest.fixture(scope="module")
def bright(orc):
    return SplitField(orc, bright=True)


@pytest.mark.gpu
def test_bright_split_follows_the_law(cel, orc, bright):
    """peaks of 1e5 .. 1e6 photons: the 32-bit photons-left plane, n > 65 535, BTPE at large n"""
    assert 65535 < bright.nelec.max() < 2e6
    ch = Chains(bright)
    ctx, images, sources = open_form(cel, orc, bright, "default")
    law = Law(ch, "bright")
    run_splits(bright, ch, images, sources, law, range(SEED0, SEED0 + 30))
    assert_holds(law, BRIGHT_HOLDS)
    law.check()


def edge_nelec(fld, chains):
    """fractional, negative and zero pixels: scattered over the frame, on boxes' first rows and columns, outside every box"""
    rs = np.random.RandomState(5)
    ne = fld.nelec.copy()
    u = rs.rand(NB, H, W)
    ne[u < 0.1] += 0.625
    neg = (u >= 0.1) & (u < 0.12)
    ne[neg] = -rs.uniform(0.1, 6.0, int(neg.sum()))
    ne[(u >= 0.12) & (u < 0.14)] = 0.0
    vals = np.array([-3.5, -0.75, 0.0, 0.5, 2.25, 17.875])
    for (b, s, y0, x0, ny, nx, _) in chains.patches[::3]:
        ne[b, y0, x0:x0 + nx] = rs.choice(vals, nx)
        ne[b, y0:y0 + ny, x0] = rs.choice(vals, ny)
    return ne


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f for f, _ in FORMS])
def test_split_edges_are_exact(cel, orc, field, chains, form):
    """every z a non-negative integer, sum_s z_s <= trunc(nelec), z = 0 where trunc(nelec) <= 0 and on a box's first row and
    column (strict rule); each band's noise sum is nelec over the uncovered pixels plus what the sources left of trunc(nelec)
    over the covered ones -- over the whole set, and over the rows an image set owns (set_noise_rows)"""
    ch = chains[form != "full_box"]
    ne = edge_nelec(field, ch)
    out = ~ch.covered
    assert np.any(out & (ne < 0)) and np.any(out & (ne != np.trunc(ne))) and np.any(out & (ne == 0))
    assert np.any(ch.covered & (ne < 0) & (ne > -1)) and np.any(ch.covered & (ne != np.trunc(ne)) & (ne > 0))
    che = ch.with_nelec(ne)
    ctx, images, sources = open_form(cel, orc, field, form, nelec=ne)
    law = Law(che, form + "/edges")
    run_splits(field, che, images, sources, law, (11, 12))
    images.set_noise_rows(64, 192)
    run_splits(field, che, images, sources, law, (13,), rows=(64, 192))
