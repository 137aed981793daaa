"""celeste_mcmc.MomentProposal: the star <-> galaxy move's proposal from the second moments of a source's photons.

CPU
  round trip     the exact central second moment of galaxy_mixture's 42 components, for a dozen shapes under the rotated, per-band
                 WCS of tests/_general_wcs.py, goes through moment_centre with the true theta and must return sigma, rho and phi
                 (modulo 180) to 1e-9 relative: 2 x 2 algebra, rounding is the only error.  A shape with sigma < 1/30 returns the
                 floor, 1/30.
  density        exp(logq) integrates to 1 to 1e-6, for a usable and an unusable chain and for periods 180 and 360, by a tensor
                 Gauss-Legendre rule per coordinate (theta; log sigma; logit rho; phi piecewise between the windows' edges); logq
                 equals a restatement written here from the issue's formulas; 20 000 draws of one chain from consecutive seeds
                 pass a chi^2 test per coordinate (20 equiprobable bins of logq's marginals, 19 degrees of freedom, bound
                 19 + 4.5 sqrt(38) = 46.7).  The streams are fixed, so the statistics are numbers:
                     theta 20.6, sigma 14.7, phi 32.7, rho 25.0                     (chain 7, period 180, seeds 0 .. 19 999)
  antisymmetry   h(star -> galaxy(shape)) == -h(galaxy(shape) -> star), exactly.
  w = 1          h = +-type_log_odds and the drawn shapes are sample_shape_prior's bits.

GPU
  detailed balance through the kernel, the count of accepted star -> galaxy moves against the prior proposal's, and the two
  engines (and the device's catalogue) chain for chain; see the tests' docstrings for the measured figures.
"""
import os
import sys
from math import erf, lgamma, log, pi, sqrt

import numpy as np
import pytest

import desi_mcmc_amd  # noqa: F401
from desi_mcmc_amd import celeste_mcmc
from desi_mcmc_amd.celeste_mcmc import MomentProposal, band_cd_at, moment_centre, psf_covariance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _general_wcs as gw  # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


# ---- CPU: the centre map ---------------------------------------------------------------------------------------------------------
SHAPES = [(0.5, 1.0, 30.0, 0.5), (0.1, 0.5, 5.0, 0.9), (0.9, 4.0, 175.0, 0.2), (0.3, 2.2, 89.0, 0.7), (0.7, 0.8, 91.0, 0.35),
          (0.05, 3.0, 135.0, 0.6), (0.95, 0.3, 45.0, 0.8), (0.5, 0.02, 60.0, 0.5), (0.6, 1.7, 0.5, 0.93), (0.2, 6.0, 179.5, 0.1),
          (0.45, 0.1, 120.0, 0.06), (0.8, 1.3, 150.0, 0.55)]


class _Img(object):
    """what galaxy_mixture asks of an image, on a band record under the general WCS"""

    def __init__(self, bands, b):
        self.bands, self.b = bands, b
        r = bands[b]
        self.weights, self.means, self.covars = r[3:6], r[6:12].reshape(3, 2), r[12:24].reshape(3, 2, 2)

    def equa2pixel(self, u):
        return gw.equa2pixel(self.bands, self.b, u)

    def cd_at_pixel(self, x, y):
        return gw.cd_at_pixel(self.bands, self.b, x, y)


def test_the_centre_map_returns_the_shape_of_an_exact_second_moment():
    from desi_mcmc_amd.celeste_galaxy_conditionals import galaxy_mixture
    H, W, B = 96, 112, 3
    bands = gw.general_bands(H, W, B)
    u = gw.pixel2equa(bands, 0, [47.3, 52.8])
    S = len(SHAPES)
    N, C, cd = np.zeros((S, B)), np.zeros((S, B, 2, 2)), np.zeros((S, B, 2, 2))
    for b in range(B):
        img = _Img(bands, b)
        mine = band_cd_at(bands[b], u[None, :])[0]
        theirs = gw.cd_at_pixel(bands, b, *gw.equa2pixel(bands, b, u))
        assert np.allclose(mine, theirs, rtol=1e-12, atol=0)
        for s, th in enumerate(SHAPES):
            pis, means, covs, _ = galaxy_mixture(np.array(th), u, img)
            m = (pis[:, None] * means).sum(axis=0) / pis.sum()
            d = means - m
            C[s, b] = (pis[:, None, None] * (covs + d[:, :, None] * d[:, None, :])).sum(axis=0) / pis.sum()
            N[s, b] = 1000.0 * (b + 1)
            cd[s, b] = mine
    usable, lam, rho, phi = moment_centre(N, C, np.stack([psf_covariance(bands[b]) for b in range(B)]), cd)
    assert usable.all()
    mp = MomentProposal().set_centre(usable, lam, rho, phi, 180.0)
    th = np.array(SHAPES)
    sig = mp.sigma_hat(th[:, 0])
    want_sig = np.maximum(th[:, 1], 1.0 / 30)
    assert np.any(th[:, 1] < 1.0 / 30)
    err = dict(sigma=np.abs(sig / want_sig - 1).max(), rho=np.abs(rho / th[:, 3] - 1).max(),
               phi=(np.abs((phi - th[:, 2] + 90.0) % 180.0 - 90.0) / th[:, 2]).max())
    print("centre map, worst relative errors:", err)
    assert err["sigma"] < 1e-9 and err["rho"] < 1e-9 and err["phi"] < 1e-9
    # fewer than n_min photons, or a moment no wider than the PSF: not usable
    few = moment_centre(N * 0 + 10.0, C, np.stack([psf_covariance(bands[b]) for b in range(B)]), cd)[0]
    thin = moment_centre(N, C * 0 + 0.5 * psf_covariance(bands[0]), np.stack([psf_covariance(bands[b]) for b in range(B)]), cd)[0]
    assert not few.any() and not thin.any()


# ---- CPU: the density ------------------------------------------------------------------------------------------------------------
def _chain(period, usable=True, n=1, **kw):
    """n copies of one chain: sigma_hat(theta = V-weighted) about 1.5 arc seconds, rho_hat 0.6, phi_hat 40 degrees"""
    mp = MomentProposal(**kw)
    lam = (1.5 / 3600.0) ** 2 * 0.5 * (mp.V_exp + mp.V_dev)
    return mp.set_centre(np.full(n, usable), np.full(n, lam), np.full(n, 0.6), np.full(n, 40.0), period)


def _Phi(x):
    return 0.5 * (1.0 + np.vectorize(erf)(np.asarray(x, dtype=np.float64) / sqrt(2.0)))


def _restated_logq(mp, sh, usable):
    """the issue's density, written out again"""
    th, sg, ph, rh = sh.T
    lp = log(2.0) - lgamma(1.5) - 4 * np.log(sg) - 1 / sg ** 2 - log(mp.period)
    if not usable:
        return lp
    sh_ = 3600.0 * np.sqrt(mp.lam_max[0] / (th * mp.V_exp + (1 - th) * mp.V_dev))
    q_s = np.exp(-0.5 * ((np.log(sg) - np.log(sh_)) / mp.s_sigma) ** 2) / (mp.s_sigma * sqrt(2 * pi) * sg)
    lg = np.log(rh / (1 - rh)) - log(0.6 / 0.4)
    q_r = np.exp(-0.5 * (lg / mp.s_rho) ** 2) / (mp.s_rho * sqrt(2 * pi) * rh * (1 - rh))
    a = min(mp.a_phi, mp.period / 2)
    images = [40.0 + 180.0 * k for k in range(4) if 40.0 + 180.0 * k < mp.period]
    q_p = np.zeros_like(ph)
    for c in images:
        d = np.abs(ph - c)
        q_p += (np.minimum(d, mp.period - d) < a) / (2 * a * len(images))
    return np.log(mp.w * np.exp(lp) + (1 - mp.w) * q_s * q_r * q_p)


@pytest.mark.parametrize("period", [180.0, 360.0])
@pytest.mark.parametrize("usable", [True, False])
def test_the_density_integrates_to_one(period, usable):
    def rule(lo, hi, panels, order):
        gl_x, gl_w = np.polynomial.legendre.leggauss(order)
        e = np.linspace(lo, hi, panels + 1)
        x = (0.5 * (e[1:] + e[:-1])[:, None] + 0.5 * (e[1:] - e[:-1])[:, None] * gl_x[None, :]).ravel()
        w = (0.5 * (e[1:] - e[:-1])[:, None] * gl_w[None, :]).ravel()
        return x, w
    tx, tw = rule(0.0, 1.0, 1, 12)                                 # theta: smooth
    lx, lw = rule(-3.0, 9.0, 24, 8)                               # log sigma: the prior's tail is sigma^-3 d log sigma, e^-27 at 9
    sx, sw = np.exp(lx), lw * np.exp(lx)
    gx, gw_ = rule(-21.0, 21.0, 14, 8)                           # logit rho: the uniform's tails are e^-21
    rx = 1 / (1 + np.exp(-gx))
    rw = gw_ * rx * (1 - rx)
    edges = sorted({0.0, period} | {(c + s * 30.0) % period for c in (40.0, 220.0) for s in (-1, 1)})
    px, pw = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):                    # phi: constant between the windows' edges
        x, w = rule(lo, hi, 1, 2)
        px.append(x), pw.append(w)
    px, pw = np.concatenate(px), np.concatenate(pw)
    # theta x sigma on a tensor grid; q is a two-term mixture of products, so the rho and phi integrals factor per term
    T, Sg = np.meshgrid(tx, sx, indexing="ij")
    mp = _chain(period, usable, n=T.size)
    base = np.stack([T.ravel(), Sg.ravel(), np.full(T.size, 41.0), np.full(T.size, 0.6)], axis=1)
    w2 = (tw[:, None] * sw[None, :]).ravel()
    I_prior = (np.exp(mp.log_prior(base)) * w2).sum() * period      # (uniform in rho and phi: 1 x period at density 1 / period)
    assert abs(I_prior - 1) < 1e-6
    total = 0.0
    # the whole of logq, coordinate by coordinate: sum over (theta, sigma) of the integral over rho and phi at that point
    for chunk in range(0, T.size, 64):
        sel = slice(chunk, min(chunk + 64, T.size))
        k = base[sel].shape[0]
        R, P = np.meshgrid(rx, px, indexing="ij")
        pts = np.empty((k, R.size, 4))
        pts[:, :, 0], pts[:, :, 1] = base[sel, 0][:, None], base[sel, 1][:, None]
        pts[:, :, 2], pts[:, :, 3] = P.ravel()[None, :], R.ravel()[None, :]
        sub = _chain(period, usable, n=k * R.size)
        val = np.exp(sub.logq(pts.reshape(-1, 4))).reshape(k, R.size)
        total += ((val * (rw[:, None] * pw[None, :]).ravel()[None, :]).sum(axis=1) * w2[sel]).sum()
    print("integral of exp(logq): 1 %+.2e (period %g, usable %s)" % (total - 1, period, usable))
    assert abs(total - 1) < 1e-6
    # and logq is the issue's formula
    rs = np.random.RandomState(3)
    n = 4000
    sh = np.stack([rs.uniform(0, 1, n), np.exp(rs.uniform(-2, 2, n)), rs.uniform(0, period, n), rs.uniform(0, 1, n)], axis=1)
    one = _chain(period, usable, n=n)
    assert np.allclose(one.logq(sh), _restated_logq(one, sh, usable), rtol=1e-12, atol=1e-12)
    out = sh.copy()
    out[::4, 0], out[1::4, 1], out[2::4, 2], out[3::4, 3] = 1.5, -1.0, period + 1.0, 0.0
    assert np.all(one.logq(out) == -np.inf) and np.all(one.log_prior(out) == -np.inf)


def test_draws_follow_logq():
    """chi^2 per coordinate of 20 000 draws of chain 7 from seeds 0 .. 19 999 against logq's marginals (20 equiprobable bins)"""
    period, n, bins = 180.0, 20000, 20
    mp = _chain(period, True, n=8)
    d = np.stack([mp.draw(seed, [7])[0] for seed in range(n)])
    assert np.all((d[:, 0] > 0) & (d[:, 0] < 1) & (d[:, 1] > 0) & (d[:, 2] > 0) & (d[:, 2] < period) & (d[:, 3] > 0) & (d[:, 3] < 1))
    w = mp.w
    # the marginal CDFs of q
    tx, tw = np.polynomial.legendre.leggauss(48)
    tx, tw = 0.5 * (tx + 1), 0.5 * tw
    lsh = np.log(3600.0 * np.sqrt(mp.lam_max[0] / (tx * mp.V_exp + (1 - tx) * mp.V_dev)))
    ls = np.linspace(-6.0, 12.0, 36001)
    dens_prior = np.exp(log(2.0) - lgamma(1.5) - 3 * ls - np.exp(-2 * ls))               # p(sigma) sigma, per d log sigma
    cdf_prior = np.concatenate([[0.0], np.cumsum(0.5 * (dens_prior[1:] + dens_prior[:-1]) * np.diff(ls))])
    assert abs(cdf_prior[-1] - 1) < 1e-6

    def cdf_sigma(s):
        l_ = np.log(s)
        loc = (_Phi((l_[:, None] - lsh[None, :]) / mp.s_sigma) * tw[None, :]).sum(axis=1)
        return w * np.interp(l_, ls, cdf_prior) + (1 - w) * loc

    def cdf_rho(r):
        return w * r + (1 - w) * _Phi((np.log(r / (1 - r)) - log(0.6 / 0.4)) / mp.s_rho)

    def cdf_phi(p):
        return w * p / period + (1 - w) * np.clip((p - 10.0) / 60.0, 0.0, 1.0)              # one window, 40 +- 30, inside (0, 180)
    stats = {}
    for name, u in (("theta", d[:, 0]), ("sigma", cdf_sigma(d[:, 1])), ("phi", cdf_phi(d[:, 2])), ("rho", cdf_rho(d[:, 3]))):
        cnt = np.histogram(u, bins=bins, range=(0.0, 1.0))[0]
        assert cnt.sum() == n
        stats[name] = float(((cnt - n / bins) ** 2 / (n / bins)).sum())
    print("chi^2 (19 dof):", {k: round(v, 1) for k, v in stats.items()})
    bound = (bins - 1) + 4.5 * sqrt(2.0 * (bins - 1))
    assert all(v < bound for v in stats.values()), stats
    # an unusable chain's draws are the prior's, bit for bit, and every chain takes the same count of numbers
    un = _chain(period, False, n=8)
    model = celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)))
    assert np.array_equal(un.draw(5, np.arange(8)), model.sample_shape_prior(5, np.arange(8)))


def test_h_is_antisymmetric_and_w_1_is_the_prior_proposal():
    rs = np.random.RandomState(8)
    n = 64
    sh = np.stack([rs.uniform(0, 1, n), np.exp(rs.uniform(-2, 2, n)), rs.uniform(0, 180, n), rs.uniform(0, 1, n)], axis=1)
    mp = MomentProposal()
    mp.set_centre(rs.rand(n) < 0.8, np.exp(rs.uniform(-17, -13, n)), rs.uniform(0, 1, n), rs.uniform(0, 180, n), 180.0)
    fwd = mp.h_of(sh, np.ones(n, bool), 0.3)
    back = mp.h_of(sh, np.zeros(n, bool), 0.3)
    assert np.all(np.isfinite(fwd)) and np.all(fwd == -back) and np.any(fwd != 0.3)
    assert np.all(fwd[~mp.usable] == 0.3)                        # the prior's own proposal: the densities cancel exactly
    one = MomentProposal(w=1.0).set_centre(mp.usable, mp.lam_max, mp.rho_hat, mp.phi0, 180.0)
    assert np.all(one.h_of(sh, np.ones(n, bool), 0.3) == 0.3) and np.all(one.h_of(sh, np.zeros(n, bool), 0.3) == -0.3)
    model = celeste_mcmc.ModelGibbs([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)))
    ids = rs.permutation(n)
    assert np.array_equal(one.draw(99, ids), model.sample_shape_prior(99, ids))
    with pytest.raises(ValueError):
        MomentProposal(w=0.0)


def test_wiring():
    empty = ([], np.zeros(0, np.int32), np.zeros((0, 2)), np.zeros((0, 5)), np.zeros((0, 4)))
    assert celeste_mcmc.ModelGibbs(*empty).type_proposal == "prior" and celeste_mcmc.ModelGibbs(*empty).moment_proposal is None
    g = celeste_mcmc.ModelGibbs(*empty, type_proposal="moments")
    assert isinstance(g.moment_proposal, MomentProposal)
    with pytest.raises(ValueError, match="type_proposal"):
        celeste_mcmc.ModelGibbs(*empty, type_proposal="data")
    custom = celeste_mcmc.ModelGibbs(*empty, type_proposal="moments", shape_logprior=lambda TH: np.zeros(TH.shape[0]))
    with pytest.raises(ValueError, match="custom proposal"):
        custom.resample_types()
    with pytest.raises(ValueError, match="custom shape prior"):
        custom.sweep(types=True)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
H = W = 128
B = 3


def _full_box(ctx, L):
    class cm(object):
        def __enter__(self):
            self.was = ctx.get_option(L.CEL_OPT_SPLIT_FULL_BOX)
            ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)

        def __exit__(self, *exc):
            ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, self.was)
    return cm()


@gpu
@pytest.mark.parametrize("conditional", ["reference", "exact"])
def test_detailed_balance_through_the_kernel(cel, conditional):
    """log_alpha of star -> galaxy(drawn shape) plus log_alpha of that galaxy -> star is zero to rounding.  Each is
    fl(fl(v' - v) + h) with h exact negatives of each other and v, v' the two rows' scores, which do not depend on the slot that
    holds the row: at most two roundings of half an ulp each per direction, of numbers no larger than 2 max(|v|, |v'|) + |h| --
    so |sum| <= 4 eps (max(|v|, |v'|) + |h|), whatever the order in which the kernel adds its bands (a band-wise sum adds B - 1
    roundings of the same size: the bound below carries the factor B).  MEASURED under either conditional: 24 of 24 chains scored
    both ways, 10 of them usable, every sum exactly 0, log alpha from -1.7e4 to 5.3e3."""
    from desi_mcmc_amd import synth
    ctx, L = cel.default_context(0), cel._lib
    S = 24
    f = synth.SyntheticField(ctx, S, B, H, W, frac_gal=0.5)
    star, gal = np.zeros(S, np.int32), np.ones(S, np.int32)
    f.sources.set(star, f.src["radec"], f.src["counts"], np.zeros((S, 4)))
    with _full_box(ctx, L):                                      # the photons of the all-star catalogue: every star row covers its own
        f.images.photon_split_resident(f.sources, seed=5)
    gf =celeste_mcmc.GibbsField(f.images, list(range(B)), f.bands[:, 2], f.bands[:, 1], H * W)
    flux5 = np.full((S, 5), 3.0)
    flux5[:, :B] = f.src["flux"]
    model = celeste_mcmc.ModelGibbs([gf], np.zeros(S, np.int32), f.src["radec"], flux5, np.zeros((S, 4)), seed=3, type_log_odds=0.4)
    mp = MomentProposal().observe(model)
    drawn = mp.draw(17, np.arange(S))
    h_sg, h_gs = mp.h_of(drawn, star == 0, 0.4), mp.h_of(drawn, gal == 0, 0.4)
    assert np.all(h_sg == -h_gs)
    f.sources.set(star, f.src["radec"], f.src["counts"], np.zeros((S, 4)))
    la_sg = f.images.type_move(f.sources, drawn, h_sg, 21, conditional=conditional)[2]
    # back: only the chains whose galaxy row lies inside its own conditional (under the exact one its box must cover the photons;
    # the move refuses a chain that starts outside)
    ids = np.where(np.isfinite(la_sg), np.arange(S), -1).astype(np.int32)
    f.sources.set(gal, f.src["radec"], f.src["counts"], drawn)
    la_gs = f.images.type_move(f.sources, drawn, h_gs, 22, chain_ids=ids, conditional=conditional)[2]
    # the scale of the scores, from the public scorer (the reference's conditional; the exact one adds counts * mass, smaller)
    prop = cel.SourceSet(ctx, 2 * S, B)
    own = np.repeat(np.arange(S), 2).astype(np.int32)
    prop.set(np.tile([0, 1], S).astype(np.int32), f.src["radec"][own], f.src["counts"][own], np.repeat(drawn, 2, axis=0))
    v = f.images.patch_loglik_resident(prop, own).reshape(S, 2)
    both = np.isfinite(la_sg) & np.isfinite(la_gs)
    tol = 4 * B * np.finfo(np.float64).eps * (np.abs(v).max(axis=1) + np.abs(h_sg))
    worst = np.abs(la_sg + la_gs)[both] / tol[both]
    print("detailed balance (%s): %d of %d chains scored both ways, usable %d, worst |sum| / tol %.3g, log alpha %.3g .. %.3g"
          % (conditional, both.sum(), S, mp.usable.sum(), worst.max(), la_sg[both].min(), la_sg[both].max()))
    # not vacuous: most chains are scored both ways, and at least a quarter take the data's q_loc (the other chains' proposal is
    # the prior's: under the all-star split a true star's second moment is no wider than the PSF's)
    assert both.sum() >= S // 2 and mp.usable.sum() >= S // 4 and np.any(h_sg[mp.usable] != 0.4)
    assert np.all(np.abs(la_sg + la_gs)[both] <= tol[both])


def _bright_galaxies():
    """a dozen COMPACT, bright galaxies (r_e 0.12" .. 0.25", a third to two thirds of a pixel; 300 .. 600 nmgy, tens of thousands
    of photons per band) on a grid of the 128 x 128 frame -- all TYPED AS STARS.
    Why compact: a star is the sigma -> 0 end of the galaxy family, so the shapes that beat a star on a true galaxy of size s are
    roughly those below ~1.4 s (as far from the truth on the other side).  For an EXTENDED galaxy that is most of the prior --
    measured on galaxies of 1.3" .. 3.5" at 5 000 - 28 000 photons per band: the prior proposal is accepted 59 times in 96, the
    moment proposal 84 -- and the prior proposal is not inert at all.  It is inert where the star is NEARLY right: below ~0.3" the
    prior (1 / sigma^2 ~ Gamma(3/2, 1)) puts 2e-5 of its mass, while at 1e5 photons the star still loses by hundreds of nats."""
    from desi_mcmc_amd import synth
    S = 12
    bands = synth.make_bands(H, W, B)
    rs = np.random.RandomState(31)
    gx, gy = np.meshgrid([20.0, 50.0, 80.0, 108.0], [22.0, 64.0, 104.0])
    pix = np.stack([gx.ravel(), gy.ravel()], axis=1) + rs.uniform(-0.5, 0.5, (S, 2))
    shape = np.stack([rs.uniform(0.2, 0.8, S), rs.uniform(0.12, 0.25, S), rs.uniform(5, 175, S), rs.uniform(0.3, 0.7, S)], axis=1)
    flux = np.exp(rs.uniform(np.log(300.0), np.log(600.0), (S, B)))
    counts = flux / bands[None, :, 2] * bands[None, :, 1]
    return dict(S=S, bands=bands, radec=synth.pixel2equa(bands[0], pix), shape=shape, flux=flux, counts=counts)


@gpu
def test_it_moves_what_the_prior_cannot(cel):
    """Twelve true galaxies (>= 1 000 photons per band), typed as stars, eight seeds, one type move each on the same photons:
    accepted star -> galaxy moves under the prior proposal against the moment proposal.
    MEASURED (50 000 - 290 000 photons per band): the prior proposal is accepted 0 times in 96, the moment proposal 61 times,
    all 12 chains at least once.  (On EXTENDED galaxies the prior proposal is not inert: _bright_galaxies' docstring.)"""
    ctx = cel.default_context(0)
    sc = _bright_galaxies()
    S = sc["S"]
    truth = cel.SourceSet(ctx, S, B).set(np.ones(S, np.int32), sc["radec"], sc["counts"], sc["shape"])
    iset = cel.ImageSet(ctx, sc["bands"], H, W)
    iset.render(truth, loglik=False)
    nelec = np.random.RandomState(32).poisson(iset.model_images()).astype(np.float64)
    iset.set_nelec(nelec)
    flux5 = np.full((S, 5), 3.0)
    flux5[:, :B] = sc["flux"]
    accepted, ever, photons = {}, {}, None
    for prop in ("prior", "moments"):
        accepted[prop], ever[prop] = 0, np.zeros(S, bool)
        for seed in range(8):
            gf = celeste_mcmc.GibbsField(iset, list(range(B)), sc["bands"][:, 2], sc["bands"][:, 1], H * W)
            g = celeste_mcmc.ModelGibbs([gf], np.zeros(S, np.int32), sc["radec"], flux5, np.zeros((S, 4)), seed=seed,
                                        type_proposal=prop)
            g.resample_photons()
            if photons is None:
                photons = iset.sample_sums()
            g.resample_types()
            accepted[prop] += int((g.typ == 1).sum())
            ever[prop] |= g.typ == 1
            assert g.timing["type_accepted"] == int((g.typ == 1).sum())
    print("star -> galaxy accepted in 8 x %d proposals: prior %d, moments %d; chains accepted at least once: prior %d, moments %d; "
          "photons per band, faintest source: %s" % (S, accepted["prior"], accepted["moments"], ever["prior"].sum(),
                                                      ever["moments"].sum(), photons.min(axis=0)))
    assert photons.min() >= 1000
    assert accepted["prior"] <= 2                                 # else the scene is too faint to show anything
    assert accepted["moments"] > accepted["prior"] and ever["moments"].sum() >= S / 4.0
    iset.close()


def _engines(cel, masked):
    from desi_mcmc_amd import synth
    Sf = 12
    ctx = cel.Context(0)
    f0 = synth.SyntheticField(ctx, Sf, B, H, W, frac_gal=0.5, seed=23)
    nelec = f0.nelec.copy()
    if masked:
        for x, y in f0.src["pix"][::2]:
            nelec[0, min(int(y), H - 1), min(int(x), W - 1)] = np.nan
        nelec[0, :, 40:44] = np.nan
        nelec[1, 63:65, :] = np.nan
    flux5 = np.full((Sf, 5), 3.0)
    flux5[:, :B] = f0.src["flux"]
    # every source starts as the WRONG type, so that moves are accepted: the galaxies as stars, the stars as compact galaxies
    typ0 = (1 - f0.src["type"]).astype(np.int32)
    shape0 = np.where((typ0 == 1)[:, None], np.array([0.5, 0.3, 45.0, 0.7])[None, :], 0.0)
    g = {}
    for e in ("host", "device"):
        imgs = cel.ImageSet(ctx, f0.bands, H, W)
        imgs.set_nelec(nelec)
        kw = dict(mask="honour", mask_engine="device") if masked else {}
        gf = celeste_mcmc.GibbsField(imgs, list(range(B)), f0.bands[:, 2], f0.bands[:, 1], H * W,
                                     npix_observed=imgs.npix_observed() if masked else None)
        g[e] = celeste_mcmc.ModelGibbs([gf], typ0, f0.src["radec"], flux5, shape0, seed=5, conditional="exact",
                                       engine=e, type_proposal="moments", type_log_odds=0.2, **kw)
    return g, Sf


@gpu
@pytest.mark.parametrize("masked", [False, True])
def test_the_engines_and_the_catalogue_agree(cel, masked):
    """ModelGibbs(type_proposal="moments") on the host and the device engine: typ, shape, u, fluxes and the acceptance counts are
    equal after each of three sweep(types=True) (once under mask="honour", mask_engine="device"), and the device's catalogue
    (cel_sources_get) holds the chain's types and shapes."""
    g, Sf = _engines(cel, masked)
    assert g["device"]._type_engine_on_device() and not g["host"]._type_engine_on_device()
    for sweep in range(3):
        for e in g:
            g[e].sweep(types=True)
        for name in ("typ", "shape", "u", "fluxes"):
            assert np.array_equal(getattr(g["host"], name), getattr(g["device"], name)), (sweep, name)
        assert g["host"].timing["type_evals"] == g["device"].timing["type_evals"] > 0
        assert g["host"].timing["type_accepted"] == g["device"].timing["type_accepted"]
        for e in g:
            for a, b in zip(g[e].moment_proposal.moments, g["host"].moment_proposal.moments):
                assert np.array_equal(a, b)
        typ, _, _, shape = g["device"].fields[0].sset.get()
        assert np.array_equal(typ[:Sf], g["device"].typ)
        isgal = g["device"].typ == 1
        assert np.array_equal(shape[:Sf][isgal], g["device"].shape[isgal])
    t = g["device"].timing
    print("ENGINES (masked %s): type evals %d, accepted %d, usable chains %d of %d"
          % (masked, t["type_evals"], t["type_accepted"], g["device"].moment_proposal.usable.sum(), Sf))
    assert t["type_accepted"] > 0
