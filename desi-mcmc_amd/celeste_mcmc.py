"""Mirror of the runnable Gibbs step of CelestePy/celeste_mcmc.py: the photon split.

sample_source_photons_single_image_cython (celeste_mcmc.py:98-150) renders every source's
counts-scaled patch (gen_src_image_with_fluxes) and calls the Cython multinomial split
(celeste_sample_sources.pyx:61-156).  Here both happen in one device pass (cel_photon_split);
the (samp_imgs, noise_sum) return shape is kept.  The rest of celeste_mcmc.py is not runnable in
the reference as written and is not mirrored.

Random numbers: the reference draws from randomkit's MT19937 through numpy's RandomState; the
device uses a counter-based Philox generator.  Results match in distribution, not draw by draw.
"""
import numpy as np

from . import celeste as _celeste
from .sources import SamplePatch


_M64 = (1 << 64) - 1
# one tag per randomised step of a sweep: no two steps share a stream key for any seed (with seed = 0 the plain
# `seed * prime + sweep` forms all collapsed to `sweep`, and a source's location, shape and flux draws were one sequence)
STEP_TAGS = dict(split=0x53504C4954000001, flux=0x464C555800000002, location=0x4C4F434154000003, shape=0x5348415045000004,
                 type=0x5459504500000005, hmc=0x484D430000000006)


def _mix64(z):
    """SplitMix64's finaliser on a Python int"""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def step_seed(seed, step, sweep, k=0):
    """the stream seed of one step (`split`, `flux`, `location`, `shape`, `type`, `hmc`) of sweep number `sweep` (of field k): a hash of
    all of them, so that the Gibbs blocks draw from unrelated streams whatever the chain's seed is"""
    return _mix64((_mix64(_mix64(int(seed) & _M64) ^ STEP_TAGS[step]) + int(sweep)) & _M64 ^ (int(k) * 0xD6E8FEB86659FD93 & _M64))


def _flux_counts(src, image):
    return (src.flux_dict[image.band] / image.calib) * image.kappa      # celeste.py:80-81,94


def sample_source_photons_multi_image(imgs, srcs, seed=None):
    """The split for several same-shape images in one pass.
    -> (samp_imgs[n][s] SamplePatch or None, noise_sums[n])"""
    if seed is None:
        seed = np.random.randint(0, 2 ** 31 - 1)
    imgs = tuple(imgs)
    iset = _celeste._image_set(imgs)
    typ, radec, counts, shape = _celeste._source_arrays(srcs, imgs, counts_fn=_flux_counts)
    sset = iset._sources(typ, radec, counts, shape)
    patches, boxes, noise = iset.photon_split(sset, seed)
    out = []
    for n in range(len(imgs)):
        row = []
        for s in range(len(srcs)):
            p = patches[n][s]
            if p is None:
                row.append(None)
            else:
                y0, y1, x0, x1 = boxes[n, s]
                row.append(SamplePatch(p, (y0, y1), (x0, x1)))
        out.append(row)
    return out, noise


def sample_source_photons_single_image_cython(img, srcs, seed=None):
    """Given a single photon-count image and a list of sources, sample source-specific images
    using the Poisson/multinomial representation  -- celeste_mcmc.py:98-150.
    returns (samp_imgs: list of SamplePatch (x0,x1,y0,y1,data) or None, noise_sum)"""
    samp, noise = sample_source_photons_multi_image((img,), srcs, seed)
    return samp[0], noise[0]


def gamma_by_stream(a, seed, ids):
    """Standard Gamma(a) variates, one per element of `a`, each from ITS OWN counter-based stream (seed, ids[i]) -- so that a
    source's flux draw does not depend on which other sources are drawn beside it, by which rank, or in what order (numpy's
    generator hands a sequential stream to a rejection sampler: the numbers an element gets depend on every element before
    it).  Marsaglia & Tsang (2000): x ~ N(0,1), v = (1 + c x)^3, accept when log u < x^2/2 + d - d v + d log v with
    d = a - 1/3, c = 1 / sqrt(9 d); a < 1 through Gamma(a + 1) U^(1/a).  Host-side, vectorised: a round over the elements
    still waiting for an acceptance (~5 % per round)."""
    from .util.infer.slicesample import ChainStreams
    a = np.asarray(a, dtype=np.float64)
    st = ChainStreams(seed, np.asarray(ids))
    n = a.shape[0]
    boost = a < 1.0
    aa = np.where(boost, a + 1.0, a)
    d = aa - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = np.empty(n)
    todo = slice(None)                   # the first round takes every element: views, not gathers
    left = n
    while left:
        x, u = st.normal(todo), st.uniform(todo)
        dt = d[todo]
        t = 1.0 + c[todo] * x
        v = t * t * t
        x2 = x * x
        # the squeeze u < 1 - 0.0331 x^4 implies the full test (Marsaglia & Tsang, step 3): ~92 % accept without a logarithm
        ok = (v > 0.0) & (u < 1.0 - 0.0331 * x2 * x2)
        rest = np.nonzero((v > 0.0) & ~ok)[0]
        if rest.size:
            vr = v[rest]
            ok[rest] = np.log(u[rest]) < 0.5 * x2[rest] + dt[rest] * (1.0 - vr + np.log(vr))
        if isinstance(todo, slice):
            out[ok] = dt[ok] * v[ok]
            todo = np.nonzero(~ok)[0]
        else:
            out[todo[ok]] = dt[ok] * v[ok]
            todo = todo[~ok]
        left = todo.size
    if boost.any():
        idx = np.nonzero(boost)[0]
        out[idx] *= st.uniform(idx) ** (1.0 / a[idx])
    return out


# ---- the type move's data-driven proposal: a galaxy shape from the second moments of the source's photons -------------------
def _profile_variances():
    """(V_exp, V_dev): the amplitude-weighted variances of mixture_profiles' two profiles, in units of r_e^2"""
    from . import mixture_profiles as mp
    return float(np.sum(mp.exp_amp * mp.exp_var)), float(np.sum(mp.dev_amp * mp.dev_var))


def psf_covariance(band):
    """the covariance of a band's PSF mixture about its own mean, in pixels^2, from its (37,) record:
    sum_k w_k (Sigma_k + mu_k mu_k^T) / sum_k w_k - mubar mubar^T"""
    band = np.asarray(band, dtype=np.float64)
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    ws = w.sum()
    mubar = (w[:, None] * mu).sum(axis=0) / ws
    return (w[:, None, None] * (cov + mu[:, :, None] * mu[:, None, :])).sum(axis=0) / ws - np.outer(mubar, mubar)


def _band_pixel2equa(band, p):
    rho, phi, ups = band[24:26], band[26:28], band[28:32].reshape(2, 2)
    iwc = (p - rho[None, :]) @ ups.T
    return iwc[:, 0] / np.cos(phi[1] / 180. * np.pi) + phi[0], iwc[:, 1] + phi[1]


def band_cd_at(band, u):
    """cd_at_pixel (fits_image.py:196-216, the 10-px finite difference the renderer takes) of a (37,) band record at the pixel
    positions of the sky positions u (S, 2) -> (S, 2, 2), degrees per pixel"""
    band = np.asarray(band, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    rho, phi, ups_inv = band[24:26], band[26:28], band[32:36].reshape(2, 2)
    iwc = np.stack([(u[:, 0] - phi[0]) * np.cos(phi[1] / 180. * np.pi), u[:, 1] - phi[1]], axis=1)
    p = iwc @ ups_inv.T + rho[None, :]
    ra0, dec0 = _band_pixel2equa(band, p)
    rax, decx = _band_pixel2equa(band, p + np.array([10., 0.]))
    ray, decy = _band_pixel2equa(band, p + np.array([0., 10.]))
    cosd = np.cos(dec0 * (np.pi / 180.))
    cd = np.empty((u.shape[0], 2, 2))
    cd[:, 0, 0], cd[:, 0, 1] = (rax - ra0) / 10. * cosd, (ray - ra0) / 10. * cosd
    cd[:, 1, 0], cd[:, 1, 1] = (decx - dec0) / 10., (decy - dec0) / 10.
    return cd


def moment_centre(N, C, psf_cov, cd, n_min=50):
    """From the photons' second moments to the centre of a shape proposal, for S chains and n (field, band) images at once.
        N        (S, n)        photons of the chain in the image
        C        (S, n, 2, 2)  their central second moment in pixels^2, S2 / N - m m^T (ignored where N < 1)
        psf_cov  (n, 2, 2)     the image's PSF covariance (psf_covariance)
        cd       (S, n, 2, 2)  the image's cd_at_pixel at the source
    D = C - psf_cov is carried to the sky, A_b = cd D cd^T (degrees^2), and pooled, A = sum N_b A_b / sum N_b.  A galaxy's stamp
    has A = vbar(theta) G G^T with G G^T = r_e^2 R diag(1, rho^2) R^T (gen_galaxy_ra_dec_basis: R's first column is
    (cos phi', -sin phi'), phi' = 90 - phi degrees), so the larger eigenvalue is vbar r_e^2, the ratio of the two rho^2 and the
    major eigenvector gives phi modulo 180.
    -> (usable (S,) bool, lam_max (S,) degrees^2, rho_hat (S,) UNCLIPPED, phi_hat (S,) in [0, 180) degrees); a chain is usable when
    sum N >= n_min and A has two positive eigenvalues (the other outputs are 1, 0.5, 0 where it is not)."""
    N = np.asarray(N, dtype=np.float64)
    S = N.shape[0]
    has = N >= 1.0
    C, P, cd = np.asarray(C, dtype=np.float64), np.asarray(psf_cov, dtype=np.float64), np.asarray(cd, dtype=np.float64)
    Nw = np.where(has, N, 0.0)
    Ntot = Nw.sum(axis=1)
    wgt = Nw / np.maximum(Ntot, 1.0)[:, None]                 # (a band without photons has weight 0: its C is never read as data)
    d00, d01, d11 = C[..., 0, 0] - P[None, :, 0, 0], 0.5 * (C[..., 0, 1] + C[..., 1, 0]) - P[None, :, 0, 1], C[..., 1, 1] - P[None, :, 1, 1]
    c00, c01, c10, c11 = cd[..., 0, 0], cd[..., 0, 1], cd[..., 1, 0], cd[..., 1, 1]
    t00, t01, t10, t11 = c00 * d00 + c01 * d01, c00 * d01 + c01 * d11, c10 * d00 + c11 * d01, c10 * d01 + c11 * d11
    with np.errstate(invalid="ignore"):                        # the 2 x 2 products cd D cd^T, written out (S x n of them per call)
        a = np.where(has, wgt * (t00 * c00 + t01 * c01), 0.0).sum(axis=1)
        b = np.where(has, wgt * (t00 * c10 + t01 * c11), 0.0).sum(axis=1)
        c = np.where(has, wgt * (t10 * c10 + t11 * c11), 0.0).sum(axis=1)
    half, diff = 0.5 * (a + c), 0.5 * (a - c)
    root = np.hypot(diff, b)
    lmax = half + root
    det = a * c - b * b
    with np.errstate(invalid="ignore", divide="ignore"):
        lmin = np.where(lmax > 0, det / lmax, -1.0)          # (the product of the two, not half - root: no cancellation)
    usable = (Ntot >= n_min) & (lmin > 0) & (lmax > 0) & np.isfinite(lmax) & np.isfinite(lmin)
    # the major eigenvector: (b, lmax - a) or (lmax - c, b), whichever is longer (both vanish only for a round A: any phi serves)
    e1x, e1y, e2x, e2y = b, lmax - a, lmax - c, b
    first = (e1x * e1x + e1y * e1y) >= (e2x * e2x + e2y * e2y)
    ex, ey = np.where(first, e1x, e2x), np.where(first, e1y, e2y)
    round_ = (ex == 0) & (ey == 0)
    ex = np.where(round_, 1.0, ex)
    phi_p = np.degrees(np.arctan2(-ey, ex))                   # e = (cos phi', -sin phi')
    phi = np.mod(90.0 - phi_p, 180.0)
    phi = np.where(phi >= 180.0, 0.0, phi)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.sqrt(np.where(usable, lmin / lmax, 0.25))
    return usable, np.where(usable, lmax, 1.0), rho, np.where(usable, phi, 0.0)


class MomentProposal(object):
    """The star <-> galaxy move's proposal that looks at the data (ModelGibbs(type_proposal="moments"); resample_types(proposal=)).

    Given the photon split a source's photons are fixed while it changes type, so a density q(shape | photons of s) serves
    both directions of the Metropolis-Hastings ratio.  The statistic is the second moment of the source's photons
    (ImageSet.photon_moments, reduced on the device) with each band's PSF taken out, carried to the sky and pooled over bands
    and fields (moment_centre): it fixes rho, phi modulo 180 and, for a given theta, sigma:
        sigma_hat(theta) = 3600 sqrt(lam_max / vbar(theta)),   vbar = theta V_exp + (1 - theta) V_dev,
        rho_hat = sqrt(lam_min / lam_max) clipped to [0.05, 0.95],   phi_hat = the major axis, every image phi_hat + 180 k inside
        (0, phi_period) with equal weight.
    For a usable chain (sum N >= n_min, two positive eigenvalues)
        q(shape | m) = w p(shape) + (1 - w) q_loc(shape | m)
    with p the normalised prior (sample_shape_prior's law) and q_loc the product of theta ~ U(0, 1),
    log sigma ~ N(log sigma_hat(theta), s_sigma^2), logit rho ~ N(logit rho_hat, s_rho^2), phi = (phi_hat_k + U(-a_phi, a_phi)) mod
    period; the Jacobians 1 / sigma and 1 / (rho (1 - rho)) are in the density.  Any other chain's proposal is the prior's.  The
    share w of the prior keeps h finite on the whole support, as cel_slice_sample demands.
    The defaults (w = 0.1, s_sigma = 0.5, s_rho = 1, a_phi = 30 degrees capped at half the period, n_min = 50) are first guesses:
    nobody has tuned them.

    draw(seed, ids) takes THIRTEEN numbers per chain from ChainStreams(seed, ids), usable or not, in this order: the uniforms
    theta, rho, phi and the normal z and uniform u of sigma exactly as sample_shape_prior takes them (five), then the uniform that
    chooses the prior (< w) or q_loc, then q_loc's: the uniform theta, the normals of log sigma and of logit rho, the uniform that
    picks the image of phi_hat and the uniform of its offset.  (A normal is two numbers of the chain's normal stream.)

    Host numpy, vectorised over the chains; the host and device engines of resample_types take the same (shapes, h)."""

    def __init__(self, w=0.1, s_sigma=0.5, s_rho=1.0, a_phi=30.0, n_min=50):
        if not (0.0 < w <= 1.0):
            raise ValueError("MomentProposal: the prior's share w must be in (0, 1]: without it h is not finite on the whole support")
        if not (s_sigma > 0 and s_rho > 0 and a_phi > 0):
            raise ValueError("MomentProposal: the widths must be positive")
        self.w, self.s_sigma, self.s_rho, self.a_phi, self.n_min = float(w), float(s_sigma), float(s_rho), float(a_phi), n_min
        self.V_exp, self.V_dev = _profile_variances()
        self.moments = None

    # -- the state: one centre per chain -----------------------------------------------------------------------------------------
    def set_centre(self, usable, lam_max, rho_hat, phi_hat, phi_period):
        """what moment_centre returned, and the period of phi"""
        self.period = float(phi_period)
        self.usable = np.asarray(usable, dtype=bool)
        self.lam_max = np.asarray(lam_max, dtype=np.float64)
        self.rho_hat = np.clip(np.asarray(rho_hat, dtype=np.float64), 0.05, 0.95)
        phi0 = np.mod(np.asarray(phi_hat, dtype=np.float64), 180.0)
        if self.period >= 180.0:
            # images phi0 + 180 k below the period: floor((period - phi0) / 180) of them beyond phi0, at least phi0 itself
            self.n_img = np.maximum(np.ceil((self.period - phi0) / 180.0), 1.0)
            self.phi0 = phi0
        else:
            self.n_img = np.ones_like(phi0)
            self.phi0 = np.mod(phi0, self.period)
        self.half = min(self.a_phi, 0.5 * self.period)
        return self

    def observe(self, model):
        """take the moments of every field's current split (once per call) and set the centres"""
        N, C, P, CD = [], [], [], []
        self.moments = []
        for f in model.fields:
            mom = f.iset.photon_moments()
            self.moments.append(mom)
            m = mom.astype(np.float64)
            n = np.maximum(m[..., 0], 1.0)
            mx, my = m[..., 1] / n, m[..., 2] / n
            c = np.empty(m.shape[:2] + (2, 2))
            c[..., 0, 0] = m[..., 3] / n - mx * mx
            c[..., 0, 1] = c[..., 1, 0] = m[..., 4] / n - mx * my
            c[..., 1, 1] = m[..., 5] / n - my * my
            N.append(m[..., 0])
            C.append(c)
            for b in range(f.iset.B):
                band = f.iset.band(b)
                P.append(psf_covariance(band))
                CD.append(band_cd_at(band, model.u))
        out = moment_centre(np.concatenate(N, axis=1), np.concatenate(C, axis=1), np.stack(P), np.stack(CD, axis=1), self.n_min)
        return self.set_centre(*out, phi_period=model.phi_period)

    # -- the density -------------------------------------------------------------------------------------------------------------
    def sigma_hat(self, theta):
        """sigma_hat(theta) per chain, arc seconds"""
        return 3600.0 * np.sqrt(self.lam_max / (theta * self.V_exp + (1.0 - theta) * self.V_dev))

    def log_prior(self, shapes):
        """log of the NORMALISED prior (sample_shape_prior's law): theta, rho ~ U(0, 1), phi ~ U(0, period),
        p(sigma) = 2 sigma^-4 exp(-1 / sigma^2) / Gamma(3/2); -inf outside the support"""
        from math import lgamma, log
        th, sg, ph, rh = (np.asarray(shapes, dtype=np.float64)[:, i] for i in range(4))
        inside = (th > 0) & (th < 1) & (sg > 0) & (ph > 0) & (ph < self.period) & (rh > 0) & (rh < 1)
        s = np.where(inside, sg, 1.0)
        return np.where(inside, (log(2.0) - lgamma(1.5) - log(self.period)) - 4.0 * np.log(s) - 1.0 / (s * s), -np.inf)

    def log_phi(self, ph):
        """log density of q_loc's phi: n_img windows of half width `half` about the images of phi_hat, wrapped into the period"""
        dens = np.zeros_like(ph)
        for k in range(int(self.n_img.max())):
            d = np.abs(ph - (self.phi0 + 180.0 * k))
            d = np.minimum(d, self.period - d)                 # distance on the circle of length `period`
            dens += np.where((k < self.n_img) & (d < self.half), 1.0, 0.0)
        with np.errstate(divide="ignore"):
            return np.log(dens / (self.n_img * 2.0 * self.half))

    def log_loc(self, shapes):
        """log q_loc(shape | m) per chain (meaningful for the usable ones); -inf outside the support"""
        from math import log, pi
        th, sg, ph, rh = (np.asarray(shapes, dtype=np.float64)[:, i] for i in range(4))
        inside = (th > 0) & (th < 1) & (sg > 0) & (ph > 0) & (ph < self.period) & (rh > 0) & (rh < 1)
        t, s, r = np.where(inside, th, 0.5), np.where(inside, sg, 1.0), np.where(inside, rh, 0.5)
        zs = (np.log(s) - np.log(self.sigma_hat(t))) / self.s_sigma
        zr = (np.log(r / (1.0 - r)) - np.log(self.rho_hat / (1.0 - self.rho_hat))) / self.s_rho
        lq = (-0.5 * zs * zs - log(self.s_sigma) - 0.5 * log(2.0 * pi) - np.log(s)
              - 0.5 * zr * zr - log(self.s_rho) - 0.5 * log(2.0 * pi) - np.log(r * (1.0 - r))
              + self.log_phi(np.where(inside, ph, self.phi0)))
        return np.where(inside, lq, -np.inf)

    def logq(self, shapes):
        """log q(shape | m) for one shape per chain, (S, 4) -> (S,)"""
        from math import log
        lp = self.log_prior(shapes)
        if self.w >= 1.0:
            return lp
        with np.errstate(invalid="ignore"):
            mix = np.logaddexp(log(self.w) + lp, log(1.0 - self.w) + self.log_loc(shapes))
        return np.where(self.usable & (lp > -np.inf), mix, lp)

    # -- the draw ----------------------------------------------------------------------------------------------------------------
    def draw(self, seed, ids):
        """one shape per chain of `ids` (indices of the chains whose centres are set) -> (len(ids), 4); the order of the thirteen
        numbers a chain takes: the class's docstring"""
        from .util.infer.slicesample import ChainStreams
        ids = np.asarray(ids)
        cs = ChainStreams(seed, ids)
        every = np.arange(len(ids))
        theta, rho = cs.uniform(every), cs.uniform(every)
        phi = cs.uniform(every) * self.period
        z, u = cs.normal(every), cs.uniform(every)
        sigma = 1.0 / np.sqrt(z * z / 2.0 - np.log(u))
        prior = np.stack([theta, sigma, phi, rho], axis=1)
        pick = cs.uniform(every)
        t2, zs, zr, ui, uo = cs.uniform(every), cs.normal(every), cs.normal(every), cs.uniform(every), cs.uniform(every)
        lam, rh = self.lam_max[ids], self.rho_hat[ids]
        s2 = 3600.0 * np.sqrt(lam / (t2 * self.V_exp + (1.0 - t2) * self.V_dev)) * np.exp(self.s_sigma * zs)
        lr = np.log(rh / (1.0 - rh)) + self.s_rho * zr
        r2 = 1.0 / (1.0 + np.exp(-lr))
        k = np.minimum(np.floor(ui * self.n_img[ids]), self.n_img[ids] - 1.0)
        p2 = np.mod(self.phi0[ids] + 180.0 * k + (2.0 * uo - 1.0) * self.half, self.period)
        loc = np.stack([t2, s2, p2, r2], axis=1)
        take_prior = (pick < self.w) | ~self.usable[ids]
        return np.where(take_prior[:, None], prior, loc)

    # -- the caller's term of the log acceptance ratio ---------------------------------------------------------------------------------
    def h_of(self, shapes, to_galaxy, type_log_odds):
        """h for the move between a star and the galaxy of shape `shapes[s]`: + (odds + log p - log q) towards the galaxy, the
        same number with the other sign towards the star -- one expression, one sign"""
        lp = self.log_prior(shapes)
        with np.errstate(invalid="ignore"):
            # (a galaxy whose row lies outside the prior's support has no density to compare: the plain odds, as the prior proposal)
            t = type_log_odds + np.where(lp > -np.inf, lp - self.logq(shapes), 0.0)
        return np.where(to_galaxy, t, -t)

    def __call__(self, model):
        self.observe(model)
        ids = np.arange(model.S)
        drawn = self.draw(model.step_seed("type", 1), ids)
        to_gal = model.typ == 0
        shapes = np.where(to_gal[:, None], drawn, model.shape)
        h = self.h_of(shapes, to_gal, model.type_log_odds)
        moves = (model.typ == 0) | (model.typ == 1)
        return drawn, np.where(moves, h, 0.0)


# ---- the whole Gibbs sweep, catalogue-wide and device-resident -------------------------------------
class GibbsField(object):
    """One field's images on the device plus what the sweep needs to know about them."""

    def __init__(self, iset, band_index, calib, kappa, npix, a_0=5, b_0=.005, trace_iset=None, npix_observed=None):
        self.iset = iset
        # a strip-partitioned chain (dist.StripDeal): `iset` holds this rank's window (strip + halo), `trace_iset` its strip
        # alone -- what this rank adds to the field's log-likelihood; npix stays the whole frame's
        self.trace_iset = trace_iset
        self.band_index = np.asarray(band_index, dtype=np.int64)      # which of u,g,r,i,z each image is
        self.calib = np.asarray(calib, dtype=np.float64)
        self.kappa = np.asarray(kappa, dtype=np.float64)
        self.npix = float(npix)
        # a masked image set: the pixels of every band that WERE observed (ImageSet.npix_observed() for a whole-frame set) -- what
        # the sky level's Gamma conditional counts in place of npix
        self.npix_observed = None if npix_observed is None else np.asarray(npix_observed, dtype=np.float64).reshape(iset.B)
        self.a_0, self.b_0 = a_0, b_0                                  # Gamma prior of the sky level (models.py:119-121)
        self.epsilon = np.array(iset.eps, copy=True)
        self.sset = None
        self.prop = None
        self.sub = None             # this rank's sources of a dealt chain (resample_fluxes)
        self.has_patch = None
        self._sums = None           # photons per (source, image) of the current split: fetched when somebody reads `sums`

    @property
    def sums(self):
        """photons per (source, image) of the resident split, read back on first use (the device flux step never reads them:
        400 KB per sweep that stay where they are)"""
        if self._sums is None:
            self._sums = self.iset.sample_sums()
        return self._sums

    @sums.setter
    def sums(self, value):
        self._sums = value


def strip_gibbs_field(ctx, bands, nelec, rows, boxes, status, world, rank, band_index=None, slack=48, device=None, edges=None,
                      solo=False, window_trace=True):
    """This rank's part of ONE chain partitioned by row strips (dist.StripDeal).
        bands (B, 37) cel_band records, nelec (B, H, W) the whole frame's pixels (every rank can read them: only the window is
        uploaded), rows (S,) the sources' pixel rows, boxes (B, S, 4) / status (B, S) their boxes on the whole frame
        (ImageSet.source_boxes): the halo is as tall as this rank's sources' boxes reach beyond its strip, plus `slack` rows
        for the few pixels they move per sweep.
        window_trace (round 5): the chain's log-likelihood trace is rendered on the WINDOW image set, whose log-likelihood adds
        the strip's tile rows only (cel_images_set_noise_rows: the rows this rank owns) -- so the model image the next photon
        split needs is already on the device (its totals come from k_strict_totals instead of a render, the flux step's stamp
        masses from the split's own sums): what the single-rank chain does.  Needs strip edges and halo on 64-row tiles (the
        default layout's); otherwise, and with window_trace=False, a second image set of the strip alone renders the trace.
    -> (StripDeal, GibbsField over the window [with the strip as its trace image set])"""
    from . import dist as _dist
    from . import field as _field
    B, H, W = nelec.shape
    align = 64 if window_trace else _dist.TILE_ROWS
    if edges is not None and any(int(e) % 64 for e in list(edges)[:-1]):
        align, window_trace = _dist.TILE_ROWS, False
    if edges is None and int(world) > -(-H // 64):
        align, window_trace = _dist.TILE_ROWS, False
    probe = _dist.StripDeal(rows, H, world, rank, edges=edges, solo=solo, align=align)       # (edges: dist.strip_edges, the same on every rank)
    mine = probe.mine
    has = status[:, mine] > 0
    reach = max(int(np.max(np.where(has, probe.strip[0] - boxes[:, mine, 0], 0), initial=0)),
                int(np.max(np.where(has, boxes[:, mine, 1] - probe.strip[1], 0), initial=0)), 0)
    deal = _dist.StripDeal(rows, H, world, rank, halo=reach + slack, device=device, edges=probe.edges, solo=solo, align=align)
    w0, w1 = deal.window
    win = _field.ImageSet(ctx, bands, w1 - w0, W, nelec=np.ascontiguousarray(nelec[:, w0:w1]))
    win.set_window(w0, H)
    win.set_noise_rows(*deal.noise_rows())
    y0, y1 = deal.strip
    strip = None
    if not window_trace:
        strip = _field.ImageSet(ctx, bands, max(y1 - y0, 1), W, nelec=np.ascontiguousarray(nelec[:, y0:max(y1, y0 + 1)]))
        strip.set_window(y0, H)
    bands = np.asarray(bands)
    gf = GibbsField(win, list(range(B)) if band_index is None else band_index, bands[:, 2], bands[:, 1], H * W, trace_iset=strip)
    return deal, gf


class ModelGibbs(object):
    """CelesteBase.resample_model (CelestePy/models.py:75-83) for a whole catalogue at once:

        for every field:  Field.resample_photons (models.py:123-160) -- the photon split of all its
                          images in one device pass, sample patches kept on the device, and the
                          sky level of every image redrawn from its Gamma conditional;
        for every source: Source.resample (sources.py:242-245) = resample_fluxes (:321-349), then
                          resample_location (:308-319) by slice sampling -- all sources in
                          lock-step: round k scores the k-th slice evaluation of every unfinished
                          source in ONE launch of cel_patch_loglik_multi against the resident patches.

    State lives in arrays (type[S], u[S,2], fluxes[S,5] in nanomaggies, shape[S,4]); nothing per
    source runs in Python.  A source that has no sample patch in any image is left alone (the
    reference asserts there, sources.py:243).

    Random numbers: Philox on the device for the split (keyed by pixel and source), one SplitMix64
    stream per source for the slice sampler and per (source, band) for the flux Gamma draws, numpy's
    generator for the sky levels' -- all derived from `seed`; a chain is reproducible and does not
    depend on batching, nor on how it is dealt over ranks."""

    BANDS = ['u', 'g', 'r', 'i', 'z']

    def __init__(self, fields, typ, u, fluxes, shape, seed=0, flux_a_0=5., flux_b_0=.005, slice_args=None, engine="auto",
                 deal=None, shape_args=None, shape_logprior=None, phi_period=180., shape_mass="reference", conditional="reference",
                 mask="refuse", type_log_odds=0.0, grad_route="dense", hmc_conditional=None, mask_engine="host", type_proposal="prior"):
        self.fields = list(fields)
        # type_proposal: what resample_types(proposal=None) offers a star.  "prior" (default): a galaxy shape from the shape prior.
        # "moments": MomentProposal -- a shape from the second moments of the source's own photons in the current split
        # (ImageSet.photon_moments), with the proposal densities of both directions in h.  Either engine takes the same (shapes, h).
        if type_proposal not in ("prior", "moments"):
            raise ValueError("type_proposal must be 'prior' or 'moments'")
        self.type_proposal = type_proposal
        self.moment_proposal = MomentProposal() if type_proposal == "moments" else None
        # mask_engine: which slice engine a masked sweep (mask="honour") may take.  "host" (default): the host engine, as ever --
        # engine="device" raises.  "device": the device samplers of the exact conditional charge the OBSERVED mass per round
        # (CEL_OPT_SAMPLER_MASK around their calls; ImageSet.slice_sample / type_move / hmc_step(mask="honour")), so engine="auto"
        # and "device" run the location, shape and type steps -- and, under hmc_conditional="exact", the HMC step -- on the device:
        # the host engine's chains, bit for bit.  A strip deal and several fields keep the host engine.
        if mask_engine not in ("host", "device"):
            raise ValueError("mask_engine must be 'host' or 'device'")
        self.mask_engine = mask_engine
        # hmc_conditional: what location_loglik_grad and resample_hmc differentiate.  None: the reference's conditional, and under
        # conditional="exact" both raise, as they always have (that default exists only because the suite pins those refusals).
        # "exact" (needs conditional="exact"): the exact conditional's value and gradient -- the proposal's stamp mass on its own
        # box and that mass's derivative at the fixed integer box (k_mass_grad.h, CEL_OPT_GRAD_CONDITIONAL around the calls), -inf
        # where the box does not cover the source's photons -- so that resample_hmc and sweep(hmc=True) run under the exact sweep,
        # on the device engine where _exact_on_device() holds and on the host engine otherwise: the same chains bit for bit.
        if hmc_conditional not in (None, "exact"):
            raise ValueError("hmc_conditional must be None or 'exact'")
        if hmc_conditional == "exact" and conditional != "exact":
            raise ValueError("hmc_conditional='exact' needs conditional='exact'")
        self.hmc_conditional = hmc_conditional
        # grad_route: where the resident gradients of resample_hmc and location_loglik_grad are summed.  "dense": over the sample
        # patches (k_patch_grad.h).  "photons": at the split's photon lists (k_patch_grad_nz.h; CEL_OPT_PHOTON_LISTS + 4 around those
        # calls): the same terms in another order, so the values agree to rounding and the host and device engines, which take the
        # same gradients, stay bit for bit.
        if grad_route not in ("dense", "photons"):
            raise ValueError("grad_route must be 'dense' or 'photons'")
        self.grad_route = grad_route
        # the type step's log prior odds, galaxy : star (resample_types; sweep(types=True))
        self.type_log_odds = float(type_log_odds)
        self.type_engine = None                 # "host" / "device": the type step's engine where it is not `engine`'s (tools/type_move_cost.py)
        # mask="refuse": masked data is refused up front.  mask="honour": the sweep on masked images (NaN counts) -- no photons at
        # a masked pixel (CEL_OPT_HONOUR_MASK around the split), the flux step's masses over the unmasked pixels, a sky step that
        # counts unmasked pixels.  Under conditional="exact" only: the reference's location conditional charges a source
        # counts * sum(psf weights) wherever it sits, but on masked data the exact term is counts * (the unit stamp summed over
        # the OBSERVED pixels of the proposal's box), which moves with the proposal -- a star one PSF sigma from a masked column
        # changes its observed mass by ~0.01 per 0.1 px, ~30 nats across one posterior width at 3 000 photons.  The exact
        # conditional charges counts * stamp_mass(proposal), and stamp_mass returns the observed mass on such a set.
        if mask not in ("refuse", "honour"):
            raise ValueError("mask must be 'refuse' or 'honour'")
        self.mask = mask
        if mask == "honour":
            if conditional != "exact":
                raise ValueError("mask='honour' needs conditional='exact': the reference's location conditional charges "
                                 "counts * sum(psf weights) wherever the source sits, but beside a mask the term is counts * (the "
                                 "stamp's mass over the OBSERVED pixels of the proposal's box), which moves with the proposal")
            if engine == "device" and mask_engine != "device":
                raise ValueError("mask='honour' runs on the host slice engine: the device slice sampler does not charge the "
                                 "observed mass per round (cel_slice_* refuse a masked set)")
            for f in self.fields:
                if int(f.iset.masked.sum()) and getattr(f, "npix_observed", None) is None:
                    raise ValueError("mask='honour': a field with masked pixels needs GibbsField(npix_observed=) "
                                     "(ImageSet.npix_observed() for a whole frame)")
        else:
            for f in self.fields:   # refused up front, before any device call
                f.iset._refuse_masked("ModelGibbs")
        self.typ = np.ascontiguousarray(typ, dtype=np.int32)
        self.S = self.typ.shape[0]
        self.u = np.array(u, dtype=np.float64).reshape(self.S, 2)
        self.fluxes = np.array(fluxes, dtype=np.float64).reshape(self.S, 5)
        self.shape = np.array(shape, dtype=np.float64).reshape(self.S, 4)
        self.seed = int(seed)
        self.rng = np.random.RandomState(self.seed & 0x7FFFFFFF)
        self.flux_a_0, self.flux_b_0 = flux_a_0, flux_b_0
        # Source.resample_location's call (sources.py:312-317): no stepping out, step = du / 5 = 0.001
        # degrees.  The reference's slicesample does not read `step=`, so what it effectively runs is an
        # interval of sigma = 1.0 degree, with which a faint source can leave the frame for good (DESIGN Q13,
        # Q15).  The default here is the call's INTENT (sigma = 0.001 deg); slice_args="literal" asks for the
        # call as the reference executes it.
        self.slice_args = self.slice_preset(slice_args)
        # the galaxies' shape step (celeste_mcmc.py:224-243, slice_sample_skew): slicesample over (theta, sigma, phi,
        # rho) along random directions with stepping out by doubling; sigma stays slicesample's default 1.0 there.
        # The log-prior added to the conditional likelihood is the caller's (priors are outside this path); the
        # default is the reference's galaxy_shape_prior_constrained with phi in the renderer's unit (degrees, Q7),
        # and phi is wrapped into [0, phi_period) after the move as :241 wraps it into [0, pi).
        self.shape_args = dict(step_out=True, doubling_step=True, compwise=False, numdir=4)
        self.shape_args.update(shape_args or {})
        self.phi_period = float(phi_period)
        # The conditional likelihood the shape step scores (Source.log_likelihood(shape=), sources.py:134-183) charges a source
        # its FULL expected photons, band_flux * sum(psf weights), whatever the shape ("model_outside ... should be small",
        # :166-170) -- but the photons it is given were split on the source's box, and how much of a proposal's stamp lies on
        # its box depends on the shape: for an extended de Vaucouleurs-dominated galaxy at high signal to noise the constant
        # term leaves sigma 10-20 % low (tests/test_calibration.py: the calibration test that found it; DESIGN Q20).
        # shape_mass="reference" keeps the reference's term; "exact" charges counts * (the proposal's unit stamp summed over its
        # own box, cel_stamp_mass) in the shape step (host engine).  That is one of three corrections: conditional="exact"
        # below makes all of them.
        if shape_mass not in ("reference", "exact"):
            raise ValueError("shape_mass must be 'reference' or 'exact'")
        self.shape_mass = shape_mass
        # conditional="exact": every block of the sweep samples the Gibbs conditional of the model the RENDERER draws from -- a
        # source's photons lie on its own box and nowhere else (celeste.py:217-219).  Three departures from the reference:
        # the photons are split on whole boxes (CEL_OPT_SPLIT_FULL_BOX; celeste_sample_sources.pyx:50-51 leaves a box's first
        # row and column out); the location AND the shape step charge counts * (the proposal's stamp mass on ITS box); and a
        # proposal whose box does not cover every photon of the source has probability zero (the reference scores the fixed
        # data patch whatever the proposal's box, sources.py:134-183).  Calibrated at 192 replicates and pi P = pi on a sigma
        # grid (tests/test_calibration.py, DESIGN Q20).  Either slice engine (the device's: cel_slice_sample under
        # CEL_OPT_SLICE_CONDITIONAL, one field of whole unmasked frames); a change of the integer box needs the ring between the two
        # boxes free of the source's photons, so big galaxies mix more slowly across box sizes than under the reference's rules.
        if conditional not in ("reference", "exact"):
            raise ValueError("conditional must be 'reference' or 'exact'")
        self.conditional = conditional
        if conditional == "exact":
            self.shape_mass = "exact"
        self._default_shape_prior = shape_logprior is None
        if shape_logprior is None:
            from .celeste_galaxy_conditionals import galaxy_shape_prior_constrained
            shape_logprior = lambda TH: galaxy_shape_prior_constrained(TH[:, 0], TH[:, 1], TH[:, 2], TH[:, 3], self.phi_period)   # noqa: E731
        self.shape_logprior = shape_logprior
        # where the slice sampler's state machine runs: "device" (cel_slice_locations: nothing but a
        # counter crosses PCIe per round; one field, the reference call's options), "host" (the numpy
        # engine of util/infer/slicesample.py: every option, any number of fields), "auto" = device
        # when it applies.  Both draw the same per-chain streams: a chain takes the same trajectory.
        if engine not in ("auto", "device", "host"):
            raise ValueError("engine must be auto, device or host")
        self.engine = engine
        self.sweeps = 0
        self.timing = dict(split=0.0, flux=0.0, location=0.0, rounds=0, evals=0, shape=0.0, shape_rounds=0, shape_evals=0,
                           type=0.0, type_evals=0, type_accepted=0, hmc=0.0, hmc_evals=0, hmc_accepted=0)
        self._hmc_p = None                      # the HMC step's momentum, kept from call to call (resample_hmc)
        # ONE chain over several GPUs: `deal` (dist.SourceDeal) names the sources this rank
        # updates.  Every rank runs the same photon split (counter-based draws: the replicas are bitwise equal) and
        # the same host draws (same seed), updates the fluxes and locations of ITS sources only, and the ranks
        # exchange the new rows with one all-gather per sweep.  The chain is the single-rank chain, bit for bit.
        self.deal = deal
        if deal is not None and deal.S != self.S:
            raise ValueError("the deal is over %d sources, the catalogue has %d" % (deal.S, self.S))
        if deal is not None and getattr(deal, "kind", "") == "strips" and self.conditional == "exact":
            raise ValueError("conditional='exact' runs on whole frames (a replicated deal or one rank): its box tests are not window-relative")
        self.noise_sums = None
        self.active = np.ones(self.S, dtype=bool)
        # the flux conditionals' Gamma variates: on the device (cel_gamma_streams) or, host_gamma=True, by the numpy form of
        # the same sampler (gamma_by_stream: the same streams and decisions, values equal to rounding)
        import os
        self.host_gamma = os.environ.get("CEL_HOST_GAMMA") == "1"
        # the flux step as ONE device call (cel_flux_conditionals) where it applies; CEL_HOST_FLUX=1 / device_flux = False: the
        # host form (sums and masses read back, variates drawn on the device, fluxes formed in numpy): the same bits
        self.device_flux = os.environ.get("CEL_HOST_FLUX") != "1"

    # -- helpers ---------------------------------------------------------------------------------
    SLICE_INTENDED = dict(step_out=False, sigma=1e-3)
    SLICE_LITERAL = dict(step_out=False)                       # sigma stays slicesample's default, 1.0 degree

    @classmethod
    def slice_preset(cls, slice_args):
        """None -> the intended call; "literal" -> the reference's effective call; a dict is laid over the
        intended call's step_out=False (its sigma is then the caller's, or slicesample's default 1.0)"""
        if slice_args is None or slice_args == "intended":
            return dict(cls.SLICE_INTENDED)
        if isinstance(slice_args, str):
            if slice_args != "literal":
                raise ValueError("slice_args preset must be 'intended' or 'literal'")
            return dict(cls.SLICE_LITERAL)
        out = dict(step_out=False)
        out.update(slice_args)
        return out

    @classmethod
    def from_images(cls, img_dicts, params, **kw):
        """fields given as the reference holds them: a list of {band letter: FitsImage} dicts
        (CelesteBase.add_field) and a list of SrcParams."""
        fields = []
        for img_dict in img_dicts:
            bands = [b for b in cls.BANDS if b in img_dict]
            imgs = [img_dict[b] for b in bands]
            honour = kw.get("mask", "refuse") == "honour"
            if kw.get("mask", "refuse") not in ("refuse", "honour"):
                raise ValueError("mask must be 'refuse' or 'honour'")
            if honour and kw.get("conditional", "reference") != "exact":
                raise ValueError("mask='honour' needs conditional='exact' (the reference's location conditional does not charge "
                                 "the observed mass of the proposal's box)")
            if kw.get("mask_engine", "host") not in ("host", "device"):
                raise ValueError("mask_engine must be 'host' or 'device'")
            if honour and kw.get("engine", "auto") == "device" and kw.get("mask_engine", "host") != "device":
                raise ValueError("mask='honour' runs on the host slice engine")
            if not honour and any(getattr(im, "n_masked", 0) for im in imgs):
                from ._lib import MaskedImagesError
                raise MaskedImagesError("ModelGibbs: the images hold masked pixels (FitsImage(mask_invvar=True)) and the Gibbs "
                                        "sweep does not honour a mask")
            iset = _celeste._image_set(tuple(imgs))
            f = GibbsField(iset, [cls.BANDS.index(b) for b in bands], [im.calib for im in imgs],
                           [im.kappa for im in imgs], imgs[0].nelec.size,
                           npix_observed=[im.nelec.size - getattr(im, "n_masked", 0) for im in imgs] if honour else None)
            f.images = imgs
            fields.append(f)
        S = len(params)
        typ = np.array([1 if p.a == 1 else 0 for p in params], dtype=np.int32)
        u = np.array([p.u for p in params], dtype=np.float64).reshape(S, 2)
        fl = np.array([[p.flux_dict[b] for b in cls.BANDS] for p in params], dtype=np.float64).reshape(S, 5)
        sh = np.array([[p.theta, p.sigma, p.phi, p.rho] if p.a == 1 else [0., 0., 0., 0.] for p in params],
                      dtype=np.float64).reshape(S, 4)
        return cls(fields, typ, u, fl, sh, **kw)

    def step_seed(self, step, k=0):
        return step_seed(self.seed, step, self.sweeps, k)

    def _honour_mask(self):
        """mask="honour": CEL_OPT_HONOUR_MASK set on every field's context around the device calls that honour a mask (photon split,
        stamp masses), and restored behind them -- as CEL_OPT_SPLIT_FULL_BOX is set around the exact split.  Otherwise nothing."""
        import contextlib
        from . import _lib

        @contextlib.contextmanager
        def cm():
            was = []
            try:
                if self.mask == "honour":
                    for ctx in {id(f.iset.ctx): f.iset.ctx for f in self.fields}.values():
                        was.append((ctx, ctx.get_option(_lib.CEL_OPT_HONOUR_MASK)))
                        ctx.set_option(_lib.CEL_OPT_HONOUR_MASK, 1)
                yield
            finally:
                for ctx, v in was:
                    ctx.set_option(_lib.CEL_OPT_HONOUR_MASK, v)
        return cm()

    def _grad_route(self):
        """grad_route="photons": the gradient bit of CEL_OPT_PHOTON_LISTS (4 on top of the caller's 0 or 1) set on every field's
        context around a resident gradient call, and what the caller had restored behind it -- as _honour_mask does it.  A
        context under 2 (no lists are built) is left alone: its gradients are dense.  Otherwise nothing."""
        import contextlib
        from . import _lib

        @contextlib.contextmanager
        def cm():
            was = []
            try:
                if self.grad_route == "photons":
                    for ctx in {id(f.iset.ctx): f.iset.ctx for f in self.fields}.values():
                        v = ctx.get_option(_lib.CEL_OPT_PHOTON_LISTS)
                        if v in (0, 1):
                            was.append((ctx, v))
                            ctx.set_option(_lib.CEL_OPT_PHOTON_LISTS, v + 4)
                yield
            finally:
                for ctx, v in was:
                    ctx.set_option(_lib.CEL_OPT_PHOTON_LISTS, v)
        return cm()

    def counts(self, f, fluxes=None, idx=None):
        """flux in nanomaggies -> expected photons in every image of field f  (sources.py:120-129)"""
        fl = self.fluxes if fluxes is None else fluxes
        if idx is not None:
            fl = fl[idx]
        return fl[:, f.band_index] / f.calib[None, :] * f.kappa[None, :]

    def _sources(self, f):
        """the catalogue at the chain's current state on the device.  It is uploaded only when it differs from what the
        device holds (three calls per sweep ask for it, one has anything new): besides the copies saved, an unchanged
        SourceSet keeps its identity, which is what lets the next photon split take its totals image from the trace
        render's model image instead of rendering it again (CEL_OPT_SPLIT_REUSE)."""
        from . import field as _field
        if f.sset is None or f.sset.capacity < self.S:
            f.sset = _field.SourceSet(f.iset.ctx, max(self.S, 1), f.iset.B)
            f._uploaded = None
        cur = (self.typ, self.u, self.counts(f), self.shape)
        last = getattr(f, "_uploaded", None)
        if last is not None and f.sset.S == self.S and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(cur, last)):
            return f.sset
        f.sset.set(*cur)
        f._uploaded = tuple(np.array(a, copy=True) for a in cur)
        return f.sset

    # -- Field.resample_photons: models.py:123-160 ---------------------------------------------------
    def resample_photons(self):
        import time
        t0 = time.perf_counter()
        self._split_photons()
        self._resample_sky()
        self.timing["split"] += time.perf_counter() - t0
        return self.noise_sums

    def _split_photons(self):
        with self._honour_mask():       # (a masked set: no photons, no sky and no draws at a masked pixel)
            self._split_photons_now()

    def _split_photons_now(self):
        """the photon split of every field at the chain's current state (celeste_sample_sources.pyx:61-156): sample patches on the
        device, photons per (source, image), the sky photons per image"""
        self.noise_sums = []
        any_patch = np.zeros(self.S, dtype=bool)
        from . import _lib
        for k, f in enumerate(self.fields):
            seed = self.step_seed("split", k)
            if self.conditional == "exact":
                # the split of the model the renderer draws from: a source takes part on its whole box (the reference's rule
                # leaves every box's first row and column out, celeste_sample_sources.pyx:50-51)
                ctx = f.iset.ctx
                was = ctx.get_option(_lib.CEL_OPT_SPLIT_FULL_BOX)
                ctx.set_option(_lib.CEL_OPT_SPLIT_FULL_BOX, 1)
                try:
                    noise = f.iset.photon_split_resident(self._sources(f), seed)
                finally:
                    ctx.set_option(_lib.CEL_OPT_SPLIT_FULL_BOX, was)
            else:
                noise = f.iset.photon_split_resident(self._sources(f), seed)
            if self.deal is not None and self.deal.kind == "strips":
                # this rank split its window and counted its strip's sky photons: the frame's sum over the ranks; and its own
                # sources' boxes have to lie inside the window (their patches must be complete)
                # (one collective for both; every rank raises if any rank's window cuts a box)
                bx, stt = f.iset.source_boxes(f.sset)
                noise = self.deal.check_boxes(bx, stt, extra=noise)
            f.sums = None                                              # photons per (source, image): read back on first use
            f.has_patch = f.iset.sample_box_areas() > 0
            any_patch |= f.has_patch.any(axis=1)
            if self.conditional == "exact":
                f.photon_rects = f.iset.photon_rects()                 # where each source's photons lie: what its box must cover
            self.noise_sums.append(noise)
        self.active = any_patch

    def _resample_sky(self):
        """the noise parameter of every image from its Gamma conditional given the sky photons of the current split
        (models.py:155-160)"""
        for f, noise in zip(self.fields, self.noise_sums):
            a_n = f.a_0 + noise
            b_n = f.b_0 + (f.npix if getattr(f, "npix_observed", None) is None else f.npix_observed)
            f.epsilon = self.rng.gamma(a_n, 1. / b_n)
            for b in range(f.iset.B):
                f.iset.set_epsilon(b, f.epsilon[b])
                if f.trace_iset is not None:
                    f.trace_iset.set_epsilon(b, f.epsilon[b])
                if getattr(f, "images", None) is not None:
                    f.images[b].epsilon = float(f.epsilon[b])

    # -- Source.resample_fluxes: sources.py:321-349 --------------------------------------------------
    def _device_flux_applies(self):
        """the whole flux step on the device (cel_flux_conditionals): one field whose resident split belongs to the catalogue on
        the device, every source this process's own, the default conditional and the device's Gamma streams, scalar priors"""
        f = self.fields[0]
        return (self.device_flux and len(self.fields) == 1 and (self.deal is None or self.deal.world == 1) and not self.host_gamma and
                self.conditional != "exact" and np.isscalar(self.flux_a_0) and np.isscalar(self.flux_b_0) and
                getattr(f, "sset", None) is not None and getattr(f, "_uploaded", None) is not None and f.sset.S == self.S and
                hasattr(f.iset, "flux_conditionals"))

    def resample_fluxes(self):
        import time
        t0 = time.perf_counter()
        if self._device_flux_applies():
            # Round 6: sums, masses, Gamma variates and the new counts never leave the device (the host form below read the
            # photon sums and the masses back, sent the Gamma shapes up, read the variates back and uploaded the whole catalogue
            # again before the location step: 0.45 ms of copies per sweep).  The values are the host form's bit for bit
            # (tests/test_gibbs.py::test_device_flux_step_is_the_host_flux_step).
            f = self.fields[0]
            new, act = f.iset.flux_conditionals(f.sset, self.step_seed("flux"), self.flux_a_0, self.flux_b_0, f.band_index, f.calib, f.kappa)
            if not np.array_equal(act, self.active):
                raise RuntimeError("cel_flux_conditionals: the device's patches are not those of the split this chain made")
            self.fluxes = np.where(self.active[:, None], new, self.fluxes)
            # the device's catalogue holds the new counts of the ACTIVE sources already: what _sources compares with is brought up
            # to date for those rows, not uploaded.  The kernel left the other rows alone, so their record stays what the device
            # holds: had their fluxes been changed on the host since the last upload, the next _sources sees it and uploads.
            cnt = f._uploaded[2].copy()
            cnt[self.active] = self.counts(f)[self.active]
            f._uploaded = (f._uploaded[0], f._uploaded[1], cnt, f._uploaded[3])
            self.timing["flux"] += time.perf_counter() - t0
            return self.fluxes
        band_counts = np.zeros((self.S, 5))
        for f in self.fields:
            for b in range(f.iset.B):
                band_counts[:, f.band_index[b]] += f.sums[:, b]
        a_n = self.flux_a_0 + band_counts

        mine = None if self.deal is None or self.deal.world == 1 else self.deal.mine

        # The device's part -- the sum of every source's unit stamp on its own box -- runs beside the host's draws: the last
        # field's kernel is queued (stamp_mass_begin), the Gamma variates are drawn, then its values are collected.  (Fields
        # before the last are summed synchronously: two pending calls may not share a context.  Round 2 used a worker thread
        # for the overlap: its hand-over through the interpreter lock made the step vary between 2 and 4 ms.)
        whole = {}                                  # fields whose masses come for the whole catalogue although this rank owns a part

        def field_sources(f):
            if mine is None:
                return f.sset
            if f.iset.stamp_mass_ready(f.sset):     # the replicated split has summed every source's stamps already: free, and
                whole[id(f)] = True                 # every rank holds the numbers the single-rank chain holds
                return f.sset
            from . import field as _field          # this rank's sources only; a (source, band) value does not depend on the batch
            if getattr(f, "sub", None) is None or f.sub.capacity < mine.size:
                f.sub = _field.SourceSet(f.iset.ctx, max(mine.size, 1), f.iset.B)
            f.sub.set(self.typ[mine], self.u[mine], self.counts(f, idx=mine), self.shape[mine])
            return f.sub

        def add_mass(psf_sums, f, m):
            if mine is None:
                mass = m * f.has_patch
            elif whole.get(id(f)):
                mass = np.zeros((self.S, f.iset.B))
                mass[mine] = m[mine] * f.has_patch[mine]
            else:
                mass = np.zeros((self.S, f.iset.B))
                mass[mine] = m * f.has_patch[mine]
            for b in range(f.iset.B):
                psf_sums[:, f.band_index[b]] += mass[:, b] * (f.kappa[b] / f.calib[b])

        psf_sums = np.zeros((self.S, 5))
        with self._honour_mask():       # (a masked set: the masses over the unmasked pixels, and no short cut from the split)
            for f in self.fields[:-1]:
                add_mass(psf_sums, f, f.iset.stamp_mass(field_sources(f)))
            last = self.fields[-1]
            last.iset.stamp_mass_begin(field_sources(last))
        try:
            # Gamma(a_n, 1 / b_n) = standard Gamma(a_n) * (1 / b_n); every (source, band) draws from its own stream -- on the
            # device, queued behind the mass kernel (cel_gamma_streams: gamma_by_stream's sampler, streams and decisions, ~10 us;
            # the numpy draws beside the kernel took 1.7 ms on an idle host and 3.5 ms on a busy one: the step's time moved
            # with the host)
            if self.host_gamma:
                g = gamma_by_stream(a_n.ravel(), self.step_seed("flux"), np.arange(self.S * 5)).reshape(self.S, 5)
            else:
                g = last.iset.ctx.gamma_streams(a_n.ravel(), self.step_seed("flux")).reshape(self.S, 5)
        finally:
            with self._honour_mask():
                m_last = last.iset.stamp_mass_end()     # whatever the draw does, the pending call is collected
        add_mass(psf_sums, last, m_last)
        new = g * (1. / (self.flux_b_0 + psf_sums))
        self.fluxes = np.where(self.active[:, None], new, self.fluxes)       # rows of other ranks' sources: merged at the sweep's end
        self.timing["flux"] += time.perf_counter() - t0
        return self.fluxes

    # -- Source.resample_location: sources.py:308-319, all sources in lock-step ------------------------
    def location_loglik(self, idx, U, typ=None, shape=None):
        """Source.location_likelihood (sources.py:185-186) of chain idx[i] at U[i], summed over fields.  typ / shape: the
        proposals' own types and shapes where they are not the chains' (the type step's two slots per chain)"""
        from . import field as _field
        idx = np.asarray(idx, dtype=np.int64)
        P = idx.shape[0]
        ll = np.zeros(P)
        typ = self.typ[idx] if typ is None else np.ascontiguousarray(typ, dtype=np.int32)
        shape = self.shape[idx] if shape is None else np.asarray(shape, dtype=np.float64).reshape(P, 4)
        owner = idx.astype(np.int32)
        for f in self.fields:
            if f.prop is None or f.prop.capacity < P:
                f.prop = _field.SourceSet(f.iset.ctx, max(2 * self.S, P, 16), f.iset.B)
            cts = getattr(f, "_counts", None)            # (S, B), fixed while the locations are sampled
            pc = self.counts(f, idx=idx) if cts is None else cts[idx]
            f.prop.set(typ, U, pc, shape)
            ll += f.iset.patch_loglik_resident(f.prop, owner)
            if self.conditional == "exact":
                ll += self._exact_terms(f, idx, pc)
        return ll

    def location_loglik_grad(self, idx, U, typ=None, shape=None, shape_grad=False):
        """location_loglik with its analytic gradient in (ra, dec), per degree, summed over fields (the gradient form of
        cel_patch_loglik_multi against the resident patches) -> (ll[P], g[P, 2]); ll is location_loglik's value, bit for bit.
        shape_grad=True: the six coordinates (ra, dec, theta, sigma, phi, rho) -> (ll[P], g[P, 6]) (a star's last four: 0).
        The exact conditional's mass term has no derivative here: conditional="exact" raises -- unless hmc_conditional="exact":
        then ll is the exact location_loglik's value, bit for bit, and g the exact conditional's gradient at the proposals' fixed
        integer boxes (ll = -inf and g = 0 where a proposal's box does not cover its source's photons).
        grad_route="photons": the gradients are summed at the split's photon lists (ll is unchanged)."""
        from . import field as _field
        exact = self.hmc_conditional == "exact"
        if self.conditional == "exact" and not exact:
            raise ValueError("location_loglik_grad: the exact conditional's stamp-mass term has no analytic derivative yet "
                             "(conditional='reference' only)")
        idx = np.asarray(idx, dtype=np.int64)
        P = idx.shape[0]
        ll, g = np.zeros(P), np.zeros((P, 6 if shape_grad else 2))
        typ = self.typ[idx] if typ is None else np.ascontiguousarray(typ, dtype=np.int32)
        shape = self.shape[idx] if shape is None else np.asarray(shape, dtype=np.float64).reshape(P, 4)
        owner = idx.astype(np.int32)
        for f in self.fields:
            if f.prop is None or f.prop.capacity < P:
                f.prop = _field.SourceSet(f.iset.ctx, max(2 * self.S, P, 16), f.iset.B)
            cts = getattr(f, "_counts", None)
            pc = self.counts(f, idx=idx) if cts is None else cts[idx]
            f.prop.set(typ, U, pc, shape)
            with self._grad_route():
                l, gr, _, gs = f.iset.patch_loglik_resident_grad(f.prop, owner, conditional="exact" if exact else "reference",
                                                                 mask=self.mask if exact else "refuse")
            ll += l
            g += np.concatenate([gr, gs], axis=1) if shape_grad else gr
        return ll, g

    def _exact_terms(self, f, sel, pc):
        """what turns Source.log_likelihood's value for the proposals in f.prop (chains `sel`, expected photons `pc`) into the
        exact conditional: -counts * (the proposal's stamp mass on its own box) in place of -counts * sum(psf weights) where
        the source has a patch, and -inf where a photon of the source lies outside the proposal's box"""
        wsum = getattr(f, "_wsum", None)
        if wsum is None:                                               # (the PSF weights of an image set do not change)
            wsum = f._wsum = np.array([f.iset.band(b)[3:6].sum() for b in range(f.iset.B)])
        with self._honour_mask():       # (a masked set: the proposal's mass over the OBSERVED pixels of its box)
            mass = f.iset.stamp_mass(f.prop)
        out = -(pc * (mass - wsum[None, :]) * f.has_patch[sel]).sum(axis=1)
        rects = getattr(f, "photon_rects", None)
        if rects is not None:
            bx, st = f.iset.source_boxes(f.prop)                       # (B, P, 4) = y0, y1, x0, x1
            bx, st, r = bx.transpose(1, 0, 2), st.T, rects[sel]
            held = r[..., 1] > r[..., 0]                               # the (source, band) pairs that hold a photon at all
            inside = (st > 0) & (bx[..., 0] <= r[..., 0]) & (bx[..., 1] >= r[..., 1]) & (bx[..., 2] <= r[..., 2]) & (bx[..., 3] >= r[..., 3])
            out = np.where((held & ~inside).any(axis=1), -np.inf, out)
        return out

    # -- the galaxies' shapes: celeste_mcmc.py:209-243 (skew_likelihood, slice_sample_skew) ---------------------------
    def shape_logprob(self, idx, TH):
        """skew_likelihood (celeste_mcmc.py:209-222) of chain idx[i] at shape TH[i] = (theta, sigma, phi, rho): the
        log-prior, and where that is finite the source's conditional likelihood given its photons
        (Source.log_likelihood(shape=...), sources.py:134-183) -- one launch for all of them"""
        from . import field as _field
        idx = np.asarray(idx, dtype=np.int64)
        TH = np.asarray(TH, dtype=np.float64).reshape(idx.shape[0], 4)
        out = np.asarray(self.shape_logprior(TH), dtype=np.float64).copy()
        ok = np.isfinite(out)                       # outside the prior's support nothing is rendered (:213-214)
        if not ok.any():
            return out
        sel = idx[ok]
        ll = np.zeros(sel.shape[0])
        owner = sel.astype(np.int32)
        for f in self.fields:
            if f.prop is None or f.prop.capacity < sel.shape[0]:
                f.prop = _field.SourceSet(f.iset.ctx, max(2 * self.S, sel.shape[0], 16), f.iset.B)
            cts = getattr(f, "_counts", None)
            pc = self.counts(f, idx=sel) if cts is None else cts[sel]
            f.prop.set(self.typ[sel], self.u[sel], pc, TH[ok])
            ll += f.iset.patch_loglik_resident(f.prop, owner)
            if self.shape_mass == "exact":
                ll += self._exact_terms(f, sel, pc)
        out[ok] += ll
        return out

    def resample_shapes(self):
        """slice_sample_skew (celeste_mcmc.py:224-243) for every galaxy at once: one slicesample update of
        (theta, sigma, phi, rho) per galaxy -- random directions, stepping out by doubling -- all galaxies in
        lock-step against the resident photon patches; phi is wrapped afterwards (:241).  Stars are skipped
        (Source.resample_shape, sources.py:321-325)."""
        import time
        from .util.infer.slicesample import ChainStreams, slicesample_lockstep
        t0 = time.perf_counter()
        mine = self.active if self.deal is None else (self.active & self.deal.mask)
        gal = np.nonzero(mine & (self.typ == 1))[0]
        seed = self.step_seed("shape")
        if self._shape_engine_on_device():
            # the state machine on the device (cel_slice_sample): the directions are drawn here, from each chain's
            # normal stream, exactly as the host engine draws them; nothing but counters crosses PCIe per round
            f = self.fields[0]
            sset = self._sources(f)
            a = self.shape_args
            dirs = None if a.get("compwise", True) else ChainStreams(seed, np.arange(self.S)).directions(int(a.get("numdir", 2)), 4)
            ids = np.where(mine & (self.typ == 1), np.arange(self.S), -1).astype(np.int32)
            new, _, st = f.iset.slice_sample(sset, 1, a.get("sigma", 1.0), seed, dirs=dirs, step_out=a.get("step_out", True),
                                             max_steps_out=a.get("max_steps_out", 1000), phi_max=self.phi_period, chain_ids=ids,
                                             conditional=self.conditional, mask=self._sampler_mask())
            new[:, 2] = np.where(ids >= 0, (new[:, 2] + self.phi_period) % self.phi_period, new[:, 2])
            self.shape = new
            f._uploaded = None                                 # (the device holds the unwrapped angles)
            self.timing["shape_rounds"] += st["rounds"]
            self.timing["shape_evals"] += st["evals"]
            self.timing["shape"] += time.perf_counter() - t0
            return self.shape
        for f in self.fields:
            f._counts = self.counts(f)
        if gal.size:
            st = {}
            new, _ = slicesample_lockstep(self.shape[gal], lambda i, TH: self.shape_logprob(gal[i], TH),
                                          seed=seed, chain_ids=gal, stats=st, **self.shape_args)
            new[:, 2] = (new[:, 2] + self.phi_period) % self.phi_period
            self.shape[gal] = new
            self.timing["shape_rounds"] += st["rounds"]
            self.timing["shape_evals"] += st["evals"]
        for f in self.fields:
            f._counts = None
        self.timing["shape"] += time.perf_counter() - t0
        return self.shape

    def _shape_engine_on_device(self):
        """the device runs the shape step when there is one field, the log-prior is the built-in one and the options are
        those of slice_sample_skew's family: no stepping out or doubling, component-wise or random directions -- under either
        conditional (the exact one: CEL_OPT_SLICE_CONDITIONAL; an unmasked set, no strip deal).  shape_mass="exact" under the
        reference's conditional is a diagnostic setting of the host engine."""
        a = self.shape_args
        ok = (len(self.fields) == 1 and self._default_shape_prior and (not a.get("step_out", True) or a.get("doubling_step", True))
              and set(a) <= {"step_out", "doubling_step", "compwise", "numdir", "sigma", "max_steps_out"}
              and a.get("accept", "reference") == "reference"
              and (self._exact_on_device() if self.conditional == "exact" else self.shape_mass == "reference"))
        if self.engine == "device" and not ok:
            raise ValueError("the device shape sampler runs one field, the built-in log-prior, stepping out by doubling or none")
        return ok and self.engine != "host"

    def _exact_on_device(self):
        """what the exact conditional needs of the chain to run on the device (cel_slice_sample under
        CEL_OPT_SLICE_CONDITIONAL): whole frames, unmasked -- or masked under mask_engine="device" (CEL_OPT_SAMPLER_MASK)"""
        return ((self.mask != "honour" or self.mask_engine == "device")
                and not (self.deal is not None and getattr(self.deal, "kind", "") == "strips"))

    def _sampler_mask(self):
        """the mask= of the device samplers' calls: "honour" on a masked sweep (they run under mask_engine="device" alone)"""
        return "honour" if self.mask == "honour" and self.conditional == "exact" else "refuse"

    def _device_engine_applies(self):
        a = self.slice_args
        if self.conditional == "exact":
            # the general sampler scores the exact conditional (cel_slice_locations does not): the options it runs
            return (len(self.fields) == 1 and self._exact_on_device()
                    and (not a.get("step_out", True) or a.get("doubling_step", True))
                    and set(a) <= {"step_out", "doubling_step", "compwise", "numdir", "sigma", "max_steps_out"})
        return (len(self.fields) == 1 and not a.get("step_out", True) and a.get("compwise", True)
                and set(a) <= {"step_out", "compwise", "sigma"})

    def _resample_locations_exact_on_device(self, t0):
        """the location step of the exact sweep on the device: cel_slice_sample(param 0) under CEL_OPT_SLICE_CONDITIONAL = 1.
        The directions are drawn here from each chain's normal stream, exactly as resample_shapes draws them."""
        import time
        from .util.infer.slicesample import ChainStreams
        f = self.fields[0]
        sset = self._sources(f)
        a = self.slice_args
        seed = self.step_seed("location")
        dirs = None if a.get("compwise", True) else ChainStreams(seed, np.arange(self.S)).directions(int(a.get("numdir", 2)), 2)
        mine = self.active if self.deal is None else (self.active & self.deal.mask)
        ids = np.where(mine, np.arange(self.S), -1).astype(np.int32)
        new_u, _, st = f.iset.slice_sample(sset, 0, a.get("sigma", 1.0), seed, dirs=dirs, step_out=a.get("step_out", True),
                                           max_steps_out=a.get("max_steps_out", 1000), chain_ids=ids, conditional="exact",
                                           mask=self._sampler_mask())
        self.u = new_u
        if getattr(f, "_uploaded", None) is not None:      # the device's catalogue moved with the chains: it IS the new state
            f._uploaded = (f._uploaded[0], new_u.copy(), f._uploaded[2], f._uploaded[3])
        self.timing["rounds"] += st["rounds"]
        self.timing["evals"] += st["evals"]
        self.timing["loc_launches"] = self.timing.get("loc_launches", 0) + st["launches"]
        self.timing["location"] += time.perf_counter() - t0
        return self.u

    def resample_locations(self):
        import time
        from .util.infer.slicesample import slicesample_lockstep
        t0 = time.perf_counter()
        use_device = self.engine == "device" or (self.engine == "auto" and self._device_engine_applies())
        if use_device:
            if not self._device_engine_applies():
                if self.conditional == "exact":
                    raise ValueError("the device slice sampler scores the exact conditional on one field of whole, unmasked frames, "
                                     "stepping out by doubling or not at all")
                raise ValueError("the device slice sampler runs one field with step_out=False, compwise=True")
            if self.conditional == "exact":
                return self._resample_locations_exact_on_device(t0)
            f = self.fields[0]
            sset = self._sources(f)                        # the catalogue with the fluxes just drawn (other ranks' rows are
            # stale until the merge: a chain reads only its own source's counts)
            ids = None if self.deal is None or self.deal.world == 1 else self.deal.chain_ids()
            new_u, _, st = f.iset.slice_locations(sset, self.slice_args.get("sigma", 1.0), self.step_seed("location"),
                                                  chain_ids=ids)
            self.u = new_u
            if getattr(f, "_uploaded", None) is not None:      # the device's catalogue moved with the chains: it IS the new state
                f._uploaded = (f._uploaded[0], new_u.copy(), f._uploaded[2], f._uploaded[3])
            self.timing["rounds"] += st["rounds"]
            self.timing["evals"] += st["evals"]
            self.timing["loc_bytes"] = self.timing.get("loc_bytes", 0) + st["algorithmic_bytes"]
            self.timing["loc_launches"] = self.timing.get("loc_launches", 0) + st["launches"]
            self.timing["location"] += time.perf_counter() - t0
            return self.u
        act = np.nonzero(self.active if self.deal is None else (self.active & self.deal.mask))[0]
        for f in self.fields:
            f._counts = self.counts(f)
        if act.size:
            st = {}
            new_u, _ = slicesample_lockstep(self.u[act], lambda i, U: self.location_loglik(act[i], U),
                                            seed=self.step_seed("location"), chain_ids=act, stats=st,
                                            **self.slice_args)
            self.u[act] = new_u
            self.timing["rounds"] += st["rounds"]
            self.timing["evals"] += st["evals"]
        for f in self.fields:
            f._counts = None
        self.timing["location"] += time.perf_counter() - t0
        return self.u

    # -- Source.resample_type: sources.py:247-306, all sources at once ---------------------------------------------
    def sample_shape_prior(self, seed, ids):
        """one draw per chain from the normalised form of galaxy_shape_prior_constrained, from ChainStreams(seed, ids): theta,
        rho ~ U(0, 1), phi ~ U(0, phi_period), sigma = 1 / sqrt(z^2 / 2 - log u) with z the stream's normal and u its uniform
        -- z^2 / 2 ~ Gamma(1/2, 1) and -log u ~ Gamma(1, 1), so 1 / sigma^2 ~ Gamma(3/2, 1), whose density in sigma is
        proportional to sigma^-4 exp(-1 / sigma^2): the prior's.  -> (len(ids), 4)"""
        from .util.infer.slicesample import ChainStreams
        cs = ChainStreams(seed, ids)
        every = np.arange(len(ids))
        theta, rho = cs.uniform(every), cs.uniform(every)
        phi = cs.uniform(every) * self.phi_period
        z, u = cs.normal(every), cs.uniform(every)
        sigma = 1.0 / np.sqrt(z * z / 2.0 - np.log(u))
        return np.stack([theta, sigma, phi, rho], axis=1)

    def _type_engine_on_device(self):
        """the device runs the type step (cel_slice_sample, param 2) where the exact slice engine applies: one field, and
        under conditional="exact" whole, unmasked frames"""
        ok = len(self.fields) == 1 and (self.conditional != "exact" or self._exact_on_device())     # (mask="honour" is exact)
        engine = self.type_engine or self.engine
        if engine == "device" and not ok:
            raise ValueError("the device type move runs one field of whole, unmasked frames")
        return ok and engine != "host"

    def resample_types(self, proposal=None):
        """Source.resample_type (sources.py:247-306) for every source at once: one Metropolis-Hastings star <-> galaxy proposal
        per source against the current photon split.  Given the split a source's conditional involves no other source, so the
        move of all sources at once is exact.  A star is offered a galaxy shape, a galaxy the star at its location with its
        expected counts;  log alpha = (score(proposal) - score(current)) + h,  the scores those of the location and shape
        steps' conditional, accepted iff log u < log alpha with u the first uniform of the chain's stream of
        step_seed("type").
        proposal: None -- a star's shape is drawn from the normalised shape prior (sample_shape_prior, the streams of
        step_seed("type", 1): not the accept test's), so proposal and prior cancel and h = +type_log_odds for star -> galaxy,
        -type_log_odds for the reverse (under ModelGibbs(type_proposal="moments"): MomentProposal, the shape the source's own photons
        imply, with both directions' proposal densities in h); or a callable(model) -> (shapes[S, 4], h[S]) with h everything of the log acceptance
        ratio that is not the likelihood (prior odds, proposal densities, Jacobian).  A custom shape prior needs one."""
        import time
        from .util.infer.slicesample import ChainStreams
        if proposal is None and not self._default_shape_prior:
            raise ValueError("resample_types: a custom shape prior (shape_logprior=) needs a custom proposal= "
                             "(a callable returning (shapes[S, 4], h[S])): the default proposal draws from the built-in prior")
        on_device = self._type_engine_on_device()
        t0 = time.perf_counter()
        ids_all = np.arange(self.S)
        if proposal is None and self.type_proposal == "moments":
            proposal = self.moment_proposal
        if proposal is None:
            shapes = self.sample_shape_prior(self.step_seed("type", 1), ids_all)
            h = np.where(self.typ == 0, self.type_log_odds, -self.type_log_odds).astype(np.float64)
        else:
            shapes, h = proposal(self)
            shapes = np.array(shapes, dtype=np.float64).reshape(self.S, 4)
            h = np.array(h, dtype=np.float64).reshape(self.S)
        seed = self.step_seed("type")
        mine = self.active if self.deal is None else (self.active & self.deal.mask)
        runs = mine & ((self.typ == 0) | (self.typ == 1))
        if not np.all(np.isfinite(h[runs])):
            raise ValueError("resample_types: h is not finite for a chain that moves")
        h = np.where(runs, h, 0.0)
        if on_device:
            f = self.fields[0]
            sset = self._sources(f)
            ids = np.where(runs, ids_all, -1).astype(np.int32)
            typ, shape, _, st = f.iset.type_move(sset, shapes, h, seed, chain_ids=ids, conditional=self.conditional,
                                                 mask=self._sampler_mask())
            self.typ, self.shape = typ, shape
            if getattr(f, "_uploaded", None) is not None:      # the device's catalogue moved with the chains: it IS the new state
                f._uploaded = (typ.copy(), f._uploaded[1], f._uploaded[2], shape.copy())
            evals, accepted = st["evals"], st["accepted"]
        else:
            act = np.nonzero(runs)[0]
            evals = accepted = 0
            if act.size:
                n = act.size
                to_gal = self.typ[act] == 0
                p_shape = np.where(to_gal[:, None], shapes[act], self.shape[act])
                inside = ~to_gal | ((p_shape[:, 0] > 0.) & (p_shape[:, 0] < 1.) & (p_shape[:, 1] > 0.) &
                                    (p_shape[:, 3] > 0.) & (p_shape[:, 3] < 1.))
                # two slots per chain: the current row, the flipped row; a shape outside the support is never rendered
                slot_idx = np.concatenate([act, act[inside]])
                slot_typ = np.concatenate([self.typ[act], 1 - self.typ[act][inside]])
                slot_shape = np.concatenate([self.shape[act], p_shape[inside]], axis=0)
                v = self.location_loglik(slot_idx, self.u[slot_idx], typ=slot_typ, shape=slot_shape)
                v0 = v[:n]
                v1 = np.full(n, -np.inf)
                v1[inside] = v[n:]
                if not np.all(v0 > -np.inf):
                    raise ValueError("resample_types: a state outside its own conditional (its current row scores -inf)")
                with np.errstate(invalid="ignore"):
                    la = (v1 - v0) + h[act]
                    log_u = np.log(ChainStreams(seed, act).uniform(np.arange(n)))
                    acc = log_u < la
                won = act[acc]
                self.typ = self.typ.copy()
                self.typ[won] = 1 - self.typ[won]
                self.shape[won] = p_shape[acc]
                evals, accepted = 2 * n, int(acc.sum())
        self.timing["type_evals"] += evals
        self.timing["type_accepted"] += accepted
        self.timing["type"] += time.perf_counter() - t0
        return self.typ

    # -- hmc_sample_galaxy_params: celeste_mcmc.py:281-331, all sources at once ------------------------------------
    #: the reference's call: step 1e-5, 50 leapfrog steps, mass (.1, .1, 1, .1 | .001, .001) for (theta, sigma, phi, rho | u),
    #: refresh_alpha .9 -- here in the order of q = (ra, dec, theta, sigma, phi, rho)
    HMC_REFERENCE = dict(eps=1e-5, steps=50, mass=(.001, .001, .1, .1, 1., .1), refresh=.9)

    @classmethod
    def hmc_preset(cls, name):
        """"reference" -> the keyword arguments of resample_hmc that make hmc_sample_galaxy_params' call
        (celeste_mcmc.py:287-314): dict(eps, steps, imass, refresh)"""
        if name != "reference":
            raise ValueError("hmc preset must be 'reference'")
        r = cls.HMC_REFERENCE
        return dict(eps=r["eps"], steps=r["steps"], imass=1.0 / np.array(r["mass"], dtype=np.float64), refresh=r["refresh"])

    def hmc_default_imass(self):
        """the library's scale-free inverse mass (S, 6): (one pixel in degrees)^2 / N for ra and dec and 1 / N for the shape,
        N = the chain's photons in the current split (at least 1) -- the order of a posterior variance when the PSF is about a
        pixel wide.  Nobody has tuned it."""
        N = np.zeros(self.S)
        for f in self.fields:
            N = N + np.asarray(f.sums, dtype=np.float64).sum(axis=1)
        N = np.maximum(N, 1.0)
        ups = np.asarray(self.fields[0].iset.band(0), dtype=np.float64)[28:32]
        pix2 = abs(ups[0] * ups[3] - ups[1] * ups[2])
        im = np.empty((self.S, 6))
        im[:, :2] = (pix2 / N)[:, None]
        im[:, 2:] = (1.0 / N)[:, None]
        return im

    def _hmc_engine_on_device(self):
        """the device runs the HMC step (cel_slice_sample, param 3) where it runs the type step under the reference's
        conditional: one field of unmasked frames"""
        ok = len(self.fields) == 1
        if self.hmc_conditional == "exact":             # (the exact step's cover test is not window-relative)
            ok = ok and self._exact_on_device()
        else:                                           # (the reference's conditional charges no observed mass)
            ok = ok and self.mask != "honour"
        if self.engine == "device" and not ok:
            raise ValueError("the device HMC step runs one field of whole, unmasked frames")
        return ok and self.engine != "host"

    def resample_hmc(self, eps=None, steps=None, imass=None, refresh=0.0):
        """hmc_sample_galaxy_params (celeste_mcmc.py:281-331) for every source at once: one HMC update of
        q = (ra, dec, theta, sigma, phi, rho) per galaxy and of (ra, dec) per star against the current photon split, the counts
        held fixed (the flux step samples their Gamma conditional exactly).  Given the split a source's conditional involves
        no other source, so the update of all sources at once is exact.  The target is the location and shape steps'
        conditional with the built-in shape prior; `steps` leapfrog steps of size eps (util/infer/hmc.py), accepted iff
        log u < log alpha with u the first uniform of the chain's stream of step_seed("hmc").
        The momentum is kept from call to call and refreshed as  refresh * p + sqrt(1 - refresh^2) * sqrt(mass) * z  with z
        the normals of the streams of step_seed("hmc", 1) (refresh=0: a fresh momentum every call); a coordinate with
        imass = 0 is frozen and its momentum is 0.  imass: (6,) or (S, 6), default hmc_default_imass(); eps default 0.5, steps
        default 8.  hmc_preset("reference") holds the reference's numbers.  phi is wrapped afterwards, as resample_shapes wraps it.
        The exact conditional's mass term has no derivative yet: conditional="exact" raises -- unless hmc_conditional="exact":
        then value and force are the exact conditional's; a trajectory that reaches a point whose box does not cover the source's
        photons is dead, and a chain whose current row fails that test is left alone (it cannot after a full-box split).
        grad_route="photons": both engines take their gradients at the split's photon lists."""
        import time
        from .util.infer.slicesample import ChainStreams
        from .util.infer.hmc import hmc_lockstep
        exact = self.hmc_conditional == "exact"
        if self.conditional == "exact" and not exact:
            raise ValueError("resample_hmc: the exact conditional's stamp-mass term has no analytic derivative yet "
                             "(conditional='reference' only)")
        if not self._default_shape_prior:
            raise ValueError("resample_hmc: a custom shape prior (shape_logprior=) has no derivative here")
        on_device = self._hmc_engine_on_device()
        t0 = time.perf_counter()
        S = self.S
        eps = 0.5 if eps is None else float(eps)
        steps = 8 if steps is None else int(steps)
        refresh = float(refresh)
        if not (eps > 0.0) or not (1 <= steps <= 1024) or not (0.0 <= refresh <= 1.0):
            raise ValueError("resample_hmc: eps > 0, 1 <= steps <= 1024 and 0 <= refresh <= 1")
        im = self.hmc_default_imass() if imass is None else np.array(np.broadcast_to(np.asarray(imass, dtype=np.float64), (S, 6)))
        if not np.all(np.isfinite(im) & (im >= 0.0)):
            raise ValueError("resample_hmc: imass must be finite and >= 0")
        mine = self.active if self.deal is None else (self.active & self.deal.mask)
        runs = mine & ((self.typ == 0) | (self.typ == 1))
        im[self.typ != 1, 2:] = 0.0                     # a star moves in (ra, dec) only
        im[~runs] = 0.0
        # the momentum: every chain's own normals, in coordinate order
        ids_all = np.arange(S)
        if self._hmc_p is None or self._hmc_p.shape != (S, 6):
            self._hmc_p = np.zeros((S, 6))
        cs = ChainStreams(self.step_seed("hmc", 1), ids_all)
        z = np.stack([cs.normal(ids_all) for _ in range(6)], axis=1)
        moves = im > 0.0
        sd = np.sqrt(1.0 / np.where(moves, im, 1.0))    # sqrt(mass)
        p = refresh * self._hmc_p + np.sqrt(1.0 - refresh * refresh) * sd * z
        p = np.where(moves, p, 0.0)
        p = np.where(runs[:, None], p, self._hmc_p)
        seed = self.step_seed("hmc")
        q0 = np.concatenate([self.u, self.shape], axis=1)
        if on_device:
            f = self.fields[0]
            sset = self._sources(f)
            ids = np.where(runs, ids_all, -1).astype(np.int32)
            with self._grad_route():
                q, pn, _, st = f.iset.hmc_step(sset, p, im, eps, steps, seed, phi_max=self.phi_period, chain_ids=ids,
                                               conditional="exact" if exact else "reference",
                                               mask=self._sampler_mask() if exact else "refuse")
            evals, accepted = st["evals"], st["accepted"]
        else:
            q, pn = q0.copy(), p.copy()
            act = np.nonzero(runs)[0]
            evals = accepted = 0
            if act.size:
                from .celeste_galaxy_conditionals import galaxy_shape_prior_constrained as prior
                period = self.phi_period
                for f in self.fields:
                    f._counts = self.counts(f)

                def value_fn(i, Q):
                    idx = act[i]
                    ll = self.location_loglik(idx, Q[:, :2], shape=Q[:, 2:])
                    gal = self.typ[idx] == 1
                    pri = np.zeros(idx.size)
                    pri[gal] = prior(Q[gal, 2], Q[gal, 3], Q[gal, 4], Q[gal, 5], period)
                    return ll + pri

                def grad_fn(i, Q):
                    idx = act[i]
                    l, g = self.location_loglik_grad(idx, Q[:, :2], shape=Q[:, 2:], shape_grad=True)
                    if exact:
                        g[l == -np.inf] = np.nan            # an uncovered point: the trajectory is dead, as the device engine has it
                    gal = self.typ[idx] == 1
                    g[~gal, 2:] = 0.0
                    s = Q[gal, 3]
                    g[gal, 3] = g[gal, 3] + (2.0 / ((s * s) * s) - 4.0 / s)
                    return g

                def support_fn(i, Q):
                    gal = self.typ[act[i]] == 1
                    inside = ((Q[:, 2] > 0.) & (Q[:, 2] < 1.) & (Q[:, 3] > 0.) & (Q[:, 5] > 0.) & (Q[:, 5] < 1.) &
                              (Q[:, 4] > 0.) & (Q[:, 4] < period))
                    return ~gal | inside

                st = {}
                try:
                    if exact:                               # a chain whose current row fails the cover test does not run
                        act = act[self.location_loglik(act, q0[act, :2], shape=q0[act, 2:]) > -np.inf]
                    log_u = np.log(ChainStreams(seed, act).uniform(np.arange(act.size)))
                    qa, pa, _, _ = hmc_lockstep(q0[act], p[act], im[act], eps, steps, value_fn, grad_fn, log_u, support_fn, stats=st)
                finally:
                    for f in self.fields:
                        f._counts = None
                q[act], pn[act] = qa, pa
                evals, accepted = st["evals"], st["accepted"]
        wrap = runs & (self.typ == 1)
        q[:, 4] = np.where(wrap, (q[:, 4] + self.phi_period) % self.phi_period, q[:, 4])
        self.u, self.shape = np.ascontiguousarray(q[:, :2]), np.ascontiguousarray(q[:, 2:])
        self._hmc_p = pn
        if on_device:
            self.fields[0]._uploaded = None            # (the device holds the unwrapped angles)
        self.timing["hmc_evals"] += evals
        self.timing["hmc_accepted"] += accepted
        self.timing["hmc"] += time.perf_counter() - t0
        return self.u, self.shape

    def _check_types(self, types):
        if types and not self._default_shape_prior:
            raise ValueError("sweep(types=True) draws a star's galaxy shape from the built-in shape prior: with a custom shape prior "
                             "(shape_logprior=) call resample_types(proposal=) with a custom proposal instead")
        if types and self.deal is not None and getattr(self.deal, "kind", "") == "strips":
            raise ValueError("sweep(types=True) runs on whole frames (a replicated deal or one rank): a source that changes its "
                             "type changes its box, and a strip's window was cut for the boxes it was dealt")

    def sweep(self, shapes=False, types=False, hmc=False):
        """CelesteBase.resample_model: every field's photons, then every source (fluxes, location) -- and, with
        shapes=True, the galaxies' shapes as sample_galaxy_params does (celeste_mcmc.py:166-243;
        Source.resample_shape is a stub in the reference, sources.py:321-325, so it is off by default); with types=True the
        star <-> galaxy move last (resample_types); with hmc=True one HMC update of every source's location and shape
        (resample_hmc with its defaults) right after the location step"""
        self._check_types(types)
        solo = self.deal is not None and getattr(self.deal, "solo", False) and self.deal.world > 1
        if solo:        # one rank of an N-rank chain played alone (bench.py --as-rank): the other ranks' rows keep their values
            before = (self.u.copy(), self.fluxes.copy(), self.shape.copy(), self.typ.copy())
        self.resample_photons()
        self.resample_fluxes()
        self.resample_locations()
        if hmc:
            self.resample_hmc()
        if shapes:
            self.resample_shapes()
        if types:
            self.resample_types()
        self.merge_ranks(types=types)
        if solo:
            other = ~self.deal.mask
            self.u[other], self.fluxes[other], self.shape[other] = before[0][other], before[1][other], before[2][other]
            if types:
                self.typ[other] = before[3][other]
        self.sweeps += 1

    def sweep_reversed(self, shapes=False, types=False, hmc=False):
        """The sweep's blocks in REVERSE order -- (shapes,) locations, fluxes, sky levels, photons -- on the augmented state (sources, sky
        levels, the current photon split): the time reversal of sweep() (types=True: the type move first; hmc=True: the HMC
        update between the shapes and the locations, reversible for a momentum refreshed in full, resample_hmc's default).  Every block is reversible with respect to its
        conditional (Gibbs draws; slice updates whose axis order is shuffled per call), so a chain run backwards from a state
        is a chain run with this.  It needs a photon split of the current state to start from (_split_photons()).  Used by the
        calibration test (tests/test_calibration.py) to put the true parameters at a random position of a stationary chain;
        a single rank."""
        if self.deal is not None and self.deal.world > 1:
            raise ValueError("sweep_reversed runs a single-rank chain")
        self._check_types(types)
        if not self.noise_sums:
            raise ValueError("sweep_reversed needs a photon split of the current state: call _split_photons() first")
        if types:
            self.resample_types()
        if shapes:
            self.resample_shapes()
        if hmc:
            self.resample_hmc()
        self.resample_locations()
        self.resample_fluxes()
        self._resample_sky()
        self._split_photons()
        self.sweeps += 1

    def merge_ranks(self, types=False):
        """one chain over several GPUs: every rank's new fluxes and locations to every rank (one all-gather); types=True: the
        types too, as one more column of it (an int32 is exact in a double)"""
        if self.deal is None or self.deal.world == 1:
            return
        import time
        t0 = time.perf_counter()
        cols = [self.u, self.fluxes, self.shape] + ([self.typ[:, None].astype(np.float64)] if types else [])
        both = self.deal.merge(np.concatenate(cols, axis=1))
        self.u, self.fluxes, self.shape = (np.ascontiguousarray(both[:, :2]), np.ascontiguousarray(both[:, 2:7]),
                                           np.ascontiguousarray(both[:, 7:11]))
        if types:
            self.typ = np.ascontiguousarray(both[:, 11]).astype(np.int32)
        self.timing["merge"] = self.timing.get("merge", 0.0) + time.perf_counter() - t0

    def log_likelihood(self):
        """sum of img_log_likelihood over every image of every field at the current state (models.py:104-108)"""
        tot = 0.0
        strips = self.deal is not None and self.deal.kind == "strips"
        for f in self.fields:
            if strips and f.trace_iset is None:
                # the window image set adds its own rows' terms only (strip_gibbs_field, window_trace): one render gives this
                # rank's share of the trace AND the model image the next split and flux step start from
                ll, _ = f.iset.render(self._sources(f), loglik=True)
            elif strips:        # this rank's strip of every image; the strips' sums added over the ranks
                from . import field as _field
                if getattr(f, "trace_sset", None) is None or f.trace_sset.capacity < self.S:
                    f.trace_sset = _field.SourceSet(f.trace_iset.ctx, max(self.S, 1), f.trace_iset.B)
                ll, _ = f.trace_iset.render(f.trace_sset.set(self.typ, self.u, self.counts(f), self.shape), loglik=True)
            else:
                ll, _ = f.iset.render(self._sources(f), loglik=True)
            tot += ll
        if strips:
            tot = float(self.deal.rank_sum([tot])[0])
        return tot
