"""One general WCS for the suite: rotated, flipped, sheared, anisotropic, different in every band, CRPIX off the frame, at a
declination where tan(dec) ~ 19 -- and ablated copies of the yardstick's WCS arithmetic (tests/test_general_wcs.py, part 5).

A helper module, not a conftest.  `general_bands(H, W, B)` is `synth.make_bands(H, W, B)` with only the WCS fields replaced;
tests/golden/make_golden.py writes the same numbers into the headers it hands the reference (general_wcs.npz).

For band b, with k = b % 3:
    CD_b    = 1.1e-4 (1 + DELTA[k]) R(THETA[k]) [[-1, 0.03], [0, 1.04]]
    CRVAL   = (188.34439, 87.0)                         the right ascension of wcs_points.npz's high-declination point, at a
                                                        declination where the "location through CD" term of d / d dec
                                                        is ~200 x the 1e-8 its gradient is checked at (63.4 degrees: 21 x)
    rho_b   = (-30, H + 20) + RHO_OFFSET[k]             CRPIX - 1: off the frame, bands a few pixels apart

The yardstick below restates in numpy the three places a WCS enters the model -- the position map (fits_image.py:166-174), the
local CD matrix (fits_image.py:196-216) and their derivatives with respect to (ra, dec) -- with switches that break each in the
way a device kernel could be broken:

    "ups_inv_T"     (i)   ups_inv transposed in the position map (hence in its Jacobian)
    "band0_wcs"     (ii)  band 0's WCS used for every band
    "no_cd_term"    (iii) d W / d (ra, dec), the "location through CD" term, dropped
    "cosd_cphi_1"   (iv)  cos(dec) / cos(phi_1) set to 1 in cd_at_pixel
    "cd_diagonal"   (v)   the off-diagonal entries of CD zeroed in cd_at_pixel only

No device code is mutated: the switches change what a test would EXPECT, and test_general_wcs.py requires that each moves an
expected value by at least 100 times the tolerance it is compared at.
"""
import numpy as np

THETA_DEG = (57.0, 57.35, 56.75)
DELTA = (0.0, 1e-3, -7e-4)
SCALE = 1.1e-4
SHEAR = np.array([[-1.0, 0.03], [0.0, 1.04]])
CRVAL = (188.34439, 87.0)
RHO_BASE = (-30.0, 20.0)                                  # (x, y - H)
RHO_OFFSET = ((0.0, 0.0), (1.7, -2.3), (-2.1, 0.9))
ABLATIONS = ("ups_inv_T", "band0_wcs", "no_cd_term", "cosd_cphi_1", "cd_diagonal")

FIX_H, FIX_W, FIX_B = 96, 112, 3                          # the frame of tests/golden/general_wcs.npz


def general_cd(b):
    k = b % 3
    t = np.deg2rad(THETA_DEG[k])
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return SCALE * (1.0 + DELTA[k]) * (R @ SHEAR)


def general_rho(H, W, b):
    k = b % 3
    return np.array([RHO_BASE[0] + RHO_OFFSET[k][0], H + RHO_BASE[1] + RHO_OFFSET[k][1]])


def general_header(H, W, b):
    """the FITS cards of band b's WCS (CRPIX is 1-based: rho + 1)"""
    cd, rho = general_cd(b), general_rho(H, W, b)
    return {"CD1_1": cd[0, 0], "CD1_2": cd[0, 1], "CD2_1": cd[1, 0], "CD2_2": cd[1, 1],
            "CRPIX1": rho[0] + 1.0, "CRPIX2": rho[1] + 1.0, "CRVAL1": CRVAL[0], "CRVAL2": CRVAL[1]}


def general_bands(H, W, B):
    """(B, 37) cel_band records: synth.make_bands(H, W, B) with rho, phi, ups, ups_inv replaced"""
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, B)
    for b in range(B):
        cd = general_cd(b)
        bands[b, 24:26] = general_rho(H, W, b)
        bands[b, 26:28] = CRVAL
        bands[b, 28:32] = cd.ravel()
        bands[b, 32:36] = np.linalg.inv(cd).ravel()
    return bands


# ---- the yardstick's WCS arithmetic, with switches ---------------------------------------------------------------------------
def _wcs(bands, b, ablate):
    """(rho, phi, ups, ups_inv) the yardstick uses for band b"""
    r = bands[0] if "band0_wcs" in ablate else bands[b]
    ups_inv = r[32:36].reshape(2, 2)
    return r[24:26], r[26:28], r[28:32].reshape(2, 2), (ups_inv.T if "ups_inv_T" in ablate else ups_inv)


def equa2pixel(bands, b, u, ablate=()):
    rho, phi, _, ups_inv = _wcs(bands, b, ablate)
    iwc = np.array([(u[0] - phi[0]) * np.cos(phi[1] / 180.0 * np.pi), u[1] - phi[1]])
    return ups_inv @ iwc + rho


def pixel2equa(bands, b, p, ablate=()):
    rho, phi, ups, _ = _wcs(bands, b, ablate)
    iwc = ups @ (np.asarray(p, dtype=np.float64) - rho)
    return np.array([iwc[0] / np.cos(phi[1] / 180.0 * np.pi) + phi[0], iwc[1] + phi[1]])


def cd_at_pixel(bands, b, x, y, ablate=()):
    """fits_image.py:196-216, step 10 px"""
    ra0, dec0 = pixel2equa(bands, b, [x, y], ablate)
    rax, decx = pixel2equa(bands, b, [x + 10.0, y], ablate)
    ray, decy = pixel2equa(bands, b, [x, y + 10.0], ablate)
    cosd = np.cos(dec0 * (np.pi / 180.0))
    if "cosd_cphi_1" in ablate:
        cosd = np.cos(_wcs(bands, b, ablate)[1][1] / 180.0 * np.pi)
    cd = np.array([[(rax - ra0) / 10.0 * cosd, (ray - ra0) / 10.0 * cosd], [(decx - dec0) / 10.0, (decy - dec0) / 10.0]])
    if "cd_diagonal" in ablate:
        cd[0, 1] = cd[1, 0] = 0.0
    return cd


def param_map(bands, b, typ, u, shape, orc, ablate=(), cd_at=None):
    """(px, py, W00, W01, W11) of a source in band b (test_loglik_grad.py's _param_map); cd_at: the (ra, dec) at which the CD
    matrix is taken, the source's own unless the "location through CD" term is being dropped"""
    p = equa2pixel(bands, b, u, ablate)
    if typ != 1:
        return np.array([p[0], p[1], 0.0, 0.0, 0.0])
    q = p if cd_at is None else equa2pixel(bands, b, cd_at, ablate)
    tinv = orc.galaxy_tinv(shape[1], shape[3], shape[2], cd_at_pixel(bands, b, q[0], q[1], ablate))
    Wm = tinv @ tinv.T
    return np.array([p[0], p[1], Wm[0, 0], Wm[0, 1], Wm[1, 1]])


def param_jacobian(bands, b, typ, u, shape, orc, ablate=(), h=1e-6):
    """d (px, py, W00, W01, W11) / d (ra, dec), (2, 5): central differences at test_loglik_grad.py's step"""
    J = np.zeros((2, 5))
    frozen = u if "no_cd_term" in ablate else None
    for i in range(2):
        e = np.zeros(2)
        e[i] = h
        J[i] = (param_map(bands, b, typ, u + e, shape, orc, ablate, frozen) - param_map(bands, b, typ, u - e, shape, orc, ablate, frozen)) / (2 * h)
    return J


def components(bands, b, typ, u, shape, orc, ablate=()):
    """[(A, A', mean, cov, var)] of a star or a type-1 galaxy in band b: the 5-tuples of test_loglik_grad.py's _comps, built from
    the position map and CD matrix above, the oracle's gen_galaxy_transformation and profile tables, and the band's PSF"""
    band = bands[b]
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    pm = param_map(bands, b, typ, np.asarray(u, dtype=np.float64), shape, orc, ablate)
    pxy = pm[:2]
    if typ == 0:
        return [(w[k], 0.0, pxy + mu[k], cov[k], 0.0) for k in range(3)]
    Wm = np.array([[pm[2], pm[3]], [pm[3], pm[4]]])
    ea, ev, da, dv = orc.profile_tables()
    amp, var = np.concatenate([ea, da]), np.concatenate([ev, dv])
    th = shape[0]
    out = []
    for j in range(14):
        tf, sg = (th, 1.0) if j < 6 else (1.0 - th, -1.0)
        for k in range(3):
            base = amp[j] * w[k]
            out.append((tf * base, sg * base, pxy + mu[k], var[j] * Wm + cov[k], var[j]))
    return out


def unit_patch(comps, box):
    """the unit-flux stamp of the components on box = (y0, y1, x0, x1)"""
    y0, y1, x0, x1 = (int(v) for v in box)
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64))
    u = np.zeros(X.shape)
    for A, _, m, Cm, _ in comps:
        a, bb, c = Cm[0, 0], Cm[0, 1], Cm[1, 1]
        det = a * c - bb * bb
        dx, dy = X - m[0], Y - m[1]
        u += A * np.exp(-0.5 * (c * dx * dx - 2 * bb * dx * dy + a * dy * dy) / det) / (2 * np.pi * np.sqrt(det))
    return u
