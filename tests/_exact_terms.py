"""The exact per-term reference the contract tests share (test_drop_contract.py, test_conditional_contract.py): every
(source, component) term t = w_k N(pixel; mu_k, Sigma_k) of a unit-flux source on its own, so that a test can say which
terms a kernel may have left out and hold the rest to rounding.  Nothing here touches the device."""
import math

import numpy as np

H = W = 256
C_R = 1e-12                          # the evaluator's relative rounding per term (derived in test_drop_contract.py)
DELTA = 1e-3                         # the drop test's documented fp32 slack (derived in test_drop_contract.py)
LD = np.longdouble
PI2 = 2 * np.arccos(LD(-1))


def components(orc, band, typ, u, shape):
    """unit-flux mixture of one source in one band: (w[K], mu[K, 2] (x, y) in pixels, cov[K, 2, 2]).  Type 2 is the
    per-profile route's source as the ABI holds it, shape = (theta, W00, W01, W11): PSF component k x profile component j has
    weight w_k a_j theta (exp) or w_k a_j (1 - theta) (dev), mean pixel + mu_k, covariance v_j W + P_k (k_prep_bin.h)"""
    if typ == 0:
        v = orc.equa2pixel(band, u)
        return band[3:6].copy(), band[6:12].reshape(3, 2) + v[None, :], band[12:24].reshape(3, 2, 2).copy()
    if typ == 2:
        ea, ev, da, dv = orc.profile_tables()
        amp, var = np.concatenate([shape[0] * ea, (1.0 - shape[0]) * da]), np.concatenate([ev, dv])
        Wm = np.array([[shape[1], shape[2]], [shape[2], shape[3]]])
        v = orc.equa2pixel(band, u)
        w = (amp[:, None] * band[3:6][None, :]).ravel()
        mu = np.broadcast_to(band[6:12].reshape(1, 3, 2) + v[None, None, :], (14, 3, 2)).reshape(42, 2).copy()
        cov = (var[:, None, None, None] * Wm[None, None] + band[12:24].reshape(1, 3, 2, 2)).reshape(42, 2, 2)
        return w, mu, cov
    w, mu, cov, _, _ = orc.galaxy_table(band, shape, u)
    return w, mu, cov


def rect_terms(w, mu, cov, y0, y1, x0, x1):
    """terms[K, ny, nx] on the rectangle rows [y0, y1) x columns [x0, x1).  Each term is one fp64 exp (a few ulp, plus |q| ulp
    for the argument: far inside C_R)"""
    det = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    ia, ib, ic = cov[:, 1, 1] / det, -0.5 * (cov[:, 0, 1] + cov[:, 1, 0]) / det, cov[:, 0, 0] / det
    dx = np.arange(x0, x1, dtype=np.float64)[None, None, :] - mu[:, 0, None, None]
    dy = np.arange(y0, y1, dtype=np.float64)[None, :, None] - mu[:, 1, None, None]
    q = ia[:, None, None] * dx * dx + 2 * ib[:, None, None] * dx * dy + ic[:, None, None] * dy * dy
    amp = w / (2 * np.pi * np.sqrt(det))
    return amp[:, None, None] * np.exp(-0.5 * q)


def source_terms(orc, band, typ, u, shape, H=H, W=W):
    """-> (box (y0, y1, x0, x1), terms[K, ny, nx], the oracle's own unit patch) or None outside the frame"""
    patch, (y0, y1), (x0, x1) = orc.source_patch(band, H, W, typ, u, shape)
    if patch is None:
        return None
    w, mu, cov = components(orc, band, typ, u, shape)
    return (y0, y1, x0, x1), rect_terms(w, mu, cov, y0, y1, x0, x1), patch


def patch_rel_err(u, patch):
    """the reference's self-check against the oracle's unit patch, where the oracle's exp(log-sum) is itself good to 1e-13
    (|log p| < 230: its argument's rounding, |log p| ulp, stays below 5e-14)"""
    m = patch >= 1e-100
    return float(np.max(np.abs(u[m] - patch[m]) / patch[m])) if m.any() else 0.0


def chunk_sub(terms, T):
    """S_sub of a unit stamp under the per-source kernels' rectangles (32 columns x 64 rows from the rectangle's corner,
    hw_source.h HW_DROP_SELF): on each, a component is dropped only below e^-T times the source's floor there, the largest of
    the components' minima"""
    sub = np.zeros(terms.shape[1:])
    for ys in range(0, terms.shape[1], 64):
        for xs in range(0, terms.shape[2], 32):
            t = terms[:, ys:ys + 64, xs:xs + 32]
            floor = float(t.reshape(t.shape[0], -1).min(axis=1).max())
            thr = floor * math.exp(-T) * (1 + DELTA)
            sub[ys:ys + 64, xs:xs + 32] = np.where(np.abs(t) <= thr, t, 0).sum(axis=0).astype(np.float64)
    return sub


# ---------------------------------------------------------------------------------------------------------------------
# the same in long double, at single pixels (the conditional kernels are held to the log of a pixel's value: 1e-12 there
# wants the reference's own digits to spare where |q| reaches 1300)
class ExactMixture(object):
    """a unit-flux mixture in long double: terms at pixels, a component's smallest value on a rectangle"""

    def __init__(self, w, mu, cov):
        w, mu, cov = np.asarray(w, LD), np.asarray(mu, LD), np.asarray(cov, LD)
        det = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
        self.ia, self.ib, self.ic = cov[:, 1, 1] / det, -(cov[:, 0, 1] + cov[:, 1, 0]) / (2 * det), cov[:, 0, 0] / det
        self.mx, self.my = mu[:, 0], mu[:, 1]
        self.amp = w / (PI2 * np.sqrt(det))
        self.K = w.shape[0]

    def q(self, xs, ys):
        dx = np.asarray(xs, LD)[None, :] - self.mx[:, None]
        dy = np.asarray(ys, LD)[None, :] - self.my[:, None]
        return self.ia[:, None] * dx * dx + 2 * self.ib[:, None] * dx * dy + self.ic[:, None] * dy * dy

    def q_abs(self, xs, ys):
        """the size of the form's three products (fp64): what an fp64 evaluation of it rounds by"""
        dx = np.asarray(xs, LD)[None, :] - self.mx[:, None]
        dy = np.asarray(ys, LD)[None, :] - self.my[:, None]
        return (np.abs(self.ia[:, None] * dx * dx) + np.abs(2 * self.ib[:, None] * dx * dy) + np.abs(self.ic[:, None] * dy * dy)).astype(np.float64)

    def terms(self, xs, ys):
        """[K, N] at the pixels (xs[i], ys[i])"""
        return self.amp[:, None] * np.exp(-self.q(xs, ys) / 2)

    def floor(self, y0, y1, x0, x1):
        """the largest over components of the component's minimum on rows [y0, y1) x columns [x0, x1): a convex form is
        largest at a corner"""
        q = self.q([x0, x1 - 1, x0, x1 - 1], [y0, y0, y1 - 1, y1 - 1]).max(axis=1)
        return (self.amp * np.exp(-q / 2)).max()
