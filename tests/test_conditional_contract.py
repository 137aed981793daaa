"""The conditional log-likelihood kernels (k_patch_ll.h), photon by photon, against an exact long-double sum of every term.

The parity tests hold a whole patch's value to 1e-11 of sum |z log m|: hundreds to tens of thousands of photons, dominated by
the core, at T = 32.  Here a single pixel's log m is read back and held between two exact bounds, at LOW thresholds, where a
term that should have been kept is far above rounding.

The dense kernels, host-buffer form.  The value is linear in the patch data, so for a rectangle R
       patch A = one photon on each corner of R (the anchors: the evaluated rectangle is R in every call),
       patch B = A + one photon on the probe pixel p,
   scored by ONE cel_patch_loglik_multi call, give  ll_B - ll_A = log m(p)  (modes 0 and 2), log(m(p) + eps) (mode 1),
   log(m(p) + bg(p)) (mode 4), formed with R's chunking and R's drop decisions.  Every probe must satisfy

       log(v(m_full - S_sub)) - tol  <=  ll_B - ll_A  <=  log(v(m_full)) + tol,     v(m) = counts m (+ eps, + bg)

   m_full: the exact sum of the source's K terms at p.  S_sub: the sum of the probe's terms at or below
       floor_chunk e^-T (1 + DELTA)      k_patch_ll_hw<0|2|4>, HW_DROP_SELF (hw_source.h): floor_chunk = the largest over
                                         components of the component's minimum on (the probe's 32 x 64 chunk of R) -- a convex
                                         form's maximum on a rectangle is at a corner, so the floor is exact;
       (eps / counts) e^-T (1 + DELTA)   k_patch_ll_hw<1>, HW_DROP_SKY;
       nothing                           T = 0 and the direct kernel k_patch_ll (CEL_OPT_KERNEL = 0).
   A kept component is also walked only on the rows where it can reach that threshold on the chunk's columns
   (quad_rows_on_columns): what is left out there is below the threshold too, so S_sub covers it.

   DELTA = 1e-3 (test_drop_contract.py derives it for the field render's Tk).  For the SELF floor hw_build adds
   fp32 arithmetic: mine = logA - 0.5f * (float) quad_max_rect.  Every probe here has m >= 1e-280, and a convex form is largest on
   R at R's corners (probes themselves), so |mine| < 650: (float) of the form rounds by 6e-8 * 1300 / 2 = 3.9e-5, the
   subtraction by half an fp32 ulp of 650 = 3.1e-5, __logf by a few ulp of a number below 64 = 1.2e-5: < 1e-4 in the log,
   with test_drop_contract's 2e-5 for Tk 1.2e-4 -- a factor 8 inside DELTA.  quad_max_rect's 1.00001 lowers the floor by
   up to 6.5e-3 in the log: towards keeping, contributes nothing.  Mode 1's floor is one __logf of eps / counts: 1e-6.

   tol, in the log domain = C_R + 2 ulp(|log v|) + 16 ulp(S_abs):
     * C_R = 1e-12, the evaluator's relative rounding per term (test_drop_contract.py: seeds, the 64-row recurrence, the
       accumulator's adds); every weight is positive, so sum |t| = m and the relative error of m is C_R, which is its log's
       absolute error; counts * m and + eps / + bg add 2 ulp relative: 2e-16, inside the rounding of 1e-12;
     * log_tab: <= 0.5 ulp of its result + 1.16e-16 absolute (k_render.h; derived and asserted in test_primitives.py, measured
       0.5 ulp + 1.11e-16) -- not "1.5 ulp of its result", which holds only where |log v| >= 0.5: the 2 ulp(|log v|) below
       take the half ulp, and the absolute part is 1.2e-4 of C_R, so tol covers it unchanged; the direct kernel's log(): 1 ulp;
     * the two sums: ll_A and ll_B are formed by the same fixed tree, and differ in the lane that holds p.  On the path from
       that lane to the result there are the lane's own adds (<= 2), six wave_sum steps (eight tree steps in k_patch_ll), the
       chunk class's add, the mass term, three class adds and the band loop: <= 14 roundings of half an ulp each per sum,
       every partial sum at most S_abs = sum of the anchors' |log v| + |log v(p)| + the mass term (counts sum w, or the
       exact sum of v over R); the subtraction in the test adds half an ulp: 16 ulp(S_abs) covers both sums.
   Condition, asserted: S_abs < 4096, hence tol < 1e-12 + 2.3e-13 + 16 * 4.5e-13 = 8.5e-12, and 100 tol <= e^-20 = 2.06e-9 with a
   factor 2 to spare: at every edge-placing threshold (T <= 20) ONE wrongly dropped term -- it is above e^-T of the floor
   and the floor is below m, so it moves log m by ... at least e^-T floor / m -- and a drop test off by a factor e (Tk - 1)
   are both far above tol wherever the floor's component carries the pixel.  The sky levels of this frame are set to 0.2 ...
   0.3 and the backgrounds to 0.1 ... 0.4 so that the sums over R of modes 1, 2 and 4 stay inside that S_abs.

   All-zero data in modes 1, 2 and 4 gives -sum (m + eps), -sum m, -sum (m + bg) over R, held between the exact sum and the
   exact sum less K e^-T (1 + DELTA) of it (hw_source.h: "the relative error ... stays below K e^-T"), with tol = 2 C_R of the
   sum (C_R per pixel; 2 800 adds on 64 lanes: 50 ulp).  cel_stamp_mass (k_patch_ll_hw<3>) is held chunk by chunk on the
   source's own box the way test_drop_contract.py holds the unit stamps.

The photon-list route (k_patch_ll_nz) runs on a resident split only, so the split is made to put photons where the test wants
them: a 640 x 640 frame of nine sources (a star, axis ratio 0.05, sigma at and below the 1/30 floor, r_e = 6 arcsec under a sharp
PSF, a type-2 W within 1e-7 of proportional to a PSF covariance, a rank-1 W, a PSF component of axis ratio 5), nelec = 0 except
on lit pixels -- the core, flanks at 1.5 / 3 / 4.5 sigma along both principal axes of the widest and the sharpest component,
the box's first and last rows and columns (CEL_OPT_SPLIT_FULL_BOX = 1), the box's corners -- each with the smallest count
(<= 65 535: the 16-bit photons-left plane) for which the exact probability of the source getting no photon there is below
1e-6; the sky level is 1e-30, so that a pixel where the unit stamp is 1e-30 still qualifies.  A box-edge or tail pixel that
no count <= 65 535 can populate is left dark (counted; never a core pixel).  After the split every lit pixel must hold a
photon of its source, and a patch holds a few tens of photons, so its value resolves per photon.  Proposals per source (itself,
shifts of 1e-3, 0.3 and 5 px, one change of each shape coordinate) are scored with CEL_OPT_PHOTON_LISTS = 1 (k_patch_ll_nz) and
2 (k_patch_ll_hw<0> on the photon rectangle) against the exact  sum z log(counts m) - counts sum w  on the fetched data.
   tol of a value = sum over photons of z (rel + 2 ulp(|log v|)) + 16 ulp(S_abs), S_abs = sum z |log v| + counts sum w, and
   rel = sum_k t_k err_k / m,  err_k = 1.5e-13 + 6 ulp kappa_k q_abs_k / 2   for the photon kernel:
     1.4015e-13 exp_tab256_p3's truncation (k_render.h) + 6.7e-16 for its table and three fma = 1.4083e-13 (derived and
     asserted in test_primitives.py; measured 1.405e-13): inside the 1.5e-13; the exponent is five fma (one multiply and one
     fma on two squares in the rotated form) of products whose sizes add up to q_abs_k / 2: <= 6 roundings of that size;
     kappa_k = cond(W) cond(P_k) for the rotated basis -- the Cholesky pivot w11 - l21^2 cancels by cond(W), the entries of
     L^-1 P_k L^-T by cond(P_k) on top, and the Jacobi angle's own error only moves the form by (l1 - l2) d(angle), which the
     same product bounds -- and 1 for the general quadratic (stars, a W without a Cholesky factor).  Computed by the reference
     from the exact pair, never read off the kernel.
   rel = C_R for the dense route.
   Which form a galaxy's component takes (rotated or general) is inferred from the exact W by the kernel's own criterion, not
   observed: were the kernel's rsqrt to round the rank-1 W's pivot 4 - (6 / 3)^2 to a tiny positive number it would take the
   rotated form there, and the value check with kappa = 1 would fail -- the assumption errs on the strict side.

Dealt and whole jobs.  cel_patch_loglik_multi deals each mode-0 job of k_patch_ll_hw<0> to PLL_PARTS = 4 blocks (chunk c to
block c % 4) while proposals x bands <= 8192 (DEAL_MAX), and gives it to one block above that; the chunk classes are summed
apart either way, so the value must not depend on it.  Both forms run, and must agree bit for bit: in the host-buffer form the
dealt call is repeated with every proposal three times over (through owner[], past DEAL_MAX); on the resident split the
reference call holds every proposal 61 times (past DEAL_MAX: whole jobs), and the proposals once and one proposal per source
in calls of <= 7 (dealt jobs) must return its bits.  With CEL_OPT_PHOTON_LISTS = 1 every patch is scored by k_patch_ll_nz,
which this entry point never deals (it launches one block per job at any size): the equality then holds one form to itself,
and the photon kernel's dealt form stays with the slice sampler's tests (test_gibbs.py), where long lists are dealt.

The probes on threshold-ellipse ends lie along the one row and the one column of R nearest the source, for three of the K
components (the largest, the smallest and the median amplitude), thinned to about 24 per case; the reference's self-check
against the oracle covers galaxies in modes 0 and 1, and the type-2 branch of components() restates k_prep_bin.h's construction
(the oracle has no type-2 patch), as test_loglik_grad.py does.

No probe is excluded: the geometry keeps every probe's exact m a normal number (>= 1e-280, asserted); the far short cut and
the subnormal range stay with test_hip_parity.py / test_gibbs.py, which price them.  The CPU reference evaluates terms only at
probes and, for the sums over R, once per case in fp64.
"""
import math

import numpy as np
import pytest

from _exact_terms import C_R, DELTA, LD, ExactMixture, chunk_sub, components, rect_terms, source_terms

gpu = pytest.mark.gpu

H = W = 256
NB = 3
SHARP_BAND = 2                       # this band's PSF is narrowed to 0.3 pixel
T_SRC = (0, 4, 8, 12, 20, 32)
T_EDGE = (4, 8, 12, 20)              # thresholds at which probes are placed on the components' threshold ellipses
M_MIN = 1e-280                       # every probe's exact unit-stamp value is a normal number
N_ADD = 16                           # roundings of the two sums, in ulp(S_abs) (docstring)
S_ABS_MAX = 4096.0
CW, CH = 32, 64                      # the chunk of the per-source kernels (HW_TW x HW_TH)
DEAL_MAX = 8192                      # cel_patch_loglik_multi, mode 0: up to this many (proposal, band) jobs each is dealt to
                                     # PLL_PARTS blocks (chunk c to block c % PLL_PARTS); above it a job is one block's

# (kernel, mode, T) -> the worst probe's error beyond what the bound allows, in units of tol; <= 1 passes.  Printed at the end
RATIOS = {}


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)))


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if RATIOS:
        print("\nworst (error - allowance) / tol, by kernel, mode and T:")
        for key in sorted(RATIOS, key=lambda k: (k[0], k[1], k[2])):
            print("  %-28s mode %-2s T=%-3g %.3g" % (key + (RATIOS[key],)))


def _note(kernel, mode, T, ratio):
    RATIOS[(kernel, mode, T)] = max(float(ratio), RATIOS.get((kernel, mode, T), -np.inf))


# ---------------------------------------------------------------------------------------------------------------------
# the scene
def make_bands(orc):
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, NB)
    bands[SHARP_BAND, 12:24] *= 0.04                       # sigma ~0.3 px
    bands[:, 0] = (0.3, 0.2, 0.25)                          # low sky levels: sum (m + eps) over R stays inside S_abs (docstring)
    for b in range(NB):
        bands[b, 36] = orc.band_radius(bands[b])            # the star radius comes with the record: the oracle's own
    return bands


# name: (type, pixel (x, y), shape, band, counts)
SOURCES = [
    ("star", 0, (100.3, 120.6), (0, 0, 0, 0), 0, 300.0),
    ("star-sharp", 0, (60.5, 200.2), (0, 0, 0, 0), SHARP_BAND, 250.0),
    ("gal-round", 1, (150.2, 90.7), (0.5, 1.5, 0.0, 0.95), 0, 400.0),
    ("gal-thin", 1, (200.0, 60.0), (0.3, 3.0, 37.0, 0.12), 1, 350.0),
    ("gal-thin-sharp", 1, (60.0, 120.0), (0.7, 2.5, 128.0, 0.1), SHARP_BAND, 300.0),
    ("gal-floor", 1, (130.4, 30.9), (0.5, 0.02, 10.0, 0.8), 0, 200.0),          # sigma below the 1/30 floor
    ("gal-floor-sharp", 1, (30.2, 40.6), (0.9, 1.0 / 30, 80.0, 0.5), SHARP_BAND, 200.0),
    ("gal-big-sharp", 1, (128.0, 180.0), (0.4, 6.0, 70.0, 0.6), SHARP_BAND, 500.0),
    ("t2-pd", 2, (190.6, 200.3), (0.35, 1.2, 0.3, 0.9), 1, 300.0),              # positive definite W
    ("t2-rank1", 2, (100.5, 215.5), (0.6, 9.0, 6.0, 4.0), 0, 300.0),           # rank-1 W (no Cholesky factor)
    ("gal-edge", 1, (1.5, 130.2), (0.5, 2.0, 20.0, 0.7), 1, 300.0),            # on the frame's left edge
    ("star-edge", 0, (254.6, 30.2), (0, 0, 0, 0), 0, 300.0),
]

# (source, R = (dy0, dx0, ny, nx) from the source's pixel): several chunks both ways (wider than 32, taller than 64), not aligned
# with the source's own box, some shifted into the tail; the sharp and compact sources reach 1e-280 within ~20 px, so their
# rectangles cut the core into chunks asymmetrically; one R is narrower than a chunk
CASES = [
    ("star", (-30, -17, 70, 40)), ("star", (-12, -9, 70, 40)), ("star", (6, 10, 70, 40)),
    ("star-sharp", (-4, -3, 9, 7)),
    ("gal-round", (-35, -20, 70, 40)), ("gal-round", (-8, 5, 70, 40)), ("gal-round", (-40, -30, 130, 70)),
    ("gal-thin", (-33, -19, 70, 40)), ("gal-thin", (-70, -6, 75, 45)),
    ("gal-thin-sharp", (-36, -21, 72, 41)), ("gal-thin-sharp", (-60, -33, 66, 37)),
    ("gal-floor", (-32, -16, 70, 40)),
    ("gal-floor-sharp", (-5, -4, 10, 9)),
    ("gal-big-sharp", (-35, -20, 70, 40)), ("gal-big-sharp", (10, -50, 70, 40)),
    ("t2-pd", (-34, -18, 70, 40)), ("t2-pd", (-3, 2, 40, 70)),
    ("t2-rank1", (-36, -22, 70, 40)), ("t2-rank1", (-66, -12, 70, 40)),
    ("gal-edge", (-30, -2, 70, 40)),
    ("star-edge", (-28, -38, 70, 40)),
]


class Scene(object):
    def __init__(self, orc):
        from desi_mcmc_amd import synth
        self.bands = make_bands(orc)
        self.names = [s[0] for s in SOURCES]
        self.typ = np.array([s[1] for s in SOURCES], np.int32)
        self.pix = np.array([s[2] for s in SOURCES], float)
        self.shape = np.array([s[3] for s in SOURCES], float)
        self.band = [s[4] for s in SOURCES]
        self.cnt = np.array([s[5] for s in SOURCES], float)
        self.radec = np.array([synth.pixel2equa(self.bands[b], self.pix[i:i + 1])[0] for i, b in enumerate(self.band)])
        self.mix, self.comps = [], []
        for i, b in enumerate(self.band):
            c = components(orc, self.bands[b], self.typ[i], self.radec[i], self.shape[i])
            self.comps.append(c)
            self.mix.append(ExactMixture(*c))
        self.cases = [Case(self, k, self.names.index(n), r) for k, (n, r) in enumerate(CASES)]


def bg_plane(y0, y1, x0, x1):
    """mode 4's background on R: positive, different on every pixel of a 7 x 5 cell"""
    yy, xx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    return 0.1 + 0.01 * ((3 * xx + 5 * yy) % 31)


class Case(object):
    """one (source, R): its probes, their exact terms, and per probe the floor of its chunk of R"""

    def __init__(self, sc, index, s, rel):
        self.s, self.b, self.name = s, sc.band[s], "%s%s" % (sc.names[s], (rel,))
        cx, cy = int(round(sc.pix[s, 0])), int(round(sc.pix[s, 1]))
        y0, x0 = max(0, cy + rel[0]), max(0, cx + rel[1])
        y1, x1 = min(H, cy + rel[0] + rel[2]), min(W, cx + rel[1] + rel[3])
        self.R = (y0, y1, x0, x1)
        self.ny, self.nx = y1 - y0, x1 - x0
        self.mix = sc.mix[s]
        self.K = self.mix.K
        self.counts = sc.cnt[s]
        self.eps = sc.bands[self.b, 0]
        self.wsum = float(sc.bands[self.b, 3:6].sum())
        self.anchors = [(y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1)]
        self.terms64 = rect_terms(*sc.comps[s], y0, y1, x0, x1)          # [K, ny, nx], once per case: the sums over R
        self.probes = self._choose(index)
        ys = np.array([p[0] for p in self.probes])
        xs = np.array([p[1] for p in self.probes])
        self.t = self.mix.terms(xs, ys)                                   # [K, N] long double
        self.m = self.t.sum(axis=0)
        self.floor = np.array([self.mix.floor(*self.chunk_of(y, x)) for (y, x) in self.probes], LD)
        self.bg = bg_plane(y0, y1, x0, x1)
        self.bg_p = self.bg[ys - y0, xs - x0]
        self.m_anchor = self.mix.terms([a[1] for a in self.anchors], [a[0] for a in self.anchors]).sum(axis=0)

    def chunk_of(self, y, x):
        y0, y1, x0, x1 = self.R
        ya, xa = y0 + (y - y0) // CH * CH, x0 + (x - x0) // CW * CW
        return ya, min(ya + CH, y1), xa, min(xa + CW, x1)

    def seams(self):
        y0, y1, x0, x1 = self.R
        return [x0 + k for k in range(CW, self.nx, CW)], [y0 + k for k in range(CH, self.ny, CH)]

    def _choose(self, index):
        y0, y1, x0, x1 = self.R
        ym, xm = (y0 + y1) // 2, (x0 + x1) // 2
        P = list(self.anchors) + [(y0, xm), (y1 - 1, xm), (ym, x0), (ym, x1 - 1)]
        sx, sy = self.seams()
        rows = sorted({y0, y0 + self.ny // 3, y1 - 1} | {y for s in sy for y in (s - 1, s)})
        cols = sorted({x0, xm, x1 - 1} | {x for s in sx for x in (s - 1, s)})
        P += [(y, x) for s in sx for x in (s - 1, s) for y in rows]      # both sides of every column seam (the crossings too)
        P += [(y, x) for s in sy for y in (s - 1, s) for x in cols]      # both sides of every row seam
        # the last partial chunk: its first column / row on R's last row / column, and the pixel inside its far corner
        xl, yl = x0 + (self.nx - 1) // CW * CW, y0 + (self.ny - 1) // CH * CH
        P += [(y1 - 1, xl), (yl, x1 - 1), (max(y1 - 2, y0), max(x1 - 2, x0))]
        # the ends of the components' threshold ellipses: along the row and the column nearest the source, the two pixels on
        # either side of every place where a component crosses its chunk's threshold
        t = self.terms64
        fl = np.zeros((self.ny, self.nx))
        for ya in range(0, self.ny, CH):
            for xa in range(0, self.nx, CW):
                c = t[:, ya:ya + CH, xa:xa + CW]
                fl[ya:ya + CH, xa:xa + CW] = c.reshape(self.K, -1).min(axis=1).max()
        yc = int(np.clip(round(float(self.mix.my[0])), y0, y1 - 1)) - y0
        xc = int(np.clip(round(float(self.mix.mx[0])), x0, x1 - 1)) - x0
        amp = np.asarray(self.mix.amp, float)
        ks = sorted({int(np.argmax(amp)), int(np.argmin(amp)), int(np.argsort(amp)[self.K // 2])})
        ends = []
        for T in T_EDGE:
            for k in ks:
                on = t[k, yc, :] > fl[yc, :] * math.exp(-T)
                for i in np.nonzero(on[1:] != on[:-1])[0][:2]:
                    ends += [(y0 + yc, x0 + int(i)), (y0 + yc, x0 + int(i) + 1)]
                on = t[k, :, xc] > fl[:, xc] * math.exp(-T)
                for i in np.nonzero(on[1:] != on[:-1])[0][:2]:
                    ends += [(y0 + int(i), x0 + xc), (y0 + int(i) + 1, x0 + xc)]
        self.n_ends = len(set(ends))
        P += sorted(set(ends))[::max(1, len(set(ends)) // 24)]
        # the deep tail: the faintest pixel of R (a corner) is an anchor already; the faintest of the interior rows
        m = t.sum(axis=0)
        i = np.unravel_index(np.argmin(m[1:-1, :]) if self.ny > 2 else 0, (max(self.ny - 2, 1), self.nx))
        P.append((y0 + 1 + int(i[0]) if self.ny > 2 else y0, x0 + int(i[1])))
        rs = np.random.RandomState(1000 + index)
        while len(set(P)) < 50 and len(set(P)) < self.ny * self.nx:
            P.append((int(rs.randint(y0, y1)), int(rs.randint(x0, x1))))
        out = []
        for p in P:
            if p not in out:
                out.append(p)
        return out

    # ---- the bounds ----
    def v(self, m, mode):
        """what the kernel takes the log of, from the unit-stamp value (long double)"""
        v = LD(self.counts) * m
        return v + LD(self.eps) if mode == 1 else (v + self.bg_p.astype(LD) if mode == 4 else v)

    def s_sub(self, T, mode, drops):
        if not drops or T <= 0:
            return np.zeros(len(self.probes), LD)
        thr = (LD(self.eps) / LD(self.counts) if mode == 1 else self.floor) * LD(math.exp(-T) * (1 + DELTA))
        return np.where(self.t <= thr[None, :] if mode != 1 else self.t <= thr, self.t, LD(0)).sum(axis=0)

    def mass_term(self, mode):
        """what both sums carry besides the photons, exactly (fp64 terms, long double adds)"""
        if mode == 0:
            return self.counts * self.wsum
        tot = float(LD(self.counts) * self.terms64.astype(LD).sum())
        return tot + (self.eps * self.ny * self.nx if mode == 1 else (float(self.bg.sum()) if mode == 4 else 0.0))

    def bounds(self, T, mode, drops=True):
        """(lo, hi, tol) per probe, log domain"""
        hi = np.log(self.v(self.m, mode))
        lo = np.log(self.v(self.m - self.s_sub(T, mode, drops), mode))
        v_anchor = LD(self.counts) * self.m_anchor
        if mode == 1:
            v_anchor = v_anchor + LD(self.eps)
        if mode == 4:
            y0, y1, x0, x1 = self.R
            v_anchor = v_anchor + np.array([self.bg[a[0] - y0, a[1] - x0] for a in self.anchors], LD)
        s_abs = float(np.abs(np.log(v_anchor)).sum()) + np.abs(hi).astype(np.float64) + abs(self.mass_term(mode))
        tol = C_R + 2 * _ulp(hi.astype(np.float64)) + N_ADD * _ulp(s_abs)
        return lo, hi, tol, s_abs


@pytest.fixture(scope="module")
def scene(orc):
    return Scene(orc)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference and the geometry
def test_reference_reproduces_the_oracle(orc, scene):
    """the per-term sum is oracle.patch_loglik on whole patches (two cases, modes 0 and 1, to 1e-12), and the long-double
    terms at the probes are the fp64 terms of the rectangle"""
    rs = np.random.RandomState(5)
    for ci in (4, 7):                                     # a round galaxy off its core, a thin one (a type-2 source is not the oracle's)
        c = scene.cases[ci]
        assert scene.typ[c.s] == 1
        y0, y1, x0, x1 = c.R
        z = rs.poisson(2.0, size=(c.ny, c.nx)).astype(float)
        m = c.counts * c.terms64.sum(axis=0)
        for mode, want in ((0, float((np.log(m) * z).sum() - c.counts * c.wsum)),
                           (1, float((np.log(m + c.eps) * z).sum() - (m + c.eps).sum()))):
            got = orc.patch_loglik(scene.bands[c.b], H, W, scene.typ[c.s], scene.radec[c.s], scene.shape[c.s], c.counts,
                                   np.array(c.R, np.int32), z, mode)
            assert abs(got - want) <= 1e-12 * float((np.abs(np.log(m)) * z).sum() + m.sum() + c.eps * z.size), (c.name, mode, got, want)
    for c in scene.cases:
        ys = np.array([p[0] for p in c.probes]) - c.R[0]
        xs = np.array([p[1] for p in c.probes]) - c.R[2]
        t64 = c.terms64[:, ys, xs]
        ok = t64 > 1e-290
        # (fp64: the determinant of a thin component cancels and the form's three products nearly cancel far out)
        assert np.all(np.abs(t64[ok] - c.t.astype(np.float64)[ok]) <= (1e-13 + 5e-15 * c.mix.q_abs(xs + c.R[2], ys + c.R[0])[ok]) * t64[ok])
        # the floor of a chunk from the corners == the brute-force minimum over the chunk's pixels
        for j in (0, len(c.probes) // 2, len(c.probes) - 1):
            ya, yb, xa, xb = c.chunk_of(*c.probes[j])
            brute = c.terms64[:, ya - c.R[0]:yb - c.R[0], xa - c.R[2]:xb - c.R[2]].reshape(c.K, -1).min(axis=1).max()
            assert abs(float(c.floor[j]) - brute) <= 1e-12 * brute or brute < 1e-290


def test_the_probes_are_where_kernels_go_wrong(scene):
    """the asserted coverage: every seam of every R probed on both sides, every last partial chunk's last row and column,
    probes on threshold-ellipse ends, no probe below a normal number, S_abs inside the tolerance's condition and
    100 tol <= e^-T at every edge-placing threshold"""
    multi = narrow = ends = 0
    for c in scene.cases:
        y0, y1, x0, x1 = c.R
        P = set(c.probes)
        assert set(c.anchors) <= P and (40 <= len(P) <= 140 or c.nx * c.ny < 100), (c.name, len(P))
        sx, sy = c.seams()
        multi += bool(sx and sy)
        narrow += (c.nx < CW and c.ny < CH)
        for s in sx:
            assert {x for (y, x) in P if y in (y0, y1 - 1)} >= {s - 1, s}, c.name
        for s in sy:
            assert {y for (y, x) in P if x in (x0, x1 - 1)} >= {s - 1, s}, c.name
        for s in sx:
            for t in sy:
                assert {(t - 1, s - 1), (t - 1, s), (t, s - 1), (t, s)} <= P, c.name
        assert (y1 - 1, x0 + (c.nx - 1) // CW * CW) in P and (y0 + (c.ny - 1) // CH * CH, x1 - 1) in P
        ends += c.n_ends
        assert float(c.m.min()) >= M_MIN and float(c.m_anchor.min()) >= M_MIN, (c.name, float(c.m.min()))
        for mode in (0, 1, 2, 4):
            lo, hi, tol, s_abs = c.bounds(20, mode)
            assert np.all(s_abs < S_ABS_MAX), (c.name, mode, float(np.max(s_abs)))
            assert np.all(100 * tol <= math.exp(-20)), (c.name, mode, float(tol.max()))
    assert multi >= 12 and narrow >= 1 and ends >= 100
    assert any(c.R[2] == 0 for c in scene.cases) and any(c.R[3] == W for c in scene.cases)       # R on the frame's edges


# ---------------------------------------------------------------------------------------------------------------------
# A. the dense kernels
class Batch(object):
    """every case's patch sets (A, then one B per probe) for one cel_patch_loglik_multi call"""

    def __init__(self, cel, ctx, scene, mode, zero=False, cases=None):
        self.mode, self.scene = mode, scene
        self.cases = scene.cases if cases is None else cases
        boxes, flat, owner_src, self.first = [], [], [], []
        for c in self.cases:
            y0, y1, x0, x1 = c.R
            self.first.append(len(boxes))
            A = np.zeros((c.ny, c.nx))
            if not zero:
                for (y, x) in c.anchors:
                    A[y - y0, x - x0] += 1.0               # (a rectangle one pixel wide or tall: anchors coincide and add up)
            for p in [None] + ([] if zero else c.probes):
                z = A.copy()
                if p is not None:
                    z[p[0] - y0, p[1] - x0] += 1.0
                bx = np.zeros((NB, 4), np.int32)
                bx[c.b] = c.R
                boxes.append(bx)
                flat.append(z.ravel())
                if mode == 4:
                    flat.append(c.bg.ravel())
                owner_src.append(c.s)
        self.boxes = np.ascontiguousarray(np.array(boxes, np.int32))
        self.NS = len(boxes)
        n = np.array([(b[:, 1] - b[:, 0]) * (b[:, 3] - b[:, 2]) for b in self.boxes], np.int64).ravel() * (2 if mode == 4 else 1)
        self.offs = np.zeros(self.NS * NB + 1, np.int64)
        np.cumsum(n, out=self.offs[1:])
        self.data = np.ascontiguousarray(np.concatenate(flat))
        assert self.data.size == self.offs[-1] and self.data.nbytes < 40e6
        src = np.array(owner_src)
        counts = np.zeros((self.NS, NB))
        counts[np.arange(self.NS), [scene.band[s] for s in src]] = scene.cnt[src]
        self._set = lambda reps: cel.SourceSet(ctx, self.NS * reps, NB).set(
            *(np.tile(a, (reps,) + (1,) * (a.ndim - 1)) for a in (scene.typ[src], scene.radec[src], counts, scene.shape[src])))
        self.props = {1: self._set(1)}

    def run(self, iset, reps=1):
        """-> ll[reps, NS]: every patch set scored by `reps` equal proposals (through owner[]; the patch data goes over once)"""
        from desi_mcmc_amd import _lib as L
        if reps not in self.props:
            self.props[reps] = self._set(reps)
        owner = np.tile(np.arange(self.NS, dtype=np.int32), reps)
        out = np.zeros(self.NS * reps)
        L.check(L.lib().cel_patch_loglik_multi(iset._h, self.props[reps]._h, owner.ctypes.data_as(L.c_int32_p), self.NS,
                                               self.boxes.ctypes.data_as(L.c_int32_p), self.offs.ctypes.data_as(L.c_int64_p),
                                               self.data.ctypes.data, L.CEL_HOST, self.mode, L.dptr(out)))
        return out.reshape(reps, self.NS)


@pytest.fixture(scope="module")
def dev(cel, scene):
    ctx = cel.Context(0)
    iset = cel.ImageSet(ctx, scene.bands, H, W)
    for b in range(NB):
        assert iset.band(b)[36] == scene.bands[b, 36]
    return ctx, iset


def _batches(cel, ctx, scene, mode):
    """every case in one call; mode 4 carries a background plane per patch set, twice the data: two calls"""
    h = len(scene.cases) // 2
    return [Batch(cel, ctx, scene, mode, cases=cs) for cs in ((scene.cases[:h], scene.cases[h:]) if mode == 4 else (scene.cases,))]


def _check_probes(batch, ll, T, mode, kernel, drops):
    for ci, c in enumerate(batch.cases):
        f = batch.first[ci]
        obs = ll[f + 1:f + 1 + len(c.probes)] - ll[f]
        lo, hi, tol, _ = c.bounds(T, mode, drops)
        r_lo = ((lo - LD(1) * obs).astype(np.float64)) / tol
        r_hi = ((LD(1) * obs - hi).astype(np.float64)) / tol
        _note(kernel, mode, T, max(r_lo.max(), r_hi.max()))
        for r, what in ((r_lo, "a term above the threshold was left out"), (r_hi, "the kernel exceeds the exact sum")):
            j = int(np.argmax(r))
            y, x = c.probes[j]
            assert r[j] <= 1.0, ("%s mode %d T=%g, case %s, probe (y %d, x %d) = R + (%d, %d), chunk %s: %s: observed %.17g, exact "
                                 "log %.17g, lower bound %.17g, tol %.3g (ratio %.3g)"
                                 % (kernel, mode, T, c.name, y, x, y - c.R[0], x - c.R[2], c.chunk_of(y, x), what, obs[j], float(hi[j]),
                                    float(lo[j]), tol[j], r[j]))


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_dense_kernel_pixel_by_pixel(cel, scene, dev, mode):
    """k_patch_ll_hw<mode>: every probe's log value between the exact bounds at T = 0 .. 32"""
    ctx, iset = dev
    batches = _batches(cel, ctx, scene, mode)
    try:
        for T in T_SRC:
            ctx.set_tail_log(T)              # (sets the per-source kernels' threshold, CEL_OPT_TAIL_LOG_SOURCE, with the render's)
            for batch in batches:
                ll = batch.run(iset)[0]
                _check_probes(batch, ll, T, mode, "k_patch_ll_hw<%d>" % mode, drops=True)
                if mode == 0:
                    # the call above has batch.NS * NB <= DEAL_MAX jobs, so each was dealt to four blocks; with every
                    # proposal there three times the same call passes DEAL_MAX and each job is one block's: the same bits
                    assert batch.NS * NB <= DEAL_MAX < 3 * batch.NS * NB
                    whole = batch.run(iset, reps=3)
                    assert np.array_equal(whole, np.tile(ll, (3, 1))), "T=%g: a whole job and its dealt form differ at patch set %s" % (
                        T, np.nonzero((whole != ll[None, :]).any(axis=0))[0][:8])
    finally:
        ctx.set_tail_log("default")


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_direct_kernel_pixel_by_pixel(cel, scene, dev, mode):
    """k_patch_ll (CEL_OPT_KERNEL = 0) drops nothing at any threshold"""
    ctx, iset = dev
    batches = _batches(cel, ctx, scene, mode)
    ctx.set_kernel("direct")
    try:
        for T in T_SRC:
            ctx.set_tail_log(T)
            for batch in batches:
                _check_probes(batch, batch.run(iset)[0], T, mode, "k_patch_ll", drops=False)
    finally:
        ctx.set_kernel("recurrence")
        ctx.set_tail_log("default")


@gpu
@pytest.mark.parametrize("mode", [1, 2, 4])
def test_dense_kernel_sums_on_zero_data(cel, scene, dev, mode):
    """all-zero data: -sum over R of (m + eps) / m / (m + bg), between the exact sum and the exact sum less K e^-T (1 + DELTA)"""
    ctx, iset = dev
    batch = Batch(cel, ctx, scene, mode, zero=True)
    exact = np.array([c.mass_term(mode) for c in scene.cases])
    K = np.array([c.K for c in scene.cases])
    tol = 2 * C_R * exact
    try:
        for T in T_SRC:
            ctx.set_tail_log(T)
            got = -batch.run(iset)[0]
            allow = K * math.exp(-T) * (1 + DELTA) * exact if T > 0 else 0.0
            r_lo, r_hi = (exact - got - allow) / tol, (got - exact) / tol
            _note("k_patch_ll_hw<%d> zero data" % mode, mode, T, max(r_lo.max(), r_hi.max()))
            j = int(np.argmax(r_lo))
            assert r_lo[j] <= 1.0, "mode %d T=%g case %s: sum %.17g below exact %.17g by more than K e^-T (%.3g tol)" % (
                mode, T, scene.cases[j].name, got[j], exact[j], r_lo[j])
            j = int(np.argmax(r_hi))
            assert r_hi[j] <= 1.0, "mode %d T=%g case %s: sum %.17g above exact %.17g (%.3g tol)" % (
                mode, T, scene.cases[j].name, got[j], exact[j], r_hi[j])
    finally:
        ctx.set_tail_log("default")


@gpu
def test_stamp_mass_chunk_by_chunk(cel, orc, scene, dev):
    """k_patch_ll_hw<3> (cel_stamp_mass with CEL_OPT_SPLIT_REUSE = 0) on each source's own box: between the exact mass and the
    exact mass less every chunk's S_sub"""
    from desi_mcmc_amd import _lib as L
    ctx, iset = dev
    S = len(SOURCES)
    counts = np.tile(scene.cnt[:, None], (1, NB))
    srcs = cel.SourceSet(ctx, S, NB).set(scene.typ, scene.radec, counts, scene.shape)
    boxes, status = iset.source_boxes(srcs)
    reuse = ctx.get_option(L.CEL_OPT_SPLIT_REUSE)
    ctx.set_option(L.CEL_OPT_SPLIT_REUSE, 0)
    try:
        for T in (4, 8, 12, 20):
            ctx.set_option(L.CEL_OPT_TAIL_LOG_SOURCE, T)
            mass = iset.stamp_mass(srcs)
            worst = -np.inf
            for s in range(S):
                for b in range(NB):
                    u = scene.radec[s]
                    if scene.typ[s] == 2:
                        assert status[b, s] > 0
                        box = tuple(int(v) for v in boxes[b, s])
                        t = rect_terms(*components(orc, scene.bands[b], 2, u, scene.shape[s]), *box)
                    else:
                        r = source_terms(orc, scene.bands[b], scene.typ[s], u, scene.shape[s], H, W)
                        if r is None:
                            assert mass[s, b] == 0.0
                            continue
                        box, t, _ = r
                        assert tuple(boxes[b, s]) == box
                    full = float(t.astype(LD).sum())
                    sub = float(chunk_sub(t, T).astype(LD).sum())
                    tol = 2 * C_R * full
                    r_lo, r_hi = (full - mass[s, b] - sub) / tol, (mass[s, b] - full) / tol
                    worst = max(worst, r_lo, r_hi)
                    assert r_lo <= 1.0, "mass of %s band %d T=%g: %.17g below exact %.17g less S_sub %.3g (%.3g tol)" % (
                        scene.names[s], b, T, mass[s, b], full, sub, r_lo)
                    assert r_hi <= 1.0, "mass of %s band %d T=%g: %.17g above exact %.17g (%.3g tol)" % (scene.names[s], b, T, mass[s, b], full, r_hi)
            _note("k_patch_ll_hw<3>", 3, T, worst)
    finally:
        ctx.set_option(L.CEL_OPT_SPLIT_REUSE, reuse)
        ctx.set_option(L.CEL_OPT_TAIL_LOG_SOURCE, float("nan"))



# ---------------------------------------------------------------------------------------------------------------------
# B. the photon-list route, one photon at a time
HB = WB = 640
NBB = 2
U64 = 1.1102230246251565e-16
LIST_R = 1.5e-13
# name, type, pixel, shape (type 2: theta, W00, W01, W11; W of "t2-psf" is set from the band's PSF below), counts per band
LIST_SOURCES = [
    ("star", 0, (64.3, 64.6), (0, 0, 0, 0), 400.0),
    ("gal-thin", 1, (192.2, 64.4), (0.5, 2.0, 30.0, 0.05), 600.0),             # axis ratio 0.05
    ("gal-floor", 1, (320.5, 64.5), (0.6, 1.0 / 30, 10.0, 0.8), 300.0),        # sigma at the floor
    ("gal-below-floor", 1, (64.7, 192.1), (0.3, 0.01, 70.0, 0.5), 300.0),      # below it
    ("gal-big", 1, (480.4, 480.8), (0.4, 6.0, 120.0, 0.6), 2000.0),             # r_e = 6 arcsec, sharp PSF in band 1
    ("t2-psf", 2, (330.2, 190.6), (0.5, 1.0, 0.0, 1.0), 500.0),                # W nearly proportional to a PSF covariance
    ("t2-rank1", 2, (64.5, 320.5), (0.6, 9.0, 6.0, 4.0), 500.0),               # rank-1 W: the general form
    ("t2-pd", 2, (200.6, 200.2), (0.35, 1.2, 0.3, 0.9), 500.0),
    ("gal-round", 1, (192.5, 330.5), (0.7, 1.2, 45.0, 0.9), 500.0),
]


def list_bands(orc):
    from desi_mcmc_amd import synth
    bands = synth.make_bands(HB, WB, NBB)
    bands[1, 12:24] *= 0.04                                  # band 1: sharp ...
    bands[1, 16:20] = (0.5, 0.0, 0.0, 0.02)                  # ... and its second component has axis ratio 5 (variances 25 : 1)
    bands[:, 0] = 1e-30                                      # a sky so low that a lit pixel in the tail still gives its source photons
    for b in range(NBB):
        bands[b, 36] = orc.band_radius(bands[b])
    return bands


def _pair_kappa(orc, band, typ, u, shape):
    """per component: the conditioning of the pair (W, P_k) the rotated basis diagonalises, cond(W) cond(P_k) -- W = L L^T's
    pivot w11 - l21^2 cancels by cond(W), L^-1 P_k L^-T's entries by cond(P_k) on top; 1 where the kernel takes the general
    quadratic (a star; a W without a Cholesky factor, w00 <= 0 or w11 - w01^2 / w00 <= 0).  -> (kappa[K], rotated?)"""
    if typ == 0:
        return np.ones(3), False
    if typ == 2:
        Wm = np.array([[shape[1], shape[2]], [shape[2], shape[3]]])
    else:
        tinv = orc.galaxy_table(band, shape, u)[4]
        Wm = tinv @ tinv.T
    if not (Wm[0, 0] > 0 and Wm[1, 1] - Wm[0, 1] ** 2 / Wm[0, 0] > 1e-12 * Wm[1, 1]):
        return np.ones(42), False
    kp = np.array([np.linalg.cond(band[12:24].reshape(3, 2, 2)[k]) for k in range(3)]) * np.linalg.cond(Wm)
    # components(): type 1 is the oracle's table, index = profile * 3 + psf; type 2 likewise (14, 3) ravelled
    return np.tile(kp, 14), True


class ListRef(object):
    """exact value and bound of one proposal on its owner's fetched photons"""

    def __init__(self, orc, bands, typ, u, shape, counts):
        self.mix, self.kappa, self.rot = [], [], []
        for b in range(NBB):
            self.mix.append(ExactMixture(*components(orc, bands[b], typ, u, shape)))
            k, r = _pair_kappa(orc, bands[b], typ, u, shape)
            self.kappa.append(k)
            self.rot.append(r)
        self.counts, self.wsum = counts, [float(bands[b, 3:6].sum()) for b in range(NBB)]

    def value(self, photons, lists):
        """photons[b] = (ys, xs, z) -> (exact value, tol, smallest m): lists = True the photon kernel's bound, False the dense one's
        (every band has a patch -- the test asserts status > 0 -- so every band's mass term counts)"""
        tot, tol, s_abs, mmin = LD(0), 0.0, 0.0, np.inf
        for b in range(NBB):
            ys, xs, z = photons[b]
            mass = self.counts[b] * self.wsum[b]
            s_abs += mass
            tot -= LD(mass)
            if len(z) == 0:
                continue
            t = self.mix[b].terms(xs, ys)
            m = t.sum(axis=0)
            mmin = min(mmin, float(m.min()))
            lv = np.log(LD(self.counts[b]) * m)
            tot += (LD(1) * z * lv).sum()
            if lists:
                err = LIST_R + 6 * U64 * self.kappa[b][:, None] * 0.5 * self.mix[b].q_abs(xs, ys)
                rel = ((t * err).sum(axis=0) / m).astype(np.float64)
            else:
                rel = C_R
            lv64 = lv.astype(np.float64)
            tol += float((z * (rel + 2 * _ulp(lv64))).sum())
            s_abs += float((z * np.abs(lv64)).sum())
        return float(tot), tol + N_ADD * float(_ulp(s_abs)), mmin


def _lit_pixels(mix, box):
    """where a source's photons are wanted: core, flanks along both principal axes of its widest and its sharpest component,
    the box's first and last rows and columns, the box's corners (the deep tail)"""
    y0, y1, x0, x1 = box
    cx, cy = float(mix.mx[0]), float(mix.my[0])
    P = [(round(cy), round(cx)), (round(cy) + 1, round(cx)), (round(cy), round(cx) - 1)]
    det = 1.0 / np.asarray(mix.ia * mix.ic - mix.ib * mix.ib, float)
    for k in (int(np.argmax(det)), int(np.argmin(det))):
        Q = np.array([[float(mix.ia[k]), float(mix.ib[k])], [float(mix.ib[k]), float(mix.ic[k])]])
        lam, vec = np.linalg.eigh(Q)
        for j in range(2):
            for r in (1.5, 3.0, 4.5):
                for sg in (1, -1):
                    d = sg * r / math.sqrt(lam[j]) * vec[:, j]
                    P.append((round(cy + d[1]), round(cx + d[0])))
    xc, yc = min(max(round(cx), x0), x1 - 1), min(max(round(cy), y0), y1 - 1)
    edge = [(y0, xc), (y1 - 1, xc), (yc, x0), (yc, x1 - 1)]
    tail = [(y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1), ((y0 + yc) // 2, (x0 + xc) // 2), ((y1 + yc) // 2, (x1 + xc) // 2)]
    keep = lambda L: [p for p in dict.fromkeys(L) if y0 <= p[0] < y1 and x0 <= p[1] < x1]
    return keep(P), edge, keep(tail)           # (the four edge pixels are inside the box by construction, and stay in this order)


@gpu
def test_photon_list_route_photon_by_photon(cel, orc):
    from desi_mcmc_amd import _lib as L, synth
    ctx = cel.Context(0)
    bands = list_bands(orc)
    S = len(LIST_SOURCES)
    names = [s[0] for s in LIST_SOURCES]
    typ = np.array([s[1] for s in LIST_SOURCES], np.int32)
    pix = np.array([s[2] for s in LIST_SOURCES], float)
    shape = np.array([s[3] for s in LIST_SOURCES], float)
    i = names.index("t2-psf")
    P1 = bands[0, 12:24].reshape(3, 2, 2)[1]
    shape[i, 1:] = (4.0 * P1[0, 0] * (1 + 1e-7), 4.0 * P1[0, 1], 4.0 * P1[1, 1])
    counts = np.array([[s[4], 0.7 * s[4]] for s in LIST_SOURCES])
    radec = synth.pixel2equa(bands[0], pix)
    iset = cel.ImageSet(ctx, bands, HB, WB)
    srcs = cel.SourceSet(ctx, S, NBB).set(typ, radec, counts, shape)
    boxes, status = iset.source_boxes(srcs)
    assert np.all(status > 0)
    refs = [ListRef(orc, bands, typ[s], radec[s], shape[s], counts[s]) for s in range(S)]
    assert any(r.rot[0] for r in refs) and any(not r.rot[0] for r in refs if r.mix[0].K == 42) and not refs[names.index("t2-rank1")].rot[0]
    assert min(shape[typ == 1, 3]) <= 0.05 and min(shape[typ == 1, 1]) < 1.0 / 30 and max(shape[typ == 1, 1]) >= 6.0
    # the lit pixels: counts such that the exact probability of the source getting no photon there is below 1e-6
    nelec = np.zeros((NBB, HB, WB))
    lit, dark = {}, []
    n_tail = 0
    for s in range(S):
        for b in range(NBB):
            core, edge, tail = _lit_pixels(refs[s].mix[b], tuple(boxes[b, s]))
            for kind, P in (("core", core), ("edge", edge), ("tail", tail)):
                for (y, x) in P:
                    rate = [float(counts[q, b] * refs[q].mix[b].terms([x], [y]).sum()) if
                            (boxes[b, q, 0] <= y < boxes[b, q, 1] and boxes[b, q, 2] <= x < boxes[b, q, 3]) else 0.0 for q in range(S)]
                    p = rate[s] / (sum(rate) + bands[b, 0])
                    n = (1 if p >= 1 - 1e-7 else int(math.ceil(math.log(1e-6) / math.log1p(-p))) + 1) if p > 0 else np.inf
                    if n > 65535 or rate[s] / counts[s, b] < M_MIN:
                        assert kind != "core", (names[s], b, kind, y, x, p)        # (a box edge of a sharp source may be out of reach)
                        dark.append((names[s], b, kind, y, x))
                        continue
                    nelec[b, y, x] = max(nelec[b, y, x], n)
                    lit[(s, b, y, x)] = kind
                    n_tail += kind == "tail"
    assert nelec.max() <= 65535 and n_tail >= S, dark
    for s in range(S):                # per source, in some band: the box's first and last rows and columns (edge = _lit_pixels' order)
        for j, side in enumerate(("first row", "last row", "first column", "last column")):
            assert any(j < len(e) and (s, b) + e[j] in lit for b in range(NBB) for e in [_lit_pixels(refs[s].mix[b], tuple(boxes[b, s]))[1]]), (
                "%s: no band in which its box's %s can be lit; left dark: %s" % (names[s], side, dark))
    iset.set_nelec(nelec)
    # the proposals: the source itself, shifts of 1e-3, 0.3 and 5 px, one change of every shape coordinate
    ptyp, pu, pshape, pcounts, own = [], [], [], [], []
    for s in range(S):
        shifts = [(0.0, 0.0), (1e-3, -1e-3), (0.3, 0.2), (-3.0, 4.0)]
        for d in shifts:
            ptyp.append(typ[s]); pshape.append(shape[s].copy()); pcounts.append(counts[s]); own.append(s)
            pu.append(synth.pixel2equa(bands[0], pix[s:s + 1] + np.array([d]))[0])
        if typ[s] > 0:
            for j, f in enumerate(((0.1, 1.0), (0.0, 1.3), (20.0, 1.0), (0.0, 0.8)) if typ[s] == 1 else ((0.1, 1.0), (0.0, 1.2), (0.0, 0.8), (0.0, 1.2))):
                sh = shape[s].copy()
                sh[j] = (sh[j] + f[0]) * f[1]
                ptyp.append(typ[s]); pshape.append(sh); pcounts.append(counts[s]); own.append(s); pu.append(radec[s])
    ptyp, pu, pshape, pcounts, own = np.array(ptyp, np.int32), np.array(pu), np.array(pshape), np.array(pcounts), np.array(own, np.int32)
    prop = cel.SourceSet(ctx, len(own), NBB).set(ptyp, pu, pcounts, pshape)
    reps = DEAL_MAX // (len(own) * NBB) + 1
    assert len(own) * NBB <= DEAL_MAX < reps * len(own) * NBB
    prop_big = cel.SourceSet(ctx, reps * len(own), NBB).set(np.tile(ptyp, reps), np.tile(pu, (reps, 1)), np.tile(pcounts, (reps, 1)),
                                                            np.tile(pshape, (reps, 1)))
    prefs = [ListRef(orc, bands, ptyp[p], pu[p], pshape[p], pcounts[p]) for p in range(len(own))]
    first = [int(np.nonzero(own == s)[0][0]) for s in range(S)]
    ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    try:
        for lists in (1, 2):
            ctx.set_option(L.CEL_OPT_PHOTON_LISTS, lists)
            iset.photon_split_resident(srcs, seed=11)
            # the reference call holds every proposal `reps` times, more than DEAL_MAX (proposal, band) jobs: k_patch_ll_hw<0>
            # takes each as a whole job.  The proposals once, and calls of <= 7, stay below DEAL_MAX: every dense job is dealt
            # to four blocks there.  All must give the same bits.
            big = iset.patch_loglik_resident(prop_big, np.tile(own, reps)).reshape(reps, len(own))
            got = big[0]
            assert np.array_equal(big, np.tile(got, (reps, 1))), (lists, "equal proposals of one call differ")
            assert np.array_equal(iset.patch_loglik_resident(prop, own), got), (lists, "dealt and whole jobs differ")
            for lo in range(0, S, 5):
                sel = np.array(first[lo:lo + 5])
                few = cel.SourceSet(ctx, len(sel), NBB).set(ptyp[sel], pu[sel], pcounts[sel], pshape[sel])
                assert np.array_equal(iset.patch_loglik_resident(few, own[sel]), got[sel]), (lists, lo, "dealt and whole jobs differ")
            fb, offs, data = iset.fetch_samples()
            photons = {}
            for s in range(S):
                for b in range(NBB):
                    y0, y1, x0, x1 = fb[s, b]
                    assert (y0, y1, x0, x1) == tuple(boxes[b, s])
                    z = data[offs[s * NBB + b]:offs[s * NBB + b + 1]].reshape(y1 - y0, x1 - x0)
                    yy, xx = np.nonzero(z)
                    photons[(s, b)] = (yy + y0, xx + x0, z[yy, xx])
                    assert len(yy) <= 64                        # a handful of photons per patch: the value resolves per photon
            for (s, b, y, x), kind in lit.items():
                y0, y1, x0, x1 = fb[s, b]
                z = data[offs[s * NBB + b]:offs[s * NBB + b + 1]].reshape(y1 - y0, x1 - x0)
                assert z[y - y0, x - x0] >= 1, "no photon of %s on its lit %s pixel (band %d, y %d, x %d)" % (names[s], kind, b, y, x)
            worst = -np.inf
            for p in range(len(own)):
                r = prefs[p]
                want, tol, mmin = r.value([photons[(int(own[p]), b)] for b in range(NBB)], lists == 1)
                assert mmin >= M_MIN, (names[own[p]], p, mmin)
                ratio = abs(got[p] - want) / tol
                worst = max(worst, ratio)
                assert ratio <= 1.0, "lists=%d proposal %d of %s (type %d, shape %s): %.17g, exact %.17g, tol %.3g (ratio %.3g)" % (
                    lists, p - first[own[p]], names[own[p]], ptyp[p], pshape[p], got[p], want, tol, ratio)
            _note("k_patch_ll_nz" if lists == 1 else "k_patch_ll_hw<0> photon rect", 0, 32, worst)
    finally:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 0)
        ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
