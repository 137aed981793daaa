"""The flux step's Gamma variates on the device against the exact law, decision by decision.

Every flux of every sweep is Gamma(a0 + photons) / (b0 + rate), the variate from gamma_stream_draw (k_slice.h): Marsaglia & Tsang
on two SplitMix64 streams per element, reached through cel_gamma_streams and cel_flux_conditionals.  Four things are held here.

1. The law, by regime of the shape a (decades from 0.05 to 1e7, the points 1, the double below 1, 1/3 and 5, and a block of
   shapes log-uniform over the whole range): N_LAW draws per regime, and on them the chi^2 of the PIT gammainc(a, x) over 256
   bins, z of sum (x - a) [variance a], z of sum (log x - digamma(a)) [variance trigamma(a)], z of sum ((x - a)^2 - a), and the
   binomial z of the count of PITs below 1e-4 and above 1 - 1e-4.  The variance of (x - a)^2 - a is mu_4 - a^2 = 2 a^2 + 6 a
   (the fourth central moment of Gamma(a) is 3 a^2 + 6 a, the squared second is a^2): the smaller, correct variance is used.
   Every |z| <= 5.  gammainc itself is held to mpmath's regularised incomplete gamma at 50 digits to 1e-12 absolute on a grid
   over all regimes (a = 1e7 and x within +-6 sd included).  scipy 1.15 meets that except in one corner, a > 200 with x more
   than 4.5 sd below a, where it is wrong by up to 8e-8 at a = 1e7 (scipy_corner): the few draws per million that lie there
   get their PIT from mpmath.  The upper tail is counted through gammaincc, which does not cancel.
2. The decisions.  The sampler is restated below (SplitMix64 in numpy.uint64; the products the kernel rounds to double rounded
   the same way, which IEEE fixes; log, cos, pow and every acceptance margin in numpy.longdouble, mpmath where a margin is small).
   It shares no code with the library.  For every element it gives the value, the number of rejections, and the smallest
   margin |u - (1 - 0.0331 x^4)|, |log u - (x^2/2 + d (1 - v + log v))|, |1 + c x| over the decisions the element took.  An
   element whose smallest margin is above 1e-9 equals the device's draw to 1e-12 relative, without exception; at most a 1e-6
   share of the elements may have a smaller margin (a condition on the inputs, met by the seeds below on the restatement alone:
   none of their elements has one; the expected share is ~1e-8).  The margin of the decision v > 0 is taken in t = 1 + c x,
   whose sign it is and in which the kernel's rounding error is ~1e-16, not in v = t^3: |v| <= 1e-9 is |t| <= 1e-3, which a
   1.2e-5 share of shapes log-uniform over the range meets (measured on the restatement; ~5e-5 per proposal below a = 2), so
   that with |v| no choice of seeds keeps to the cap and thousands of decisions that are nowhere near their boundary would be
   excused.  Every element this rule excuses the |v| rule excuses too.  A constant that is off by a little moves decisions,
   not moments: this is the part that sees it.
3. Independence, on the normal scores ndtri(PIT): neighbouring elements, the five letters of one source, seed and seed + 1,
   consecutive sweeps' flux seeds, the flux seed against the location seed of the same sweep (the Gamma draws under both, and
   the draw against the first uniform of the slice chain that shares its index), an 8 x 8 table of neighbouring PITs, and the
   draw against the number of rejections it took -- not zero by construction, so compared with what the same restatement
   gives on numpy's generator.
4. k_flux_step end to end on a crowded field (stars and galaxies on 256^2, some off the frame), band letters [0,1,2,3,4] and
   [2,2,4], a0 = 5 and 0.3: a_n from cel_samples_fetch's sums, the rate from the ORACLE's unit-stamp masses (not cel_stamp_mass)
   with the header's rule for a band without a patch, the PIT of flux_new (b0 + rate) under Gamma(a_n) over many seeds through
   the statistics of part 1; exactly: letters without an image are Gamma(a0) / b0 of the restated sampler, inactive sources keep
   their counts in the device catalogue bit for bit, active ones hold fnew / calib * kappa.  The library's masses (shipping
   thresholds) enter the draw, the oracle's the PIT: a relative difference delta moves the mean statistic by
   sum(delta a_n) / sqrt(sum a_n) per seed, which the test bounds at 0.01 sigma over all its seeds (measured delta: see the
   printed report; the documented agreement is 1e-10) -- far below what 5 sigma could see, so the strict threshold is not needed.

Also here: ModelGibbs.resample_fluxes leaves the device catalogue equal to the chain's state when fluxes were edited on the host
(the record of what the device holds is brought up to date for the rows the kernel rewrote, no others).

Seeds are fixed: a run is deterministic.  The statistics' calibration (numpy's exact sampler passes at the same N and regimes; a
boost exponent 1 / (a + 1) and neighbours sharing their normal fail) needs no GPU; every other test is marked gpu.

Run time on one MI355X box, same session: this module 86 s (30 s of it the two tests that need no GPU), tests/test_split_law.py
59 s.  Nearly all of it is host-side scipy and longdouble arithmetic.
"""
import numpy as np
import pytest

Z_MAX = 5.0
N_LAW = 2000000
PIT_BINS = 256
TAIL = 1e-4
MARGIN = 1e-9                 # a decision closer to its boundary than this may fall either way in double arithmetic
MARGIN_SHARE = 1e-6           # ... and at most this share of the elements may hold one
VALUE_RTOL = 1e-12
A_MIN, A_MAX = 0.05, 1e7      # the shapes the header vouches for
REGIMES = ([("a=%g" % a, a) for a in (0.05, 0.1, 0.5, 10.0, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7)] +
           [("a=1", 1.0), ("a=1-ulp", float(np.nextafter(1.0, 0.0))), ("a=1/3", 1.0 / 3.0), ("a=5", 5.0), ("loguniform", None)])
STATS = ("pit chi2", "mean", "log mean", "square", "tail low", "tail high")
REPORT = {}

_M1, _M2, _M3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_KEY_MUL, _NKEY_XOR = np.uint64(0xD1342543DE82EF95), np.uint64(0xA0761D6478BD642F)
LD = np.longdouble


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
    if REPORT:
        print("\nflux law statistics (z-scores; counts where named so):")
        for k in sorted(REPORT):
            print("  %-34s %-30s %11.4g" % (k[0], k[1], REPORT[k]))


# ---------------------------------------------------------------------------------------------------------------------
# the statistics (parts 1 and 3): plain functions of draws and shapes, used on the device's draws and on numpy's alike
def loguniform_shapes(n, seed):
    return np.exp(np.random.RandomState(seed).uniform(np.log(A_MIN), np.log(A_MAX), n))


def mp_lower(a, x):
    """P(X <= x) under Gamma(a) by mpmath at 50 digits: gammainc(a, 0, x, regularized=True), and where its series stops short
    (large a) the same series, x^a e^-x / Gamma(a + 1) 1F1(1; a + 1; x), allowed the terms it needs"""
    import mpmath
    with mpmath.workdps(50):
        am, xm = mpmath.mpf(float(a)), mpmath.mpf(float(x))
        try:
            return mpmath.gammainc(am, 0, xm, regularized=True)
        except mpmath.libmp.NoConvergence:
            return mpmath.exp(am * mpmath.log(xm) - xm - mpmath.loggamma(am + 1)) * mpmath.hyp1f1(1, am + 1, xm, maxterms=10 ** 7)


def scipy_corner(a, x):
    """where scipy's gammainc is not good to 1e-12: a > 200 and x more than 4.5 sd below a, where it leaves its uniform
    expansion for a series of at most 2000 terms -- from a ~ 7e5 on the error passes 1e-12 and reaches 8e-8 at a = 1e7 (4 % of
    a PIT of 2e-6).  A few draws per million lie there."""
    return (a > 200.0) & (x < a - 4.5 * np.sqrt(a))


def pit(x, a):
    """(P(X <= x), P(X > x)) under Gamma(a): scipy's two functions, neither cancels; mpmath in scipy's inaccurate corner"""
    from scipy import special
    x, a = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(a, dtype=np.float64))
    p, q = special.gammainc(a, x), special.gammaincc(a, x)
    for i in zip(*np.nonzero(scipy_corner(a, x))):
        r = mp_lower(a[i], x[i])
        p[i], q[i] = float(r), float(1 - r)
    return p, q


def law_stats(x, a):
    """-> {statistic: z} of draws x against Gamma(a), a scalar or one shape per draw"""
    from scipy import special
    x = np.asarray(x, dtype=np.float64)
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), x.shape)
    n = x.size
    p, q = pit(x, a)
    h = np.bincount(np.minimum((p * PIT_BINS).astype(np.int64), PIT_BINS - 1), minlength=PIT_BINS)
    E = n / float(PIT_BINS)
    out = {"pit chi2": (((h - E) ** 2 / E).sum() - (PIT_BINS - 1)) / np.sqrt(2.0 * (PIT_BINS - 1))}
    out["mean"] = np.sum(x - a) / np.sqrt(np.sum(a))
    out["log mean"] = np.sum(np.log(x) - special.digamma(a)) / np.sqrt(np.sum(special.polygamma(1, a)))
    out["square"] = np.sum((x - a) ** 2 - a) / np.sqrt(np.sum(2.0 * a * a + 6.0 * a))
    sd = np.sqrt(n * TAIL * (1.0 - TAIL))
    out["tail low"] = (np.count_nonzero(p < TAIL) - n * TAIL) / sd
    out["tail high"] = (np.count_nonzero(q < TAIL) - n * TAIL) / sd
    return out


def scores(x, a):
    """the normal scores of the PITs, through whichever tail is the smaller"""
    from scipy import special
    p, q = pit(np.asarray(x, dtype=np.float64), a)
    tiny = 1e-300
    return np.where(p < 0.5, special.ndtri(np.maximum(p, tiny)), -special.ndtri(np.maximum(q, tiny)))


def corr_z(s, t):
    """z of the correlation of two sets of standard normal scores: sum s t has variance n when they are independent"""
    return float(np.sum(s * t) / np.sqrt(s.size))


def adjacent_z(s):
    return corr_z(s[:-1], s[1:])          # (neighbouring products share one factor: still uncorrelated under independence)


def letter_pairs_z(s):
    """z of every pair of letters of one source: elements s * 5 + L and s * 5 + L'"""
    t = s[:s.size // 5 * 5].reshape(-1, 5)
    return dict((("letters %d,%d" % (i, j)), corr_z(t[:, i], t[:, j])) for i in range(5) for j in range(i + 1, 5))


def table_z(x, a, k=8):
    """chi^2 of the k x k table of the PITs of elements (2 i, 2 i + 1), as z over its k^2 - 1 degrees of freedom"""
    p = pit(np.asarray(x, dtype=np.float64), a)[0]
    c = np.minimum((p * k).astype(np.int64), k - 1)
    m = c.size // 2 * 2
    h = np.bincount(c[0:m:2] * k + c[1:m:2], minlength=k * k)
    E = (m // 2) / float(k * k)
    return float((((h - E) ** 2 / E).sum() - (k * k - 1)) / np.sqrt(2.0 * (k * k - 1)))


def reject_slope(s, nrej):
    """(mean of score * centred rejection count, its variance): the draw against the rejections it took"""
    w = s * (nrej - nrej.mean())
    return float(w.mean()), float(w.var() / w.size)


def hold(name, zs):
    for k, v in zs.items():
        REPORT[(name, k)] = float(v)
    bad = dict((k, float(v)) for k, v in zs.items() if not abs(v) <= Z_MAX)
    assert not bad, "%s: %s" % (name, bad)


def worst(zs):
    return max(abs(float(v)) for v in zs.values())


# ---------------------------------------------------------------------------------------------------------------------
# the sampler restated (part 2)
def _mix(x):
    """SplitMix64's step on uint64 arrays"""
    with np.errstate(over="ignore"):
        x = x + _M1
        z = (x ^ (x >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        return z ^ (z >> np.uint64(31))


def _unit(key, count):
    """the count-th uniform of the stream `key`: 53 bits, centred -- every step exact or IEEE-rounded, so float64 is the kernel's"""
    with np.errstate(over="ignore"):
        z = _mix(key + count * _M1)
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


class SplitMixSource(object):
    """the kernel's streams of elements `ids` under `seed`: uniforms on key, pairs for Box-Muller on nkey"""

    def __init__(self, seed, ids):
        with np.errstate(over="ignore"):
            self.key = _mix(np.uint64(int(seed) & (2 ** 64 - 1)) ^ (np.asarray(ids).astype(np.uint64) * _KEY_MUL))
        self.nkey = _mix(self.key ^ _NKEY_XOR)
        self.cnt = np.zeros(self.key.shape, np.uint64)
        self.ncnt = np.zeros(self.key.shape, np.uint64)

    def normal(self, idx):
        u1 = _unit(self.nkey[idx], self.ncnt[idx])
        u2 = _unit(self.nkey[idx], self.ncnt[idx] + np.uint64(1))
        self.ncnt[idx] += np.uint64(2)
        ang = 2.0 * 3.14159265358979323846 * u2                     # the kernel's product, rounded to double as it rounds it
        return np.sqrt(LD(-2.0) * np.log(u1.astype(LD))) * np.cos(ang.astype(LD))

    def uniform(self, idx):
        u = _unit(self.key[idx], self.cnt[idx])
        self.cnt[idx] += np.uint64(1)
        return u


class NumpySource(object):
    """numpy's generator in the same role: what the rejection statistic is compared with"""

    def __init__(self, seed):
        self.g = np.random.Generator(np.random.PCG64(seed))

    def normal(self, idx):
        return self.g.standard_normal(idx.size).astype(LD)

    def uniform(self, idx):
        return self.g.random(idx.size)


def _mp_margins(x, u, d):
    """the three margins of one proposal at 50 digits: 1 + c x, the squeeze's, the full test's"""
    import mpmath
    with mpmath.workdps(50):
        x, u, d = mpmath.mpf(float(x)) + mpmath.mpf(float(x - LD(float(x)))), mpmath.mpf(float(u)), mpmath.mpf(float(d))
        c = mpmath.mpf(float(1.0 / np.sqrt(9.0 * np.float64(d))))
        v = (1 + c * x) ** 3
        m1 = u - (1 - mpmath.mpf("0.0331") * x ** 4)
        m2 = mpmath.log(u) - (x * x / 2 + d * (1 - v + mpmath.log(v))) if v > 0 else mpmath.mpf(1)
        return float(1 + c * x), float(m1), float(m2)


def restated_gamma(a, src):
    """Marsaglia & Tsang (2000) with the squeeze, a < 1 through Gamma(a + 1) U^(1/a), on the streams of `src`
    -> (value[n] float64, rejections[n], smallest margin[n] over the decisions taken)"""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    boost = a < 1.0
    aa = np.where(boost, a + 1.0, a)
    d = aa - 1.0 / 3.0                      # double, as the kernel forms them (IEEE: the same bits)
    c = 1.0 / np.sqrt(9.0 * d)
    val = np.zeros(n, LD)
    nrej = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    todo = np.arange(n)
    for _ in range(1000):
        if not todo.size:
            break
        x = src.normal(todo)
        u = src.uniform(todo)
        dl, cl = d[todo].astype(LD), c[todo].astype(LD)
        t = LD(1.0) + cl * x
        v = t * t * t
        x2 = x * x
        m1 = u.astype(LD) - (LD(1.0) - LD(0.0331) * x2 * x2)
        pos = v > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            m2 = np.where(pos, np.log(u.astype(LD)) - (x2 / 2 + dl * (LD(1.0) - v + np.log(np.where(pos, v, LD(1.0))))), LD(1.0))
        m_v, m_1, m_2 = np.abs(t).astype(np.float64), np.abs(m1).astype(np.float64), np.abs(m2).astype(np.float64)
        for j in np.nonzero(np.minimum(m_v, np.minimum(m_1, m_2)) < 1e-7)[0]:          # longdouble is good to ~1e-12 here: decide at 50 digits
            ev, e1, e2 = _mp_margins(x[j], u[j], d[todo[j]])
            pos[j], m_v[j], m_1[j], m_2[j] = ev > 0, abs(ev), abs(e1), abs(e2)
            m1[j], m2[j] = e1, e2
        squeeze = pos & (m1 < 0)
        ok = squeeze | (pos & (m2 < 0))
        # the decisions this proposal took: v > 0 (the sign of t), the squeeze (when v > 0), the full test (when the squeeze did not accept)
        m = np.where(pos, np.where(squeeze, np.minimum(m_v, m_1), np.minimum(m_v, np.minimum(m_1, m_2))), m_v)
        margin[todo] = np.minimum(margin[todo], m)
        val[todo[ok]] = dl[ok] * v[ok]
        nrej[todo[~ok]] += 1
        todo = todo[~ok]
    assert not todo.size
    if boost.any():
        idx = np.nonzero(boost)[0]
        u = src.uniform(idx)
        val[idx] *= np.power(u.astype(LD), (1.0 / a[idx]).astype(LD))            # (1 / a in double, as the kernel forms it)
    return val.astype(np.float64), nrej, margin


def assert_explained(dev, a, seed, what, ids=None):
    """every element equals the restatement to VALUE_RTOL unless one of its decisions lay within MARGIN of its boundary, and at
    most a MARGIN_SHARE share of the elements does -> (mismatches explained by a margin, elements with a small margin)"""
    a = np.asarray(a, dtype=np.float64)
    ids = np.arange(a.size) if ids is None else ids
    val, nrej, margin = restated_gamma(a, SplitMixSource(seed, ids))
    small = margin <= MARGIN
    assert small.sum() <= MARGIN_SHARE * a.size, "%s: %d of %d elements within %g of a decision boundary" % (what, small.sum(), a.size, MARGIN)
    close = np.abs(dev - val) <= VALUE_RTOL * np.abs(val)
    bad = np.nonzero(~close & ~small)[0]
    assert bad.size == 0, "%s: %d unexplained mismatches, first %s" % (
        what, bad.size, [(int(i), float(a[i]), float(dev[i]), float(val[i]), float(margin[i]), int(nrej[i])) for i in bad[:5]])
    REPORT[(what, "elements")] = a.size
    REPORT[(what, "small margins (count)")] = int(small.sum())
    REPORT[(what, "mismatches explained (count)")] = int(np.count_nonzero(~close))
    return int(np.count_nonzero(~close)), int(small.sum()), (val, nrej, margin)


# ---------------------------------------------------------------------------------------------------------------------
# part 6: the statistics on numpy's exact sampler, and on two wrong ones (no GPU)
def regime_shapes(name, a, seed):
    return loguniform_shapes(N_LAW, seed) if a is None else np.full(N_LAW, a)


def test_gammainc_agrees_with_mpmath():
    """the PIT this module uses (scipy's regularised incomplete gamma, both tails; mpmath inside scipy_corner) against
    mpmath.gammainc(..., regularized=True) at 50 digits to 1e-12 absolute: every regime's shape with x at the mean +- 0 .. 6 sd
    and near the 1e-6 .. 1 - 1e-4 quantiles, a = 1e7 included; and scipy alone is that good everywhere outside the corner"""
    from scipy import special
    pts = []
    shapes = [a for _, a in REGIMES if a is not None] + list(loguniform_shapes(12, 3)) + [201.0, 3e5, 7e5, 3e6]
    for a in shapes:
        sd = np.sqrt(a)
        for k in (-6, -5, -4.6, -4.4, -4, -3, -2, -1, -0.5, 0, 0.5, 1, 2, 3, 4, 4.4, 4.6, 5, 6):
            if a + k * sd > 0:
                pts.append((a, a + k * sd))
        for p in (1e-6, 1e-4, 1e-2, 0.3, 0.9, 1 - 1e-4):               # where small shapes put their mass: far below the mean
            pts.append((a, float(special.gammaincinv(a, p)) * 1.0001))
    assert len(pts) >= 300
    A, X = np.array(pts).T
    P, Q = pit(X, A)
    corner = scipy_corner(A, X)
    assert 10 <= corner.sum() <= len(pts) // 4
    ref = [mp_lower(a, x) for a, x in pts]
    err_p = np.abs(P - np.array([float(r) for r in ref]))
    err_q = np.abs(Q - np.array([float(1 - r) for r in ref]))              # (50 digits: the difference keeps 40 of them here)
    raw = np.abs(special.gammainc(A, X) - np.array([float(r) for r in ref]))
    REPORT[("gammainc vs mpmath", "max abs error, lower")] = err_p.max()
    REPORT[("gammainc vs mpmath", "max abs error, upper")] = err_q.max()
    REPORT[("gammainc vs mpmath", "scipy alone, in its corner")] = raw[corner].max()
    assert err_p.max() <= 1e-12 and err_q.max() <= 1e-12, (err_p.max(), err_q.max())
    assert raw[~corner].max() <= 1e-12, raw[~corner].max()


def test_statistics_calibrated_on_numpy():
    """numpy's standard_gamma meets every bound at the same N and regimes; the same functions see a boost exponent 1 / (a + 1)
    and neighbours that share their normal; the restatement on numpy's generator meets the law as well"""
    g = np.random.Generator(np.random.PCG64(20260))
    for k, (name, a0) in enumerate(REGIMES):
        a = regime_shapes(name, a0, 100 + k)
        hold("numpy " + name, law_stats(g.standard_gamma(a), a))
    a = loguniform_shapes(N_LAW, 7)
    x, y = g.standard_gamma(a), g.standard_gamma(a)
    s, t = scores(x, a), scores(y, a)
    ind = {"adjacent": adjacent_z(s), "two draws": corr_z(s, t), "table": table_z(x, a)}
    ind.update(letter_pairs_z(s))
    hold("numpy independence", ind)
    # wrong on purpose, 1: Gamma(a + 1) U^(1 / (a + 1)) below 1
    for a0 in (0.05, 0.5):
        xb = g.standard_gamma(a0 + 1.0, N_LAW) * g.random(N_LAW) ** (1.0 / (a0 + 1.0))
        zs = law_stats(xb, a0)
        assert worst(zs) > Z_MAX and abs(zs["log mean"]) > Z_MAX, zs
    # wrong on purpose, 2: elements 2 i and 2 i + 1 accept the same normal (Marsaglia-Tsang on numpy's streams, no squeeze needed)
    aa = np.full(N_LAW, 7.5)
    d = aa - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    xs = np.zeros(N_LAW)
    todo = np.arange(0, N_LAW, 2)
    while todo.size:
        nrm = g.standard_normal(todo.size)
        v = (1.0 + c[todo] * nrm) ** 3
        ok0, ok1 = [(v > 0) & (np.log(g.random(todo.size)) < 0.5 * nrm * nrm + d[todo] * (1.0 - v + np.log(np.where(v > 0, v, 1.0))))
                    for _ in range(2)]
        ok = ok0 & ok1
        xs[todo[ok]] = xs[todo[ok] + 1] = d[todo][ok] * v[ok]
        todo = todo[~ok]
    ss = scores(xs, aa)
    assert abs(adjacent_z(ss)) > Z_MAX and abs(table_z(xs, aa)) > Z_MAX, (adjacent_z(ss), table_z(xs, aa))
    # the restatement on numpy's generator is a Gamma sampler too (what the rejection statistic of part 3 is compared with)
    ar = loguniform_shapes(200000, 9)
    val, nrej, margin = restated_gamma(ar, NumpySource(5))
    hold("restated on numpy", dict((k, v) for k, v in law_stats(val, ar).items() if not k.startswith("tail")))
    assert 0.002 < nrej.mean() < 0.05, nrej.mean()          # (a few per cent at a ~ 1, a few per mille at large a)


# ---------------------------------------------------------------------------------------------------------------------
# parts 1-3 on the device
LAW_SEED = 424200


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(REGIMES)), ids=[n for n, _ in REGIMES])
def test_gamma_streams_follow_the_law(cel, k):
    name, a0 = REGIMES[k]
    ctx = cel.default_context(0)
    a = regime_shapes(name, a0, 300 + k)
    x = ctx.gamma_streams(a, LAW_SEED + k)
    assert np.all(np.isfinite(x)) and np.all(x > 0)
    zs = law_stats(x, a)
    s = scores(x, a)
    zs["adjacent"] = adjacent_z(s)
    zs["table"] = table_z(x, a)
    zs.update(letter_pairs_z(s))
    hold("device " + name, zs)


@pytest.mark.gpu
def test_shapes_below_the_vouched_range(cel):
    """a < 0.05 (u^(1/a) underflows to 0 more and more often): what the header promises -- finite, >= 0 and the host form's value
    (to 1e-12 relative; a denormal carries fewer bits, so a few of its 4.9e-324 steps besides). No more than that."""
    from desi_mcmc_amd.celeste_mcmc import gamma_by_stream
    ctx = cel.default_context(0)
    a = np.concatenate([np.exp(np.random.RandomState(2).uniform(np.log(1e-4), np.log(0.05), 50000)), [1e-3, 1e-4, 0.049999]])
    for seed in (5, 2 ** 63 + 99):
        dev = ctx.gamma_streams(a, seed)
        host = gamma_by_stream(a, seed, np.arange(a.size))
        assert np.all(np.isfinite(dev)) and np.all(dev >= 0)
        assert np.all(np.abs(dev - host) <= VALUE_RTOL * np.abs(host) + 4 * 4.9406564584124654e-324)


N_DEC = 1000000
DEC_SEEDS = (11, 2 ** 63 + 12345)


def decision_shapes():
    return np.concatenate([loguniform_shapes(N_DEC // 2 - 4, 41), [1.0, float(np.nextafter(1.0, 0.0)), 1.0 / 3.0, 5.0]])


@pytest.mark.gpu
def test_every_draw_is_the_restated_samplers(cel):
    """part 2, and the rejection statistic of part 3 on the same elements"""
    ctx = cel.default_context(0)
    a = decision_shapes()
    slopes = []
    for seed in DEC_SEEDS:
        dev = ctx.gamma_streams(a, seed)
        _, _, (val, nrej, margin) = assert_explained(dev, a, seed, "decisions seed %d" % (seed % 1000))
        slopes.append(reject_slope(scores(dev, a), nrej))
    ref = []
    for seed in (1, 2):
        val, nrej, _ = restated_gamma(a, NumpySource(seed))
        ref.append(reject_slope(scores(val, a), nrej))
    m_dev, v_dev = np.mean([s[0] for s in slopes]), np.sum([s[1] for s in slopes]) / len(slopes) ** 2
    m_ref, v_ref = np.mean([s[0] for s in ref]), np.sum([s[1] for s in ref]) / len(ref) ** 2
    REPORT[("rejections", "slope, device streams")] = m_dev
    REPORT[("rejections", "slope, numpy streams")] = m_ref
    hold("rejections", {"draw against its rejections, device - numpy": (m_dev - m_ref) / np.sqrt(v_dev + v_ref)})


@pytest.mark.gpu
def test_streams_of_different_seeds_are_unrelated(cel):
    """part 3 across seeds: seed and seed + 1, the flux seeds of sweeps k and k + 1, the flux and the location seed of sweep k"""
    from desi_mcmc_amd.celeste_mcmc import step_seed
    from scipy import special
    ctx = cel.default_context(0)
    a = loguniform_shapes(N_LAW, 77)
    chain, k = 20260, 3

    def draw(seed):
        return scores(ctx.gamma_streams(a, seed), a)

    s0, s1 = draw(LAW_SEED), draw(LAW_SEED + 1)
    f0, f1, l0 = draw(step_seed(chain, "flux", k)), draw(step_seed(chain, "flux", k + 1)), draw(step_seed(chain, "location", k))
    # the slice chain of source i keys its stream as the Gamma element i does: its first uniforms, under the location seed
    loc = SplitMixSource(step_seed(chain, "location", k), np.arange(N_LAW))
    idx = np.arange(N_LAW)
    c0, c1 = special.ndtri(loc.uniform(idx)), special.ndtri(loc.uniform(idx))
    hold("seeds", {"seed, seed + 1": corr_z(s0, s1), "flux k, k + 1": corr_z(f0, f1), "flux k, location k": corr_z(f0, l0),
                   "flux k, slice chain's 1st uniform": corr_z(f0, c0), "flux k, slice chain's 2nd uniform": corr_z(f0, c1),
                   "seed, seed + 1, next element": corr_z(s0[:-1], s1[1:])})


# ---------------------------------------------------------------------------------------------------------------------
# part 4: k_flux_step end to end
FH = FW = 256
FS = 600
F_OFF = (7, 311)             # sources moved off the frame: no patch anywhere, inactive
B0 = 0.005
N_SPLITS = 4


class FluxField(object):
    """a crowded field of stars and galaxies with images of the given band letters, and the oracle's unit-stamp masses"""

    def __init__(self, cel, orc, letters):
        from desi_mcmc_amd import synth
        self.letters = list(letters)
        B = self.B = len(letters)
        bands = np.stack([synth.make_bands(FH, FW, 5)[L] for L in letters])
        self.lib_bands = bands.copy()
        src = synth.make_sources(FS, FH, FW, synth.make_bands(FH, FW, 5), frac_gal=0.5, seed=23)
        self.typ, self.shape = src["type"], src["shape"]
        self.radec = src["radec"].copy()
        self.radec[list(F_OFF)] = synth.pixel2equa(bands[0], np.array([[5000.0, 40.0], [-3000.0, 9000.0]]))
        flux = src["flux"][:, self.letters]
        flux[::7] *= 30.0                                   # some bright ones: shapes up to ~1e6
        flux[3::11] *= 3e-4                                 # and faint ones: a_n = a0 + 0 or 1
        self.calib, self.kappa = bands[:, 2].copy(), bands[:, 1].copy()
        self.counts = flux / self.calib[None, :] * self.kappa[None, :]
        ctx = self.ctx = cel.default_context(0)
        self.images = cel.ImageSet(ctx, self.lib_bands, FH, FW)
        self.sources = cel.SourceSet(ctx, FS, B).set(self.typ, self.radec, self.counts, self.shape)
        self.images.render(self.sources)
        self.nelec = np.random.RandomState(24).poisson(self.images.model_images()).astype(np.float64)
        self.images.set_nelec(self.nelec)
        obands = bands.copy()
        for b in range(B):
            obands[b, 36] = orc.checked_radius(self.lib_bands[b], self.images.band(b)[36])
        self.mass = orc.estep_stats(obands, FH, FW, self.typ, self.radec, self.counts, self.shape, self.nelec)[1]

    def reset(self):
        self.sources.set(self.typ, self.radec, self.counts, self.shape)
        return self.sources


@pytest.mark.gpu
@pytest.mark.parametrize("a0", [5.0, 0.3])
@pytest.mark.parametrize("letters", [[0, 1, 2, 3, 4], [2, 2, 4]], ids=["ugriz", "rrz"])
def test_flux_step_end_to_end(cel, orc, letters, a0):
    fld = FluxField(cel, orc, letters)
    B, im = fld.B, fld.images
    name = "flux step %s a0=%g" % ("".join("ugriz"[L] for L in letters), a0)
    absent = [L for L in range(5) if L not in letters]
    nseeds = -(-N_LAW // (FS * 5 * N_SPLITS))
    X, A = [], []
    shift_num = shift_den = 0.0
    for k in range(N_SPLITS):
        src = fld.reset()
        im.photon_split_resident(src, 900 + k)
        sums = im.sample_sums()
        has = im.sample_box_areas() > 0
        active = has.any(axis=1)
        assert not active[list(F_OFF)].any() and active.sum() >= FS - 20
        lib_mass = im.stamp_mass(src)
        cnt, rate, lib_rate = np.zeros((FS, 5)), np.zeros((FS, 5)), np.zeros((FS, 5))
        for b, L in enumerate(letters):
            cnt[:, L] += sums[:, b]
            rate[:, L] += fld.mass[:, b] * has[:, b] * (fld.kappa[b] / fld.calib[b])       # no patch in a band: nothing to the rate
            lib_rate[:, L] += lib_mass[:, b] * has[:, b] * (fld.kappa[b] / fld.calib[b])
        a_n = a0 + cnt
        # the library's masses against the oracle's, as the PIT's mean statistic feels them (see the module docstring)
        delta = np.abs(lib_rate - rate) / (B0 + rate)
        for j in range(nseeds):
            seed = 31000 + 1000 * k + j
            new, act = im.flux_conditionals(src, seed, a0, B0, letters, fld.calib, fld.kappa)
            assert np.array_equal(act, active)
            assert np.all(np.isfinite(new)) and np.all(new > 0)
            if j == 0:
                # every element is the restated draw of its a_n over the library's own rate (the masses of this first call are
                # the ones stamp_mass has just returned; later calls sum the stamps again, which agrees to ~1e-10)
                val, _, margin = restated_gamma(a_n.ravel(), SplitMixSource(seed, np.arange(FS * 5)))
                ref = val * (1.0 / (B0 + lib_rate.ravel()))
                okm = margin > MARGIN
                assert (~okm).sum() <= MARGIN_SHARE * okm.size
                assert np.all(np.abs(new.ravel() - ref)[okm] <= VALUE_RTOL * ref[okm])
                again = im.stamp_mass(src)                  # the catalogue has moved: the mass kernel proper, as later calls use it
                for b, L in enumerate(letters):
                    lib_rate[:, L] += (again[:, b] - lib_mass[:, b]) * has[:, b] * (fld.kappa[b] / fld.calib[b])
                delta = np.maximum(delta, np.abs(lib_rate - rate) / (B0 + rate))
                REPORT[(name, "max rel rate error vs oracle, split %d" % k)] = float(delta.max())
                shift_num += nseeds * float(np.sum(delta * a_n))
                shift_den += nseeds * float(a_n.sum())
            if j % 40 == 0:
                got = src.get()[2]
                want = np.where(active[:, None], new[:, letters] / fld.calib[None, :] * fld.kappa[None, :], fld.counts)
                assert np.array_equal(got, want), np.nonzero(got != want)      # inactive rows untouched, active rows fnew / calib * kappa
                ids = (np.arange(FS)[:, None] * 5 + np.array(absent, dtype=np.int64)[None, :]).ravel() if absent else np.zeros(0, np.int64)
                if absent:                                                      # no image of the letter: Gamma(a0) / b0 from its own streams
                    val, _, margin = restated_gamma(np.full(ids.size, a0), SplitMixSource(seed, ids))
                    ref = val * (1.0 / B0)
                    okm = margin > MARGIN
                    assert (~okm).sum() <= MARGIN_SHARE * okm.size
                    assert np.all(np.abs(new[:, absent].ravel() - ref)[okm] <= VALUE_RTOL * ref[okm])
            X.append((new * (B0 + rate)).ravel())
            A.append(a_n.ravel())
    shift = shift_num / np.sqrt(shift_den)              # sum(delta a_n) / sqrt(sum a_n) over every draw of the run
    assert shift <= 0.01, shift
    REPORT[(name, "mean statistic's shift by the mass error (sigma)")] = shift
    X, A = np.concatenate(X), np.concatenate(A)
    assert X.size >= N_LAW and A.min() < 1.0 + a0 and A.max() > 1e4
    zs = law_stats(X, A)
    s = scores(X, A)
    zs["adjacent"] = adjacent_z(s)
    zs.update(letter_pairs_z(s))
    hold(name, zs)
    if absent:                                                                  # the prior's draws alone, as a regime of their own
        sel = np.isin(np.arange(X.size) % 5, absent)
        assert np.all(A[sel] == a0)
        hold(name + " absent letters", law_stats(X[sel], a0))


# ---------------------------------------------------------------------------------------------------------------------
# part 5: the device catalogue after a flux step on fluxes edited on the host
@pytest.mark.gpu
def test_flux_step_leaves_the_device_catalogue_at_the_chains_state(cel):
    """ModelGibbs.resample_fluxes on the device rewrites the active rows of the catalogue; fluxes changed on the host for an
    active and for an inactive source (its box misses every image) before the call must both be on the device after the next
    _sources -- the device catalogue, read back, is g.counts(f), and is what a fresh ModelGibbs at the same state uploads"""
    from desi_mcmc_amd import celeste_mcmc, synth
    ctx = cel.default_context(0)
    S, B = 80, 5
    f0 = synth.SyntheticField(ctx, S, B, 160, 192, frac_gal=0.5, seed=29)
    u = f0.src["radec"].copy()
    off = 13
    u[off] = synth.pixel2equa(f0.bands[0], np.array([[5000.0, 40.0]]))[0]
    letters = [0, 1, 2, 3, 4]

    def chain(fluxes):
        imgs = cel.ImageSet(ctx, f0.bands, f0.H, f0.W, nelec=f0.nelec)
        gf = celeste_mcmc.GibbsField(imgs, letters, f0.bands[:, 2], f0.bands[:, 1], f0.H * f0.W)
        return celeste_mcmc.ModelGibbs([gf], f0.src["type"], u, fluxes, f0.src["shape"], seed=8), gf

    g, f = chain(f0.flux5())
    g.resample_photons()
    assert g._device_flux_applies() and not g.active[off] and g.active[20]
    g.fluxes[20] *= 1.5
    g.fluxes[off] *= 2.0
    changed = g.fluxes[off].copy()
    g.resample_fluxes()
    assert np.array_equal(g.fluxes[off], changed)                      # an inactive source keeps the flux it has
    sset = g._sources(f)
    typ, radec, counts, shape = sset.get()
    assert np.array_equal(counts, g.counts(f)), np.nonzero(counts != g.counts(f))
    assert np.array_equal(typ, g.typ) and np.array_equal(radec, g.u) and np.array_equal(shape, g.shape)
    g2, f2 = chain(g.fluxes)
    fresh = g2._sources(f2).get()
    assert all(np.array_equal(x, y) for x, y in zip(fresh, (typ, radec, counts, shape)))
