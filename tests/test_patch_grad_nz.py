"""The resident mode-8 gradient at the photon lists: CEL_OPT_PHOTON_LISTS = 4 / 5, k_patch_grad_nz.h (pgrad_nz_sums).

  1. identity with the derivative stamps contracted with r = z / m at the listed pixels, options 5 and 4
  2. the two routes against each other (option 1 against 5 on the same split), same bar
  3. the list kernel actually ran: on the longest list the two routes' rows are not the same bits
  4. contract: slot 0, repeatability, one proposal = its batch row, > 8192 jobs, both kernel settings, the type -3 row
  5. fallback (a split without lists), the calls that keep the dense kernel, the option's values
  6. one galaxy and one star under the rotated, per-band WCS of tests/_general_wcs.py
  7. (no GPU) the resource row and the budget

The scene: 2 bands on 96 x 112, sky 1e-30, a frame that is dark except on chosen lit pixels, each with so many counts that by the
exact binomial its source is left without a photon there with probability below 1e-6 -- and any OTHER source whose list length
the test relies on gets one there with a total expectation below 1e-6.  The (source, band) list lengths are then known in advance:
0, 1, 63, 64, 65, one below / at / one above PGNZ_TRIP (the photons of a trip) and PGNZ_DEAL_PHOTONS (the longest list that part 0
takes whole) -- the smallest shapes at which a trip's tail, a trip-class boundary or a part boundary can go wrong.  The big
galaxy's lists are the longest and are not controlled: it collects photons on everybody's pixels.

An owner of -1 cannot reach the kernel through cel_patch_loglik_multi (the call refuses it, pinned by tests/test_patch_grad.py); the
HMC step is what launches the kernel over chains without an owner, and tests/test_hmc_nz.py holds that case.
"""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B = 96, 112, 2
gpu = pytest.mark.gpu
BAR = 1e-10                         # x sum |r plane|: tests/test_patch_grad.py's bar for the same identity

#: name, type, pixel position, shape, counts per band, wanted list length per band (None: not controlled)
SOURCES = [
    ("star", 0, (15.3, 14.2), (0, 0, 0, 0), (8000.0, 12000.0), (63, 64)),
    ("edge star", 0, (2.3, 52.7), (0, 0, 0, 0), (6000.0, 9000.0), (65, 0)),
    ("big galaxy", 1, (60.4, 55.3), (0.5, 2.2, 30.0, 0.6), (40000.0, 50000.0), (None, None)),
    ("floored galaxy", 1, (24.6, 87.1), (0.4, 0.02, 40.0, 0.7), (7000.0, 5000.0), (127, 128)),
    ("type-2 galaxy", 2, (100.1, 19.5), (0.35, 1.2, 0.3, 0.9), (15000.0, 11000.0), (512, 130)),
    ("mid galaxy", 1, (52.5, 16.4), (0.6, 0.5, 120.0, 0.5), (9000.0, 14000.0), (513, 514)),
    ("one-photon star", 0, (99.2, 84.4), (0, 0, 0, 0), (5000.0, 7000.0), (1, 129)),
    ("star off the frame", 0, (-60.0, 50.0), (0, 0, 0, 0), (9000.0, 8000.0), (None, None)),
]
NAMES = [s[0] for s in SOURCES]
S_BIG, S_EDGE, S_STAR, S_OFF = NAMES.index("big galaxy"), NAMES.index("edge star"), NAMES.index("star"), NAMES.index("star off the frame")


def _kernel_constants():
    """(PGNZ_TRIP, PGNZ_DEAL_PHOTONS) as the header defines them"""
    text = open(os.path.join(ROOT, "desi-mcmc_amd", "csrc", "k_patch_grad_nz.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, text).group(1)) for n in ("PGNZ_TRIP", "PGNZ_DEAL_PHOTONS"))


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- the CPU side: component tables, unit stamps, the lit pixels -----------------------------------------------------------------
def _comps(band, typ, radec, shape, orc):
    """(amplitude, mean, covariance) of every component of one source in one band, from the oracle's tables"""
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    if typ == 0:
        v = orc.equa2pixel(band, radec)
        return w.copy(), v[None, :] + mu, cov.copy()
    if typ == 2:
        ea, ev, da, dv = orc.profile_tables()
        amp, var = np.concatenate([ea, da]), np.concatenate([ev, dv])
        pxy = orc.equa2pixel(band, radec)
        Wm = np.array([[shape[1], shape[2]], [shape[2], shape[3]]])
        A, M, Cv = [], [], []
        for j in range(14):
            tf = shape[0] if j < 6 else 1.0 - shape[0]
            for k in range(3):
                A.append(tf * amp[j] * w[k]); M.append(pxy + mu[k]); Cv.append(var[j] * Wm + cov[k])
        return np.array(A), np.array(M), np.array(Cv)
    pis, means, covs, _, _ = orc.galaxy_table(band, shape, radec)
    return pis, means, covs


def _unit_at(comps, ys, xs):
    """the unit stamp at pixels (ys, xs)"""
    X, Y = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    u = np.zeros(X.shape)
    for A, m, Cm in zip(*comps):
        a, b, c = Cm[0, 0], Cm[0, 1], Cm[1, 1]
        det = a * c - b * b
        dx, dy = X - m[0], Y - m[1]
        u += A * np.exp(-(c * dx * dx - 2 * b * dx * dy + a * dy * dy) / det / 2) / (2 * np.pi * np.sqrt(det))
    return u


def make_bands(orc):
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, B)
    bands[:, 0] = 1e-30                                  # a sky so low that a lit pixel gives its photons to the sources
    for b in range(B):
        bands[b, 36] = orc.band_radius(bands[b])
    return bands


def design(orc, bands, boxes, trip, deal):
    """the lit pixels and their counts.  boxes[b, s] = y0, y1, x0, x1 (the sources' own boxes: the split's patches).
    -> (nelec, lit {(s, b): (ys, xs)}, wanted {(s, b): length})"""
    from desi_mcmc_amd import synth
    S = len(SOURCES)
    typ = [s[1] for s in SOURCES]
    pix = np.array([s[2] for s in SOURCES], float)
    radec = synth.pixel2equa(bands[0], pix)
    counts = np.array([s[4] for s in SOURCES])
    comps = [[_comps(bands[b], typ[s], radec[s], SOURCES[s][3], orc) for b in range(B)] for s in range(S)]
    ctrl = [s for s in range(S) if SOURCES[s][5][0] is not None]
    yy, xx = np.mgrid[0:H, 0:W]

    def rates(b, ys, xs):
        """(S, n): every source's rate at the pixels, 0 outside its own box (the split gives a source photons on its box only)"""
        out = np.zeros((S, len(ys)))
        for q in range(S):
            y0, y1, x0, x1 = boxes[b, q]
            ins = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
            if ins.any():
                out[q, ins] = counts[q, b] * _unit_at(comps[q][b], ys[ins], xs[ins])
        return out

    nelec = np.zeros((B, H, W))
    lit, wanted = {}, {}
    stray = 0.0                                          # expected photons of a controlled source on somebody else's lit pixel
    taken = np.zeros((B, H, W), dtype=bool)
    for s in ctrl:
        for b in range(B):
            n = SOURCES[s][5][b]
            wanted[(s, b)] = n
            y0, y1, x0, x1 = boxes[b, s]
            centre = orc.equa2pixel(bands[b], radec[s])
            ins = (yy > y0) & (yy < y1 - 1) & (xx > x0) & (xx < x1 - 1) & ~taken[b]      # the box's interior
            d2 = np.where(ins, (xx - centre[0]) ** 2 + (yy - centre[1]) ** 2, np.inf).ravel()
            pick = np.argsort(d2, kind="stable")[:n]
            assert np.all(np.isfinite(d2[pick])), (NAMES[s], b, "its box holds fewer than %d interior pixels" % n)
            ys, xs = pick // W, pick % W
            lit[(s, b)] = (ys, xs)
            taken[b, ys, xs] = True
            if n == 0:
                continue
            r = rates(b, ys, xs)
            p = r[s] / (r.sum(axis=0) + bands[b, 0])
            assert np.all(p > 1e-3), (NAMES[s], b, float(p.min()))
            # the exact binomial: P(no photon of s among k) = (1 - p)^k < 1e-6
            k = np.where(p >= 1 - 1e-7, 1, np.ceil(math.log(1e-6) / np.log1p(-np.minimum(p, 1 - 1e-7))) + 1)
            assert np.all((1.0 - p) ** k < 1e-6) and k.max() <= 65535
            nelec[b, ys, xs] = k
            for q in ctrl:
                if q != s:
                    stray += float((k * r[q] / (r.sum(axis=0) + bands[b, 0])).sum())
    # the big galaxy: every pixel of its box on which the controlled sources expect next to nothing
    for b in range(B):
        y0, y1, x0, x1 = boxes[b, S_BIG]
        cand = (yy > y0) & (yy < y1 - 1) & (xx > x0) & (xx < x1 - 1) & ~taken[b]
        ys, xs = yy[cand], xx[cand]
        r = rates(b, ys, xs)
        tot = r.sum(axis=0) + bands[b, 0]
        p = r[S_BIG] / tot
        others = r[ctrl].sum(axis=0) / tot
        keep = (p > 0.5) & (others < 1e-13)
        ys, xs, p, others = ys[keep], xs[keep], p[keep], others[keep]
        k = np.ceil(math.log(1e-6) / np.log1p(-np.minimum(p, 1 - 1e-7))) + 1
        assert np.all((1.0 - p) ** k < 1e-6)
        nelec[b, ys, xs] = k
        lit[(S_BIG, b)] = (ys, xs)
        stray += float((k * others).sum())
    assert stray < 1e-6, stray
    return nelec, lit, wanted


# ---- the device side ------------------------------------------------------------------------------------------------------------------
def _proposals(orc, bands):
    """several per source through `owner`: itself, shifts of 1e-3, 0.3 and 5 px, one change of each shape coordinate; a proposal
    displaced to an overlap-test miss (-3), proposals whose own box is empty (-1, -2)"""
    from desi_mcmc_amd import synth
    R = float(np.max(bands[:, 36]))
    ptyp, ppix, pshape, pcounts, own, label = [], [], [], [], [], []
    for s, (name, typ, pix, shape, counts, _) in enumerate(SOURCES):
        for d in ((0.0, 0.0), (1e-3, -1e-3), (0.3, 0.2), (-3.0, 4.0)):
            ptyp.append(typ); ppix.append((pix[0] + d[0], pix[1] + d[1])); pshape.append(list(shape)); pcounts.append(counts); own.append(s)
            label.append("%s shifted by %s" % (name, d))
        if typ > 0:
            for j, f in enumerate(((0.1, 1.0), (0.0, 1.3), (20.0, 1.0), (0.0, 0.8)) if typ == 1 else ((0.1, 1.0), (0.0, 1.2), (0.0, 0.8), (0.0, 1.2))):
                sh = list(shape)
                sh[j] = (sh[j] + f[0]) * f[1]
                ptyp.append(typ); ppix.append(pix); pshape.append(sh); pcounts.append(counts); own.append(s)
                label.append("%s, shape[%d] changed" % (name, j))
    # a galaxy beside the frame whose own box is empty: the nearest such column, found with the oracle
    gshape = [0.6, 0.5, 70.0, 0.8]
    gx = -3.0
    while True:
        u = synth.pixel2equa(bands[0], np.array([[gx, 52.4]]))[0]
        if all(orc.source_patch(bands[b], H, W, 1, u, gshape)[0] is None for b in range(B)):
            break
        gx -= 1.0
    special = [("miss (-3) on the star's patches", 0, (-60.0, 50.0), [0, 0, 0, 0], (9000.0, 8000.0), S_STAR, -3),
               ("star, own box empty (-1), on the edge star's patches", 0, (-(R + 1.2), 52.2), [0, 0, 0, 0], (4e5, 5e5), S_EDGE, -1),
               ("galaxy, own box empty (-2), on the edge star's patches", 1, (gx - 0.3, 52.4), gshape, (3e6, 4e6), S_EDGE, -2)]
    kinds = {}
    for name, typ, pix, shape, counts, o, kind in special:
        kinds[len(own)] = kind
        ptyp.append(typ); ppix.append(pix); pshape.append(shape); pcounts.append(counts); own.append(o); label.append(name)
    radec = synth.pixel2equa(bands[0], np.array(ppix, float))
    # the record kinds of the specials, from the oracle
    for p, kind in kinds.items():
        for b in range(B):
            if ptyp[p] == 0:
                okb, _, bx = orc.star_box(bands[b], H, W, radec[p])
                got = -3 if not okb else (0 if (bx[1] > bx[0] and bx[3] > bx[2]) else -1)
            else:
                got = 1 if orc.source_patch(bands[b], H, W, 1, radec[p], pshape[p])[0] is not None else -2
            assert got == kind, (label[p], b, got)
    return dict(typ=np.array(ptyp, np.int32), radec=radec, shape=np.array(pshape, float), counts=np.array(pcounts, float),
                own=np.array(own, np.int32), label=label, kinds=kinds, P=len(own))


def _flat(res):
    ll, gr, gc, gs = res
    return np.column_stack([ll, gr, gs, gc])              # the library's row: value, ra dec, shape, counts


@pytest.fixture(scope="module")
def dev(cel, orc):
    """the scene, its resident split (made under CEL_OPT_KERNEL 1, photon lists for every patch) and the batch's rows under
    options 1 (dense gradient), 5 and 4 -- computed once and left unchanged"""
    from desi_mcmc_amd import _lib as L, synth
    trip, deal = _kernel_constants()
    assert (trip, deal) == (L.PGNZ_TRIP, L.PGNZ_DEAL_PHOTONS)
    ctx = cel.Context(0)
    bands = make_bands(orc)
    S = len(SOURCES)
    typ = np.array([s[1] for s in SOURCES], np.int32)
    radec = synth.pixel2equa(bands[0], np.array([s[2] for s in SOURCES], float))
    shape = np.array([s[3] for s in SOURCES], float)
    counts = np.array([s[4] for s in SOURCES])
    iset = cel.ImageSet(ctx, bands, H, W)
    srcs = cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape)
    boxes, status = iset.source_boxes(srcs)
    assert np.all(status[:, S_OFF] <= 0) and np.all(np.delete(status, S_OFF, axis=1) > 0)
    y0, y1, x0, x1 = boxes[0, S_BIG]
    assert 70 <= y1 - y0 <= 96 and 80 <= x1 - x0 <= 112, boxes[0, S_BIG]          # "about 80 x 90", cut by nothing but the frame
    assert boxes[0, S_EDGE, 2] == 0                                                # the frame's edge cuts this patch
    nelec, lit, wanted = design(orc, bands, boxes, trip, deal)
    iset.set_nelec(nelec)
    ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 1)
    ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)
    iset.photon_split_resident(srcs, seed=11)
    ctx.set_option(L.CEL_OPT_SPLIT_FULL_BOX, 0)
    fb, offs, data = iset.fetch_samples()
    z = {}
    for s in range(S):
        for b in range(B):
            a0, a1, c0, c1 = fb[s, b]
            z[(s, b)] = data[offs[s * B + b]:offs[s * B + b + 1]].reshape(max(a1 - a0, 0), max(c1 - c0, 0))
    # every lit pixel holds a photon of its source
    for (s, b), (ys, xs) in lit.items():
        a0, a1, c0, c1 = fb[s, b]
        assert tuple(fb[s, b]) == tuple(boxes[b, s])
        assert np.all(z[(s, b)][ys - a0, xs - c0] >= 1), "no photon of %s on one of its lit pixels (band %d)" % (NAMES[s], b)
    length = {k: int(np.count_nonzero(v)) for k, v in z.items()}
    for k, n in wanted.items():
        assert length[k] == n, (NAMES[k[0]], k[1], length[k], n)
    prop = _proposals(orc, bands)
    pset = cel.SourceSet(ctx, prop["P"], B).set(prop["typ"], prop["radec"], prop["counts"], prop["shape"])
    rows = {}
    for opt in (1, 5, 4):
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, opt)
        rows[opt] = _flat(iset.patch_loglik_resident_grad(pset, prop["own"]))
    ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)
    return dict(ctx=ctx, iset=iset, srcs=srcs, bands=bands, nelec=nelec, boxes=boxes, fb=fb, z=z, length=length, prop=prop, pset=pset, rows=rows,
                trip=trip, deal=deal, L=L)


@gpu
def test_the_list_lengths_the_kernel_can_go_wrong_at_occur(dev):
    """0, 1, 63, 64, 65; one below, at and one above the photons of a trip; the longest list part 0 takes whole, and the lengths
    on both sides of it (one below and one above the length from which a list is dealt)"""
    trip, deal = dev["trip"], dev["deal"]
    have = set(dev["length"][(s, b)] for s in range(len(SOURCES)) if s != S_OFF for b in range(B))
    need = {0, 1, 63, 64, 65, trip - 1, trip, trip + 1, deal, deal + 1, deal + 2}
    assert need <= have, sorted(need - have)
    assert min(dev["length"][(S_BIG, b)] for b in range(B)) > deal + 2 * trip


def _identity(iset, pset, prop, bands, boxes_of, z_of, got, label):
    """each entry of slots 1 .. against the derivative stamps on the patch limits contracted with r = z / m at the listed pixels
    by math.fsum, bands in order -> the worst |difference| / sum |r plane|"""
    P = prop["P"]
    sj, uj = [], []
    for b in range(B):
        lim = np.array([boxes_of(p, b) for p in range(P)], dtype=np.int32)
        sj.append(iset.stamp_jacobians(pset, b, scaled=True, boxes_in=lim)[0])
        uj.append(iset.stamp_jacobians(pset, b, scaled=False, boxes_in=lim)[0])
    worst, seen = 0.0, 0
    for p in range(P):
        if prop["kinds"].get(p) == -3:
            continue
        acc, mag = [[] for _ in range(6)], [[] for _ in range(6)]
        for b in range(B):
            if sj[b][p] is None:
                assert got[p, 7 + b] == 0.0                 # no patch in this band
                continue
            u, z, c = uj[b][p][0], z_of(p, b), prop["counts"][p, b]
            yy, xx = np.nonzero(z)                          # the list: exactly the pixels with z != 0
            m = c * u[yy, xx]
            r = np.where(m > 0, z[yy, xx] / np.where(m > 0, m, 1.0), 0.0)
            t = r * u[yy, xx]
            want = math.fsum(t) - float((bands[b, 3] + bands[b, 4]) + bands[b, 5])
            d, mg = abs(got[p, 7 + b] - want), math.fsum(np.abs(t))
            assert d <= BAR * mg, (label, prop["label"][p], "counts", b, got[p, 7 + b], want, mg)
            worst = max(worst, d / mg) if mg > 0 else worst
            for i in range(1, sj[b][p].shape[0]):
                t = r * sj[b][p][i][yy, xx]
                acc[i - 1].append(math.fsum(t)); mag[i - 1].append(math.fsum(np.abs(t)))
            seen += 1
        for i in range(6):
            want, mg = sum(acc[i]), sum(mag[i])
            d = abs(got[p, 1 + i] - want)
            assert d <= BAR * mg, (label, prop["label"][p], i, got[p, 1 + i], want, mg)
            if mg > 0:
                worst = max(worst, d / mg)
        if prop["typ"][p] == 0:
            assert np.all(got[p, 3:7] == 0.0)
    assert np.all(np.isfinite(got))
    return worst, seen


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("opt", [5, 4])
def test_identity_with_the_derivative_stamps_at_the_photons(dev, opt):
    """bar 1e-10 sum |r plane| per entry.  Worst measured ratio: 6.5e-13 under both values."""
    prop = dev["prop"]
    worst, seen = _identity(dev["iset"], dev["pset"], prop, dev["bands"], lambda p, b: dev["boxes"][b, prop["own"][p]],
                            lambda p, b: dev["z"][(int(prop["own"][p]), b)], dev["rows"][opt], "option %d" % opt)
    assert seen >= 2 * (prop["P"] - 8)
    print("option %d: identity at the photons, worst |difference| / sum |r plane| = %.3g over %d (proposal, band) lists" % (opt, worst, seen))


# ---- 2, 3 ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_two_routes_agree_and_differ_in_the_last_bits(dev):
    """option 1 (dense) against 5 (lists) on the same split: within the identity's bar of each other, entry by entry, with
    sum |r plane| from the derivative stamps; the value in slot 0 is the same bits.  And on the longest list the rows are NOT the
    same bits: the routes sum in different orders and take different exponentials -- a build that accepted 5 and ran the dense
    kernel would pass everything else here."""
    prop, iset, pset = dev["prop"], dev["iset"], dev["pset"]
    a, c = dev["rows"][1], dev["rows"][5]
    assert np.array_equal(a[:, 0], c[:, 0])
    mag = np.zeros((prop["P"], 6 + B))
    for b in range(B):
        lim = np.array([dev["boxes"][b, prop["own"][p]] for p in range(prop["P"])], dtype=np.int32)
        sj = iset.stamp_jacobians(pset, b, scaled=True, boxes_in=lim)[0]
        uj = iset.stamp_jacobians(pset, b, scaled=False, boxes_in=lim)[0]
        for p in range(prop["P"]):
            if sj[p] is None or prop["kinds"].get(p) == -3:
                continue
            z = dev["z"][(int(prop["own"][p]), b)]
            yy, xx = np.nonzero(z)
            u = uj[p][0][yy, xx]
            m = prop["counts"][p, b] * u
            r = np.where(m > 0, z[yy, xx] / np.where(m > 0, m, 1.0), 0.0)
            mag[p, 6 + b] = math.fsum(np.abs(r * u))
            for i in range(1, sj[p].shape[0]):
                mag[p, i - 1] += math.fsum(np.abs(r * sj[p][i][yy, xx]))
    d = np.abs(a[:, 1:] - c[:, 1:])
    assert np.all(d <= BAR * mag), np.argwhere(d > BAR * mag)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("dense against lists: worst |difference| / sum |r plane| = %.3g" % np.nanmax(np.where(mag > 0, d / mag, 0.0)))
    p_big = int(np.nonzero(prop["own"] == S_BIG)[0][0])
    assert not np.array_equal(a[p_big, 1:], c[p_big, 1:])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_contract_of_the_list_route(cel, dev):
    L, ctx, iset, pset, prop = dev["L"], dev["ctx"], dev["iset"], dev["pset"], dev["prop"]
    P = prop["P"]
    ref = dev["rows"][5]
    try:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 5)
        # slot 0: the plain mode-0 call, bit for bit; a repeated call: the same bits
        assert np.array_equal(iset.patch_loglik_resident(pset, prop["own"]), ref[:, 0])
        assert np.array_equal(_flat(iset.patch_loglik_resident_grad(pset, prop["own"])), ref)
        # each proposal scored alone = its row in the batch
        for p in range(P):
            one = cel.SourceSet(ctx, 1, B).set(prop["typ"][p:p + 1], prop["radec"][p:p + 1], prop["counts"][p:p + 1], prop["shape"][p:p + 1])
            assert np.array_equal(_flat(iset.patch_loglik_resident_grad(one, prop["own"][p:p + 1]))[0], ref[p]), prop["label"][p]
        # the batch replicated through `owner` past 8192 (proposal, band) jobs
        reps = 8192 // (P * B) + 1
        big = cel.SourceSet(ctx, reps * P, B).set(np.tile(prop["typ"], reps), np.tile(prop["radec"], (reps, 1)),
                                                  np.tile(prop["counts"], (reps, 1)), np.tile(prop["shape"], (reps, 1)))
        out = _flat(iset.patch_loglik_resident_grad(big, np.tile(prop["own"], reps)))
        assert reps * P * B > 8192 and np.array_equal(out, np.tile(ref, (reps, 1)))
        # CEL_OPT_KERNEL at call time (the split was made under 1): slots 1 .. are the same bits
        ctx.set_option(L.CEL_OPT_KERNEL, 0)
        try:
            k0 = _flat(iset.patch_loglik_resident_grad(pset, prop["own"]))
        finally:
            ctx.set_option(L.CEL_OPT_KERNEL, 1)
        assert np.array_equal(k0[:, 1:], ref[:, 1:])
    finally:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)
    # a type -3 row: exactly - wsum_b in the counts entries and 0 elsewhere
    (p3,) = [p for p, k in prop["kinds"].items() if k == -3]
    wsum = np.array([(dev["bands"][b, 3] + dev["bands"][b, 4]) + dev["bands"][b, 5] for b in range(B)])
    assert np.array_equal(ref[p3, 7:], -wsum) and np.all(ref[p3, 1:7] == 0.0)
    # the source without a patch: zeros
    for p in np.nonzero(prop["own"] == S_OFF)[0]:
        assert np.all(ref[p, 1:] == 0.0)
    assert np.all(np.isfinite(ref))
    # the public call refuses an owner of -1 on either route (the HMC step is what runs such jobs: tests/test_hmc_nz.py)
    with pytest.raises(ValueError):
        iset.patch_loglik_resident_grad(pset, np.where(np.arange(P) == 0, -1, prop["own"]).astype(np.int32))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_fallback_without_lists(cel, dev):
    """a split made under option 2 has no lists: option 5 at call time gives the dense route's bits"""
    L, ctx, prop = dev["L"], dev["ctx"], dev["prop"]
    iset = cel.ImageSet(ctx, dev["bands"], H, W)
    iset.set_nelec(dev["nelec"])
    try:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 2)
        iset.photon_split_resident(dev["srcs"], seed=11)
        dense = _flat(iset.patch_loglik_resident_grad(dev["pset"], prop["own"]))
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 5)
        assert np.array_equal(_flat(iset.patch_loglik_resident_grad(dev["pset"], prop["own"])), dense)
    finally:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)


@gpu
def test_calls_that_keep_the_dense_kernel(cel, dev):
    """modes 9 and 10 and the explicit mode 8 under option 5 give the bits they give under option 1"""
    L, ctx, iset, pset, prop = dev["L"], dev["ctx"], dev["iset"], dev["pset"], dev["prop"]
    sel = [int(np.nonzero(prop["own"] == s)[0][1]) for s in range(len(SOURCES)) if s != S_OFF]
    out = {}
    try:
        for opt in (1, 5):
            ctx.set_option(L.CEL_OPT_PHOTON_LISTS, opt)
            few = cel.SourceSet(ctx, len(sel), B).set(prop["typ"][sel], prop["radec"][sel], prop["counts"][sel], prop["shape"][sel])
            boxes = np.array([[dev["boxes"][b, prop["own"][p]] for b in range(B)] for p in sel], dtype=np.int32)
            patches = [[dev["z"][(int(prop["own"][p]), b)] for b in range(B)] for p in sel]
            own = np.arange(len(sel), dtype=np.int32)
            out[opt] = [_flat(iset.patch_loglik_resident_grad(pset, prop["own"], isolated=True))] + \
                       [_flat(iset.patch_loglik_multi_grad(few, own, boxes, patches, mode=m)) for m in (0, 1, 2)]
    finally:
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)
    for a, c in zip(out[1], out[5]):
        assert np.array_equal(a, c)
    # ... and the explicit mode 8 is the dense route's resident rows, as tests/test_patch_grad.py holds it on the default option
    assert np.array_equal(out[5][1][:, 1:], dev["rows"][1][sel, 1:])


@gpu
def test_the_options_values(cel):
    from desi_mcmc_amd import _lib as L
    ctx = cel.Context(0)
    assert ctx.get_option(L.CEL_OPT_PHOTON_LISTS) == 0
    for was in (0, 1, 2, 4, 5):
        ctx.set_option(L.CEL_OPT_PHOTON_LISTS, was)              # (the parent refuses 4 and 5)
        assert ctx.get_option(L.CEL_OPT_PHOTON_LISTS) == was
        for v in (3, 6, 7, 8, -1, 4.5):
            with pytest.raises(ValueError):
                ctx.set_option(L.CEL_OPT_PHOTON_LISTS, v)
            assert ctx.get_option(L.CEL_OPT_PHOTON_LISTS) == was


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_identity_under_the_rotated_per_band_wcs(cel, orc):
    """one galaxy and one star under tests/_general_wcs.py's WCS (3 bands: every band its own): the identity, same bar.  The frame
    here is a Poisson draw of the model itself: the WCS enters the kernel through the records and the chain rule, not the lists."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _general_wcs as G
    from desi_mcmc_amd import _lib as L
    nb = 3
    ctx = cel.Context(0)
    bands = G.general_bands(H, W, nb)
    pix = np.array([[40.3, 50.2], [75.6, 30.4]])
    radec = np.array([G.pixel2equa(bands, 0, p) for p in pix])
    typ = np.array([1, 0], np.int32)
    shape = np.array([[0.45, 1.1, 25.0, 0.55], [0, 0, 0, 0]], float)
    counts = np.array([[30000.0, 25000.0, 20000.0], [9000.0, 8000.0, 7000.0]])
    iset = cel.ImageSet(ctx, bands, H, W)
    srcs = cel.SourceSet(ctx, 2, nb).set(typ, radec, counts, shape)
    iset.render(srcs)
    iset.set_nelec(np.random.RandomState(5).poisson(iset.model_images()).astype(np.float64))
    ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 5)
    iset.photon_split_resident(srcs, seed=3)
    fb, offs, data = iset.fetch_samples()
    # proposals: both sources, moved by 0.3 px and (the galaxy) turned
    d = np.array([G.pixel2equa(bands, 0, p + 0.3) for p in pix])
    sh2 = shape.copy(); sh2[0, 2] += 10.0
    pset = cel.SourceSet(ctx, 2, nb).set(typ, d, counts, sh2)
    own = np.arange(2, dtype=np.int32)
    got = _flat(iset.patch_loglik_resident_grad(pset, own))
    ctx.set_option(L.CEL_OPT_PHOTON_LISTS, 1)
    dense = _flat(iset.patch_loglik_resident_grad(pset, own))
    assert not np.array_equal(got[0, 1:], dense[0, 1:])
    worst = 0.0
    acc = [[[] for _ in range(6)] for _ in range(2)]
    mag = [[[] for _ in range(6)] for _ in range(2)]
    for b in range(nb):
        lim = np.array([fb[p, b] for p in range(2)], dtype=np.int32)
        sj = iset.stamp_jacobians(pset, b, scaled=True, boxes_in=lim)[0]
        uj = iset.stamp_jacobians(pset, b, scaled=False, boxes_in=lim)[0]
        for p in range(2):
            a0, a1, c0, c1 = fb[p, b]
            z = data[offs[p * nb + b]:offs[p * nb + b + 1]].reshape(a1 - a0, c1 - c0)
            yy, xx = np.nonzero(z)
            assert len(yy) > 0
            u = uj[p][0][yy, xx]
            m = counts[p, b] * u
            r = np.where(m > 0, z[yy, xx] / np.where(m > 0, m, 1.0), 0.0)
            t = r * u
            want = math.fsum(t) - float((bands[b, 3] + bands[b, 4]) + bands[b, 5])
            dd, mg = abs(got[p, 7 + b] - want), math.fsum(np.abs(t))
            assert dd <= BAR * mg, (p, b, got[p, 7 + b], want)
            worst = max(worst, dd / mg)
            for i in range(1, sj[p].shape[0]):
                t = r * sj[p][i][yy, xx]
                acc[p][i - 1].append(math.fsum(t)); mag[p][i - 1].append(math.fsum(np.abs(t)))
    for p in range(2):
        for i in range(6):
            want, mg = sum(acc[p][i]), sum(mag[p][i])
            dd = abs(got[p, 1 + i] - want)
            assert dd <= BAR * mg, (p, i, got[p, 1 + i], want, mg)
            if mg > 0:
                worst = max(worst, dd / mg)
    print("general WCS: identity at the photons, worst |difference| / sum |r plane| = %.3g" % worst)


# ---- 7 (no GPU) ------------------------------------------------------------------------------------------------------------------
def test_resource_row_and_budget():
    import json
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    k = resource_usage.collect()
    assert "pgrad_nz_sums" in k, sorted(k)
    r = k["pgrad_nz_sums"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0
    assert "`pgrad_nz_sums`" in resource_usage.table(k)
    budget = json.load(open(resource_usage.BUDGET))["kernels"]
    assert "pgrad_nz_sums" in budget
    assert [m for m in resource_usage.check(k) if m.startswith("pgrad_nz_sums")] == []
    assert r["occupancy"] >= budget["pgrad_nz_sums"]["min_occupancy"]


def test_the_header_names_the_constants_the_mirror_holds():
    from desi_mcmc_amd import _lib as L
    assert _kernel_constants() == (L.PGNZ_TRIP, L.PGNZ_DEAL_PHOTONS)
