"""Analytic gradient of the per-source conditional log-likelihoods: cel_patch_loglik[_multi](mode = 8 + m), k_patch_grad.h,
ImageSet.patch_loglik*_grad, galaxy_source_like_grad(analytic=True), ModelGibbs.location_loglik_grad.

  1. identity with the derivative stamps (k_stamp_jac.h) contracted with r on the host, modes 8, 9, 10
  2. the m > 0 rule: z > 0 where the model is exactly 0, and counts = 0
  3. Richardson-combined central differences of the CPU oracle's value in all 6 + B coordinates (types -1, -2, -3 included);
     the quotients' own consistency is checked on the CPU first
  4. contract: slot 0, repeatability, both kernel settings, multi = single, resident = explicit, refusals, resources
  5. the mirror;  6. (no GPU) header, CEL_PLL_GRAD, the frozen boundary

The scene: 2 bands on a 96 x 112 frame, eleven proposals on five sets of patch limits -- every proposal with photons of its own, so
the batch call takes eleven patch sets, listed in reverse (owner is not the identity; test 4 also shares sets): a star; a star cut by the frame's
edge; a type-1 galaxy on an 81 x 89 patch (more than 64 rows and columns, neither a multiple of the four parts); a type-1 galaxy
under the sigma floor; a type-2 galaxy; a star and a galaxy whose band-0 patch is empty; a star and a galaxy beside the frame whose
own box is empty while the patch is imposed (types -1, -2); an overlap-test miss (type -3); a star on patches of 1 x 1 and 3 rows
(set 0's band-0 patch has 13 rows).  z is a Poisson draw from the proposal's own m (+ eps for mode 1), fixed seed.
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

P_STAR, P_EDGE, P_BIG, P_FLOOR, P_T2, P_HALF, P_OWN_EMPTY, P_MISS, P_GAL_EMPTY, P_SMALL, P_HALF_GAL = range(11)
NAMES = ["star", "edge star", "big galaxy", "floored galaxy", "type-2 galaxy", "star, band 0 empty", "star, own box empty (-1)",
         "overlap-test miss (-3)", "galaxy, own box empty (-2)", "star on 1 x 1 / 3 rows", "galaxy, band 0 empty"]
COORDS = ["ra", "dec", "shape0", "shape1", "shape2", "shape3"] + ["counts%d" % b for b in range(B)]
#: entries test 3 leaves to test 1: (proposal, coordinate).  The unresolved galaxy's theta, phi and rho (the planes are
#: 1e-3 to 6e-6 of u per unit and the quotient's own rounding is of their size); they are summed over the bands, so one entry each.
LEFT_TO_TEST_1 = [(P_FLOOR, "shape0"), (P_FLOOR, "shape2"), (P_FLOOR, "shape3")]


@pytest.fixture(scope="module")
def cel():
    import desi_mcmc_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(cel):
    return cel.Context(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- the CPU yardstick --------------------------------------------------------------------------------------------------------
def _prof(orc):
    ea, ev, da, dv = orc.profile_tables()
    return np.concatenate([ea, da]), np.concatenate([ev, dv])


def _comps(band, typ, radec, shape, orc):
    """(amplitude, mean, covariance) of every component of one source in one band, from the oracle's tables (as
    test_stamp_jacobians.py forms them); a star renders whether or not it passes the overlap test"""
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    if typ == 0:
        v = orc.equa2pixel(band, radec)
        return w.copy(), v[None, :] + mu, cov.copy()
    if typ == 2:
        amp, var = _prof(orc)
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


def _unit(comps, box, dtype=np.float64):
    """the unit stamp on the fixed box, evaluated in `dtype` from the (double) component tables"""
    y0, y1, x0, x1 = box
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=dtype), np.arange(y0, y1, dtype=dtype))
    u = np.zeros(X.shape, dtype=dtype)
    two_pi = 2 * dtype(np.pi)
    for A, m, Cm in zip(*comps):
        a, b, c = dtype(Cm[0, 0]), dtype(Cm[0, 1]), dtype(Cm[1, 1])
        det = a * c - b * b
        dx, dy = X - dtype(m[0]), Y - dtype(m[1])
        u += dtype(A) * np.exp(-(c * dx * dx - 2 * b * dx * dy + a * dy * dy) / det / 2) / (two_pi * np.sqrt(det))
    return u


def _wsum(band):
    return (band[3] + band[4]) + band[5]


def _value(orc, mode, band, typ, radec, shape, counts, box, z, extended=False):
    """one band's term of the plain value in mode 0, 1 or 2.  The oracle's patch_loglik where it holds the case (modes 0 and 1 of
    a star or a type-1 galaxy; it has no mode 2, no type 2, and gives an overlap-test miss its mode-0 value in every mode); the
    numpy restatement from the oracle's component tables otherwise.  extended: the restatement in x87 long double throughout,
    returned as such -- for a quotient that the value's own last bit (a double of ~1e6 to 1e7: 1e-10 to 2e-9) would spoil."""
    if box[1] <= box[0] or box[3] <= box[2]:
        return 0.0
    miss = typ == 0 and not orc.star_box(band, H, W, radec)[0]
    if not extended and mode in (0, 1) and typ in (0, 1) and not (miss and mode == 1):
        return orc.patch_loglik(band, H, W, typ, radec, shape, counts, box, np.ascontiguousarray(z).ravel(), mode=mode)
    dt = np.longdouble if extended else np.float64
    if miss and mode == 0:
        return -dt(counts) * dt(_wsum(band))
    tot = (lambda a: np.sum(a)) if extended else (lambda a: math.fsum(a.ravel()))
    m = dt(counts) * _unit(_comps(band, typ, radec, shape, orc), box, dt)
    z = z.astype(dt)
    if mode == 1:
        m = m + dt(band[0])
        return tot(np.log(m) * z) - tot(m)
    ok = m > 0
    a = tot(np.log(m[ok]) * z[ok])
    return a - dt(counts) * dt(_wsum(band)) if mode == 0 else a - tot(m[ok])


def _make_scene(orc):
    from desi_mcmc_amd import synth
    bands = synth.make_bands(H, W, B)
    ob = bands.copy()                                   # the oracle's records carry the star radius
    for b in range(B):
        ob[b, 36] = orc.band_radius(bands[b])
    R = float(np.max(ob[:, 36]))
    # patch sets: (set, band) -> y0, y1, x0, x1
    boxes = np.zeros((5, B, 4), dtype=np.int32)
    boxes[0] = [[34, 47, 20, 42], [30, 50, 20, 43]]     # 13 rows; 20 rows
    boxes[1] = [[7, 88, 11, 100], [7, 88, 11, 100]]     # 81 x 89
    boxes[2] = [[40, 61, 0, 12], [41, 60, 0, 11]]       # at the frame's left edge
    boxes[3] = [[70, 71, 80, 81], [69, 72, 75, 86]]     # 1 x 1; 3 rows
    boxes[4] = [[0, 0, 0, 0], [30, 50, 60, 81]]         # band 0: no patch
    # a galaxy beside the frame whose own box is empty: the nearest such column, found with the oracle
    gshape = [0.6, 0.5, 70.0, 0.8]
    gx = -3.0
    while True:
        u = synth.pixel2equa(bands[0], np.array([[gx, 50.4]]))[0]
        if all(orc.source_patch(ob[b], H, W, 1, u, gshape)[0] is None for b in range(B)):
            break
        gx -= 1.0
    pix = np.array([[31.3, 40.2], [2.3, 50.7], [55.4, 47.3], [30.6, 41.1], [32.1, 39.5], [70.3, 40.6], [-(R + 1.2), 50.2],
                    [-60.0, 50.0], [gx - 0.3, 50.4], [80.2, 70.4], [69.5, 40.2]])
    typ = np.array([0, 0, 1, 1, 2, 0, 0, 0, 1, 0, 1], dtype=np.int32)
    shape = np.zeros((11, 4))
    shape[P_BIG] = [0.5, 3.0, 30.0, 0.6]
    shape[P_FLOOR] = [0.4, 0.02, 40.0, 0.7]             # below k_prep's floor 1/30
    shape[P_T2] = [0.35, 1.2, 0.3, 0.9]                 # theta, W00, W01, W11
    shape[P_GAL_EMPTY] = gshape
    shape[P_HALF_GAL] = [0.6, 1.0, 120.0, 0.5]
    owner = np.array([0, 2, 1, 0, 0, 4, 2, 2, 2, 3, 4], dtype=np.int32)
    counts = np.array([[8000.0, 12000.0], [6000.0, 9000.0], [40000.0, 50000.0], [7000.0, 5000.0], [15000.0, 11000.0], [5000.0, 7000.0],
                       [4e5, 5e5], [9000.0, 8000.0], [3e6, 4e6], [20000.0, 16000.0], [9000.0, 14000.0]])
    radec = synth.pixel2equa(bands[0], pix)
    P = len(typ)
    # the record kinds, from the oracle: own box empty (-1, -2), overlap-test miss (-3)
    kind = np.zeros((P, B), dtype=np.int32)
    for p in range(P):
        for b in range(B):
            if typ[p] == 0:
                okb, _, bx = orc.star_box(ob[b], H, W, radec[p])
                kind[p, b] = -3 if not okb else (0 if (bx[1] > bx[0] and bx[3] > bx[2]) else -1)
            else:
                kind[p, b] = 1 if orc.source_patch(ob[b], H, W, 1, radec[p], shape[p] if typ[p] == 1 else [0.5, 1.0, 0.0, 0.5])[0] is not None else -2
    assert np.all(kind[P_OWN_EMPTY] == -1) and np.all(kind[P_MISS] == -3) and np.all(kind[P_GAL_EMPTY] == -2)
    assert np.all(kind[[P_STAR, P_EDGE, P_SMALL, P_HALF]] == 0) and np.all(kind[[P_BIG, P_FLOOR, P_T2, P_HALF_GAL]] == 1)
    # z per mode: a Poisson draw from the proposal's own m (+ eps in mode 1)
    rs = np.random.RandomState(11)
    z = {}
    for mode in (0, 1, 2):
        for p in range(P):
            for b in range(B):
                bx = boxes[owner[p], b]
                if bx[1] <= bx[0] or bx[3] <= bx[2]:
                    z[mode, p, b] = None
                    continue
                m = counts[p, b] * _unit(_comps(ob[b], typ[p], radec[p], shape[p], orc), bx)
                z[mode, p, b] = rs.poisson(m + (ob[b, 0] if mode == 1 else 0.0)).astype(np.float64)
    return dict(bands=bands, ob=ob, boxes=boxes, typ=typ, shape=shape, owner=owner, counts=counts, radec=radec, z=z, P=P, kind=kind)


@pytest.fixture(scope="module")
def scene(orc):
    return _make_scene(orc)


def _steps(p, sc):
    """(coordinate index, kind, index, h): test_loglik_grad.py's shape steps, 3e-8 degrees (3e-4 px: at 1e-8 the value's last bit shows in the big galaxy's quotient; in mode 1 an entry is a cancelling sum and
    the h^2 term of a 1e-7 quotient reached 4e-7 of the column), and 1e-5 of the counts (the h^2 term of a quotient is ~2.5e-11 N / c; in mode 1 the column itself is only ~1e-2)"""
    t, sh = sc["typ"][p], sc["shape"][p]
    out = [(0, "u", 0, 3e-8), (1, "u", 1, 3e-8)]
    if t == 1:
        out += [(2, "sh", 0, 1e-6), (3, "sh", 1, 1e-6 * sh[1]), (4, "sh", 2, 1e-4), (5, "sh", 3, 1e-6)]
    if t == 2:
        out += [(2, "sh", 0, 1e-6), (3, "sh", 1, 1e-6), (4, "sh", 2, 1e-6), (5, "sh", 3, 1e-6)]
    out += [(6 + b, "c", b, 1e-5 * sc["counts"][p, b]) for b in range(B)]
    return out


def _total(orc, sc, mode, p, radec, shape, counts, extended=False):
    tot = 0.0
    for b in range(B):                                   # band order
        tot = tot + _value(orc, mode, sc["ob"][b], sc["typ"][p], radec, shape, counts[b], sc["boxes"][sc["owner"][p], b],
                           sc["z"][mode, p, b], extended)
    return tot


def _quotient(orc, sc, mode, p, kind, i, h, extended=False):
    vals = []
    for sgn in (1.0, -1.0):
        ra, sh, ct = sc["radec"][p].copy(), sc["shape"][p].copy(), sc["counts"][p].copy()
        {"u": ra, "sh": sh, "c": ct}[kind][i] += sgn * h
        vals.append((_total(orc, sc, mode, p, ra, sh, ct, extended), {"u": ra, "sh": sh, "c": ct}[kind][i]))
    return float((vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1]))


def _compared(p, col):
    return (p, COORDS[col]) not in LEFT_TO_TEST_1


@pytest.fixture(scope="module")
def fd(orc, scene):
    return _fd_pairs(orc, scene)


def _fd_pairs(orc, scene):
    """per mode: (fd_h, fd_h/2) of the oracle's value, (P, 6 + B) each; a coordinate a source does not have stays 0.
    A pair of quotients that disagrees by more than a tenth of test 3's bar, or whose step does not keep the value's last bit
    below that tenth -- both judged from the yardstick alone -- is formed again
    from the extended-precision restatement (the rule of tests/test_stamp_jacobians.py, test 3): steps, bar and tables stay."""
    assert np.finfo(np.longdouble).eps < 2e-19
    out = {}
    for mode in (0, 1, 2):
        q1, q2 = np.zeros((scene["P"], 6 + B)), np.zeros((scene["P"], 6 + B))
        for p in range(scene["P"]):
            for col, kind, i, h in _steps(p, scene):
                q1[p, col] = _quotient(orc, scene, mode, p, kind, i, h)
                q2[p, col] = _quotient(orc, scene, mode, p, kind, i, 0.5 * h)
        top = np.max(np.abs((4.0 * q2 - q1) / 3.0), axis=0)
        vmag = [max(abs(_value(orc, mode, scene["ob"][b], scene["typ"][p], scene["radec"][p], scene["shape"][p], scene["counts"][p, b],
                               scene["boxes"][scene["owner"][p], b], scene["z"][mode, p, b])) for b in range(B)) for p in range(scene["P"])]
        again = []
        for p in range(scene["P"]):
            for col, kind, i, h in _steps(p, scene):
                # the value is a double: its last bit, 2^-52 |value|, shows in the finer quotient as 2^-52 |value| / h.  (Two
                # quotients of the oracle can agree with each other and still carry it: the big galaxy's rho, mode 1, gave
                # 98.866411 at h and h / 2 and 98.865945 at 4 h; extended precision gives 98.865974 at all three.)
                last_bit = 2.0 ** -52 * vmag[p] / h
                if _compared(p, col) and (abs(q1[p, col] - q2[p, col]) > 1e-7 * top[col] or last_bit > 1e-7 * top[col]):
                    q1[p, col] = _quotient(orc, scene, mode, p, kind, i, h, True)
                    q2[p, col] = _quotient(orc, scene, mode, p, kind, i, 0.5 * h, True)
                    again.append((scene.get("names", NAMES)[p], COORDS[col]))
        print("mode %d: %d quotient pairs formed in extended precision: %s" % (mode, len(again), again))
        out[mode] = (q1, q2)
    return out


def test_the_yardsticks_own_quotients_agree(scene, fd):
    """before any GPU run: the oracle's central differences at h and h / 2 agree within a tenth of test 3's bar (1e-6 x the
    column's largest |entry| over the batch) for every entry test 3 compares; the list of entries left to test 1 holds at most
    the unresolved galaxy's theta, phi and rho"""
    assert set(LEFT_TO_TEST_1) <= {(P_FLOOR, "shape0"), (P_FLOOR, "shape2"), (P_FLOOR, "shape3")}
    for mode in (0, 1, 2):
        q1, q2 = fd[mode]
        rich = (4.0 * q2 - q1) / 3.0
        top = np.max(np.abs(rich), axis=0)
        assert np.all(top > 0)
        worst = 0.0
        for p in range(scene["P"]):
            for col in range(6 + B):
                if _compared(p, col):
                    d = abs(q1[p, col] - q2[p, col]) / top[col]
                    worst = max(worst, d)
                    assert d <= 1e-7, (mode, NAMES[p], COORDS[col], q1[p, col], q2[p, col], top[col])
        print("mode %d: worst |fd_h - fd_h/2| / column max = %.3g" % (mode, worst))


# ---- the device side ------------------------------------------------------------------------------------------------------------
def _patches(sc, mode):
    """(boxes[p], patches[p][band]) of every proposal: its set's limits and its own photons"""
    P = sc["P"]
    boxes = np.array([sc["boxes"][sc["owner"][p]] for p in range(P)], dtype=np.int32)
    patches = [[sc["z"][mode, p, b] for b in range(B)] for p in range(P)]
    return boxes, patches


def _batch(sc, mode):
    """the batch call's arguments: the P patch sets in REVERSE order, owner[p] = P - 1 - p"""
    boxes, patches = _patches(sc, mode)
    return np.arange(sc["P"] - 1, -1, -1, dtype=np.int32), np.ascontiguousarray(boxes[::-1]), patches[::-1]


@pytest.fixture(scope="module")
def dev(cel, ctx, scene):
    """the image set, the proposals and per mode the gradient form's output for the whole batch in ONE multi call"""
    iset = cel.ImageSet(ctx, scene["bands"], H, W)
    prop = cel.SourceSet(ctx, scene["P"], B).set(scene["typ"], scene["radec"], scene["counts"], scene["shape"])
    out = {}
    for mode in (0, 1, 2):
        own, boxes, patches = _batch(scene, mode)
        out[mode] = iset.patch_loglik_multi_grad(prop, own, boxes, patches, mode=mode)
    return dict(iset=iset, prop=prop, out=out)


def _flat(res):
    ll, gr, gc, gs = res
    return np.column_stack([gr, gs, gc])


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_identity_with_the_derivative_stamps(scene, dev):
    """modes 8, 9, 10: each entry = the derivative stamps on the patch box contracted with r (formed on the host from z and
    plane 0) by math.fsum, bands in order; bar 1e-10 sum |r plane| per entry (the kernel's fp64 sum of n <= 1e4 terms is bounded
    by about n 2^-53 of that sum: two orders of margin; tests/test_stamp_jacobians.py's bar for the same identity).
    Worst measured ratio: 5.6e-15."""
    iset, prop, P = dev["iset"], dev["prop"], scene["P"]
    sj, uj = [], []
    for b in range(B):
        lim = np.array([scene["boxes"][scene["owner"][p], b] for p in range(P)], dtype=np.int32)
        sj.append(iset.stamp_jacobians(prop, b, scaled=True, boxes_in=lim)[0])
        uj.append(iset.stamp_jacobians(prop, b, scaled=False, boxes_in=lim)[0])
    worst, seen = 0.0, 0
    for mode in (0, 1, 2):
        got = _flat(dev["out"][mode])
        for p in range(P):
            if all(sj[b][p] is None for b in range(B)):
                continue
            acc, mag = [[] for _ in range(6)], [[] for _ in range(6)]
            for b in range(B):
                if sj[b][p] is None:
                    continue
                u, z, c = uj[b][p][0], scene["z"][mode, p, b], scene["counts"][p, b]
                m = c * u
                with np.errstate(divide="ignore", invalid="ignore"):
                    if mode == 0:
                        r = np.where(m > 0, z / m, 0.0)
                    elif mode == 2:
                        r = np.where(m > 0, z / m - 1.0, 0.0)
                    else:
                        r = z / (m + scene["bands"][b, 0]) - 1.0
                t = (r * u).ravel()
                want = math.fsum(t) - (_wsum(scene["bands"][b]) if mode == 0 else 0.0)
                d, mg = abs(got[p, 6 + b] - want), math.fsum(np.abs(t))
                assert d <= 1e-10 * mg, (mode, NAMES[p], "counts", b, got[p, 6 + b], want, mg)
                worst = max(worst, d / mg) if mg > 0 else worst
                for i in range(1, sj[b][p].shape[0]):
                    t = (r * sj[b][p][i]).ravel()
                    acc[i - 1].append(math.fsum(t)); mag[i - 1].append(math.fsum(np.abs(t)))
                seen += 1
            for i in range(6):
                want, mg = sum(acc[i]), sum(mag[i])      # bands in order (an entry a star does not have: 0)
                d = abs(got[p, i] - want)
                assert d <= 1e-10 * mg, (mode, NAMES[p], COORDS[i], got[p, i], want, mg)
                if mg > 0:
                    worst = max(worst, d / mg)
            if scene["typ"][p] == 0:
                assert np.all(got[p, 2:6] == 0.0)
    assert seen >= 3 * 12
    # the floored galaxy's sigma entry is exactly 0, its phi entry is not
    for mode in (0, 1, 2):
        assert dev["out"][mode][3][P_FLOOR, 1] == 0.0 and dev["out"][mode][3][P_FLOOR, 2] != 0.0
    print("identity with the derivative stamps: worst |difference| / sum |r plane| = %.3g" % worst)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_pixels_the_model_does_not_reach_add_nothing(cel, ctx, scene, dev):
    """z > 0 where every exponential underflows to exactly 0: all outputs finite, location entries 0, the counts entry exactly
    -wsum_b (mode 8) and exactly 0 (mode 10).  (On a 96 x 112 frame no two points lie the 211 px apart that the widest PSF
    component needs to underflow, so the star sits 300 rows below the frame -- it passes the overlap test, which has no upper
    bound on the row -- with its patch in the frame's top right corner.)  The same with counts = 0 on an ordinary patch."""
    from desi_mcmc_amd import synth
    iset = dev["iset"]
    u_far = synth.pixel2equa(scene["bands"][0], np.array([[2.0, 400.0]]))
    box = np.array([[2, 14, 95, 110], [3, 16, 96, 111]], dtype=np.int32)
    zz = [np.full((12, 15), 3.0), np.full((13, 15), 2.0)]
    wsum = np.array([_wsum(scene["bands"][b]) for b in range(B)])
    cases = [(u_far, np.array([[5000.0, 7000.0]]), box, zz),
             (scene["radec"][P_STAR][None, :], np.zeros((1, B)), scene["boxes"][0], [np.full((13, 22), 2.0), np.full((20, 23), 1.0)])]
    for radec, counts, bx, z in cases:
        one = cel.SourceSet(ctx, 1, B).set(np.zeros(1, dtype=np.int32), radec, counts, np.zeros((1, 4)))
        if counts[0, 0] > 0:
            un = [iset.stamp_jacobians(one, b, scaled=False, boxes_in=bx[b][None, :])[0][0] for b in range(B)]
            assert all(p is not None and np.all(p[0] == 0.0) for p in un)      # the model is exactly 0 on the patch
        for mode in (0, 2):
            ll, gr, gc, gs = iset.patch_loglik_grad(one, bx, z, mode=mode)
            assert np.all(np.isfinite(ll)) and np.all(np.isfinite(gr)) and np.all(np.isfinite(gc)) and np.all(np.isfinite(gs))
            assert np.all(gr == 0.0) and np.all(gs == 0.0)
            assert np.array_equal(gc[0], -wsum if mode == 0 else np.zeros(B)), (mode, gc)
            assert ll[0] == iset.patch_loglik(one, bx, z, mode=mode)[0]


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_against_central_differences_of_the_oracle(scene, dev, fd, mode):
    """every entry against (4 fd_{h/2} - fd_h) / 3 of the CPU oracle's value (its patch_loglik where it holds the case, the
    numpy restatement from its tables otherwise); bar 1e-6 x the largest |entry| of the column over the batch
    (tests/test_loglik_grad.py's bar for its central differences).  Entries in LEFT_TO_TEST_1 are not compared.
    Worst measured ratios: 2.8e-8, 5.3e-8 and 1.2e-7 in modes 8, 9 and 10."""
    q1, q2 = fd[mode]
    rich = (4.0 * q2 - q1) / 3.0
    got = _flat(dev["out"][mode])
    top = np.max(np.abs(rich), axis=0)
    worst, over = 0.0, []
    for p in range(scene["P"]):
        for col in range(6 + B):
            if not _compared(p, col):
                continue
            d = abs(got[p, col] - rich[p, col]) / top[col]
            worst = max(worst, d)
            if not d <= 1e-6:
                over.append((NAMES[p], COORDS[col], got[p, col], rich[p, col], d))
    print("mode %d: worst |entry - fd| / column max = %.3g" % (8 + mode, worst))
    assert not over, over
    # an overlap-test miss in mode 8: only -wsum in its counts entries
    if mode == 0:
        assert np.all(got[P_MISS, :6] == 0.0)
        assert np.array_equal(got[P_MISS, 6:], [-_wsum(scene["bands"][b]) for b in range(B)])
    else:
        assert np.any(got[P_MISS, :2] != 0.0)            # ... and a star in modes 9 and 10
    # a band with an empty patch contributes nothing
    assert got[P_HALF, 6] == 0.0 and got[P_HALF_GAL, 6] == 0.0


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _raw(iset, prop, owner, NB, boxes, offs, data, mode, out):
    from desi_mcmc_amd import _lib as L
    return L.lib().cel_patch_loglik_multi(iset._h, prop._h, None if owner is None else owner.ctypes.data_as(L.c_int32_p), NB,
                                          None if boxes is None else boxes.ctypes.data_as(L.c_int32_p),
                                          None if offs is None else offs.ctypes.data_as(L.c_int64_p),
                                          None if data is None else data.ctypes.data, L.CEL_HOST, mode, L.dptr(out))


def _pack(boxes, patches):
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, B, 4)
    offs = [0]
    flat = []
    for o in range(boxes.shape[0]):
        for b in range(B):
            if patches[o][b] is not None:
                flat.append(np.asarray(patches[o][b], dtype=np.float64).ravel())
            offs.append(offs[-1] + (0 if patches[o][b] is None else patches[o][b].size))
    return boxes, np.array(offs, dtype=np.int64), (np.concatenate(flat) if flat else np.zeros(1))


@gpu
def test_contract_values_repeatability_and_kernel_settings(ctx, scene, dev):
    from desi_mcmc_amd import _lib as L
    iset, prop, P = dev["iset"], dev["prop"], scene["P"]
    before = ctx.get_option(L.CEL_OPT_KERNEL)
    try:
        for mode in (0, 1, 2):
            own, rboxes, rpatches = _batch(scene, mode)
            boxes, patches = _patches(scene, mode)
            ref = dev["out"][mode]
            for kern in ("direct", "recurrence"):
                ctx.set_kernel(kern)
                plain = iset.patch_loglik_multi(prop, own, rboxes, rpatches) if mode == 0 else None
                if mode == 1:
                    plain = iset.patch_loglik_multi(prop, own, rboxes, rpatches, isolated=True)
                ctx.profile(True)
                res = iset.patch_loglik_multi_grad(prop, own, rboxes, rpatches, mode=mode)
                ms, launches = ctx.profile_get("patch_ll")
                ctx.profile(False)
                assert launches >= 2 and ms > 0.0            # the plain path's launch and the gradient's, under CEL_K_PATCH_LL
                if plain is not None:
                    assert np.array_equal(res[0], plain), (mode, kern)       # slot 0: the plain mode's bits
                for a, b in zip(res[1:], ref[1:]):
                    assert np.array_equal(a, b), (mode, kern)                # slots 1..: the same bits, both settings, every call
            # (mode 2's plain value has no multi mirror: it is compared one proposal at a time, below)
            ctx.set_option(L.CEL_OPT_KERNEL, before)
            # the multi call = the single-source calls, bit for bit
            for p in range(P):
                one = type(prop)(ctx, 1, B).set(scene["typ"][p:p + 1], scene["radec"][p:p + 1], scene["counts"][p:p + 1], scene["shape"][p:p + 1])
                single = iset.patch_loglik_grad(one, boxes[p], patches[p], mode=mode)
                for a, b in zip(single, dev["out"][mode]):
                    assert np.array_equal(a[0], b[p]), (mode, NAMES[p])
                assert single[0][0] == iset.patch_loglik(one, boxes[p], patches[p], mode=mode)[0]
    finally:
        ctx.profile(False)
        ctx.set_option(L.CEL_OPT_KERNEL, before)
    # proposals of several sources on shared patch sets (owner mixes them): the same entries as on sets of their own, where
    # the data is the same -- the star, the floored galaxy and the type-2 galaxy scored on set 0 with the star's photons
    sel = np.array([P_STAR, P_FLOOR, P_T2, P_BIG, P_STAR], dtype=np.int32)
    sub = type(prop)(ctx, len(sel), B).set(scene["typ"][sel], scene["radec"][sel], scene["counts"][sel], scene["shape"][sel])
    sets = scene["boxes"][[0, 1]]
    data = [[scene["z"][0, P_STAR, b] for b in range(B)], [scene["z"][0, P_BIG, b] for b in range(B)]]
    mixed = iset.patch_loglik_multi_grad(sub, np.array([0, 0, 0, 1, 0], dtype=np.int32), sets, data)
    for a, b in zip(mixed, dev["out"][0]):
        assert np.array_equal(a[0], b[P_STAR]) and np.array_equal(a[4], b[P_STAR]) and np.array_equal(a[3], b[P_BIG])
    assert np.all(np.isfinite(_flat(mixed)))


@gpu
def test_resident_form_agrees_with_the_explicit_call(cel, ctx, scene):
    """after photon_split_resident: mode 8 against the explicit call fed the samples_fetch patches (int32 against double data:
    the same terms in the same order), mode 9 against the nelec boxes; bar 1e-13 sum |r plane|, bounded below by
    1e-13 x the entry's own size"""
    sel = [P_STAR, P_EDGE, P_BIG, P_FLOOR, P_SMALL, P_HALF_GAL]
    typ, radec, counts, shape = scene["typ"][sel], scene["radec"][sel], scene["counts"][sel], scene["shape"][sel]
    S = len(sel)
    iset = cel.ImageSet(ctx, scene["bands"], H, W)
    cat = cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape)
    iset.render(cat)
    nelec = np.random.RandomState(5).poisson(iset.model_images()).astype(np.float64)
    iset.set_nelec(nelec)
    iset.photon_split_resident(cat, seed=9)
    rb, roff, rdata = iset.fetch_samples()
    rs = np.random.RandomState(6)
    own = np.repeat(np.arange(S, dtype=np.int32), 2)
    pr = radec[own] + rs.normal(0, 2e-5, (2 * S, 2))
    prop = cel.SourceSet(ctx, 2 * S, B).set(typ[own], pr, counts[own] * rs.uniform(0.9, 1.1, (2 * S, B)), shape[own])
    hp = [[None if roff[s * B + b + 1] == roff[s * B + b] else
           rdata[roff[s * B + b]:roff[s * B + b + 1]].reshape(rb[s, b, 1] - rb[s, b, 0], rb[s, b, 3] - rb[s, b, 2]).astype(np.float64)
           for b in range(B)] for s in range(S)]
    hb = rb.copy()
    for s in range(S):
        for b in range(B):
            if hp[s][b] is None:
                hb[s, b] = 0
    assert sum(p is not None for row in hp for p in row) >= 2 * S - 2
    for iso in (False, True):
        res = iset.patch_loglik_resident_grad(prop, own, isolated=iso)
        data = hp if not iso else [[None if hp[s][b] is None else nelec[b, hb[s, b, 0]:hb[s, b, 1], hb[s, b, 2]:hb[s, b, 3]]
                                    for b in range(B)] for s in range(S)]
        exp = iset.patch_loglik_multi_grad(prop, own, hb, data, isolated=iso)
        assert np.array_equal(res[0], iset.patch_loglik_resident(prop, own, isolated=iso))       # slot 0: the plain resident call
        a, b = _flat(res), _flat(exp)
        # sum |r plane| >= |sum r plane|: the entry's own size bounds the bar from below
        assert np.all(np.abs(a - b) <= 1e-13 * np.abs(b)), (iso, np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
        print("resident mode %d: bit-equal to the explicit call: %s" % (9 if iso else 8, np.array_equal(a, b)))
        assert np.any(a != 0.0)
        again = iset.patch_loglik_resident_grad(prop, own, isolated=iso)
        assert np.array_equal(_flat(again), a)


@gpu
def test_refusals_leave_the_output_untouched(cel, ctx, scene, dev):
    from desi_mcmc_amd import _lib as L
    iset, prop, P = dev["iset"], dev["prop"], scene["P"]
    own = np.arange(P, dtype=np.int32)
    boxes, offs, data = _pack(*_patches(scene, 0))
    n = P * (7 + B)
    sent = np.full(n + 3, -7.25)

    def refused(rc):
        assert rc == L.CEL_ERR_INVALID and np.all(sent == -7.25)

    assert _raw(iset, prop, own, P, boxes, offs, data, 8, sent) == L.CEL_OK and np.all(sent[n:] == -7.25) and np.all(sent[:n] != -7.25)
    sent[:] = -7.25
    for bad in (8 + 3, 8 + 4, 16, 7, -8, 3, 5):
        refused(_raw(iset, prop, own, P, boxes, offs, data, bad, sent))
    # offsets sized for 7 + B planes
    refused(_raw(iset, prop, own, P, boxes, offs * (7 + B), np.zeros(int(offs[-1]) * (7 + B)), 8, sent))
    # bad offsets and owners, as the plain mode refuses them
    off1 = offs.copy(); off1[0] = 1
    refused(_raw(iset, prop, own, P, boxes, off1, data, 8, sent))
    bad_own = own.copy(); bad_own[3] = P
    refused(_raw(iset, prop, bad_own, P, boxes, offs, data, 9, sent))
    bad_own[3] = -1
    refused(_raw(iset, prop, bad_own, P, boxes, offs, data, 10, sent))
    refused(_raw(iset, prop, None, P, boxes, offs, data, 8, sent))                     # NB > 1 without owners
    out_of_frame = boxes.copy(); out_of_frame[0, 0] = [34, 47, 100, 122]
    refused(_raw(iset, prop, own, P, out_of_frame, offs, data, 8, sent))
    # the resident form: no split; m = 2
    refused(_raw(iset, prop, own, P, None, None, None, 8, sent))
    refused(_raw(iset, prop, own, P, None, None, None, 10, sent))
    with pytest.raises(ValueError):
        iset.patch_loglik_resident_grad(prop, own)
    with pytest.raises(ValueError):
        iset.patch_loglik_multi_grad(prop, own, boxes, _patches(scene, 0)[1], mode=3)
    # a masked set in m = 1
    masked = cel.ImageSet(ctx, scene["bands"], H, W)
    ne = np.ones((B, H, W)); ne[0, 5, 5] = np.nan
    masked.set_nelec(ne)
    refused(_raw(masked, prop, own, P, boxes, offs, data, 9, sent))
    with pytest.raises(ValueError):
        masked.patch_loglik_multi_grad(prop, own, boxes, _patches(scene, 1)[1], mode=1)
    assert _raw(masked, prop, own, P, boxes, offs, data, 8, sent) == L.CEL_OK           # (m = 0 does not read the image)
    sent[:] = -7.25
    # a row window, as cel_loglik_grad refuses it
    win = cel.ImageSet(ctx, scene["bands"], 64, W)
    win.set_window(16, H)
    wb = boxes.copy(); wb[:, :, :2] = np.minimum(wb[:, :, :2], 0)                        # (no patch anywhere: only the window is at stake)
    woffs = np.zeros_like(offs)
    for m in (8, 9, 10):
        refused(_raw(win, prop, own, P, wb, woffs, np.zeros(1), m, sent))
    assert _raw(win, prop, own, P, wb, woffs, np.zeros(1), 0, sent) == L.CEL_OK
    with pytest.raises(ValueError):
        win.patch_loglik_grad(type(prop)(ctx, 1, B).set(scene["typ"][:1], scene["radec"][:1], scene["counts"][:1], scene["shape"][:1]),
                              np.zeros((B, 4), dtype=np.int32), [None] * B)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
def _fits(sc, b, nelec):
    from desi_mcmc_amd.fits_image import FitsImage
    r = sc["bands"][b]
    return FitsImage("ugriz"[b], nelec, epsilon=r[0], kappa=r[1], calib=r[2], weights=r[3:6], means=r[6:12].reshape(3, 2),
                     covars=r[12:24].reshape(3, 2, 2), rho_n=r[24:26], phi_n=r[26:28], Ups_n=r[28:32].reshape(2, 2))


def _reference_recipe(gc, th, Z_s, images, limits):
    """galaxy_source_like_grad's default arithmetic as it stood before `analytic` existed, written out"""
    theta_s, sig_s, phi_s, rho_s = th[0:4]
    u_s = th[4:6]
    bs = dict(zip(gc.BANDS, th[-5:]))
    grad_theta_s = 0.
    grad_bs = dict(zip(gc.BANDS, np.zeros(5)))
    for n, img in enumerate(images):
        (ylim, xlim), Z = limits[n], np.asarray(Z_s[n], dtype=np.float64)
        R_s = gc.gen_galaxy_transformation(sig_s, rho_s, phi_s, img.Ups_n)
        f_exp, _, _ = gc.gen_galaxy_prof_psf_image('exp', R_s, u_s, img, xlim=xlim, ylim=ylim)
        f_dev, _, _ = gc.gen_galaxy_prof_psf_image('dev', R_s, u_s, img, xlim=xlim, ylim=ylim)
        f = theta_s * f_exp + (1. - theta_s) * f_dev
        ok = f > 0.
        grad_theta_s += np.sum((Z[ok] / f[ok] - bs[img.band]) * (f_exp - f_dev)[ok])
        grad_bs[img.band] += 1. / bs[img.band] * np.sum(Z) - np.sum(f)
    ths = np.tile(th, (10, 1))
    for i, th_i in enumerate([1, 2, 3, 4, 5]):
        ths[2 * i, th_i] += 1e-5
        ths[2 * i + 1, th_i] -= 1e-5
    lls = gc._source_like_batch(ths, Z_s, images, limits)
    return np.concatenate([[grad_theta_s], (lls[0::2] - lls[1::2]) / (2. * 1e-5), np.array([grad_bs[b] for b in gc.BANDS])])


@gpu
def test_mirror_galaxy_source_like_grad(cel, scene):
    """analytic=True against Richardson differences of galaxy_source_like itself in all 11 coordinates (test 3's bar, the
    column being this one gradient: 1e-6 x its largest |entry| among the coordinates of its kind); its sigma, phi, rho, ra, dec
    entries agree with the default form at that form's own accuracy (|its 1e-5 quotient - the Richardson value|, plus the bar);
    analytic=False returns the earlier arithmetic's bits"""
    from desi_mcmc_amd import celeste_galaxy_conditionals as gc
    imgs = [_fits(scene, b, np.zeros((H, W))) for b in range(B)]
    th = np.array([0.45, 1.4, 35.0, 0.6, scene["radec"][P_STAR, 0], scene["radec"][P_STAR, 1], 9.0, 14.0, 3.0, 3.0, 3.0])
    limits = [((28, 54), (18, 46)), ((27, 55), (17, 47))]
    rs = np.random.RandomState(3)
    Z_s = []
    for b, ((y0, y1), (x0, x1)) in enumerate(limits):
        R = gc.gen_galaxy_transformation(th[1], th[3], th[2], imgs[b].Ups_n)
        fe, _, _ = gc.gen_galaxy_prof_psf_image('exp', R, th[4:6], imgs[b], xlim=(x0, x1), ylim=(y0, y1))
        fv, _, _ = gc.gen_galaxy_prof_psf_image('dev', R, th[4:6], imgs[b], xlim=(x0, x1), ylim=(y0, y1))
        Z_s.append(rs.poisson(th[6 + b] / imgs[b].calib * imgs[b].kappa * (th[0] * fe + (1 - th[0]) * fv)).astype(np.float64))
    g = gc.galaxy_source_like_grad(th, Z_s, imgs, limits=limits, analytic=True)
    assert g.shape == (11,) and np.all(np.isfinite(g)) and np.all(g[8:] == 0.0)      # bands without an image: no dependence
    steps = [1e-6, 1e-6 * th[1], 1e-4, 1e-6, 1e-7, 1e-7] + [1e-5 * th[6 + b] for b in range(5)]
    ths = []
    for i, h in enumerate(steps):
        for f in (1.0, 0.5):
            for sgn in (1.0, -1.0):
                t = th.copy(); t[i] += sgn * f * h
                ths.append(t)
    ths.append(th.copy())
    ths = np.array(ths)
    lls = gc._source_like_batch(ths, Z_s, imgs, limits)
    rich = np.zeros(11)
    for i in range(11):
        v = lls[4 * i:4 * i + 4]
        t = ths[4 * i:4 * i + 4, i]
        q1, q2 = (v[0] - v[1]) / (t[0] - t[1]), (v[2] - v[3]) / (t[2] - t[3])
        rich[i] = (4 * q2 - q1) / 3
    assert lls[44] == gc.galaxy_source_like(th, Z_s, imgs, limits=limits)
    kinds = [[0, 1, 2, 3], [4, 5], [6, 7, 8, 9, 10]]
    worst = 0.0
    for cols in kinds:
        top = np.max(np.abs(rich[cols]))
        for i in cols:
            d = abs(g[i] - rich[i]) / top
            worst = max(worst, d)
            assert d <= 1e-6, (i, g[i], rich[i], top)
    print("galaxy_source_like_grad(analytic=True): worst |entry - fd| / largest of its kind = %.3g" % worst)
    default = gc.galaxy_source_like_grad(th, Z_s, imgs, limits=limits)
    assert np.array_equal(default, gc.galaxy_source_like_grad(th, Z_s, imgs, limits=limits, analytic=False))
    assert np.array_equal(default, _reference_recipe(gc, th, Z_s, imgs, limits))
    for i in (1, 2, 3, 4, 5):
        own = abs(default[i] - rich[i])                     # the 1e-5 quotient's distance from the Richardson value
        top = np.max(np.abs(rich[kinds[0] if i < 4 else kinds[1]]))
        # |g - default| <= |g - rich| + |rich - default|: the first is within the bar asserted above, the second is `own`
        assert abs(g[i] - default[i]) <= own + 1e-6 * top, (i, g[i], default[i], rich[i])


@gpu
def test_mirror_location_loglik_grad(cel, ctx):
    """ll is location_loglik's bits, g the sum over fields of the resident gradient; twenty steps of plain gradient ascent
    bring a star displaced by 0.3 px back to within 0.05 px of the conditional's maximum (found by the same ascent from the
    true position); conditional='exact' raises"""
    from desi_mcmc_amd import celeste_mcmc, synth
    S, Bf, Hf, Wf = 12, 2, 96, 112
    f0 = synth.SyntheticField(ctx, S, Bf, Hf, Wf, frac_gal=0.0, seed=23)
    pix = f0.src["pix"].copy()
    pix[0] = [56.3, 48.6]
    u = synth.pixel2equa(f0.bands[0], pix)
    flux5 = np.full((S, 5), 3.0)
    flux5[:, :Bf] = f0.src["flux"]
    flux5[0, :Bf] = 60.0
    imgs = cel.ImageSet(ctx, f0.bands, Hf, Wf)
    cat = cel.SourceSet(ctx, S, Bf).set(f0.src["type"], u, flux5[:, :Bf] / f0.bands[None, :, 2] * f0.bands[None, :, 1], f0.src["shape"])
    imgs.render(cat)
    imgs.set_nelec(np.random.RandomState(4).poisson(imgs.model_images()).astype(np.float64))

    def chain(conditional):
        gf = celeste_mcmc.GibbsField(imgs, list(range(Bf)), f0.bands[:, 2], f0.bands[:, 1], Hf * Wf)
        g = celeste_mcmc.ModelGibbs([gf], f0.src["type"], u, flux5, f0.src["shape"], seed=5, conditional=conditional)
        g.resample_photons()
        return g, gf

    g, gf = chain("reference")
    idx = np.arange(S)
    U = u + np.random.RandomState(2).normal(0, 2e-5, (S, 2))
    ll, gr = g.location_loglik_grad(idx, U)
    assert np.array_equal(ll, g.location_loglik(idx, U))
    res = gf.iset.patch_loglik_resident_grad(gf.prop, idx.astype(np.int32))
    assert np.array_equal(gr, res[1]) and np.array_equal(ll, res[0]) and np.any(gr != 0.0)
    # gradient ascent on source 0's conditional: the step is a Newton-like one for a Gaussian PSF core, photons x 1 / sigma^2
    one = np.array([0])
    px = 1.1e-4                                              # degrees per pixel of the synthetic WCS
    n_phot = float(np.sum(gf.sums[0]))
    assert n_phot > 1000
    step = (1.5 * px) ** 2 / n_phot                          # deg^2 per unit of d ll / d deg: ~ sigma^2 / N, sigma = 1.5 px

    def ascend(start):
        x = start.copy()
        for _ in range(20):
            _, gg = g.location_loglik_grad(one, x[None, :])
            x = x + step * gg[0]
        return x

    top = ascend(u[0])
    back = ascend(u[0] + np.array([0.3 * px / np.cos(np.deg2rad(u[0, 1])), 0.0]))
    d = (back - top) * np.array([np.cos(np.deg2rad(u[0, 1])), 1.0]) / px
    print("gradient ascent: %.4f px from the conditional's maximum after 20 steps (started 0.3 px away)" % np.hypot(*d))
    assert np.hypot(*d) <= 0.05
    ge, _ = chain("exact")
    with pytest.raises(ValueError):
        ge.location_loglik_grad(idx, U)


# ---- 6 (no GPU) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import desi_mcmc_amd
    return desi_mcmc_amd


def test_header_constant_and_the_frozen_boundary(built):
    import subprocess
    from desi_mcmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    doc = header[header.index("/* ---- per-source conditional log-likelihoods"):header.index("int cel_patch_loglik(")]
    assert re.search(r"mode 8 \+ m", doc) and "CEL_PLL_GRAD = 8" in doc and "P * (7 + B) doubles" in doc
    assert "row window" in doc and "CEL_ERR_INVALID" in doc and "Slot 0 and slots 1 .. differ" in doc
    assert _lib.CEL_PLL_GRAD == 8
    # the boundary: 56 symbols, CEL_K_COUNT = 15, as tests/test_masked_host.py reads them
    assert re.search(r"CEL_K_COUNT = 15\b", header)
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    bound = [s[0] for s in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) == 56 and declared == exported == set(bound)
    assert _lib.lib().cel_abi_version() == 1
    assert not hasattr(_lib, "CEL_OPT_PATCH_GRAD") and max(_lib.KERNELS.values()) == 14


def test_resource_table_and_budget(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    k = resource_usage.collect()
    mine = sorted(n for n in k if n.startswith("k_patch_grad<"))
    assert mine == ["k_patch_grad<0, double>", "k_patch_grad<0, int>", "k_patch_grad<1, double>", "k_patch_grad<2, double>"], sorted(k)
    budget = __import__("json").load(open(resource_usage.BUDGET))["kernels"]
    tab = resource_usage.table(k)
    for n in mine:
        assert k[n]["scratch"] == 0 and k[n]["vgpr_spill"] == 0 and k[n]["occupancy"] >= 4 and k[n]["vgpr"] <= 128
        assert "| `%s` |" % n in tab and n in budget and budget[n]["min_occupancy"] == 4 and budget[n]["max_scratch"] == 0
    assert "k_patch_grad_chain" in k
    assert not [m for m in resource_usage.check(k) if m.startswith("k_patch_grad")]
