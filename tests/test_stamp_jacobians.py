"""Derivative stamps: cel_render_stamps(scaled = 2 | 3), ImageSet.stamp_jacobians, celeste.gen_src_image_jac (k_stamp_jac.h).

  1. contracted with r = nelec / lambda - 1 over the boxes and summed over the bands, the planes ARE cel_loglik_grad
  2. plane 0 is the stamp of cel_render_stamps(scaled = 0 | 1) under the direct kernel, caller limits included
  3. every derivative plane against Richardson-combined central differences of a CPU restatement on the fixed box
  4. layout, refusals, device output, repeatability, the profile bracket, both kernel settings
  5. a windowed image set;  6. the mirror;  7. (no GPU) header, symbols, resource table

The scene is test_loglik_grad.py's (192 x 256, 3 bands, 48 sources: one galaxy under the sigma floor, two of type 2 with theta
0.35 and 1), restated here, plus a galaxy whose box spans several chunks both ways, a star cut by the frame's edge and a star
that fails the overlap test.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import tail_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B = 192, 256, 3
S_BASE = 48
S_BIG, S_EDGE, S_MISS = S_BASE, S_BASE + 1, S_BASE + 2       # the three sources added to the scene
S_FLOOR, S_T2, S_T2_EXP = 0, 1, 2                            # sigma under the floor; type 2 with theta 0.35 and theta 1

gpu = pytest.mark.gpu


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


def _scene(cel, ctx, seed=7, S=S_BASE, bands=None):
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(seed)
    if bands is None:
        bands = synth.make_bands(H, W, B)
    pix = np.column_stack([rs.uniform(12, W - 12, S), rs.uniform(12, H - 12, S)])
    typ = (rs.rand(S) < 0.55).astype(np.int32)
    typ[:3] = [1, 2, 2]
    shape = np.column_stack([rs.uniform(0.1, 0.9, S), np.exp(rs.uniform(np.log(0.4), np.log(3.0), S)),
                             rs.uniform(0, 180, S), rs.uniform(0.3, 0.95, S)])
    shape[S_FLOOR, 1] = 0.02                                     # below k_prep's floor 1/30
    shape[S_T2] = [0.35, 1.2, 0.3, 0.9]                          # type 2: theta, W00, W01, W11
    shape[S_T2_EXP] = [1.0, 0.8, -0.2, 1.5]
    shape[(typ == 0)] = 0.0
    counts = np.exp(rs.uniform(np.log(300.0), np.log(3e4), size=(S, B)))
    # on the same frame: a galaxy over several chunks both ways, a star cut by the frame's edge, a star failing the overlap test
    pix = np.vstack([pix, [[128.4, 96.3], [2.3, 50.7], [-60.0, 80.0]]])
    typ = np.concatenate([typ, [1, 0, 0]]).astype(np.int32)
    shape = np.vstack([shape, [[0.5, 3.0, 30.0, 0.6], [0.0] * 4, [0.0] * 4]])
    counts = np.vstack([counts, np.full((3, B), 5000.0)])
    S = S + 3
    # counts as FitsImage.nmgy2counts forms them from a flux, so that the mirror's SrcParams give the same doubles
    flux = counts * bands[None, :, 2] / bands[None, :, 1]
    counts = (flux / bands[None, :, 2]) * bands[None, :, 1]
    radec = synth.pixel2equa(bands[0], pix)
    radec_t = synth.pixel2equa(bands[0], pix + rs.normal(0, 0.3, (S, 2)))
    iset = cel.ImageSet(ctx, bands, H, W)
    sset = cel.SourceSet(ctx, S, B).set(typ, radec_t, counts * rs.uniform(0.95, 1.05, (S, B)), shape)
    iset.render(sset)
    nelec = rs.poisson(iset.model_images()).astype(np.float64)
    iset.set_nelec(nelec)
    sset = cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape)
    return dict(bands=bands, typ=typ, radec=radec, counts=counts, flux=flux, shape=shape, nelec=nelec, iset=iset, sset=sset, S=S)


@pytest.fixture(scope="module")
def scene(cel, ctx):
    return _scene(cel, ctx)


@pytest.fixture(scope="module")
def jac(ctx, scene):
    return _jac(ctx, scene)


def _jac(ctx, scene):
    """the calls every test shares: the gradient and lambda with nothing dropped, and per band the scaled = 3 and scaled = 2
    planes on the sources' own boxes"""
    iset, sset = scene["iset"], scene["sset"]
    with tail_log(ctx, 0.0):
        ll, gr, gc, gs = iset.loglik_grad(sset)
        lam = iset.model_images()
    p3, p2, boxes = [], [], []
    for b in range(B):
        a, bx = iset.stamp_jacobians(sset, b, scaled=True)
        u, bx2 = iset.stamp_jacobians(sset, b, scaled=False)
        assert np.array_equal(bx, bx2)
        p3.append(a); p2.append(u); boxes.append(bx)
    return dict(gr=gr, gc=gc, gs=gs, lam=lam, p3=p3, p2=p2, boxes=boxes)


def _nplanes(t):
    return 7 if t in (1, 2) else 3


# ---- 1 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_planes_contract_to_loglik_grad(scene, jac):
    """sum_b sum_p r_b(p) plane(p) = g_radec / g_shape (scaled = 3) and = g_counts (scaled = 2, plane 0), both thresholds 0.
    Bound 1e-10 sum |r plane|: fp64 sums of <= ~1e5 terms in two orders (n 2^-53 of the absolute sum) plus ~1e-13 per term
    of exp and chain-rule rounding."""
    S, typ = scene["S"], scene["typ"]
    r = scene["nelec"] / jac["lam"] - 1.0
    worst = 0.0
    seen = 0
    for s in range(S):
        acc, mag = np.zeros(6), np.zeros(6)
        for b in range(B):
            P3, P2 = jac["p3"][b][s], jac["p2"][b][s]
            assert (P3 is None) == (P2 is None)
            if P3 is None:
                assert jac["gc"][s, b] == 0.0
                continue
            y0, y1, x0, x1 = jac["boxes"][b][s]
            rb = r[b, y0:y1, x0:x1]
            assert P3.shape == (_nplanes(typ[s]), y1 - y0, x1 - x0) == P2.shape
            t = rb * P2[0]
            d, m = abs(np.sum(t) - jac["gc"][s, b]), np.sum(np.abs(t))
            assert d <= 1e-10 * m, ("counts", s, b, d, m)
            worst = max(worst, d / m)
            for i in range(1, P3.shape[0]):
                t = rb * P3[i]
                acc[i - 1] += np.sum(t)
                mag[i - 1] += np.sum(np.abs(t))
            seen += 1
        want = np.concatenate([jac["gr"][s], jac["gs"][s]])
        for i in range(6):
            d = abs(acc[i] - want[i])
            assert d <= 1e-10 * mag[i], (s, i, acc[i], want[i], mag[i])
            if mag[i] > 0:
                worst = max(worst, d / mag[i])
        if typ[s] == 0:
            assert np.all(jac["gs"][s] == 0.0)
    assert seen > 2 * S
    print("identity with cel_loglik_grad: worst |difference| / sum |r plane| = %.3g" % worst)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------
def _limits_cases(scene, boxes):
    """caller limits for band 0: every source's own box, but one star's limits moved off its centre, one galaxy's box empty"""
    typ = scene["typ"]
    lim = boxes.copy()
    star = [s for s in range(3, S_BASE) if typ[s] == 0 and boxes[s, 1] > boxes[s, 0]][0]
    galaxy = [s for s in range(3, S_BASE) if typ[s] == 1][0]
    y0, y1, x0, x1 = boxes[star]
    w = x1 - x0
    lim[star] = [y0, y1, x1 + 3, x1 + 3 + w] if x1 + 3 + w <= W else [y0, y1, x0 - 3 - w, x0 - 3]     # beside the source's own box
    lim[galaxy] = [lim[galaxy][0], lim[galaxy][0], lim[galaxy][2], lim[galaxy][3]]                # no rows
    lim[S_MISS] = [70, 90, 0, 12]                                                                  # a miss stays a miss
    return lim, star, galaxy


@gpu
def test_plane_zero_is_the_stamp(ctx, scene, jac):
    """scaled = 2 against 0 and 3 against 1 under CEL_OPT_KERNEL = 0 (k_stamps: nothing dropped, make_comp's form):
    |difference| <= 1e-12 max |stamp| -- per term the relative error is at most (h + a few) 2^-53 with h <= 745"""
    from desi_mcmc_amd import _lib as L
    iset, sset = scene["iset"], scene["sset"]
    before = ctx.get_option(L.CEL_OPT_KERNEL)
    ctx.set_kernel("direct")
    try:
        for b in range(B):
            for scaled, planes in ((False, jac["p2"][b]), (True, jac["p3"][b])):
                st, bx = iset.stamps(sset, b, scaled=scaled)
                assert np.array_equal(bx, jac["boxes"][b])
                for s in range(scene["S"]):
                    assert (st[s] is None) == (planes[s] is None), (b, s)
                    if st[s] is not None:
                        assert np.max(np.abs(planes[s][0] - st[s])) <= 1e-12 * np.max(np.abs(st[s])), (b, s, scaled)
        # caller limits: off the centre, empty, and on the overlap-test miss
        lim, star, galaxy = _limits_cases(scene, jac["boxes"][0])
        for scaled in (False, True):
            st, _ = iset.stamps(sset, 0, scaled=scaled, boxes_in=lim)
            pl, bx = iset.stamp_jacobians(sset, 0, scaled=scaled, boxes_in=lim)
            assert np.array_equal(bx, lim)
            assert [p is None for p in pl] == [p is None for p in st]
            assert pl[galaxy] is None and pl[S_MISS] is None and pl[star] is not None
            cx = 0.5 * (jac["boxes"][0][star, 2] + jac["boxes"][0][star, 3])
            assert not (lim[star, 2] <= cx < lim[star, 3])
            for s in range(scene["S"]):
                if st[s] is not None:
                    assert pl[s].shape == (_nplanes(scene["typ"][s]),) + st[s].shape
                    assert np.max(np.abs(pl[s][0] - st[s])) <= 1e-12 * np.max(np.abs(st[s])), (s, scaled)
            assert np.any(pl[star][1] != 0.0)
    finally:
        ctx.set_option(L.CEL_OPT_KERNEL, before)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------
def _prof(orc):
    ea, ev, da, dv = orc.profile_tables()
    return np.concatenate([ea, da]), np.concatenate([ev, dv])


def _comps(band, typ, radec, shape, orc):
    """(amplitude, mean, covariance) of every component of one source in one band: the oracle's tables (type 0 / 1) or the
    same construction with W given (type 2), as test_loglik_grad.py forms them"""
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


def _patch(comps, box, dtype=np.float64):
    """the unit stamp on the fixed box: sum_k A_k N(p; m_k, C_k), evaluated in `dtype` from the (double) component tables"""
    y0, y1, x0, x1 = box
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=dtype), np.arange(y0, y1, dtype=dtype))
    u = np.zeros(X.shape, dtype=dtype)
    two_pi = 2 * dtype(np.pi)
    for A, m, Cm in zip(*comps):
        a, b, c = dtype(Cm[0, 0]), dtype(Cm[0, 1]), dtype(Cm[1, 1])
        det = a * c - b * b
        dx, dy = X - dtype(m[0]), Y - dtype(m[1])
        q = (c * dx * dx - 2 * b * dx * dy + a * dy * dy) / det
        u += dtype(A) * np.exp(-q / 2) / (two_pi * np.sqrt(det))
    return u


def _steps(t, shape):
    """(plane, kind, index, h) of every parameter of a source: test_loglik_grad.py's steps"""
    out = [(1, "u", 0, 1e-7), (2, "u", 1, 1e-7)]
    if t == 1:
        out += [(3, "sh", 0, 1e-6), (4, "sh", 1, 1e-6 * shape[1]), (5, "sh", 2, 1e-4), (6, "sh", 3, 1e-6)]
    if t == 2:
        out += [(3, "sh", 0, 1e-6), (4, "sh", 1, 1e-6), (5, "sh", 2, 1e-6), (6, "sh", 3, 1e-6)]
    return out


def _central(band, t, radec, shape, kind, i, h, box, orc, dtype=np.float64):
    pts = []
    for sgn in (1.0, -1.0):
        ra, sh = radec.copy(), shape.copy()
        (ra if kind == "u" else sh)[i] += sgn * h
        pts.append((ra, sh))
    step = (pts[0][0][i] - pts[1][0][i]) if kind == "u" else (pts[0][1][i] - pts[1][1][i])
    return (_patch(_comps(band, t, pts[0][0], pts[0][1], orc), box, dtype) - _patch(_comps(band, t, pts[1][0], pts[1][1], orc), box, dtype)) / step


def _richardson(band, t, radec, shape, kind, i, h, box, orc, dtype=np.float64):
    f1 = _central(band, t, radec, shape, kind, i, h, box, orc, dtype)
    f2 = _central(band, t, radec, shape, kind, i, 0.5 * h, box, orc, dtype)
    return (4.0 * f2 - f1) / 3.0


@gpu
@pytest.mark.parametrize("b", range(B))
def test_planes_against_central_differences(scene, jac, orc, b):
    """every derivative plane of the unit stamp (scaled = 2) against fd = (4 fd_{h/2} - fd_h) / 3 of the CPU restatement on
    the fixed box, per plane |plane - fd| <= 1e-7 max |plane|.  The combined truncation term is ~(h / sigma)^4 ~ 1e-12
    relative; a missing chain term (the cos(dec) term, a factor 2 on W01, the pi / 180 of phi) lies orders above the bound.

    The restatement's own rounding: a stamp summed in fp64 carries ~4 x 2^-53 max u, so its difference quotient carries
    ~4 x 2^-53 max u / h.  Against most planes that is 1e-10 to 1e-8 of the plane's largest value.  Against the planes of the
    galaxy under the sigma floor it is not: the galaxy is unresolved, its theta, phi and rho planes are 1e-3 to 6e-6 of u per
    unit, and the fp64 restatement came out 1.4e-7 to 4.8e-7 away from the library on them -- the same distance two fp64
    difference quotients at steps h and 1.3 h lie from each other (2e-7 to 5e-7).  So a plane whose fp64 quotient could carry
    more than a tenth of the bound -- judged from the restatement alone, 4 x 2^-53 max u / h > 1e-8 max |fd| -- is differenced
    again in extended precision (x87 long double, 2^-64) from the same fp64 component tables; two such quotients at h and
    1.3 h agree to 2.5e-8 or better.  Bound, steps and reference are the same for every plane.
    Worst measured |plane - fd| / max |plane|: 1.5e-8, 2.6e-8 and 1.6e-8 in bands 0, 1, 2 (212 planes each, 5 of them in
    extended precision); DESIGN.md section 5d2."""
    typ, bands = scene["typ"], scene["bands"]
    assert np.finfo(np.longdouble).eps < 2e-19
    worst, checked, extended, over = 0.0, 0, 0, []
    for s in range(scene["S"]):
        P = jac["p2"][b][s]
        if P is None:
            continue
        box = jac["boxes"][b][s]
        args = (bands[b], typ[s], scene["radec"][s], scene["shape"][s])
        umax = np.max(_patch(_comps(*args, orc), box))
        for plane, kind, i, h in _steps(typ[s], scene["shape"][s]):
            fd = _richardson(*args, kind, i, h, box, orc)
            if 4 * 2.0 ** -53 * umax / h > 1e-8 * np.max(np.abs(fd)):
                fd = _richardson(*args, kind, i, h, box, orc, np.longdouble).astype(np.float64)
                extended += 1
            top = np.max(np.abs(P[plane]))
            err = np.max(np.abs(P[plane] - fd))
            if not err <= 1e-7 * top:
                over.append((s, plane, err / top if top > 0 else np.inf))
            if top > 0:
                worst = max(worst, err / top)
            checked += 1
    print("band %d: worst |plane - fd| / max |plane| = %.3g over %d planes (%d in extended precision)" % (b, worst, checked, extended))
    assert not over, "(source, plane, |plane - fd| / max |plane|) above 1e-7: %s" % over
    assert checked > 2 * S_BASE
    # the floored galaxy's sigma plane is exactly 0; a theta = 1 type-2 galaxy keeps both profiles in its theta plane
    assert scene["shape"][S_FLOOR, 1] < 1.0 / 30 and np.all(jac["p2"][b][S_FLOOR][4] == 0.0) and np.all(jac["p3"][b][S_FLOOR][4] == 0.0)
    assert np.any(jac["p2"][b][S_FLOOR][5] != 0.0)
    assert scene["shape"][S_T2_EXP, 0] == 1.0 and np.max(np.abs(jac["p2"][b][S_T2_EXP][3])) > 0.0


# ---- 4 ---------------------------------------------------------------------------------------------------------------------
def _raw(scene, band, scaled, offs, out_ptr, mem, boxes_in=None):
    from desi_mcmc_amd import _lib as L
    return L.lib().cel_render_stamps(scene["iset"]._h, scene["sset"]._h, int(band), int(scaled),
                                     boxes_in.ctypes.data_as(L.c_int32_p) if boxes_in is not None else None,
                                     offs.ctypes.data_as(L.c_int64_p), out_ptr, mem)


def _layout(scene, boxes, status):
    area = np.where(status > 0, (boxes[:, 1] - boxes[:, 0]).astype(np.int64) * (boxes[:, 3] - boxes[:, 2]), 0)
    planes = np.array([_nplanes(t) for t in scene["typ"]], dtype=np.int64)
    return area, planes


@gpu
def test_layout_refusals_and_repeatability(ctx, scene, jac):
    from desi_mcmc_amd import _lib as L
    iset, sset, S, typ = scene["iset"], scene["sset"], scene["S"], scene["typ"]
    boxes, status = iset.stamp_boxes(sset, 1)
    area, planes = _layout(scene, boxes, status)
    # the big galaxy spans several chunks both ways, the edge star is cut, the miss is a miss
    assert boxes[S_BIG, 1] - boxes[S_BIG, 0] > 64 and boxes[S_BIG, 3] - boxes[S_BIG, 2] > 32 and status[S_BIG] == 1
    assert boxes[S_EDGE, 2] == 0 and status[S_EDGE] == 1 and status[S_MISS] == -1
    for s in range(S):
        if status[s] > 0:
            assert jac["p3"][1][s].size == planes[s] * area[s] and jac["p3"][1][s].shape[0] == (3 if typ[s] == 0 else 7)
    # sources without a stamp own a slot all the same (sized by the caller): zero-filled in full, sentinel elsewhere untouched
    slot = planes * np.where(status > 0, area, 5)
    offs = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(slot, out=offs[1:])
    assert np.any(status <= 0)
    flat = np.full(int(offs[-1]) + 4, -7.25)
    assert _raw(scene, 1, 3, offs, flat.ctypes.data, L.CEL_HOST) == L.CEL_OK
    assert np.all(flat[offs[-1]:] == -7.25)
    for s in range(S):
        got = flat[offs[s]:offs[s + 1]]
        if status[s] > 0:
            assert np.array_equal(got.reshape(jac["p3"][1][s].shape), jac["p3"][1][s])
        else:
            assert got.size == 5 * planes[s] and np.all(got == 0.0)
    # a slot of 1 x area under scaled = 2: refused before anything is written
    one = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(np.where(status > 0, area, 5), out=one[1:])
    sent = np.full(int(one[-1]), -7.25)
    assert _raw(scene, 1, 2, one, sent.ctypes.data, L.CEL_HOST) == L.CEL_ERR_INVALID
    assert np.all(sent == -7.25)
    assert _raw(scene, 1, 4, offs, flat.ctypes.data, L.CEL_HOST) == L.CEL_ERR_INVALID
    assert _raw(scene, 1, -1, offs, flat.ctypes.data, L.CEL_HOST) == L.CEL_ERR_INVALID
    assert _raw(scene, 1, 4, one, sent.ctypes.data, L.CEL_HOST) == L.CEL_ERR_INVALID and np.all(sent == -7.25)
    # values 0 and 1 still take slots of one plane
    assert _raw(scene, 1, 1, one, sent.ctypes.data, L.CEL_HOST) == L.CEL_OK
    # device output = host output, bit for bit
    hip = C.CDLL(L.LIB_PATH)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    n = int(offs[-1])
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), 8 * n) == 0
    try:
        assert hip.hipMemset(d, 0x55, 8 * n) == 0
        assert _raw(scene, 1, 3, offs, d, L.CEL_DEVICE) == L.CEL_OK
        dev = np.zeros(n)
        assert hip.hipMemcpy(dev.ctypes.data, d, 8 * n, 2) == 0
    finally:
        hip.hipFree(d)
    assert np.array_equal(dev, flat[:n])
    # a catalogue uploaded from device memory (the host holds no copy of its types: the call reads them back): the same bits
    import desi_mcmc_amd as cel
    host = [np.ascontiguousarray(scene["typ"], dtype=np.int32), scene["radec"], scene["counts"], scene["shape"]]
    ptrs = []
    try:
        for h in host:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), h.nbytes) == 0
            ptrs.append(p)
            assert hip.hipMemcpy(p, h.ctypes.data, h.nbytes, 1) == 0
        dset = cel.SourceSet(ctx, S, B).set_device(S, *[p.value for p in ptrs])
        from_dev = np.full(n, -7.25)
        assert L.lib().cel_render_stamps(iset._h, dset._h, 1, 3, None, offs.ctypes.data_as(L.c_int64_p), from_dev.ctypes.data,
                                         L.CEL_HOST) == L.CEL_OK
    finally:
        for p in ptrs:
            hip.hipFree(p)
    assert np.array_equal(from_dev, flat[:n])
    # two calls, and both kernel settings, give the same bits; the launch is bracketed under CEL_K_STAMPS
    before = ctx.get_option(L.CEL_OPT_KERNEL)
    try:
        for kern in ("direct", "recurrence"):
            ctx.set_kernel(kern)
            ctx.profile(True)
            again = np.full(n, -7.25)
            assert _raw(scene, 1, 3, offs, again.ctypes.data, L.CEL_HOST) == L.CEL_OK
            ms, launches = ctx.profile_get("stamps")
            ctx.profile(False)
            assert launches == 1 and ms > 0.0
            assert np.array_equal(again, flat[:n]), kern
    finally:
        ctx.profile(False)
        ctx.set_option(L.CEL_OPT_KERNEL, before)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_windowed_set(cel, ctx, scene, jac):
    """an image set holding rows [32, 160) of the frame: on the rows a box shares with the window the planes are the whole
    frame's to 1e-12 max |plane| (the positions are window-relative: no bit equality)"""
    y_lo, y_hi = 32, 160
    win = cel.ImageSet(ctx, scene["bands"], y_hi - y_lo, W)
    win.set_window(y_lo, H)
    shared = 0
    for b in (0, 2):
        pw, bw = win.stamp_jacobians(scene["sset"], b, scaled=True)
        for s in range(scene["S"]):
            full, fb = jac["p3"][b][s], jac["boxes"][b][s]
            lo, hi = max(fb[0], y_lo), min(fb[1], y_hi)
            if full is None or hi <= lo:
                assert pw[s] is None, (b, s)
                continue
            assert pw[s] is not None and list(bw[s]) == [lo - y_lo, hi - y_lo, fb[2], fb[3]], (b, s, bw[s], fb)
            want = full[:, lo - fb[0]:hi - fb[0], :]
            assert pw[s].shape == want.shape
            for i in range(want.shape[0]):
                assert np.max(np.abs(pw[s][i] - want[i])) <= 1e-12 * np.max(np.abs(full[i])), (b, s, i)
            shared += 1
    assert shared > S_BASE


# ---- 6 ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_mirror(cel, scene, jac):
    """celeste.gen_src_image_jac for one star and one galaxy: the planes of the catalogue call, bit for bit, with its limits;
    ImageSet.stamp_jacobians is None exactly where stamps is"""
    from desi_mcmc_amd import celeste
    from desi_mcmc_amd.fits_image import FitsImage
    b = 1
    r = scene["bands"][b]
    img = FitsImage("ugriz"[b], scene["nelec"][b], epsilon=r[0], kappa=r[1], calib=r[2], weights=r[3:6], means=r[6:12].reshape(3, 2),
                    covars=r[12:24].reshape(3, 2, 2), rho_n=r[24:26], phi_n=r[26:28], Ups_n=r[28:32].reshape(2, 2))
    typ = scene["typ"]
    star = [s for s in range(3, S_BASE) if typ[s] == 0 and jac["p3"][b][s] is not None][0]
    for s in (star, S_BIG, S_MISS):
        fl = np.zeros(5)
        fl[b] = scene["flux"][s, b]
        sh = scene["shape"][s]
        src = cel.SrcParams(u=scene["radec"][s], a=int(typ[s]), fluxes=fl, theta=sh[0], sigma=sh[1], phi=sh[2], rho=sh[3])
        planes, ylim, xlim = celeste.gen_src_image_jac(src, img)
        if s == S_MISS:
            assert planes is None and ylim is None and xlim is None
            continue
        assert celeste.expected_photons(src, img) == scene["counts"][s, b]
        assert (ylim + xlim) == tuple(int(v) for v in jac["boxes"][b][s])
        assert np.array_equal(planes, jac["p3"][b][s])
        # caller limits go through as they do for the stamps
        y0, y1, x0, x1 = jac["boxes"][b][s]
        cut, yl, xl = celeste.gen_src_image_jac(src, img, xlim=(x0 + 1, x1), ylim=(y0, y1 - 2))
        assert yl == (y0, y1 - 2) and xl == (x0 + 1, x1)
        assert np.max(np.abs(cut - jac["p3"][b][s][:, :y1 - y0 - 2, 1:])) <= 1e-12 * np.max(np.abs(planes))
    st, _ = scene["iset"].stamps(scene["sset"], b)
    assert [p is None for p in st] == [p is None for p in jac["p2"][b]] and st[S_MISS] is None


# ---- 7 (no GPU) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    import desi_mcmc_amd
    return desi_mcmc_amd


def test_header_symbols_and_resources(built):
    import subprocess
    from desi_mcmc_amd import _lib
    header = open(os.path.join(ROOT, "include", "celeste_hip.h")).read()
    doc = header[header.index("/* gen_point_source_psf_image"):header.index("int cel_stamp_boxes(")]
    assert re.search(r"\b2, 3 = DERIVATIVE STAMPS", doc) and "planes * area" in doc and "CEL_ERR_INVALID" in doc
    assert "never documented" in doc
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\*?(cel_\w+)\s*\(", header, flags=re.M))
    exported = set(re.findall(r" T (cel_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()))
    assert declared == exported == set(s[0] for s in _lib.SYMBOLS)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import resource_usage
    finally:
        sys.path.pop(0)
    k = resource_usage.collect()
    assert "k_stamp_jac" in k, sorted(k)
    assert k["k_stamp_jac"]["scratch"] == 0 and k["k_stamp_jac"]["vgpr_spill"] == 0
    assert "| `k_stamp_jac` |" in resource_usage.table(k)
    assert "k_stamp_jac" in __import__("json").load(open(resource_usage.BUDGET))["kernels"]
    assert not [m for m in resource_usage.check(k) if m.startswith("k_stamp_jac")]
