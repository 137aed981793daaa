"""cel_loglik_grad: the gradient of the field log-likelihood with every source's box held fixed (k_grad.h).

  1. the seven per-(source, band) sums restated in numpy from the oracle's component tables and lambda, taken to the public
     coordinates through the Jacobian of the smooth parameter map (pixel position, W) -- at T = 0 (nothing dropped)
  2. end-to-end central differences of the box-restricted log-likelihood (the chain rule, cos(dec) term included)
  3. the shipping drop thresholds against T = 0
  4. d ll / d counts = xtilde / counts - mass (cel_estep_stats) on the benchmark field
  5. API properties;  6. plain gradient ascent on positions only
"""
import ctypes as C

import numpy as np
import pytest

from conftest import tail_log

pytestmark = pytest.mark.gpu

H, W, B = 192, 256, 3


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


def _prof(orc):
    ea, ev, da, dv = orc.profile_tables()
    return np.concatenate([ea, da]), np.concatenate([ev, dv])


def _type2_comps(band, pxy, th, Wm, orc):
    """(A, A', mean, cov, var) of a type-2 galaxy: PSF x profile, W given"""
    amp, var = _prof(orc)
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    out = []
    for j in range(14):
        tf, sg = (th, 1.0) if j < 6 else (1.0 - th, -1.0)
        for k in range(3):
            base = amp[j] * w[k]
            out.append((tf * base, sg * base, pxy + mu[k], var[j] * Wm + cov[k], var[j]))
    return out


def _comps(band, typ, radec, shape, orc):
    """the components of one source in one band, the oracle's tables (type 0 / 1) or the same construction (type 2)"""
    w, mu, cov = band[3:6], band[6:12].reshape(3, 2), band[12:24].reshape(3, 2, 2)
    if typ == 0:
        v = orc.equa2pixel(band, radec)
        return [(w[k], 0.0, v + mu[k], cov[k], 0.0) for k in range(3)]
    if typ == 2:
        Wm = np.array([[shape[1], shape[2]], [shape[2], shape[3]]])
        return _type2_comps(band, orc.equa2pixel(band, radec), shape[0], Wm, orc)
    amp, var = _prof(orc)
    pis, means, covs, _, _ = orc.galaxy_table(band, shape, radec)
    out = []
    for i in range(42):
        j, k = divmod(i, 3)
        sg = 1.0 if j < 6 else -1.0
        out.append((pis[i], sg * amp[j] * w[k], means[i], covs[i], var[j]))
    return out


def _patch(comps, box):
    y0, y1, x0, x1 = box
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=float), np.arange(y0, y1, dtype=float))
    u = np.zeros(X.shape)
    for A, _, m, Cm, _ in comps:
        P = np.linalg.inv(Cm)
        dx, dy = X - m[0], Y - m[1]
        q = P[0, 0] * dx * dx + 2 * P[0, 1] * dx * dy + P[1, 1] * dy * dy
        u += A * np.exp(-0.5 * q) / (2 * np.pi * np.sqrt(np.linalg.det(Cm)))
    return u


def _seven(comps, box, r):
    """S_u, S_m (2), S_W (00, 01, 11), S_th of k_grad.h over the box"""
    y0, y1, x0, x1 = box
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=float), np.arange(y0, y1, dtype=float))
    out = np.zeros(7)
    for A, Ab, m, Cm, var in comps:
        P = np.linalg.inv(Cm)
        dx, dy = X - m[0], Y - m[1]
        pdx, pdy = P[0, 0] * dx + P[0, 1] * dy, P[1, 0] * dx + P[1, 1] * dy
        N = np.exp(-0.5 * (dx * pdx + dy * pdy)) / (2 * np.pi * np.sqrt(np.linalg.det(Cm)))
        g = A * N
        out[0] += np.sum(r * g)
        out[1] += np.sum(r * g * pdx)
        out[2] += np.sum(r * g * pdy)
        out[3] += np.sum(r * 0.5 * var * g * (pdx * pdx - P[0, 0]))
        out[4] += np.sum(r * 0.5 * var * g * (pdx * pdy - P[0, 1]))
        out[5] += np.sum(r * 0.5 * var * g * (pdy * pdy - P[1, 1]))
        out[6] += np.sum(r * Ab * N)
    return out


def _param_map(band, typ, radec, shape, orc):
    """(px, py, W00, W01, W11) of a source in a band: what its components depend on besides theta"""
    if typ == 1:
        _, _, _, pxy, tinv = orc.galaxy_table(band, shape, radec)
        Wm = tinv @ tinv.T
        return np.array([pxy[0], pxy[1], Wm[0, 0], Wm[0, 1], Wm[1, 1]])
    p = orc.equa2pixel(band, radec)
    return np.array([p[0], p[1], 0.0, 0.0, 0.0])


def _catalogue(bands, seed=7, S=48):
    """the scene's catalogue (no device work) and the generator, left where the perturbed catalogue's draws begin"""
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(seed)
    pix = np.column_stack([rs.uniform(12, W - 12, S), rs.uniform(12, H - 12, S)])
    typ = (rs.rand(S) < 0.55).astype(np.int32)
    typ[:3] = [1, 2, 2]
    shape = np.column_stack([rs.uniform(0.1, 0.9, S), np.exp(rs.uniform(np.log(0.4), np.log(3.0), S)),
                             rs.uniform(0, 180, S), rs.uniform(0.3, 0.95, S)])
    shape[0, 1] = 0.02                                           # below k_prep's floor 1/30
    shape[1] = [0.35, 1.2, 0.3, 0.9]                             # type 2: theta, W00, W01, W11
    shape[2] = [1.0, 0.8, -0.2, 1.5]
    shape[(typ == 0)] = 0.0
    counts = np.exp(rs.uniform(np.log(300.0), np.log(3e4), size=(S, B)))
    radec = synth.pixel2equa(bands[0], pix)
    return dict(pix=pix, typ=typ, shape=shape, counts=counts, radec=radec), rs


def _scene(cel, ctx, seed=7, S=48, bands=None):
    """~48 stars and galaxies over 3 bands at 192 x 256: one galaxy below the sigma floor, two of type 2 (theta 0.35 and
    1); nelec drawn from a catalogue perturbed away from the one the gradient is taken at.  bands: the band records
    (synth.make_bands' unless given)"""
    from desi_mcmc_amd import synth
    if bands is None:
        bands = synth.make_bands(H, W, B)
    cat, rs = _catalogue(bands, seed, S)
    pix, typ, shape, counts, radec = cat["pix"], cat["typ"], cat["shape"], cat["counts"], cat["radec"]
    # the observed image: a render of the catalogue moved by ~0.3 px and 5 % in counts, with Poisson noise
    radec_t = synth.pixel2equa(bands[0], pix + rs.normal(0, 0.3, (S, 2)))
    iset = cel.ImageSet(ctx, bands, H, W)
    sset = cel.SourceSet(ctx, S, B).set(typ, radec_t, counts * rs.uniform(0.95, 1.05, (S, B)), shape)
    iset.render(sset)
    nelec = rs.poisson(iset.model_images()).astype(np.float64)
    iset.set_nelec(nelec)
    sset = cel.SourceSet(ctx, S, B).set(typ, radec, counts, shape)
    return dict(bands=bands, typ=typ, radec=radec, counts=counts, shape=shape, nelec=nelec, iset=iset, sset=sset, S=S)


@pytest.fixture(scope="module")
def scene(cel, ctx):
    return _scene(cel, ctx)


def _oracle_lambda(sc, boxes, orc):
    """lambda of the scene from the oracle's render (types 0 / 1) plus the type-2 stamps on the library's boxes"""
    bands, typ = sc["bands"], sc["typ"]
    ob = bands.copy()
    ob[:, 36] = [orc.checked_radius(ob[b], sc["iset"].band(b)[36]) for b in range(B)]
    keep = typ != 2
    lam, _, _ = orc.render_field(ob, H, W, typ[keep], sc["radec"][keep], sc["counts"][keep], sc["shape"][keep])
    for s in np.nonzero(~keep)[0]:
        for b in range(B):
            bx = boxes[b, s]
            if bx[1] > bx[0] and bx[3] > bx[2]:
                lam[b, bx[0]:bx[1], bx[2]:bx[3]] += sc["counts"][s, b] * _patch(_comps(ob[b], 2, sc["radec"][s], sc["shape"][s], orc), bx)
    return ob, lam


def _restated_grad(sc, orc):
    """(g_radec, g_counts, g_shape) from the numpy sums and the parameter map's Jacobian"""
    S, typ, radec, shape, counts = sc["S"], sc["typ"], sc["radec"], sc["shape"], sc["counts"]
    boxes, status = sc["iset"].source_boxes(sc["sset"])
    ob, lam = _oracle_lambda(sc, boxes, orc)
    r_all = sc["nelec"] / lam - 1.0
    gr, gc, gs = np.zeros((S, 2)), np.zeros((S, B)), np.zeros((S, 4))
    for s in range(S):
        for b in range(B):
            bx = boxes[b, s]
            if status[b, s] <= 0 or bx[1] <= bx[0] or bx[3] <= bx[2]:
                continue
            q = _seven(_comps(ob[b], typ[s], radec[s], shape[s], orc), bx, r_all[b, bx[0]:bx[1], bx[2]:bx[3]])
            c = counts[s, b]
            gc[s, b] = q[0]
            dv = c * np.array([q[1], q[2], q[3], 2.0 * q[4], q[5]])       # d ll / d (px, py, W00, W01, W11)
            if typ[s] == 2:
                gs[s] += [c * q[6], dv[2], dv[3], dv[4]]
                J = np.zeros((2, 5))
                for i, h in enumerate((1e-6, 1e-6)):
                    e = np.zeros(2); e[i] = h
                    J[i] = (_param_map(ob[b], 0, radec[s] + e, shape[s], orc) - _param_map(ob[b], 0, radec[s] - e, shape[s], orc)) / (2 * h)
                gr[s] += J @ dv
                continue
            for i, h in enumerate((1e-6, 1e-6)):
                e = np.zeros(2); e[i] = h
                d = (_param_map(ob[b], typ[s], radec[s] + e, shape[s], orc) - _param_map(ob[b], typ[s], radec[s] - e, shape[s], orc)) / (2 * h)
                gr[s, i] += d @ dv
            if typ[s] == 1:
                gs[s, 0] += c * q[6]
                for i, h in ((1, 1e-4 * shape[s, 1]), (2, 1e-4), (3, 1e-5)):
                    e = np.zeros(4); e[i] = h
                    d = (_param_map(ob[b], 1, radec[s], shape[s] + e, orc) - _param_map(ob[b], 1, radec[s], shape[s] - e, orc)) / (2 * h)
                    gs[s, i] += d @ dv
    return gr, gc, gs


def _close(got, want, rtol):
    """per entry relative, with a floor of rtol * max |column| for the entries near zero"""
    floor = rtol * np.max(np.abs(want), axis=0, keepdims=True)
    bad = np.abs(got - want) > np.maximum(rtol * np.abs(want), floor)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def test_grad_matches_numpy_restatement(ctx, scene, orc):
    """the seven sums and the chain rule against the test's own statement of them, nothing dropped anywhere"""
    with tail_log(ctx, 0.0):
        ll, gr, gc, gs = scene["iset"].loglik_grad(scene["sset"])
    wr, wc, ws = _restated_grad(scene, orc)
    _close(gc, wc, 1e-8)
    _close(gr, wr, 1e-8)
    gal = scene["typ"] != 0
    _close(gs[gal], ws[gal], 1e-8)
    assert np.all(gs[~gal] == 0.0)
    assert gs[0, 1] == 0.0                                        # sigma below the floor
    assert np.all(np.abs(gs[gal & (np.arange(scene["S"]) != 0), 1]) > 0)


def _box_dll(sc, s, plus, minus, lam, boxes, ob, orc):
    """ll(plus) - ll(minus) of source s on its FIXED boxes, summed over bands, formed per pixel as a difference (so that
    the sum's rounding stays far below the change); plus / minus = (radec, shape)"""
    tot = 0.0
    for b in range(B):
        bx = boxes[b, s]
        if bx[1] <= bx[0] or bx[3] <= bx[2]:
            continue
        ys, xs = slice(bx[0], bx[1]), slice(bx[2], bx[3])
        c = sc["counts"][s, b]
        old = _patch(_comps(ob[b], sc["typ"][s], sc["radec"][s], sc["shape"][s], orc), bx)
        dp = c * (_patch(_comps(ob[b], sc["typ"][s], plus[0], plus[1], orc), bx) - old)
        dm = c * (_patch(_comps(ob[b], sc["typ"][s], minus[0], minus[1], orc), bx) - old)
        l0 = lam[b, ys, xs]
        tot += np.sum(sc["nelec"][b, ys, xs] * (np.log1p(dp / l0) - np.log1p(dm / l0)) - (dp - dm))
    return tot


def test_grad_central_differences(ctx, cel, scene, orc):
    """end to end: d ll / d parameter against central differences of the log-likelihood with the boxes held fixed (and
    checked to be the boxes the library forms at +- h)"""
    with tail_log(ctx, 0.0):
        _, gr, gc, gs = scene["iset"].loglik_grad(scene["sset"])
    sc = scene
    boxes, _ = sc["iset"].source_boxes(sc["sset"])
    ob, lam = _oracle_lambda(sc, boxes, orc)
    one = cel.SourceSet(ctx, 1, B)

    def box_of(s, radec, shape):
        one.set(sc["typ"][s:s + 1], radec[None, :], sc["counts"][s:s + 1], shape[None, :])
        return sc["iset"].source_boxes(one)[0][:, 0]

    checked = 0
    for s in range(sc["S"]):
        base = box_of(s, sc["radec"][s], sc["shape"][s])
        assert np.array_equal(base, boxes[:, s]), (s, base, boxes[:, s])
        params = [("u", 0, 1e-7), ("u", 1, 1e-7)]
        if sc["typ"][s] == 1:
            params += [("sh", 1, 1e-6 * sc["shape"][s, 1]), ("sh", 2, 1e-4), ("sh", 3, 1e-6)]
        if sc["typ"][s] == 2:
            params += [("sh", 1, 1e-6), ("sh", 2, 1e-6), ("sh", 3, 1e-6)]
        for kind, i, h in params:
            # a box edge within h of the point: smaller steps (the derivative holds on the box's own piece), else skip
            for h in (h, 0.1 * h, 0.01 * h):
                pts = []
                for sgn in (1.0, -1.0):
                    ra, sh = sc["radec"][s].copy(), sc["shape"][s].copy()
                    (ra if kind == "u" else sh)[i] += sgn * h
                    pts.append((ra, sh))
                if all(np.array_equal(box_of(s, *p), base) for p in pts):
                    break
            else:
                continue
            fd = _box_dll(sc, s, pts[0], pts[1], lam, boxes, ob, orc) / (2 * h)
            got = gr[s, i] if kind == "u" else gs[s, i]
            ref = np.abs(gr[:, i]).max() if kind == "u" else np.abs(gs[sc["typ"] == sc["typ"][s], i]).max()
            assert abs(got - fd) <= 1e-6 * max(abs(fd), 1e-3 * ref), (s, kind, i, got, fd)
            checked += 1
    assert checked > 2 * sc["S"]


def test_grad_shipping_defaults_against_strict(ctx, scene):
    """the shipping thresholds (render 24, per-source 32) against nothing dropped: within 1e-7 of each column's largest
    entry (k_grad.h: the drop rule's own share is below 4e-11; the render's T = 24 moves every r(p) by <= n e^-24 nelec / lambda)"""
    with tail_log(ctx, 0.0):
        s_ = scene["iset"].loglik_grad(scene["sset"])
    d_ = scene["iset"].loglik_grad(scene["sset"])
    for got, want in zip(d_[1:], s_[1:]):
        floor = 1e-7 * np.max(np.abs(want), axis=0, keepdims=True)
        assert np.all(np.abs(got - want) <= floor + 1e-7 * np.abs(want))
    assert abs(d_[0] - s_[0]) <= 1e-9 * abs(s_[0])


def test_grad_counts_is_estep_identity_on_benchmark_field(ctx):
    """d ll / d counts = xtilde / counts - mass on configs[2] (10 000 sources, 5 bands, 2048^2)"""
    from desi_mcmc_amd import synth
    f = synth.SyntheticField.from_config(ctx, "mixed10k_2048")
    ll, gr, gc, gs = f.images.loglik_grad(f.sources)
    xt, ms, _ = f.images.estep_stats(f.sources)
    counts = f.src["counts"]
    want = xt / counts - ms
    assert np.all(np.abs(gc - want) <= 1e-9 * (xt / counts + ms))
    assert np.all(np.isfinite(gr)) and np.all(np.isfinite(gs))
    ll_r, _ = f.images.render(f.sources, loglik=True)
    assert ll == ll_r


def test_grad_api_properties(ctx, cel, scene):
    from desi_mcmc_amd import _lib as L
    iset, sset, S = scene["iset"], scene["sset"], scene["S"]
    a = iset.loglik_grad(sset)
    b = iset.loglik_grad(sset)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    ll_r, _ = iset.render(sset, loglik=True)
    assert a[0] == b[0] == ll_r                                   # bit for bit cel_render_field's
    # NULL outputs
    tot = C.c_double(0.0)
    L.check(L.lib().cel_loglik_grad(iset._h, sset._h, C.byref(tot), None, None, None, L.CEL_HOST))
    assert tot.value == ll_r
    gc = np.zeros((S, B))
    L.check(L.lib().cel_loglik_grad(iset._h, sset._h, None, None, gc.ctypes.data, None, L.CEL_HOST))
    assert np.array_equal(gc, a[2])
    # device outputs
    hip = C.CDLL(L.LIB_PATH)                      # dlsym through the library finds the HIP runtime it is linked to
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    outs = [np.zeros((S, 2)), np.zeros((S, B)), np.zeros((S, 4))]
    dptr = []
    for h in outs:
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), h.nbytes) == 0
        dptr.append(d)
    try:
        L.check(L.lib().cel_loglik_grad(iset._h, sset._h, None, dptr[0], dptr[1], dptr[2], L.CEL_DEVICE))
        for h, d in zip(outs, dptr):
            assert hip.hipMemcpy(h.ctypes.data, d, h.nbytes, 2) == 0
    finally:
        for d in dptr:
            hip.hipFree(d)
    for h, want in zip(outs, a[1:]):
        assert np.array_equal(h, want)
    # no nelec; a row window
    bare = cel.ImageSet(ctx, scene["bands"], H, W)
    with pytest.raises(ValueError):
        bare.loglik_grad(sset)
    win = cel.ImageSet(ctx, scene["bands"], 128, W)
    win.set_window(32, H)
    win.set_nelec(scene["nelec"][:, 32:160])
    with pytest.raises(ValueError):
        win.loglik_grad(sset)


def test_multi_image_grad(ctx, cel):
    """celeste_likelihood_multi_image_grad: the ll of celeste_likelihood_multi_image, "fluxes" = "counts" chained"""
    from desi_mcmc_amd import celeste, synth
    f = synth.SyntheticField(ctx, 40, 5, 128, 160, frac_gal=0.5, seed=11)
    imgs = synth.fits_images(f)
    fl5 = f.flux5()
    srcs = [cel.SrcParams(u=f.src["radec"][s], a=int(f.src["type"][s]), fluxes=fl5[s], theta=f.src["shape"][s, 0],
                          sigma=f.src["shape"][s, 1], phi=f.src["shape"][s, 2], rho=f.src["shape"][s, 3]) for s in range(f.S)]
    srcs.append(cel.SrcParams(u=f.src["radec"][0], a=None, fluxes=fl5[0]))      # kappa * flux
    ll, g = celeste.celeste_likelihood_multi_image_grad(srcs, imgs)
    assert ll == celeste.celeste_likelihood_multi_image(srcs, imgs)
    assert g["u"].shape == (41, 2) and g["counts"].shape == (41, 5) and g["shape"].shape == (41, 4)
    kappa = np.array([im.kappa for im in imgs])
    calib = np.array([im.calib for im in imgs])
    want = g["counts"] * (kappa / calib)[None, :]
    want[-1] = g["counts"][-1] * kappa
    np.testing.assert_array_equal(g["fluxes"], want)
    assert np.any(g["counts"] != 0.0)


def test_gradient_ascent_recovers_positions(ctx, cel):
    """20 steps of fixed-size gradient ascent on positions alone, from ~0.5 px off: ll rises at every step and every source
    ends closer to its true position"""
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(3)
    h, w, nb, S = 96, 128, 3, 10
    bands = synth.make_bands(h, w, nb)
    pix = np.column_stack([rs.uniform(20, w - 20, S), rs.uniform(20, h - 20, S)])
    typ = (np.arange(S) % 2).astype(np.int32)
    shape = np.where(typ[:, None] == 1, np.column_stack([np.full(S, 0.5), np.full(S, 0.8), rs.uniform(0, 180, S),
                                                         np.full(S, 0.7)]), 0.0)
    counts = np.full((S, nb), 3000.0)
    truth = synth.pixel2equa(bands[0], pix)
    iset = cel.ImageSet(ctx, bands, h, w)
    sset = cel.SourceSet(ctx, S, nb).set(typ, truth, counts, shape)
    iset.render(sset)
    iset.set_nelec(iset.model_images())                           # noise-free: the truth is the maximum
    ang = rs.uniform(0, 2 * np.pi, S)
    start = pix + 0.5 * np.column_stack([np.cos(ang), np.sin(ang)])
    radec = synth.pixel2equa(bands[0], start)
    # pixels per degree and a fixed diagonal preconditioner (counts over the PSF's variance, an over-estimate of the curvature)
    ups_inv = bands[0, 32:36].reshape(2, 2)
    J = ups_inv @ np.diag([np.cos(bands[0, 27] / 180 * np.pi), 1.0])          # d pix / d (ra, dec)
    psf_var = np.array([np.sum(bands[b, 3:6] * bands[b, 12:24].reshape(3, 2, 2)[:, 0, 0]) for b in range(nb)])
    curv = np.sum(counts / psf_var[None, :], axis=1)
    lls = []
    for it in range(21):                                          # 21 evaluations, 20 steps
        sset.set(typ, radec, counts, shape)
        ll, gr, _, _ = iset.loglik_grad(sset)
        lls.append(ll)
        if it == 20:
            break
        g_pix = gr @ np.linalg.inv(J)                             # d ll / d pix = J^-T d ll / d u
        step_pix = 0.15 * g_pix / curv[:, None]
        radec = radec + step_pix @ np.linalg.inv(J).T
    assert np.all(np.diff(lls) > 0), lls
    end = (radec - truth) @ J.T                                   # pixel offsets from the truth
    assert np.all(np.hypot(end[:, 0], end[:, 1]) < 0.9 * np.hypot(*(start - pix).T)), end
