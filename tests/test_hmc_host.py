"""The lock-step host HMC engine (desi-mcmc_amd/util/infer/hmc.py) on targets with a known value and gradient.  No GPU.

  1. against a plain per-chain loop on Python floats, bit for bit
  2. reversibility: L steps, negate p, L steps
  3. the energy error is second order in eps
  4. a frozen coordinate keeps its bits
  5. a trajectory that leaves the support: -inf, rejected, and no further grad_fn call for that chain
  6. the accept and reject momentum rule
  7. law: a 1-D standard normal
"""
import math

import numpy as np
import pytest

D = 6
A = np.array([1.0, 0.25, 4.0, 2.0, 0.5, 9.0])            # the Gaussian's precisions
M = np.array([0.3, -1.2, 0.5, 2.0, -0.7, 0.1])           # its means


@pytest.fixture(scope="module")
def hmc():
    import desi_mcmc_amd  # noqa: F401  (makes the package importable under its alias)
    from desi_mcmc_amd.util.infer import hmc as mod
    return mod


def value_fn(idx, Q):
    acc = np.zeros(Q.shape[0])
    for i in range(Q.shape[1]):
        d = Q[:, i] - M[i]
        acc = acc + A[i] * (d * d)
    return -0.5 * acc


def grad_fn(idx, Q):
    return -(A[None, :] * (Q - M[None, :]))


def _chains(n, seed=3):
    rs = np.random.RandomState(seed)
    q0 = M[None, :] + rs.randn(n, D) / np.sqrt(A)[None, :]
    imass = np.exp(rs.uniform(-1.0, 1.0, size=(n, D)))
    p0 = rs.randn(n, D) / np.sqrt(imass)
    return q0, p0, imass


def _plain_chain(q0, p0, imass, eps, L, log_u, inside=None):
    """one chain on Python floats: the arithmetic of the module's docstring, restated"""
    q, p = [float(x) for x in q0], [float(x) for x in p0]
    im = [float(x) for x in imass]

    def v(x):
        acc = 0.0
        for i in range(D):
            d = x[i] - float(M[i])
            acc = acc + float(A[i]) * (d * d)
        return -0.5 * acc

    def g(x):
        return [-(float(A[i]) * (x[i] - float(M[i]))) for i in range(D)]

    def kin(x):
        acc = 0.0
        for i in range(D):
            acc = acc + im[i] * (x[i] * x[i])
        return 0.5 * acc

    dead = False
    gr = g(q)
    p = [p[i] + (0.5 * eps) * gr[i] for i in range(D)]
    for l in range(L):
        q = [q[i] + (eps * im[i]) * p[i] for i in range(D)]
        if inside is not None and not inside(q):
            dead = True
            break
        gr = g(q)
        h = 0.5 * eps if l == L - 1 else eps
        p = [p[i] + h * gr[i] for i in range(D)]
    if dead:
        return list(map(float, q0)), [-float(x) for x in p0], -math.inf, False
    la = (v(q) - v(list(map(float, q0)))) + (kin(list(map(float, p0))) - kin(p))
    if log_u < la:
        return q, p, la, True
    return list(map(float, q0)), [-float(x) for x in p0], la, False


def test_against_a_plain_loop_bit_for_bit(hmc):
    q0, p0, imass = _chains(9)
    rs = np.random.RandomState(8)
    for eps, L in ((0.05, 1), (0.3, 3), (0.9, 7)):
        log_u = np.log(rs.uniform(size=9))
        st = {}
        q, p, la, acc = hmc.hmc_lockstep(q0, p0, imass, eps, L, value_fn, grad_fn, log_u, stats=st)
        assert st["evals"] == 9 * (L + 1) and st["steps"] == L and st["accepted"] == int(acc.sum())
        assert 0 < acc.sum() or eps > 0.5
        for c in range(9):
            qc, pc, lac, accc = _plain_chain(q0[c], p0[c], imass[c], eps, L, log_u[c])
            assert np.array_equal(q[c], np.array(qc)) and np.array_equal(p[c], np.array(pc)), (eps, L, c)
            assert la[c] == lac and bool(acc[c]) == accc, (eps, L, c)


def test_reversibility(hmc):
    q0, p0, imass = _chains(16, seed=5)
    always = np.full(16, -np.inf)
    for eps, L in ((0.1, 5), (0.4, 12)):
        q1, p1, la1, acc1 = hmc.hmc_lockstep(q0, p0, imass, eps, L, value_fn, grad_fn, always)
        assert acc1.all()
        q2, p2, la2, acc2 = hmc.hmc_lockstep(q1, -p1, imass, eps, L, value_fn, grad_fn, always)
        assert acc2.all()
        scale = np.maximum(np.abs(q0), np.abs(q1)).max(axis=0)
        ulp = np.spacing(scale)
        worst = (np.abs(q2 - q0) / ulp[None, :]).max()
        print("REVERSIBILITY eps %g L %d: worst %.1f ulp of max|q| per coordinate" % (eps, L, worst))
        assert worst <= 64.0
        assert np.allclose(-p2, p0, rtol=0, atol=1e-12 * np.abs(p0).max())


def test_energy_error_is_second_order(hmc):
    q0, p0, imass = _chains(12, seed=7)
    always = np.full(12, -np.inf)
    # the ratio tends to 4 where eps * omega << 1; the stiffest oscillator here has omega^2 = 9 e < 25, so eps <= 0.025 keeps
    # eps * omega below 1 / 8 (at eps = 0.2 one chain's leading term nearly cancels at this T and the next order shows)
    T = 1.2
    for L in (48, 96):
        eps = T / L
        _, _, la_a, _ = hmc.hmc_lockstep(q0, p0, imass, eps, L, value_fn, grad_fn, always)
        _, _, la_b, _ = hmc.hmc_lockstep(q0, p0, imass, eps / 2, 2 * L, value_fn, grad_fn, always)
        ea, eb = np.abs(la_a), np.abs(la_b)
        assert np.all(ea > 1e-10) and np.all(eb > 1e-10), (ea.min(), eb.min())
        ratio = ea / eb
        print("ENERGY L %d: |dH| %.3e .. %.3e, ratio on halving eps %.3f .. %.3f" % (L, ea.min(), ea.max(), ratio.min(), ratio.max()))
        assert np.all((ratio >= 3.0) & (ratio <= 5.0)), ratio


def test_a_frozen_coordinate_keeps_its_bits(hmc):
    q0, p0, imass = _chains(8, seed=9)
    imass[:, 2] = 0.0
    imass[3, :] = 0.0
    q, p, la, acc = hmc.hmc_lockstep(q0, p0, imass, 0.2, 6, value_fn, grad_fn, np.full(8, -np.inf))
    assert acc.all()
    assert np.array_equal(q[:, 2], q0[:, 2]) and np.array_equal(q[3], q0[3])
    moved = np.ones((8, D), dtype=bool)
    moved[:, 2] = False
    moved[3] = False
    assert np.all(q[moved] != q0[moved])


def test_leaving_the_support(hmc):
    q0, p0, imass = _chains(6, seed=11)
    # chain 2 is pushed over the wall at q[0] < 1.5 within a few steps; the others stay far from it
    q0[:, 0] = 0.0
    p0[:, 0] = 0.0
    q0[2, 0], p0[2, 0], imass[2, 0] = 1.4, 3.0, 1.0
    calls = []

    def grad_logged(idx, Q):
        calls.append(np.array(idx))
        return grad_fn(idx, Q)

    def support(idx, Q):
        return Q[:, 0] < 1.5

    def inside(q):
        return q[0] < 1.5

    log_u = np.full(6, -np.inf)
    st = {}
    q, p, la, acc = hmc.hmc_lockstep(q0, p0, imass, 0.1, 8, value_fn, grad_logged, log_u, support, stats=st)
    assert la[2] == -np.inf and not acc[2] and np.array_equal(q[2], q0[2]) and np.array_equal(p[2], -p0[2])
    assert acc[[0, 1, 3, 4, 5]].all()
    left_at = max(k for k, idx in enumerate(calls) if 2 in idx)
    assert left_at < 8 and all(2 not in idx for idx in calls[left_at + 1:])
    assert st["evals"] == 5 * 9 + (left_at + 1)
    for c in range(6):
        qc, pc, lac, accc = _plain_chain(q0[c], p0[c], imass[c], 0.1, 8, log_u[c], inside)
        assert np.array_equal(q[c], np.array(qc)) and np.array_equal(p[c], np.array(pc)) and la[c] == lac and bool(acc[c]) == accc
    # a chain that starts outside is dead from the start: no gradient at all
    calls.clear()
    q0[4, 0] = 2.0
    q, p, la, acc = hmc.hmc_lockstep(q0, p0, imass, 0.1, 3, value_fn, grad_logged, log_u, support)
    assert la[4] == -np.inf and not acc[4] and all(4 not in idx for idx in calls)
    # a gradient that is not finite kills the chain as well
    calls.clear()
    q0[4, 0] = 0.0

    def grad_nan(idx, Q):
        calls.append(np.array(idx))
        g = grad_fn(idx, Q)
        if len(calls) == 2:
            g[list(idx).index(1), 3] = np.nan
        return g

    q, p, la, acc = hmc.hmc_lockstep(q0, p0, imass, 0.1, 3, value_fn, grad_nan, log_u, support)
    assert la[1] == -np.inf and not acc[1] and all(1 not in idx for idx in calls[2:]) and np.array_equal(q[1], q0[1])


def test_the_momentum_rule(hmc):
    q0, p0, imass = _chains(10, seed=13)
    _, _, la, _ = hmc.hmc_lockstep(q0, p0, imass, 0.9, 4, value_fn, grad_fn, np.full(10, -np.inf))
    log_u = np.where(np.arange(10) % 2 == 0, la - 1e-3, la)              # even chains accept; log u == log alpha rejects
    q, p, la2, acc = hmc.hmc_lockstep(q0, p0, imass, 0.9, 4, value_fn, grad_fn, log_u)
    assert np.array_equal(la, la2) and np.array_equal(acc, np.arange(10) % 2 == 0)
    qa, pa, _, _ = hmc.hmc_lockstep(q0, p0, imass, 0.9, 4, value_fn, grad_fn, np.full(10, -np.inf))
    assert np.array_equal(q[acc], qa[acc]) and np.array_equal(p[acc], pa[acc])
    assert np.array_equal(q[~acc], q0[~acc]) and np.array_equal(p[~acc], -p0[~acc])
    with pytest.raises(ValueError, match="-inf"):
        hmc.hmc_lockstep(q0, p0, imass, 0.1, 2, lambda i, Q: np.full(len(i), -np.inf), grad_fn, log_u)


def _batch_check(x, nb=40):
    """mean within 5 batch-means standard errors of 0, variance within 5 of 1 -> (ok, figures)"""
    b = x.reshape(nb, -1)
    m = b.mean(axis=1)
    se_m = m.std(ddof=1) / math.sqrt(nb)
    v = ((b - x.mean()) ** 2).mean(axis=1)
    se_v = v.std(ddof=1) / math.sqrt(nb)
    fig = (x.mean(), se_m, v.mean(), se_v)
    return abs(x.mean()) <= 5 * se_m and abs(v.mean() - 1.0) <= 5 * se_v, fig


def test_law_of_a_standard_normal(hmc):
    N, SEED = 4000, 17
    rs = np.random.RandomState(SEED)
    ok_ref, fig_ref = _batch_check(rs.randn(N))
    print("LAW reference sampler: mean %.4f (se %.4f), variance %.4f (se %.4f)" % fig_ref)
    assert ok_ref, "the seed has to let numpy's own normals pass at the same bar"
    rs = np.random.RandomState(SEED)
    one = np.ones((1, 1))
    q = np.zeros((1, 1))
    xs = np.empty(N)
    accepted = 0
    for k in range(N):
        p0 = rs.randn(1, 1)                                   # full refresh, unit mass
        q, _, _, acc = hmc.hmc_lockstep(q, p0, one, 0.7, 3, lambda i, Q: -0.5 * (Q[:, 0] * Q[:, 0]), lambda i, Q: -Q,
                                        np.log(rs.uniform(size=1)))
        accepted += int(acc[0])
        xs[k] = q[0, 0]
    ok, fig = _batch_check(xs)
    print("LAW hmc_lockstep: mean %.4f (se %.4f), variance %.4f (se %.4f), acceptance %.3f" % (fig + (accepted / N,)))
    assert ok, fig
