"""Lock-step HMC: one leapfrog update of many independent chains at once, on the host.

What CelestePy/util/infer/hmc.py does for one state with num_iter = 1 and the momentum already refreshed by the caller (Neal
2010: half kick, L drifts with kicks between them, half kick; negate, accept, negate), vectorised over chains whose targets
do not involve one another.  Not a port of that file: the arithmetic below is the device engine's (k_hmc.h, cel_slice_sample
param 3), in its order, so that a chain takes the same trajectory on either engine bit for bit:

    p = p0 + (0.5 eps) g(q0)
    for l in 0 .. L-1:   q = q + (eps imass) p;   p = p + (l == L-1 ? 0.5 eps : eps) g(q)
    K(p) = 0.5 sum_i imass_i (p_i p_i)          (added in coordinate order from 0.0)
    log alpha = (v(qL) - v(q0)) + (K(p0) - K(pL));   accepted iff log u < log alpha

A trajectory that leaves the support, or meets a position or a gradient entry that is not finite, is dead: it is rejected with
log alpha = -inf and takes no part in any later grad_fn or value_fn call.
"""
import numpy as np


def kinetic(imass, p):
    """K(p) = 0.5 sum_i imass_i (p_i p_i), added in coordinate order from 0.0 -> (n,)"""
    acc = np.zeros(p.shape[0])
    for i in range(p.shape[1]):
        acc = acc + imass[:, i] * (p[:, i] * p[:, i])
    return 0.5 * acc


def hmc_lockstep(q0, p0, imass, eps, L, value_fn, grad_fn, log_u, support_fn=None, stats=None):
    """One HMC update per chain.

    q0, p0, imass   (n, D): position, momentum (refreshed by the caller), inverse mass (0 freezes a coordinate)
    eps, L          step size and leapfrog steps
    value_fn(idx, Q) -> v[len(idx)]      the log target of chains idx at Q[i]
    grad_fn(idx, Q)  -> g[len(idx), D]   its gradient
    log_u           (n,): log of each chain's accept uniform
    support_fn(idx, Q) -> bool[len(idx)] or None: is Q[i] inside the support of chain idx[i]
    stats           dict or None: gets steps, evals (gradient evaluations), accepted

    -> (q[n, D], p[n, D], log_alpha[n], accepted[n]): the new position, the momentum to carry on with (pL on accept, -p0 on
    reject), the log acceptance ratio (-inf for a dead trajectory), the decision.  A chain whose q0 lies outside its support
    is dead from the start.  Raises ValueError when a live chain's v(q0) is -inf or NaN."""
    q0 = np.array(q0, dtype=np.float64)
    p0 = np.array(p0, dtype=np.float64)
    imass = np.asarray(imass, dtype=np.float64)
    n, D = q0.shape
    eps, L = float(eps), int(L)
    if L < 1:
        raise ValueError("hmc_lockstep: L must be at least 1")
    q, p = q0.copy(), p0.copy()
    alive = np.ones(n, dtype=bool)
    every = np.arange(n)
    if support_fn is not None and n:
        alive &= np.asarray(support_fn(every, q), dtype=bool)
    alive &= np.isfinite(q).all(axis=1)
    evals = 0
    for l in range(L + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        g = np.asarray(grad_fn(idx, q[idx]), dtype=np.float64).reshape(idx.size, D)
        evals += idx.size
        ok = np.isfinite(g).all(axis=1)
        alive[idx[~ok]] = False
        idx, g = idx[ok], g[ok]
        h = 0.5 * eps if l in (0, L) else eps
        p[idx] = p[idx] + h * g
        if l < L:
            qn = q[idx] + (eps * imass[idx]) * p[idx]
            q[idx] = qn
            ok = np.isfinite(qn).all(axis=1)
            if support_fn is not None and idx.size:
                ok &= np.asarray(support_fn(idx, qn), dtype=bool)
            alive[idx[~ok]] = False
    la = np.full(n, -np.inf)
    idx = np.nonzero(alive)[0]
    if idx.size:
        v0 = np.asarray(value_fn(idx, q0[idx]), dtype=np.float64)
        v1 = np.asarray(value_fn(idx, q[idx]), dtype=np.float64)
        if not np.all(v0 > -np.inf):
            raise ValueError("hmc_lockstep: a state outside its own target (its current position scores -inf)")
        with np.errstate(invalid="ignore"):
            la[idx] = (v1 - v0) + (kinetic(imass[idx], p0[idx]) - kinetic(imass[idx], p[idx]))
    with np.errstate(invalid="ignore"):
        acc = alive & (np.asarray(log_u, dtype=np.float64) < la)
    q_new = np.where(acc[:, None], q, q0)
    p_new = np.where(acc[:, None], p, -p0)
    if stats is not None:
        stats.update(steps=L, evals=int(evals), accepted=int(acc.sum()))
    return q_new, p_new, la, acc
