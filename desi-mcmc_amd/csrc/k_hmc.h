// k_hmc.h -- one HMC update of the location and shape of every source at once (cel_slice_sample, param 3)
//
// hmc_sample_galaxy_params (CelestePy/celeste_mcmc.py:281-331) runs util/infer/hmc.py's leapfrog on one galaxy, driven by
// galaxy_source_like_grad.  Given the photon split a source's conditional involves no other source, so here every source runs
// its trajectory in the same call, exactly: q = (ra, dec, theta, sigma, phi, rho), a star in (ra, dec) only, counts held fixed
// (their conditional is a Gamma that cel_flux_conditionals samples exactly).  One update per chain, the momentum p0 and the
// inverse mass being the caller's:
//     p = p0 + (0.5 eps) g(q0)
//     for l in 0 .. L-1:   q = q + (eps imass) p;   p = p + (l == L-1 ? 0.5 eps : eps) g(q)
//     K(p) = 0.5 sum_i imass_i (p_i p_i)          (added in coordinate order from 0.0)
//     log alpha = (v(qL) - v(q0)) + (K(p0) - K(pL));   accepted iff log u < log alpha
// v is the score params 0-2 form under the reference's conditional (the bands' mode-0 values added in band order from 0.0, a
// band's parts first; for a galaxy under phi_max > 0 plus sg_shape_prior); g is its gradient: slots 1-6 of the mode-8 row
// (k_patch_grad<0, int> and k_patch_grad_chain on the proposal set, one slot per chain), the prior's derivative added to the
// sigma entry.  A trajectory that leaves the support, or meets a position or a gradient entry that is not finite, is dead: its
// slot is never rendered again (owner = -1) and it is rejected with log alpha = -inf.
//
// The kernels below are the step's own, one thread per chain: the state and the first proposal row (k_hmc_fill), a kick and a
// drift per leapfrog step (k_hmc_step), the last half kick and the two slots per chain whose values are scored as the type move
// scores its two (k_hmc_slots; k_tm_jobs builds the job lists from a view that carries this step's `run`), and the decision
// (k_hmc_decide).  Random numbers: the FIRST uniform of the chain's SplitMix64 stream keyed by (seed, chain id), as k_tm_fill
// forms it.  No FMA contraction: the host engine (util/infer/hmc.py, ModelGibbs.resample_hmc) takes the same trajectory bit
// for bit.
#pragma once
#include "k_type_move.h"

#define HMC_D 6

struct Hmc {                   // SoA over chains
    double *q;                 // position, HMC_D per chain
    double *p;                 // momentum, HMC_D per chain
    double *p0;                // the caller's momentum (a running star's entries 2-5: 0)
    double *im;                // inverse mass (a star's entries 2-5, and every entry of a chain left alone: 0)
    double *log_u;             // log of the chain's uniform
    double *k0;                // K(p0)
    double *pri;               // per slot (2 per chain: q0, qL): the log-prior, or -inf for a slot that is not scored
    int *run;                  // the chain makes an update in this call
    int *dead;                 // its trajectory left the support or met a value that is not finite
    int *nev;                  // gradient evaluations of the chain
};

// the support: theta in (0, 1), sigma > 0, rho in (0, 1), phi in (0, phi_max) where phi_max > 0; every coordinate finite
__device__ inline bool hmc_inside(int t, const double *q, double phi_max) {
    bool ok = isfinite(q[0]) && isfinite(q[1]);
    if (t == 1) {
        ok = ok && isfinite(q[2]) && isfinite(q[3]) && isfinite(q[4]) && isfinite(q[5]);
        ok = ok && q[2] > 0.0 && q[2] < 1.0 && q[3] > 0.0 && q[5] > 0.0 && q[5] < 1.0;
        if (phi_max > 0.0) ok = ok && q[4] > 0.0 && q[4] < phi_max;
    }
    return ok;
}

// g(q) from the chain's mode-8 row (slot 0 the value's place, 1 2 ra dec, 3..6 the shape); -> every entry read is finite
__device__ inline bool hmc_grad(int t, const double *row, const double *q, double phi_max, double g[HMC_D]) {
#pragma clang fp contract(off)
    g[0] = row[1]; g[1] = row[2];
    for (int i = 2; i < HMC_D; i++) g[i] = (t == 1) ? row[1 + i] : 0.0;
    if (t == 1 && phi_max > 0.0) {
        const double s = q[3];
        g[3] = g[3] + (2.0 / ((s * s) * s) - 4.0 / s);
    }
    bool ok = true;
    for (int i = 0; i < HMC_D; i++) ok = ok && isfinite(g[i]);
    return ok;
}

__device__ inline double hmc_kinetic(const double *im, const double *p) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < HMC_D; i++) acc += im[i] * (p[i] * p[i]);
    return 0.5 * acc;
}

// the state of every chain, the run flags, the first proposal row (q0: the first half kick's gradient is taken there) and log u
__global__ void __launch_bounds__(256)
k_hmc_fill(Hmc hm, int64_t S, int B, double phi_max, const int *__restrict__ type, const double *__restrict__ radec,
           const double *__restrict__ counts, const double *__restrict__ shape, const double *__restrict__ dirs /* [S][12] */,
           const int *__restrict__ chain_ids, const int64_t *__restrict__ soff, unsigned long long seed,
           int *__restrict__ ptype, double *__restrict__ pradec, double *__restrict__ pcounts, double *__restrict__ pshape,
           int *__restrict__ owner /* S */, int *__restrict__ err) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t = type[s];
    // left alone: a source without any sample patch, one whose chain id is negative (another rank's), and a source that is
    // neither a star nor a galaxy (the per-profile route)
    const bool runs = soff[(s + 1) * B] > soff[s * B] && !(chain_ids && chain_ids[s] < 0) && (t == 0 || t == 1);
    const int nd = (t == 1) ? HMC_D : 2;
    double q[HMC_D];
    q[0] = radec[2 * s]; q[1] = radec[2 * s + 1];
    for (int k = 0; k < 4; k++) q[2 + k] = shape[4 * s + k];
    const double *d = dirs + 2 * HMC_D * s;
    for (int i = 0; i < HMC_D; i++) {
        const bool moves = runs && i < nd;
        const double p0 = (runs && i >= nd) ? 0.0 : d[i];
        hm.q[HMC_D * s + i] = q[i];
        hm.p0[HMC_D * s + i] = p0;
        hm.p[HMC_D * s + i] = p0;
        hm.im[HMC_D * s + i] = moves ? d[HMC_D + i] : 0.0;
    }
    hm.k0[s] = hmc_kinetic(hm.im + HMC_D * s, hm.p0 + HMC_D * s);
    const bool inside = hmc_inside(t, q, phi_max);
    if (runs && !inside) atomicOr(err, 1);             // the state lies outside its own conditional
    const bool alive = runs && inside;
    hm.run[s] = runs ? 1 : 0;
    hm.dead[s] = (runs && !inside) ? 1 : 0;
    hm.nev[s] = alive ? 1 : 0;
    ptype[s] = t;
    pradec[2 * s] = q[0]; pradec[2 * s + 1] = q[1];
    for (int b = 0; b < B; b++) pcounts[s * B + b] = counts[s * B + b];
    for (int k = 0; k < 4; k++) pshape[4 * s + k] = q[2 + k];
    owner[s] = alive ? (int)s : -1;
    const unsigned long long id = (unsigned long long)(chain_ids ? chain_ids[s] : (int)s);
    const unsigned long long key = sl_mix(seed ^ (id * 0xD1342543DE82EF95ull));
    const double u = ((double)(sl_mix(key) >> 11) + 0.5) * (1.0 / 9007199254740992.0);      // the stream's uniform 0
    hm.log_u[s] = log(u);
}

// one leapfrog step: the kick with the gradient rows just produced (half a step the first time), the drift, the support
// test, the proposal row and its owner
__global__ void __launch_bounds__(256)
k_hmc_step(Hmc hm, int64_t S, int B, int first, double eps, double phi_max, const int *__restrict__ type,
           const double *__restrict__ grad /* [S][7 + B] */, double *__restrict__ pradec, double *__restrict__ pshape,
           int *__restrict__ owner /* S */) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (!hm.run[s] || hm.dead[s]) return;
    const int t = type[s];
    const int nd = (t == 1) ? HMC_D : 2;
    double *q = hm.q + HMC_D * s, *p = hm.p + HMC_D * s;
    const double *im = hm.im + HMC_D * s;
    double g[HMC_D];
    bool ok = hmc_grad(t, grad + s * (7 + B), q, phi_max, g);
    if (ok) {
        const double h = first ? 0.5 * eps : eps;
        for (int i = 0; i < nd; i++) p[i] = p[i] + h * g[i];
        for (int i = 0; i < nd; i++) q[i] = q[i] + (eps * im[i]) * p[i];
        ok = hmc_inside(t, q, phi_max);
    }
    if (!ok) {
        hm.dead[s] = 1;
        owner[s] = -1;
        return;
    }
    pradec[2 * s] = q[0]; pradec[2 * s + 1] = q[1];
    if (t == 1)
        for (int k = 0; k < 4; k++) pshape[4 * s + k] = q[2 + k];
    hm.nev[s] += 1;
}

// the last half kick with the gradient at qL, then the two slots per chain whose values decide: slot 2 s the catalogue's row
// (q0), slot 2 s + 1 the row at qL.  A dead chain's slots are not scored.
__global__ void __launch_bounds__(256)
k_hmc_slots(Hmc hm, int64_t S, int B, double eps, double phi_max, const int *__restrict__ type, const double *__restrict__ radec,
            const double *__restrict__ counts, const double *__restrict__ shape, const double *__restrict__ grad /* [S][7 + B] */,
            int *__restrict__ ptype, double *__restrict__ pradec, double *__restrict__ pcounts, double *__restrict__ pshape,
            int *__restrict__ owner /* 2S */) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t = type[s];
    const int nd = (t == 1) ? HMC_D : 2;
    double *q = hm.q + HMC_D * s, *p = hm.p + HMC_D * s;
    bool alive = hm.run[s] && !hm.dead[s];
    if (alive) {
        double g[HMC_D];
        if (hmc_grad(t, grad + s * (7 + B), q, phi_max, g)) {
            for (int i = 0; i < nd; i++) p[i] = p[i] + (0.5 * eps) * g[i];
        } else {
            hm.dead[s] = 1;
            alive = false;
        }
    }
    for (int k = 0; k < 2; k++) {
        const int64_t i = 2 * s + k;
        const bool at_q = (k == 1) && alive;
        ptype[i] = t;
        pradec[2 * i] = at_q ? q[0] : radec[2 * s];
        pradec[2 * i + 1] = at_q ? q[1] : radec[2 * s + 1];
        for (int b = 0; b < B; b++) pcounts[i * B + b] = counts[s * B + b];
        for (int j = 0; j < 4; j++) pshape[4 * i + j] = (at_q && t == 1) ? q[2 + j] : shape[4 * s + j];
        double lp = -INFINITY;
        if (alive) lp = (t == 1 && phi_max > 0.0) ? sg_shape_prior(pshape + 4 * i, phi_max) : 0.0;
        hm.pri[i] = lp;
        owner[i] = (lp > -INFINITY) ? (int)s : -1;
    }
}

// The decision, one thread per chain: a slot's score is its bands' log-likelihoods added in band order from 0.0 (a band's
// PLL_PARTS slots first, in order) plus the prior; log alpha = (v(qL) - v(q0)) + (K(p0) - K(pL)); accepted iff log u < log alpha.
// An accepted row replaces the catalogue's location and (a galaxy's) shape.  out (doubles): per chain the new q and the momentum
// to carry on with (pL on accept, -p0 on reject: the reference's negate, accept, negate; a chain left alone: its row and the
// caller's momentum), then log alpha per chain (NaN for a chain left alone, -inf for a dead trajectory); flag: -1 left alone,
// 0 rejected, 1 accepted.  err |= 1: a running chain whose current state scores -inf (or NaN): it stays where it is.
__global__ void __launch_bounds__(256)
k_hmc_decide(Hmc hm, int64_t S, int B, int nparts, const double *__restrict__ ll_pb,
             const double *__restrict__ exact /* 2S: the exact conditional's term per slot (k_sg_exact_terms), or nullptr */,
             const int *__restrict__ type,
             double *__restrict__ radec, double *__restrict__ shape, double *__restrict__ out /* [S][12], then [S] */,
             int *__restrict__ flag /* S */, int *__restrict__ err) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t = type[s];
    const double *q = hm.q + HMC_D * s, *p = hm.p + HMC_D * s, *p0 = hm.p0 + HMC_D * s;
    double la = NAN;
    int f = -1;
    if (hm.run[s]) {
        f = 0;
        if (hm.dead[s]) {
            la = -INFINITY;
        } else {
            double v[2];
            for (int k = 0; k < 2; k++) {
                double acc = 0.0;
                for (int b = 0; b < B; b++) {
                    const double *x = ll_pb + ((2 * s + k) * B + b) * nparts;
                    double y = x[0];
                    for (int j = 1; j < nparts; j++) y += x[j];
                    acc += y;
                }
                if (exact) acc += exact[2 * s + k];         // ll = patch sum; ll += e; v = ll + prior
                v[k] = acc + hm.pri[2 * s + k];
            }
            if (!(v[0] > -INFINITY)) {
                atomicOr(err, 1);                   // the state lies outside its own conditional
            } else {
                la = (v[1] - v[0]) + (hm.k0[s] - hmc_kinetic(hm.im + HMC_D * s, p));
                f = (hm.log_u[s] < la) ? 1 : 0;
            }
        }
    }
    double *o = out + 2 * HMC_D * s;
    if (f == 1) {
        radec[2 * s] = q[0]; radec[2 * s + 1] = q[1];
        if (t == 1)
            for (int k = 0; k < 4; k++) shape[4 * s + k] = q[2 + k];
    }
    o[0] = radec[2 * s]; o[1] = radec[2 * s + 1];
    for (int k = 0; k < 4; k++) o[2 + k] = shape[4 * s + k];
    for (int i = 0; i < HMC_D; i++) o[HMC_D + i] = (f == 1) ? p[i] : (f == 0 ? -p0[i] : p0[i]);
    out[2 * HMC_D * S + s] = la;
    flag[s] = f;
}

// ---- the exact conditional (CEL_OPT_GRAD_CONDITIONAL = 1) -------------------------------------------------------------------
// v and g are the exact conditional's: per gradient evaluation the proposals' records are written WITH their boxes, k_sg_cover
// retires the slot of a proposal whose box does not cover its source's photons, and this kernel, one thread per chain, tells
// the state machine: at the first evaluation (the catalogue's own row) the chain does not run at all -- it is reported as a
// chain left alone; later the trajectory is dead, exactly like one that left the support (the evaluation is counted: k_hmc_step
// counted it when it named the point).  The force is a function of q alone, piecewise smooth with jumps where the integer box
// changes: the leapfrog stays reversible and volume-preserving, and the Metropolis test on the exact v keeps the update exact.
__global__ void __launch_bounds__(256)
k_hmc_cover(Hmc hm, int64_t S, const int *__restrict__ owner /* S, after k_sg_cover */, int first) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (!hm.run[s] || hm.dead[s] || owner[s] >= 0) return;
    if (first) {
        hm.run[s] = 0;
        hm.nev[s] = 0;
    } else {
        hm.dead[s] = 1;
    }
}
