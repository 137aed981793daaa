// k_type_move.h -- the star <-> galaxy move of every source at once (cel_slice_sample, param 2)
//
// Source.resample_type (CelestePy/sources.py:247-306) proposes the other type for one source and accepts by a
// Metropolis-Hastings test on the image likelihood.  Given the photon split a source's conditional involves no other
// source, so here every source makes its proposal in the same call, exactly: two slots per chain in the proposal set,
// slot 2 s the current row and slot 2 s + 1 the row with the type flipped (a star's proposed galaxy shape is the
// caller's; a galaxy's proposed star sits at the same location with the same expected counts).  Both slots are scored
// by the kernels the slice samplers use (the conditional likelihoods, and under CEL_OPT_SLICE_CONDITIONAL = 1 the cover
// test, the stamp masses and k_sg_exact_terms); the three kernels below are the move's own: the proposal set and the
// chains' uniforms, the job lists, and the decision.
//
// Random numbers: a chain's SplitMix64 stream keyed by (seed, chain id), its FIRST uniform -- what
// util/infer/slicesample.ChainStreams(seed, ids).uniform hands out first.  No FMA contraction: the host engine
// (ModelGibbs.resample_types) takes the same decisions bit for bit.
#pragma once
#include "k_slice_gen.h"

struct TypeMove {              // SoA over chains
    double *log_u;             // log of the chain's uniform
    double *h;                 // the caller's term of the log acceptance ratio
    double *pri;               // per slot (2 per chain): 0, or -inf for a shape outside the support / a box that does not cover
    int *run;                  // the chain makes a proposal in this call
};

// the proposal set and the chains: one thread per slot
__global__ void __launch_bounds__(256)
k_tm_fill(TypeMove tm, int64_t S, int B, const int *__restrict__ type, const double *__restrict__ radec,
          const double *__restrict__ counts, const double *__restrict__ shape, const double *__restrict__ dirs /* [S][5] */,
          const int *__restrict__ chain_ids, const int64_t *__restrict__ soff, unsigned long long seed,
          int *__restrict__ ptype, double *__restrict__ pradec, double *__restrict__ pcounts, double *__restrict__ pshape,
          int *__restrict__ owner /* 2S */) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * S) return;
    const int64_t s = i >> 1;
    const int q = (int)(i & 1);
    const int t = type[s];
    // left alone: a source without any sample patch, one whose chain id is negative (another rank's), and a source that is
    // neither a star nor a galaxy (the per-profile route)
    const bool runs = soff[(s + 1) * B] > soff[s * B] && !(chain_ids && chain_ids[s] < 0) && (t == 0 || t == 1);
    const bool to_gal = q == 1 && runs && t == 0;
    ptype[i] = (q == 1 && runs) ? 1 - t : t;
    pradec[2 * i] = radec[2 * s]; pradec[2 * i + 1] = radec[2 * s + 1];
    for (int b = 0; b < B; b++) pcounts[i * B + b] = counts[s * B + b];
    double lp = 0.0;
    if (to_gal) {
        const double *d = dirs + 5 * s;
        const bool inside = d[0] > 0.0 && d[0] < 1.0 && d[1] > 0.0 && d[3] > 0.0 && d[3] < 1.0;
        if (!inside) lp = -INFINITY;                 // never rendered, and rejected
        for (int k = 0; k < 4; k++) pshape[4 * i + k] = d[k];
    } else {
        for (int k = 0; k < 4; k++) pshape[4 * i + k] = shape[4 * s + k];       // (a galaxy turned star keeps its shape row)
    }
    tm.pri[i] = lp;
    owner[i] = (runs && lp > -INFINITY) ? (int)s : -1;
    if (q == 0) {
        tm.run[s] = runs ? 1 : 0;
        tm.h[s] = dirs[5 * s + 4];
        const unsigned long long id = (unsigned long long)(chain_ids ? chain_ids[s] : (int)s);
        const unsigned long long key = sl_mix(seed ^ (id * 0xD1342543DE82EF95ull));
        const double u = ((double)(sl_mix(key) >> 11) + 0.5) * (1.0 / 9007199254740992.0);      // the stream's uniform 0
        tm.log_u[s] = log(u);
    }
}

// The (slot, band) jobs of the running chains, both slots of each: the likelihood kernels' block descriptors
// job << 3 | part << 1 | dealt (job = slot * B + band; k_sg_live_jobs' layout, what launch_resident_ll takes) in the dense
// list or the at-the-photons list, and the mass kernel's plain job numbers.  A list that is not wanted is nullptr.  One
// atomic per wave and list (wave_reserve); a slot that is not scored retires in the kernels by its owner.
__global__ void __launch_bounds__(256)
k_tm_jobs(TypeMove tm, int64_t S, int B, const int *__restrict__ nzmode, const int *__restrict__ nnz,
          const int4 *__restrict__ nzbox, int deal_all, int *__restrict__ list, int *__restrict__ count,
          int *__restrict__ list_nz, int *__restrict__ count_nz, int *__restrict__ list_mass, int *__restrict__ count_mass) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // (chain, band)
    const int64_t s = (i < S * B) ? i / B : 0;
    const int b = (int)(i - s * B);
    const bool alive = i < S * B && tm.run[s] != 0;
    bool nz = false, deal = deal_all != 0;
    if (alive && list) {
        nz = nzmode && nzmode[i];
        if (!deal) {
            if (nz) deal = nnz[i] > NZ_SPLIT_PHOTONS;
            else {
                const int4 q = nzbox[i];
                deal = (q.y > q.x && q.w > q.z) && (long long)((q.y - q.x + HW_TW - 1) / HW_TW) * ((q.w - q.z + HW_TH - 1) / HW_TH) > PLL_SPLIT_CHUNKS;
            }
        }
    }
    const int per = deal ? PLL_PARTS : 1;
    // (every lane of the wave takes part in a reservation: no return above)
    const int at_d = list ? wave_reserve(count, (alive && !nz) ? 2 * per : 0) : 0;
    const int at_n = (list && nzmode) ? wave_reserve(count_nz, (alive && nz) ? 2 * per : 0) : 0;
    const int at_m = list_mass ? wave_reserve(count_mass, alive ? 2 : 0) : 0;
    if (!alive) return;
    if (list) {
        int *dst = nz ? list_nz : list;
        const int at = nz ? at_n : at_d;
        for (int q = 0; q < 2; q++) {
            const int job = (int)((2 * s + q) * B + b);
            for (int part = 0; part < per; part++) dst[at + q * per + part] = (job << 3) | (part << 1) | (deal ? 1 : 0);
        }
    }
    if (list_mass) {
        list_mass[at_m] = (int)((2 * s) * B + b);
        list_mass[at_m + 1] = (int)((2 * s + 1) * B + b);
    }
}

// The decision, one thread per chain: a slot's score is its bands' log-likelihoods added in band order from 0.0 (a band's
// PLL_PARTS slots first, in order) plus the exact conditional's term; log alpha = (score(proposal) - score(current)) + h;
// accepted iff log u < log alpha.  An accepted row replaces the catalogue's type and shape.  out (doubles): per chain the
// new type and shape (5), then log alpha per chain (NaN for a chain left alone); flag: -1 left alone, 0 rejected,
// 1 accepted.  err |= 1: a running chain whose current state scores -inf (or NaN): it stays where it is.
__global__ void __launch_bounds__(256)
k_tm_decide(TypeMove tm, int64_t S, int B, int nparts, const double *__restrict__ ll_pb, const double *__restrict__ exact /* 2S or nullptr */,
            const double *__restrict__ pshape /* 2S rows of 4 */, int *__restrict__ type, double *__restrict__ shape,
            double *__restrict__ out /* [S][5], then [S] */, int *__restrict__ flag /* S */, int *__restrict__ err) {
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    int t = type[s];
    double la = NAN;
    int f = -1;
    if (tm.run[s]) {
        double v[2];
        for (int q = 0; q < 2; q++) {
            if (tm.pri[2 * s + q] > -INFINITY) {
                double acc = 0.0;
                for (int b = 0; b < B; b++) {
                    const double *p = ll_pb + ((2 * s + q) * B + b) * nparts;
                    double x = p[0];
                    for (int k = 1; k < nparts; k++) x += p[k];
                    acc += x;
                }
                if (exact) acc += exact[2 * s + q];
                v[q] = acc;
            } else {
                v[q] = -INFINITY;
            }
        }
        if (!(v[0] > -INFINITY)) {
            atomicOr(err, 1);                       // the state lies outside its own conditional
            f = 0;
        } else {
            la = (v[1] - v[0]) + tm.h[s];
            f = (tm.log_u[s] < la) ? 1 : 0;
        }
        if (f == 1) {
            t = 1 - t;
            type[s] = t;
            for (int k = 0; k < 4; k++) shape[4 * s + k] = pshape[4 * (2 * s + 1) + k];
        }
    }
    out[5 * s] = (double)t;
    for (int k = 0; k < 4; k++) out[5 * s + 1 + k] = shape[4 * s + k];
    out[5 * S + s] = la;
    flag[s] = f;
}
