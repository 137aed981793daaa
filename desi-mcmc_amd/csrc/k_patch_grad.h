// k_patch_grad.h -- analytic gradient of the per-source conditional log-likelihoods (cel_patch_loglik[_multi], mode = 8 + m)
//
// Definition.  The gradient of the value k_patch_ll.h documents for mode m (0, 1 or 2), on the FIXED patch limits: no integer
// box of the source enters, so nothing has to be held fixed.  With u the proposal's unit stamp on the patch, m(pix) =
// counts_b u(pix), wsum_b the sum of the band's PSF weights and dq = d u / d q for a coordinate q,
//     every location and shape entry   sum_b counts_b sum_pix r(pix) dq(pix)
//     the counts entry of band b       sum_pix r(pix) u(pix)          (mode 0: - wsum_b on top, the value's mass term)
//     mode 0:  r = z / m where m > 0, else 0
//     mode 1:  r = z / (m + eps_b) - 1
//     mode 2:  r = z / m - 1 where m > 0, else 0
// z = the patch datum (a caller's doubles, the resident split's int32 photons, or nelec on the boxes).  A pixel with m == 0
// adds nothing in modes 0 and 2 whatever z holds: no 0 / 0 is formed and every output is finite whenever the value is.
//
// Record types follow k_patch_ll: a band with an empty patch contributes nothing; types -1 / -2 (own box empty) render their
// kind on the imposed limits, and so do their derivatives; type -3 (overlap-test miss) contributes only - wsum_b to its
// counts entry in mode 0 and renders as a star in modes 1 and 2.
//
// Nothing is dropped: CEL_OPT_TAIL_LOG[_SOURCE] is not read.  r = z / m magnifies a relative error of m exactly where m is
// small, and a derivative can be large where the value is not (k_stamp_jac.h's reasoning), so a rule relative to the value
// bounds nothing here.  The value in slot 0 comes from the plain mode's kernels and carries whatever rule they apply.
//
// k_patch_grad<MODE, TZ>: one wave per (proposal, band, part).  A job's rows are dealt to PGRAD_PARTS parts from the patch's
// size alone (part q takes rows [ny q / PARTS, ny (q + 1) / PARTS)): a batch of one source x five bands (HMC) is twenty waves
// and not five as long as their longest.  Lanes below K build the component table in LDS (grad_tab_fill, k_grad_common.h: A
// and A' with the theta factor apart, the mean, the precision, var_k; no drop threshold); the part's pixels are lane-strided
// as in grad_box; per pixel K direct exponentials, the seven quantities u; m0, m1; w00, w01, w11; th (grad_pixel), the residual
// from the datum and seven FMAs.  In MODE 0 a pixel with z == 0 is not evaluated at all (r = 0 there, and most pixels of a faint
// source's box hold no photon).  wave_sum closes the sums; one lane writes GRAD_NS doubles.  Fixed order, no atomics: the bits
// depend on the inputs alone.
//
// k_patch_grad_chain: one thread per proposal; adds the parts in part order and the bands in band order, and takes the sums to
// the public coordinates.  The chain rule is k_grad_chain's (grad_chain_band, k_grad_common.h); the record-type rules above
// replace its `rec.type < 0: continue`.  It writes the 7 + B layout: slot 0 (the value) is left to the host.
#pragma once
#include "k_grad.h"

#define PGRAD_PARTS 4

template <int MODE, bool GAL, typename TZ>
__device__ __forceinline__ void pgrad_rows(const double *__restrict__ tab, int x0, int ya, int nx, int n, const TZ *__restrict__ zd,
                                           const double *__restrict__ zn, int64_t zpitch, double counts, double eps, int lane,
                                           double acc[7]) {
    for (int i = lane; i < n; i += 64) {
        const int yy = i / nx, xx = i - yy * nx;
        const int64_t zi = (int64_t)yy * zpitch + xx;
        const double z = zd ? (double)zd[zi] : zn[zi];
        if (MODE == 0 && z == 0.0) continue;                  // r = 0: the pixel contributes exactly nothing
        double q[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        grad_pixel<false>(tab, nullptr, GAL ? K_GAL : K_PSF, GAL, (double)(x0 + xx), (double)(ya + yy), q);
        const double m = counts * q[0];
        double r;
        if (MODE == 0) r = (m > 0.0) ? z / m : 0.0;
        else if (MODE == 2) r = (m > 0.0) ? z / m - 1.0 : 0.0;
        else r = z / (m + eps) - 1.0;
        grad_weigh(r, q, GAL, acc);
    }
}

// TZ: the patch data's element type, as k_patch_ll's -- double for a caller's patches and for nelec, int for the resident split
template <int MODE, typename TZ>
__global__ void __launch_bounds__(64)
k_patch_grad(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs,
             const int *__restrict__ owner /* P, or nullptr = 0 */, const int4 *__restrict__ pbox /* NB*B: x0, x1, y0, y1 */,
             const int64_t *__restrict__ offsets /* NB*B+1 */, const TZ *__restrict__ data,
             const double *__restrict__ nelec /* used when data == nullptr */, int H, int W,
             double *__restrict__ sums /* P*B*PGRAD_PARTS*GRAD_NS */) {
    __shared__ double tab[GRAD_TAB];
    const int lane = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)PGRAD_PARTS);
    const int64_t job = (int64_t)(blockIdx.x / (unsigned)PGRAD_PARTS);
    const int b = (int)(job % B);
    const int64_t p = job / B;
    double *out = sums + (job * PGRAD_PARTS + part) * GRAD_NS;
    const int own = owner ? owner[p] : 0;
    const SrcRec *rp = recs + (int64_t)b * P + p;
    int type = rp->type;
    int4 bx = make_int4(0, 0, 0, 0);
    if (own >= 0) bx = pbox[(int64_t)own * B + b];
    const int nx = bx.y - bx.x, ny = bx.w - bx.z;
    // the part's rows, from the patch's size alone
    const int ra = (int)(((int64_t)ny * part) / PGRAD_PARTS), rb = (int)(((int64_t)ny * (part + 1)) / PGRAD_PARTS);
    // no patch in this band; a part without rows; the overlap-test miss of mode 0 (only the mass term, which the chain adds)
    if (own < 0 || nx <= 0 || ny <= 0 || rb <= ra || (type == -3 && MODE == 0)) {
        if (lane < GRAD_NS) out[lane] = 0.0;
        return;
    }
    if (type < 0) type = (type == -2) ? 1 : 0;           // imposed limits: the kind still renders
    const BandDev *bd = bands + b;
    const bool gal = (type != 0);
    const int K = gal ? K_GAL : K_PSF;
    if (lane < K) grad_tab_fill(bd, *rp, gal, lane, tab);
    __syncthreads();
    // the part's first datum: a packed patch (pitch nx), or -- none given -- the observed image on the box (pitch W)
    const int64_t ob = (int64_t)own * B + b;
    const TZ *zd = data ? data + offsets[ob] + (int64_t)ra * nx : nullptr;
    const double *zn = data ? nullptr : nelec + (int64_t)b * H * W + (int64_t)(bx.z + ra) * W + bx.x;
    const int64_t zpitch = data ? nx : W;
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int n = nx * (rb - ra);
    if (gal) pgrad_rows<MODE, true, TZ>(tab, bx.x, bx.z + ra, nx, n, zd, zn, zpitch, rp->scale, bd->eps, lane, acc);
    else pgrad_rows<MODE, false, TZ>(tab, bx.x, bx.z + ra, nx, n, zd, zn, zpitch, rp->scale, bd->eps, lane, acc);
    grad_store_sums(acc, lane, out);
}

// ---- chain rule to the public coordinates, one thread per proposal -------------------------------------------------------
__global__ void __launch_bounds__(256)
k_patch_grad_chain(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs,
                   const int *__restrict__ owner, const int4 *__restrict__ pbox, const int *__restrict__ type,
                   const double *__restrict__ shape, const double *__restrict__ counts, const double *__restrict__ sums,
                   int mode, double *__restrict__ out /* P*(7+B): 0 the value (the host's), 1 2 ra dec, 3..6 shape, 7+b counts */) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int t = type[p];
    const int own = owner ? owner[p] : 0;
    double *o = out + p * (7 + B);
    double gra = 0.0, gdec = 0.0, gsh[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; b++) {
        const BandDev &bd = bands[b];
        const SrcRec &rec = recs[(int64_t)b * P + p];
        int4 bx = make_int4(0, 0, 0, 0);
        if (own >= 0) bx = pbox[(int64_t)own * B + b];
        if (bx.y - bx.x <= 0 || bx.w - bx.z <= 0) {         // no sample image in this band: it contributes nothing
            o[7 + b] = 0.0;
            continue;
        }
        // the job's parts, in part order
        double q[7];
        const double *sp = sums + ((int64_t)p * B + b) * PGRAD_PARTS * GRAD_NS;
        for (int i = 0; i < 7; i++) {
            double x = sp[i];
            for (int k = 1; k < PGRAD_PARTS; k++) x += sp[k * GRAD_NS + i];
            q[i] = x;
        }
        // mode 0: the value's - counts * wsum term depends on the counts alone (an overlap-test miss has nothing else)
        o[7 + b] = (mode == 0) ? q[0] - (bd.w[0] + bd.w[1] + bd.w[2]) : q[0];
        if (rec.type == -3 && mode == 0) continue;
        const bool gal = (rec.type == 1 || rec.type == -2);  // -1 and -3 render as stars, -2 as a galaxy
        // (the entry points take whole frames only: the record's row is the frame's)
        grad_chain_band(bd, rec.px, rec.py, shape + 4 * p, q, counts[p * B + b], gal, t, gra, gdec, gsh);
    }
    o[0] = 0.0;
    o[1] = gra; o[2] = gdec;
    for (int i = 0; i < 4; i++) o[3 + i] = gsh[i];
}
