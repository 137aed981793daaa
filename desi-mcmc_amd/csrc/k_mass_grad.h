// k_mass_grad.h -- derivative of a proposal's stamp mass on its OWN box (CEL_OPT_GRAD_CONDITIONAL = 1)
//
// The exact conditional of ModelGibbs(conditional="exact") charges a proposal  counts_b * mass_b  in every band where its source has
// a sample patch, mass_b = the proposal's unit stamp u summed over the proposal's own integer box (k_patch_ll_hw<3>).  Its gradient
// needs  d mass_b / d q = sum over the box of d u / d q  at the FIXED integer box: the box moves in jumps, between two jumps the
// sum's limits are constants.  That is k_patch_grad's sum with r = 1 at every pixel and the record's box in place of a patch.
//
// k_mass_grad: one wave per (proposal, band, part), the seven sums u; m0, m1; w00, w01, w11; th of k_patch_grad's layout (GRAD_NS
// doubles per part), so that k_patch_grad_chain (mode 2: no - wsum on the counts entry) takes them to the public coordinates
// unchanged.  The rows of the box are dealt to PGRAD_PARTS parts from the box's size alone.  The component table and the
// per-pixel terms are k_patch_grad's (grad_tab_fill and grad_pixel, k_grad_common.h); the pixels of a part are lane-strided;
// per pixel K direct exponentials.  NOTHING IS DROPPED: this is the plain form, every component at every pixel; neither
// CEL_OPT_TAIL_LOG_SOURCE nor CEL_OPT_KERNEL is read, so the bits depend on the inputs alone (fixed order, wave_sum, no atomics).
// A proposal without a stamp (record type < 0: own box empty, overlap-test miss) and a retired slot (owner < 0) write zeros:
// their mass is 0 whatever q is.  The kernel reads the records and the band table only -- no pixel data, no box table.
// k_mass_grad_masked is the same sum over the OBSERVED pixels of the box (it reads the counts to find the NaNs): the derivative of
// the mass k_stamp_mass_masked forms, for the samplers on a masked image set (CEL_OPT_SAMPLER_MASK).
//
// k_mass_grad_apply: one thread per proposal, the exact row from the reference's row:
//     slots 1..6   += -(sum_b counts_b d mass_b / d q_i)      (the chain's band-order sum over the bands that have a patch)
//     slot 7 + b   += -(mass_b - wsum_b) * has_patch_b        (mass_b: the mass kernel's value, as k_sg_exact_terms reads it)
// No FMA contraction.  A retired slot's row is left as the reference's kernels wrote it: zeros.
#pragma once
#include "k_patch_grad.h"

// the two kernels' body.  MASKED: the band's counts are read at the pixel and a pixel whose count is NaN is skipped BEFORE any
// arithmetic (no r = 0 multiply), so a box without a masked pixel leaves the unmasked kernel's bits and a box masked everywhere
// exact zeros
template <bool MASKED>
__device__ __forceinline__ void mass_grad_sums(const BandDev *bands, int B, int64_t P, const SrcRec *recs, const int *owner,
                                               const double *nelec, int H, int W, double *sums, double *tab) {
    const int lane = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)PGRAD_PARTS);
    const int64_t job = (int64_t)(blockIdx.x / (unsigned)PGRAD_PARTS);
    if (job >= P * B) return;
    const int b = (int)(job % B);
    const int64_t p = job / B;
    double *out = sums + (job * PGRAD_PARTS + part) * GRAD_NS;
    const int own = owner ? owner[p] : 0;
    const SrcRec *rp = recs + (int64_t)b * P + p;
    const int type = rp->type;
    const int x0 = rp->x0, y0 = rp->y0;
    const int nx = rp->x1 - x0, ny = rp->y1 - y0;
    // the part's rows, from the box's size alone
    const int ra = (int)(((int64_t)ny * part) / PGRAD_PARTS), rb = (int)(((int64_t)ny * (part + 1)) / PGRAD_PARTS);
    if (own < 0 || type < 0 || nx <= 0 || ny <= 0 || rb <= ra) {
        if (lane < GRAD_NS) out[lane] = 0.0;
        return;
    }
    const BandDev *bd = bands + b;
    const bool gal = (type != 0);
    const int K = gal ? K_GAL : K_PSF;
    if (lane < K) grad_tab_fill(bd, *rp, gal, lane, tab);
    __syncthreads();
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int n = nx * (rb - ra);
    // (MASKED: the box lies inside the frame -- 0 <= y0, y1 <= H, 0 <= x0, x1 <= W: k_prep cuts it -- so every address is a pixel's)
    const double *zn = MASKED ? nelec + (int64_t)b * H * W + (int64_t)(y0 + ra) * W + x0 : nullptr;
    for (int i = lane; i < n; i += 64) {
        const int yy = i / nx, xx = i - yy * nx;
        if (MASKED) {
            const double z = zn[(int64_t)yy * W + xx];
            if (z != z) continue;                                                                      // NaN: not observed
        }
        grad_pixel<false>(tab, nullptr, K, gal, (double)(x0 + xx), (double)(y0 + ra + yy), acc);      // r = 1 at every pixel
    }
    grad_store_sums(acc, lane, out);
}

__global__ void __launch_bounds__(64)
k_mass_grad(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs /* [B][P], WITH boxes */,
            const int *__restrict__ owner /* P, or nullptr */, double *__restrict__ sums /* P*B*PGRAD_PARTS*GRAD_NS */) {
    __shared__ double tab[GRAD_TAB];
    mass_grad_sums<false>(bands, B, P, recs, owner, nullptr, 0, 0, sums, tab);
}

// the derivative of the OBSERVED mass (CEL_OPT_SAMPLER_MASK on a masked image set): k_mass_grad's table, dealing of rows, pixel
// order and sums, over the pixels of the box whose count is not NaN.  No drop threshold, no CEL_OPT_KERNEL: the bits depend on the
// inputs alone.  nelec: [B][H][W], the whole frame (a row window is refused before the launch)
__global__ void __launch_bounds__(64)
k_mass_grad_masked(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs /* [B][P], WITH boxes */,
                   const int *__restrict__ owner /* P, or nullptr */, const double *__restrict__ nelec, int H, int W,
                   double *__restrict__ sums /* P*B*PGRAD_PARTS*GRAD_NS */) {
    __shared__ double tab[GRAD_TAB];
    mass_grad_sums<true>(bands, B, P, recs, owner, nelec, H, W, sums, tab);
}

__global__ void __launch_bounds__(256)
k_mass_grad_apply(int64_t P, int B, const int *__restrict__ owner /* P, after the cover test */, const BandDev *__restrict__ bands,
                  const int64_t *__restrict__ soff /* [S * B + 1]: the sample patches' offsets */,
                  const double *__restrict__ mass /* [P][B]: the mass kernel's values */,
                  const double *__restrict__ mg /* [P][7 + B]: k_patch_grad_chain (mode 2) on k_mass_grad's sums */,
                  double *__restrict__ row /* [P][7 + B]: the reference's rows in, the exact rows out (slot 0 is not touched) */) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int s = owner[p];
    if (s < 0) return;
    double *o = row + p * (7 + B);
    const double *m = mg + p * (7 + B);
    for (int i = 1; i < 7; i++) o[i] = o[i] + (-m[i]);
    for (int b = 0; b < B; b++) {
        const double wsum = bands[b].w[0] + bands[b].w[1] + bands[b].w[2];
        const int64_t ob = (int64_t)s * B + b;
        const double has_patch = soff[ob + 1] > soff[ob] ? 1.0 : 0.0;
        o[7 + b] = o[7 + b] + (-(mass[p * B + b] - wsum) * has_patch);
    }
}
