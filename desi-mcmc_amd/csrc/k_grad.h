// k_grad.h -- gradient of the field log-likelihood with respect to every source's parameters (cel_loglik_grad)
//
// Definition.  For the catalogue in `src` and the image set `img`:
//     ll = sum_b sum_p  nelec log(lambda) - lambda,    lambda_b(p) = eps_b + sum_s counts[s][b] unit_stamp(s, b)(p)
// The gradient is taken with every source's INTEGER BOX HELD FIXED (the box the render uses): lambda is piecewise smooth in
// the parameters and the boxes are where it is not.  The outputs are the partial derivatives of ll with respect to the
// quantities cel_sources_set takes, in its units (ra / dec per degree, counts, theta, sigma per arcsec, phi per degree, rho;
// a type-2 galaxy's own shape coordinates theta, W00, W01, W11).
//
// Per (source, band) the unit stamp is u(p) = sum_k g_k(p), g_k = A_k N(p; mu_k, C_k), with d = p - mu_k, P_k = C_k^-1 and
// r(p) = nelec / lambda - 1.  k_grad_src reduces seven sums over the box (each summed over the components at the pixel):
//   S_u  = sum r u                                          d ll / d counts
//   S_m  = sum r sum_k g_k P_k d                    (2)     d ll / d (px, py) through the means, per count
//   S_W  = sum r sum_k var_k g_k (P_k d d^T P_k - P_k) / 2  (3: 00, 01, 11)  d ll / d W (entry-wise), per count; galaxies
//   S_th = sum r (f_exp - f_dev)                            d ll / d theta, per count; galaxies
// in a fixed order (lane-strided pixels, then a shuffle tree): bitwise reproducible, no atomics.  k_grad_chain multiplies in
// the counts, takes the sums to the public coordinates analytically and adds the bands in order.  The component table, the
// per-pixel loop, the closing sums and the chain rule are k_grad_common.h's, shared with every other derivative kernel.
//
// Drop rule: HW_DROP_SKY at the context's per-source threshold T (CEL_OPT_TAIL_LOG_SOURCE, default 32; 0 = nothing is
// dropped), decided per component and pixel: component k is skipped at p when max(counts, 1) * |A_k'| e^(-d^T P d / 2) <
// eps e^-T (A_k' = the amplitude without the theta factor, so that d/d theta keeps both profiles).  A skipped term is below
// e^-T lambda(p) at that pixel, so each of the seven per-pixel sums loses at most
//     K e^-T |nelec - lambda|  x  (1;  sqrt(|P_k| 2 T_k);  var_k |P_k| (T_k + 1))   for (S_u;  S_m;  S_W)
// where T_k = T + log(max(counts, 1) A_k' / eps) is where the component was cut: the d^T P d factor grows toward the edge of
// the kept region, so the mean and shape sums lose up to ~T_k times what the counts sum does.  Relative to the sums of
// |r| |term| over the box that is below K T_k e^-T: at T = 32 and T_k <= 80, 42 * 80 * 1.3e-14 = 4e-11.
#pragma once
#include "k_grad_common.h"

// one wave per (source, band), job = s * B + b; the component table in LDS, the box's pixels strided over the lanes
// MASKED (a masked image set, k_grad_src_masked): a NaN count marks a pixel that was not observed -- r = 0 there
template <bool GAL, bool MASKED = false>
__device__ __forceinline__ void grad_box(const double *__restrict__ tab, const double *__restrict__ tT, int K, int x0, int y0,
                                         int nx, int n, const double *__restrict__ ne_p, const double *__restrict__ la_p, int W,
                                         int lane, double acc[7]) {
    for (int i = lane; i < n; i += 64) {
        const int yy = i / nx, xx = i - yy * nx;
        double q[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        grad_pixel<true>(tab, tT, K, GAL, (double)(x0 + xx), (double)(y0 + yy), q);   // dropped where h > tT (never when T = 0: +inf)
        const int64_t idx = (int64_t)(y0 + yy) * W + (x0 + xx);
        const double ne = ne_p[idx], la = la_p[idx];
        const double r = (!MASKED || ne == ne) ? ne / la - 1.0 : 0.0;
        grad_weigh(r, q, GAL, acc);
    }
}

template <bool MASKED>
__device__ __forceinline__ void grad_src_body(const BandDev *__restrict__ bands, int B, int H, int W, int64_t S, const SrcRec *__restrict__ recs,
                                              const double *__restrict__ nelec, const double *__restrict__ lambda, double tail_T,
                                              double *__restrict__ sums /* S*B*GRAD_NS */) {
    __shared__ double tab[GRAD_TAB], tT[K_GAL];
    const int lane = threadIdx.x;
    const int64_t job = blockIdx.x;
    const int b = (int)(job % B);
    const int64_t s = job / B;
    const SrcRec *rp = recs + (int64_t)b * S + s;
    const int type = rp->type;
    double *out = sums + job * GRAD_NS;
    const int x0 = rp->x0, y0 = rp->y0, nx = rp->x1 - rp->x0, ny = rp->y1 - rp->y0;
    if (type < 0 || nx <= 0 || ny <= 0) {
        if (lane < GRAD_NS) out[lane] = 0.0;
        return;
    }
    const BandDev *bd = bands + b;
    const bool gal = (type != 0);
    const int K = gal ? K_GAL : K_PSF;
    if (lane < K) {
        const double a1 = grad_tab_fill(bd, *rp, gal, lane, tab);
        // HW_DROP_SKY: keep where max(counts, 1) |A'| e^-h >= eps e^-T  <=>  h <= T + log(max(counts, 1) |A'| / eps)
        tT[lane] = (tail_T > 0.0) ? tail_T + log(fmax(fabs(rp->scale), 1.0) * fabs(a1) / bd->eps) : INFINITY;
    }
    __syncthreads();
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t plane = (int64_t)b * H * W;
    if (gal)
        grad_box<true, MASKED>(tab, tT, K, x0, y0, nx, nx * ny, nelec + plane, lambda + plane, W, lane, acc);
    else
        grad_box<false, MASKED>(tab, tT, K, x0, y0, nx, nx * ny, nelec + plane, lambda + plane, W, lane, acc);
    grad_store_sums(acc, lane, out);
}

__global__ void __launch_bounds__(64)
k_grad_src(const BandDev *__restrict__ bands, int B, int H, int W, int64_t S, const SrcRec *__restrict__ recs,
           const double *__restrict__ nelec, const double *__restrict__ lambda, double tail_T,
           double *__restrict__ sums /* S*B*GRAD_NS */) {
    grad_src_body<false>(bands, B, H, W, S, recs, nelec, lambda, tail_T, sums);
}

// the same sums on a masked image set: r(p) = 0 where nelec is NaN, nothing else differs
__global__ void __launch_bounds__(64)
k_grad_src_masked(const BandDev *__restrict__ bands, int B, int H, int W, int64_t S, const SrcRec *__restrict__ recs,
                  const double *__restrict__ nelec, const double *__restrict__ lambda, double tail_T,
                  double *__restrict__ sums /* S*B*GRAD_NS */) {
    grad_src_body<true>(bands, B, H, W, S, recs, nelec, lambda, tail_T, sums);
}

// ---- chain rule to the public coordinates (grad_chain_band), one thread per source ------------------------------------
__global__ void __launch_bounds__(256)
k_grad_chain(const BandDev *__restrict__ bands, int B, int64_t S, const SrcRec *__restrict__ recs, const int *__restrict__ type,
             const double *__restrict__ shape, const double *__restrict__ counts, const double *__restrict__ sums,
             double *__restrict__ g_radec /* S*2 or null */, double *__restrict__ g_counts /* S*B or null */,
             double *__restrict__ g_shape /* S*4 or null */) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t = type[s];
    double gra = 0.0, gdec = 0.0, gsh[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; b++) {
        const BandDev &bd = bands[b];
        const SrcRec &rec = recs[(int64_t)b * S + s];
        const double *q = sums + ((int64_t)s * B + b) * GRAD_NS;
        if (g_counts) g_counts[s * B + b] = q[0];
        if (rec.type < 0) continue;
        // (the entry point takes whole frames only: the record's row is the frame's)
        grad_chain_band(bd, rec.px, rec.py, shape + 4 * s, q, counts[s * B + b], t == 1 || t == 2, t, gra, gdec, gsh);
    }
    if (g_radec) { g_radec[2 * s] = gra; g_radec[2 * s + 1] = gdec; }
    if (g_shape) for (int i = 0; i < 4; i++) g_shape[4 * s + i] = gsh[i];
}
