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
// the counts, takes the sums to the public coordinates analytically and adds the bands in order.
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
#include "hw_source.h"

#define GRAD_NS 8      // doubles per (source, band) of k_grad_src's output: S_u, S_m (2), S_W (3), S_th, 0

// one wave per (source, band), job = s * B + b; the component table in LDS, the box's pixels strided over the lanes
// MASKED (a masked image set, k_grad_src_masked): a NaN count marks a pixel that was not observed -- r = 0 there
template <bool GAL, bool MASKED = false>
__device__ __forceinline__ void grad_box(const double *__restrict__ tA, const double *__restrict__ tB,
                                         const double *__restrict__ tmx, const double *__restrict__ tmy,
                                         const double *__restrict__ tqa, const double *__restrict__ tqb,
                                         const double *__restrict__ tqc, const double *__restrict__ tvar,
                                         const double *__restrict__ tT, int K, int x0, int y0, int nx, int n,
                                         const double *__restrict__ ne_p, const double *__restrict__ la_p, int W, int lane,
                                         double acc[7]) {
    for (int i = lane; i < n; i += 64) {
        const int yy = i / nx, xx = i - yy * nx;
        const double x = (double)(x0 + xx), y = (double)(y0 + yy);
        double u = 0.0, m0 = 0.0, m1 = 0.0, w00 = 0.0, w01 = 0.0, w11 = 0.0, th = 0.0;
        for (int k = 0; k < K; k++) {
            const double dx = x - tmx[k], dy = y - tmy[k];
            const double qa = tqa[k], qb = tqb[k], qc = tqc[k];
            const double pdx = fma(qa, dx, qb * dy), pdy = fma(qb, dx, qc * dy);
            const double h = 0.5 * fma(dx, pdx, dy * pdy);
            if (h > tT[k]) continue;                          // dropped at this pixel (never when T = 0: tT = +inf)
            const double e = exp(-h);
            const double g = tA[k] * e;
            u += g;
            m0 = fma(g, pdx, m0);
            m1 = fma(g, pdy, m1);
            if (GAL) {
                const double hv = 0.5 * tvar[k] * g;
                w00 = fma(hv, fma(pdx, pdx, -qa), w00);
                w01 = fma(hv, fma(pdx, pdy, -qb), w01);
                w11 = fma(hv, fma(pdy, pdy, -qc), w11);
                th = fma(tB[k], e, th);
            }
        }
        const int64_t idx = (int64_t)(y0 + yy) * W + (x0 + xx);
        const double ne = ne_p[idx], la = la_p[idx];
        const double r = (!MASKED || ne == ne) ? ne / la - 1.0 : 0.0;
        acc[0] = fma(r, u, acc[0]);
        acc[1] = fma(r, m0, acc[1]);
        acc[2] = fma(r, m1, acc[2]);
        if (GAL) {
            acc[3] = fma(r, w00, acc[3]);
            acc[4] = fma(r, w01, acc[4]);
            acc[5] = fma(r, w11, acc[5]);
            acc[6] = fma(r, th, acc[6]);
        }
    }
}

template <bool MASKED>
__device__ __forceinline__ void grad_src_body(const BandDev *__restrict__ bands, int B, int H, int W, int64_t S, const SrcRec *__restrict__ recs,
                                              const double *__restrict__ nelec, const double *__restrict__ lambda, double tail_T,
                                              double *__restrict__ sums /* S*B*GRAD_NS */) {
    __shared__ double tA[K_GAL], tB[K_GAL], tmx[K_GAL], tmy[K_GAL], tqa[K_GAL], tqb[K_GAL], tqc[K_GAL], tvar[K_GAL], tT[K_GAL];
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
        // make_comp's arithmetic, with the theta factor kept apart: A = theta_k A', theta_k = theta (exp) / 1 - theta (dev)
        const int kk = gal ? lane / K_PROF : lane;
        double cxx = bd->cxx[kk], cxy = bd->cxy[kk], cyy = bd->cyy[kk], wt = bd->w[kk];
        double var = 0.0, tf = 1.0, sg = 0.0;
        if (gal) {
            const int j = c_prof_order[lane - kk * K_PROF];
            var = c_prof_var[j];
            cxx += var * rp->w00; cxy += var * rp->w01; cyy += var * rp->w11;
            wt *= c_prof_amp[j];
            const bool ex = (j < K_EXP);
            tf = ex ? rp->theta : 1.0 - rp->theta;
            sg = ex ? 1.0 : -1.0;
        }
        const double det = cxx * cyy - cxy * cxy;
        const double inv = 1.0 / det;
        const double a1 = wt * (0.5 / PI_D) * sqrt(inv);
        tA[lane] = tf * a1;
        tB[lane] = sg * a1;
        tmx[lane] = rp->px + bd->mux[kk];
        tmy[lane] = rp->py + bd->muy[kk];
        tqa[lane] = cyy * inv; tqb[lane] = -cxy * inv; tqc[lane] = cxx * inv;
        tvar[lane] = var;
        // HW_DROP_SKY: keep where max(counts, 1) |A'| e^-h >= eps e^-T  <=>  h <= T + log(max(counts, 1) |A'| / eps)
        tT[lane] = (tail_T > 0.0) ? tail_T + log(fmax(fabs(rp->scale), 1.0) * fabs(a1) / bd->eps) : INFINITY;
    }
    __syncthreads();
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t plane = (int64_t)b * H * W;
    if (gal)
        grad_box<true, MASKED>(tA, tB, tmx, tmy, tqa, tqb, tqc, tvar, tT, K, x0, y0, nx, nx * ny, nelec + plane, lambda + plane, W, lane, acc);
    else
        grad_box<false, MASKED>(tA, tB, tmx, tmy, tqa, tqb, tqc, tvar, tT, K, x0, y0, nx, nx * ny, nelec + plane, lambda + plane, W, lane, acc);
#pragma unroll
    for (int i = 0; i < 7; i++) acc[i] = wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = acc[i];
        out[7] = 0.0;
    }
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

// ---- chain rule to the public coordinates, one thread per source --------------------------------------------------------
// 2 x 2 helpers, row-major
__device__ inline void m2mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] + a[1] * b[2]; o[1] = a[0] * b[1] + a[1] * b[3];
    o[2] = a[2] * b[0] + a[3] * b[2]; o[3] = a[2] * b[1] + a[3] * b[3];
}
// <G, dW> for dW = dT T^T + T dT^T, with G the entry-wise gradient of a symmetric W held as (G00, G01, G11): the single
// off-diagonal parameter w01 enters C_k in both off-diagonal places, so it carries 2 G01
__device__ inline double contract_dw(const double G[3], const double T[4], const double dT[4]) {
    const double d00 = 2.0 * (dT[0] * T[0] + dT[1] * T[1]);
    const double d01 = dT[0] * T[2] + dT[1] * T[3] + T[0] * dT[2] + T[1] * dT[3];
    const double d11 = 2.0 * (dT[2] * T[2] + dT[3] * T[3]);
    return G[0] * d00 + 2.0 * G[1] * d01 + G[2] * d11;
}

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
        const double c = counts[s * B + b];
        double gpx = c * q[1], gpy = c * q[2];
        const double G[3] = {c * q[3], c * q[4], c * q[5]};
        const double cphi = cos(bd.phi[1] / 180.0 * PI_D);
        if (t == 1) {
            // W = Tinv Tinv^T, Tinv = D Gm, D = CD^-1, Gm = re [[cp, sp rho], [-sp, cp rho]] (k_prep; Q7: phi in degrees).
            // cd_at_pixel's CD = [[ups0, ups1] cos(dec0) / cos(phi1), [ups2, ups3]] with dec0 the pixel's declination:
            // affine in (px, py), so d CD / d px = -sin(dec0) (pi/180) ups2 / cos(phi1) [[ups0, ups1], [0, 0]] (ups3 for py)
            const double sig = shape[4 * s + 1], phs = shape[4 * s + 2], rho = shape[4 * s + 3];
            const double dec0 = bd.ups[2] * (rec.px - bd.rho[0]) + bd.ups[3] * (rec.py - bd.rho[1]) + bd.phi[1];
            const double dr = dec0 * (PI_D / 180.0);
            const double cosd = cos(dr), sind = sin(dr);
            const double CD[4] = {bd.ups[0] * cosd / cphi, bd.ups[1] * cosd / cphi, bd.ups[2], bd.ups[3]};
            const double cdet = CD[0] * CD[3] - CD[1] * CD[2];
            const double D[4] = {CD[3] / cdet, -CD[1] / cdet, -CD[2] / cdet, CD[0] / cdet};
            const double phi = (90.0 - phs) * PI_D / 180.0;
            const double re = fmax(1.0 / 30, sig) / 3600.0;
            const double cp = cos(phi), sp = sin(phi);
            const double Gm[4] = {re * cp, re * sp * rho, -re * sp, re * cp * rho};
            double Ti[4];
            m2mul(D, Gm, Ti);
            double dT[4], tmp[4], tmp2[4];
            // sigma: Tinv is proportional to re; zero where the floor 1/30 holds
            if (sig > 1.0 / 30) {
                const double k = 1.0 / sig;
                for (int i = 0; i < 4; i++) dT[i] = Ti[i] * k;
                gsh[1] += contract_dw(G, Ti, dT);
            }
            // phi [degrees]: d phi / d phi_s = -pi / 180
            {
                const double f = -PI_D / 180.0;
                const double dG[4] = {-re * sp * f, re * cp * rho * f, -re * cp * f, -re * sp * rho * f};
                m2mul(D, dG, dT);
                gsh[2] += contract_dw(G, Ti, dT);
            }
            // rho
            {
                const double dG[4] = {0.0, re * sp, 0.0, re * cp};
                m2mul(D, dG, dT);
                gsh[3] += contract_dw(G, Ti, dT);
            }
            // location through CD: dTinv = dD Gm = -D dCD D Gm = -D dCD Tinv
            const double f = -sind * (PI_D / 180.0) / cphi;
            for (int ax = 0; ax < 2; ax++) {
                const double a = f * bd.ups[2 + ax];
                const double dCD[4] = {a * bd.ups[0], a * bd.ups[1], 0.0, 0.0};
                m2mul(dCD, Ti, tmp);
                m2mul(D, tmp, tmp2);
                for (int i = 0; i < 4; i++) dT[i] = -tmp2[i];
                const double gl = contract_dw(G, Ti, dT);
                if (ax == 0) gpx += gl; else gpy += gl;
            }
            gsh[0] += c * q[6];
        } else if (t == 2) {
            gsh[0] += c * q[6];
            gsh[1] += G[0];
            gsh[2] += 2.0 * G[1];
            gsh[3] += G[2];
        }
        // equa2pixel: px = ups_inv0 (ra - phi0) cos(phi1) + ups_inv1 (dec - phi1) + rho0, and py likewise
        gra += (gpx * bd.ups_inv[0] + gpy * bd.ups_inv[2]) * cphi;
        gdec += gpx * bd.ups_inv[1] + gpy * bd.ups_inv[3];
    }
    if (g_radec) { g_radec[2 * s] = gra; g_radec[2 * s + 1] = gdec; }
    if (g_shape) for (int i = 0; i < 4; i++) g_shape[4 * s + i] = gsh[i];
}
