// k_grad_common.h -- the pieces every derivative kernel shares (k_grad.h, k_stamp_jac.h, k_patch_grad.h, k_patch_grad_nz.h,
// k_mass_grad.h): each exists here once, force-inlined into its callers
//
//   grad_tab_fill    the component table in LDS, 8 rows of K_GAL doubles: A, B, mx, my, qa, qb, qc, var
//                    (A = theta_k A', B = +-A' = d A / d theta, the mean, the precision, var_k)
//   grad_pixel       the seven quantities of one pixel, summed over the table's components
//                        u;  m = sum g_k P_k d (2);  w = sum var_k g_k (P_k d d^T P_k - P_k) / 2 (00, 01, 11);  th = sum +-A_k' N_k
//   grad_store_sums  wave_sum the seven, lane 0 writes GRAD_NS doubles
//   grad_geom        a type-1 galaxy's Tinv in one band and its five derivatives (sigma, phi, rho, px, py), one at a time
//   grad_dw          (d00, 2 d01, d11) of dW = dT T^T + T dT^T
//   grad_chain_band  one band's sums taken to the public coordinates (ra, dec, the four shape coordinates)
// The families agree to the last bit because they are these functions: HMC, the exact conditional (which adds one family's
// rows to another's) and the derivative stamps rely on that.
#pragma once
#include "hw_source.h"

#define GRAD_NS 8      // doubles per set of sums: S_u, S_m (2), S_W (3), S_th, 0
#define GRAD_TAB (8 * K_GAL)

// lane (< K) writes its column of the table: make_comp's arithmetic with the theta factor kept apart, A = theta_k A',
// theta_k = theta (exp) / 1 - theta (dev), B = d A / d theta_k's sign times A'.  A star (gal = false) has its PSF components
// alone (var = 0, A = A', B = 0) and its record's shape is not read.  Returns A'.
// (The record goes by reference so that its loads stay where the table needs them, and no parameter here is __restrict__: either
// moves the callers' instruction schedule.)
__device__ __forceinline__ double grad_tab_fill(const BandDev *bd, const SrcRec &rec, bool gal, int lane, double *tab) {
    const int kk = gal ? lane / K_PROF : lane;
    double cxx = bd->cxx[kk], cxy = bd->cxy[kk], cyy = bd->cyy[kk], wt = bd->w[kk];
    double var = 0.0, tf = 1.0, sg = 0.0;
    if (gal) {
        const int j = c_prof_order[lane - kk * K_PROF];
        var = c_prof_var[j];
        cxx += var * rec.w00; cxy += var * rec.w01; cyy += var * rec.w11;
        wt *= c_prof_amp[j];
        const bool ex = (j < K_EXP);
        tf = ex ? rec.theta : 1.0 - rec.theta;
        sg = ex ? 1.0 : -1.0;
    }
    const double det = cxx * cyy - cxy * cxy;
    const double inv = 1.0 / det;
    const double a1 = wt * (0.5 / PI_D) * sqrt(inv);
    tab[lane] = tf * a1;
    tab[K_GAL + lane] = sg * a1;
    tab[2 * K_GAL + lane] = rec.px + bd->mux[kk];
    tab[3 * K_GAL + lane] = rec.py + bd->muy[kk];
    tab[4 * K_GAL + lane] = cyy * inv; tab[5 * K_GAL + lane] = -cxy * inv; tab[6 * K_GAL + lane] = cxx * inv;
    tab[7 * K_GAL + lane] = var;
    return a1;
}

// adds the K components' terms at (x, y) into q[7] = u, m0, m1, w00, w01, w11, th (the last four of galaxies only).
// DROP: tT holds, per component, the largest exponent that is kept; otherwise nothing is dropped and tT is not read
template <bool DROP>
__device__ __forceinline__ void grad_pixel(const double *tab, const double *tT, int K, bool gal,
                                           double x, double y, double q[7]) {
    const double *tA = tab, *tB = tab + K_GAL, *tmx = tab + 2 * K_GAL, *tmy = tab + 3 * K_GAL, *tqa = tab + 4 * K_GAL,
                 *tqb = tab + 5 * K_GAL, *tqc = tab + 6 * K_GAL, *tvar = tab + 7 * K_GAL;
    for (int k = 0; k < K; k++) {
        const double dx = x - tmx[k], dy = y - tmy[k];
        const double qa = tqa[k], qb = tqb[k], qc = tqc[k];
        const double pdx = fma(qa, dx, qb * dy), pdy = fma(qb, dx, qc * dy);
        const double h = 0.5 * fma(dx, pdx, dy * pdy);
        if (DROP && h > tT[k]) continue;
        const double e = exp(-h);
        const double g = tA[k] * e;
        q[0] += g;
        q[1] = fma(g, pdx, q[1]);
        q[2] = fma(g, pdy, q[2]);
        if (gal) {
            const double hv = 0.5 * tvar[k] * g;
            q[3] = fma(hv, fma(pdx, pdx, -qa), q[3]);
            q[4] = fma(hv, fma(pdx, pdy, -qb), q[4]);
            q[5] = fma(hv, fma(pdy, pdy, -qc), q[5]);
            q[6] = fma(tB[k], e, q[6]);
        }
    }
}

// acc += r q, the residual's weight on a pixel's seven
__device__ __forceinline__ void grad_weigh(double r, const double q[7], bool gal, double acc[7]) {
    acc[0] = fma(r, q[0], acc[0]);
    acc[1] = fma(r, q[1], acc[1]);
    acc[2] = fma(r, q[2], acc[2]);
    if (gal) {
        acc[3] = fma(r, q[3], acc[3]);
        acc[4] = fma(r, q[4], acc[4]);
        acc[5] = fma(r, q[5], acc[5]);
        acc[6] = fma(r, q[6], acc[6]);
    }
}

// closes a wave's sums in a fixed order (a shuffle tree: no atomics); lane 0 writes the GRAD_NS doubles
__device__ __forceinline__ void grad_store_sums(double acc[7], int lane, double *out) {
#pragma unroll
    for (int i = 0; i < 7; i++) acc[i] = wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = acc[i];
        out[7] = 0.0;
    }
}

// ---- chain rule to the public coordinates ------------------------------------------------------------------------------
// 2 x 2, row-major
__device__ __forceinline__ void m2mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] + a[1] * b[2]; o[1] = a[0] * b[1] + a[1] * b[3];
    o[2] = a[2] * b[0] + a[3] * b[2]; o[3] = a[2] * b[1] + a[3] * b[3];
}
// v = (d00, 2 d01, d11) of dW = dT T^T + T dT^T.  With G = (G00, G01, G11) the entry-wise gradient of a symmetric W,
// <G, dW> = G . v: the single off-diagonal parameter w01 enters C_k in both off-diagonal places, so it carries 2 G01
__device__ __forceinline__ void grad_dw(const double T[4], const double dT[4], double v[3]) {
    v[0] = 2.0 * (dT[0] * T[0] + dT[1] * T[1]);
    v[1] = 2.0 * (dT[0] * T[2] + dT[1] * T[3] + T[0] * dT[2] + T[1] * dT[3]);
    v[2] = 2.0 * (dT[2] * T[2] + dT[3] * T[3]);
}
__device__ __forceinline__ double grad_dw_dot(const double G[3], const double T[4], const double dT[4]) {
    double v[3];
    grad_dw(T, dT, v);
    return G[0] * v[0] + G[1] * v[1] + G[2] * v[2];
}

// A type-1 galaxy in one band: W = Tinv Tinv^T, Tinv = D Gm, D = CD^-1, Gm = re [[cp, sp rho], [-sp, cp rho]] (k_prep; phi in
// degrees).  cd_at_pixel's CD = [[ups0, ups1] cos(dec0) / cos(phi1), [ups2, ups3]] with dec0 the declination of the pixel
// (px, row), row counted in the FULL frame (the caller adds a window's first row): affine in (px, py), so
// d CD / d px = -sin(dec0) (pi/180) ups2 / cos(phi1) [[ups0, ups1], [0, 0]] (ups3 for py).
//   sh = the source's shape row (theta, sigma [arcsec], phi [degrees], rho);  cphi = cos(phi1)
// Calls each(i, Tinv, dTinv) with dTinv = d Tinv / d (sigma, phi_s, rho, px, py) for i = 0 .. 4, one after the other so that a
// caller holds one derivative at a time; i = 0 is left out where k_prep's floor max(1/30, sigma) holds (the derivative is zero).
template <typename F>
__device__ __forceinline__ void grad_geom(const BandDev &bd, double px, double row, const double *sh, double cphi, F &&each) {
    const double sig = sh[1], phs = sh[2], rho = sh[3];
    const double dec0 = bd.ups[2] * (px - bd.rho[0]) + bd.ups[3] * (row - bd.rho[1]) + bd.phi[1];
    const double dr = dec0 * (PI_D / 180.0);
    const double cosd = cos(dr), sind = sin(dr);
    const double CD[4] = {bd.ups[0] * cosd / cphi, bd.ups[1] * cosd / cphi, bd.ups[2], bd.ups[3]};
    const double cdet = CD[0] * CD[3] - CD[1] * CD[2];
    const double D[4] = {CD[3] / cdet, -CD[1] / cdet, -CD[2] / cdet, CD[0] / cdet};
    const double phi = (90.0 - phs) * PI_D / 180.0;
    const double re = fmax(1.0 / 30, sig) / 3600.0;
    const double cp = cos(phi), sp = sin(phi);
    const double Gm[4] = {re * cp, re * sp * rho, -re * sp, re * cp * rho};
    double Ti[4], dT[4], tmp[4], tmp2[4];
    m2mul(D, Gm, Ti);
    // sigma: Tinv is proportional to re
    if (sig > 1.0 / 30) {
        const double k = 1.0 / sig;
#pragma unroll
        for (int i = 0; i < 4; i++) dT[i] = Ti[i] * k;
        each(0, Ti, dT);
    }
    // phi [degrees]: d phi / d phi_s = -pi / 180
    {
        const double f = -PI_D / 180.0;
        const double dG[4] = {-re * sp * f, re * cp * rho * f, -re * cp * f, -re * sp * rho * f};
        m2mul(D, dG, dT);
        each(1, Ti, dT);
    }
    // rho
    {
        const double dG[4] = {0.0, re * sp, 0.0, re * cp};
        m2mul(D, dG, dT);
        each(2, Ti, dT);
    }
    // location through CD: dTinv = dD Gm = -D dCD D Gm = -D dCD Tinv
    const double f = -sind * (PI_D / 180.0) / cphi;
#pragma unroll
    for (int ax = 0; ax < 2; ax++) {
        const double a = f * bd.ups[2 + ax];
        const double dCD[4] = {a * bd.ups[0], a * bd.ups[1], 0.0, 0.0};
        m2mul(dCD, Ti, tmp);
        m2mul(D, tmp, tmp2);
#pragma unroll
        for (int i = 0; i < 4; i++) dT[i] = -tmp2[i];
        each(3 + ax, Ti, dT);
    }
}

// One band of a source: q[7] = the band's sums per count, c = the band's counts, gal = the record renders as a galaxy,
// t = the public type (1: sigma, phi, rho;  2: W's entries), row = the record's row in the full frame.  Adds into the
// gradient with respect to ra, dec [per degree] and the four shape coordinates cel_sources_set takes.
__device__ __forceinline__ void grad_chain_band(const BandDev &bd, double px, double row, const double *sh,
                                                const double q[7], double c, bool gal, int t, double &gra, double &gdec,
                                                double gsh[4]) {
    double gpx = c * q[1], gpy = c * q[2];
    const double cphi = cos(bd.phi[1] / 180.0 * PI_D);
    if (gal) {
        const double G[3] = {c * q[3], c * q[4], c * q[5]};
        gsh[0] += c * q[6];                                  // theta: both profiles, the theta factor kept apart
        if (t == 2) {
            gsh[1] += G[0];
            gsh[2] += 2.0 * G[1];
            gsh[3] += G[2];
        } else {
            double *const to[5] = {&gsh[1], &gsh[2], &gsh[3], &gpx, &gpy};
            grad_geom(bd, px, row, sh, cphi, [&](int i, const double *Ti, const double *dT) { *to[i] += grad_dw_dot(G, Ti, dT); });
        }
    }
    // equa2pixel: px = ups_inv0 (ra - phi0) cos(phi1) + ups_inv1 (dec - phi1) + rho0, and py likewise
    gra += (gpx * bd.ups_inv[0] + gpy * bd.ups_inv[2]) * cphi;
    gdec += gpx * bd.ups_inv[1] + gpy * bd.ups_inv[3];
}
