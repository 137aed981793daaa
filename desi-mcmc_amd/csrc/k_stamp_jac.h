// k_stamp_jac.h -- derivative stamps: a source's stamp and its per-pixel derivatives with respect to the source's own
// parameters (cel_render_stamps, scaled = 2 | 3)
//
// Planes of one source, packed row-major one after another in its slot (each the size of the output box):
//   0        the stamp (unit, or times counts[s][band])
//   1, 2     d / d ra, d / d dec, per degree
//   3 .. 6   galaxies only: d / d of the four shape coordinates cel_sources_set takes
//            (type 1: theta, sigma [arcsec], phi [degrees], rho;  type 2: theta, W00, W01, W11)
// The conventions are k_grad.h's: the integer box is held fixed; ra / dec act through equa2pixel and, for a type-1 galaxy,
// through cd_at_pixel's cos(dec) term in W; d / d sigma is 0 where k_prep's floor max(1/30, sigma) holds.
//
// Per pixel the kernel forms the seven quantities of grad_box (k_grad.h), each summed over the K components,
//   u;  m = sum g_k P_k d (2);  w = sum var_k g_k (P_k d d^T P_k - P_k) / 2 (00, 01, 11);  th = sum +-A_k' N_k
// and takes them to the public planes with ONE matrix per (source, band): k_grad_chain's chain rule is linear in the seven
// and its coefficients depend on the source and the band only.  One lane builds that matrix (6 x 7, planes 1 .. 6) in LDS
// while the lanes below K build the component table; a pixel then costs K exponentials, the seven accumulations and a small
// matrix-vector product.  The chain is restated here and k_grad.h is left as it is (its outputs stay bit for bit).
//
// Nothing is dropped: every component is evaluated at every pixel of the box, whatever CEL_OPT_TAIL_LOG[_SOURCE] says.  A
// derivative can vanish where the value does not (and the reverse), so a drop rule relative to the pixel's value bounds
// nothing here.
//
// Layout: one wave per StampJob chunk (a strip of sw = 32 or 64 columns, <= 64 rows), lanes along x -- 64 / sw rows at a
// time -- so every plane's row segment is one coalesced store.
#pragma once
#include "k_misc.h"

#define JAC_NQ 7       // internal per-pixel quantities: u, m0, m1, w00, w01, w11, th
#define JAC_NP 6       // derivative planes (1 .. 6)

// (d00, 2 d01, d11) of dW = dT T^T + T dT^T: <G, dW> of k_grad.h's contract_dw is G . v (w01 enters C_k in both
// off-diagonal places)
__device__ __forceinline__ void jac_dw(const double T[4], const double dT[4], double v[3]) {
    v[0] = 2.0 * (dT[0] * T[0] + dT[1] * T[1]);
    v[1] = 2.0 * (dT[0] * T[2] + dT[1] * T[3] + T[0] * dT[2] + T[1] * dT[3]);
    v[2] = 2.0 * (dT[2] * T[2] + dT[3] * T[3]);
}
__device__ __forceinline__ void jac_m2mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] + a[1] * b[2]; o[1] = a[0] * b[1] + a[1] * b[3];
    o[2] = a[2] * b[0] + a[3] * b[2]; o[3] = a[2] * b[1] + a[3] * b[3];
}

// the matrix M[plane - 1][quantity] of one (source, band); c = counts or 1; t = the public type (1 or 2; a star has gal = false)
__device__ __forceinline__ void jac_matrix(const BandDev &bd, const SrcRec &rec, bool gal, int t, const double *__restrict__ sh,
                                           int win_y0, double c, double *__restrict__ M) {
#pragma unroll
    for (int i = 0; i < JAC_NP * JAC_NQ; i++) M[i] = 0.0;
    const double cphi = cos(bd.phi[1] / 180.0 * PI_D);
    // d (px, py) per unit of (m0, m1, w00, w01, w11): the means, and for type 1 the location's way into W through CD
    double lx[3] = {0.0, 0.0, 0.0}, ly[3] = {0.0, 0.0, 0.0};
    if (gal) {
        M[2 * JAC_NQ + 6] = c;                                   // theta: both profiles, the theta factor kept apart
        if (t == 2) {
            M[3 * JAC_NQ + 3] = c;
            M[4 * JAC_NQ + 4] = 2.0 * c;
            M[5 * JAC_NQ + 5] = c;
        } else {
            // W = Tinv Tinv^T, Tinv = D Gm, D = CD^-1, Gm = re [[cp, sp rho], [-sp, cp rho]] (k_prep); cd_at_pixel's
            // CD = [[ups0, ups1] cos(dec0) / cos(phi1), [ups2, ups3]] with dec0 the pixel's declination (full-frame row)
            const double sig = sh[1], phs = sh[2], rho = sh[3];
            const double dec0 = bd.ups[2] * (rec.px - bd.rho[0]) + bd.ups[3] * ((rec.py + (double)win_y0) - bd.rho[1]) + bd.phi[1];
            const double dr = dec0 * (PI_D / 180.0);
            const double cosd = cos(dr), sind = sin(dr);
            const double CD[4] = {bd.ups[0] * cosd / cphi, bd.ups[1] * cosd / cphi, bd.ups[2], bd.ups[3]};
            const double cdet = CD[0] * CD[3] - CD[1] * CD[2];
            const double D[4] = {CD[3] / cdet, -CD[1] / cdet, -CD[2] / cdet, CD[0] / cdet};
            const double phi = (90.0 - phs) * PI_D / 180.0;
            const double re = fmax(1.0 / 30, sig) / 3600.0;
            const double cp = cos(phi), sp = sin(phi);
            const double Gm[4] = {re * cp, re * sp * rho, -re * sp, re * cp * rho};
            double Ti[4], dT[4], v[3];
            jac_m2mul(D, Gm, Ti);
            // sigma: Tinv is proportional to re; zero where the floor 1/30 holds
            if (sig > 1.0 / 30) {
                const double k = 1.0 / sig;
#pragma unroll
                for (int i = 0; i < 4; i++) dT[i] = Ti[i] * k;
                jac_dw(Ti, dT, v);
                M[3 * JAC_NQ + 3] = c * v[0]; M[3 * JAC_NQ + 4] = c * v[1]; M[3 * JAC_NQ + 5] = c * v[2];
            }
            // phi [degrees]: d phi / d phi_s = -pi / 180
            {
                const double f = -PI_D / 180.0;
                const double dG[4] = {-re * sp * f, re * cp * rho * f, -re * cp * f, -re * sp * rho * f};
                jac_m2mul(D, dG, dT);
                jac_dw(Ti, dT, v);
                M[4 * JAC_NQ + 3] = c * v[0]; M[4 * JAC_NQ + 4] = c * v[1]; M[4 * JAC_NQ + 5] = c * v[2];
            }
            // rho
            {
                const double dG[4] = {0.0, re * sp, 0.0, re * cp};
                jac_m2mul(D, dG, dT);
                jac_dw(Ti, dT, v);
                M[5 * JAC_NQ + 3] = c * v[0]; M[5 * JAC_NQ + 4] = c * v[1]; M[5 * JAC_NQ + 5] = c * v[2];
            }
            // location through CD: dTinv = -D dCD Tinv, dCD / d px = -sin(dec0) (pi/180) ups2 / cos(phi1) [[ups0, ups1], [0, 0]]
            const double f = -sind * (PI_D / 180.0) / cphi;
            double tmp[4], tmp2[4];
            {
                const double a = f * bd.ups[2];
                const double dCD[4] = {a * bd.ups[0], a * bd.ups[1], 0.0, 0.0};
                jac_m2mul(dCD, Ti, tmp);
                jac_m2mul(D, tmp, tmp2);
#pragma unroll
                for (int i = 0; i < 4; i++) dT[i] = -tmp2[i];
                jac_dw(Ti, dT, lx);
            }
            {
                const double a = f * bd.ups[3];
                const double dCD[4] = {a * bd.ups[0], a * bd.ups[1], 0.0, 0.0};
                jac_m2mul(dCD, Ti, tmp);
                jac_m2mul(D, tmp, tmp2);
#pragma unroll
                for (int i = 0; i < 4; i++) dT[i] = -tmp2[i];
                jac_dw(Ti, dT, ly);
            }
        }
    }
    // equa2pixel: px = ups_inv0 (ra - phi0) cos(phi1) + ups_inv1 (dec - phi1) + rho0, and py likewise
    const double ax = c * bd.ups_inv[0] * cphi, ay = c * bd.ups_inv[2] * cphi;     // ra:  d px, d py
    const double bx = c * bd.ups_inv[1], by = c * bd.ups_inv[3];                   // dec
    M[0 * JAC_NQ + 1] = ax; M[0 * JAC_NQ + 2] = ay;
    M[1 * JAC_NQ + 1] = bx; M[1 * JAC_NQ + 2] = by;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        M[0 * JAC_NQ + 3 + i] = ax * lx[i] + ay * ly[i];
        M[1 * JAC_NQ + 3 + i] = bx * lx[i] + by * ly[i];
    }
}

// tab: 8 rows of K_GAL doubles: A, B, mx, my, qa, qb, qc, var
template <bool GAL>
__device__ __forceinline__ void jac_rows(const double *__restrict__ tab, const double *__restrict__ M, double c, int xi,
                                         int ya, int y1, int ystep, double *__restrict__ o /* at (row ya, column xi) */,
                                         int64_t nx, int64_t area) {
    const double *tA = tab, *tB = tab + K_GAL, *tmx = tab + 2 * K_GAL, *tmy = tab + 3 * K_GAL, *tqa = tab + 4 * K_GAL,
                 *tqb = tab + 5 * K_GAL, *tqc = tab + 6 * K_GAL, *tvar = tab + 7 * K_GAL;
    const int K = GAL ? K_GAL : K_PSF;
    const double x = (double)xi;
    for (int yi = ya; yi < y1; yi += ystep, o += (int64_t)ystep * nx) {
        const double y = (double)yi;
        double u = 0.0, m0 = 0.0, m1 = 0.0, w00 = 0.0, w01 = 0.0, w11 = 0.0, th = 0.0;
        for (int k = 0; k < K; k++) {
            const double dx = x - tmx[k], dy = y - tmy[k];
            const double qa = tqa[k], qb = tqb[k], qc = tqc[k];
            const double pdx = fma(qa, dx, qb * dy), pdy = fma(qb, dx, qc * dy);
            const double h = 0.5 * fma(dx, pdx, dy * pdy);
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
        o[0] = c * u;
        if (GAL) {
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const double *r = M + p * JAC_NQ;
                o[(p + 1) * area] = fma(r[1], m0, fma(r[2], m1, fma(r[3], w00, fma(r[4], w01, r[5] * w11))));
            }
            o[3 * area] = M[2 * JAC_NQ + 6] * th;
#pragma unroll
            for (int p = 3; p < JAC_NP; p++) {
                const double *r = M + p * JAC_NQ;
                o[(p + 1) * area] = fma(r[3], w00, fma(r[4], w01, r[5] * w11));
            }
        } else {
            o[area] = fma(M[1], m0, M[2] * m1);
            o[2 * area] = fma(M[JAC_NQ + 1], m0, M[JAC_NQ + 2] * m1);
        }
    }
}

__global__ void __launch_bounds__(64)
k_stamp_jac(const BandDev *__restrict__ bands, int band, const SrcRec *__restrict__ recs /* the band's slice */,
            const StampJob *__restrict__ jobs, const int4 *__restrict__ obox, const int64_t *__restrict__ offsets,
            const int *__restrict__ type, const double *__restrict__ shape, int win_y0, int sw /* strip width: 32 or 64 */,
            int scaled, double *__restrict__ out) {
    __shared__ double tab[8 * K_GAL];
    __shared__ double M[JAC_NP * JAC_NQ];
    const int lane = threadIdx.x;
    const StampJob jb = jobs[blockIdx.x];
    const SrcRec *rp = recs + jb.src;
    const int4 ob = obox[jb.src];           // output box: x0, x1, y0, y1
    const int nx = ob.y - ob.x;
    const int64_t area = (int64_t)nx * (ob.w - ob.z);
    // the slot's size, which the host has checked against the catalogue's types, says how many planes there are: a star's 3
    // or a galaxy's 7 -- so that nothing this kernel reads can take a store outside the slot
    const bool gal = (offsets[jb.src + 1] - offsets[jb.src]) == 7 * area;
    const int K = gal ? K_GAL : K_PSF;
    const BandDev *bd = bands + band;
    const double c = scaled ? rp->scale : 1.0;
    if (lane < K) {
        // grad_src_body's arithmetic (make_comp's, with the theta factor kept apart): A = theta_k A'
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
        tab[lane] = tf * a1;
        tab[K_GAL + lane] = sg * a1;
        tab[2 * K_GAL + lane] = rp->px + bd->mux[kk];
        tab[3 * K_GAL + lane] = rp->py + bd->muy[kk];
        tab[4 * K_GAL + lane] = cyy * inv; tab[5 * K_GAL + lane] = -cxy * inv; tab[6 * K_GAL + lane] = cxx * inv;
        tab[7 * K_GAL + lane] = var;
    }
    if (lane == 63) jac_matrix(*bd, *rp, gal, type[jb.src], shape + 4 * (int64_t)jb.src, win_y0, c, M);
    __syncthreads();
    const int xi = jb.x0 + (lane & (sw - 1));
    if (xi >= ob.y) return;
    const int ystep = 64 / sw, ya = jb.y0 + lane / sw;
    double *o = out + offsets[jb.src] + (int64_t)(ya - ob.z) * nx + (xi - ob.x);
    if (gal) jac_rows<true>(tab, M, c, xi, ya, jb.y1, ystep, o, nx, area);
    else jac_rows<false>(tab, M, c, xi, ya, jb.y1, ystep, o, nx, area);
}
