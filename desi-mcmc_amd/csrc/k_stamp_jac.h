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
// Per pixel the kernel forms the seven quantities of grad_pixel (k_grad_common.h), each summed over the K components,
//   u;  m = sum g_k P_k d (2);  w = sum var_k g_k (P_k d d^T P_k - P_k) / 2 (00, 01, 11);  th = sum +-A_k' N_k
// and takes them to the public planes with ONE matrix per (source, band): k_grad_chain's chain rule is linear in the seven
// and its coefficients depend on the source and the band only.  One lane builds that matrix (6 x 7, planes 1 .. 6) in LDS
// while the lanes below K build the component table; a pixel then costs K exponentials, the seven accumulations and a small
// matrix-vector product.  The table, the seven and the chain's geometry are k_grad_common.h's, shared with k_grad.h.
//
// Nothing is dropped: every component is evaluated at every pixel of the box, whatever CEL_OPT_TAIL_LOG[_SOURCE] says.  A
// derivative can vanish where the value does not (and the reverse), so a drop rule relative to the pixel's value bounds
// nothing here.
//
// Layout: one wave per StampJob chunk (a strip of sw = 32 or 64 columns, <= 64 rows), lanes along x -- 64 / sw rows at a
// time -- so every plane's row segment is one coalesced store.
#pragma once
#include "k_misc.h"
#include "k_grad_common.h"

#define JAC_NQ 7       // internal per-pixel quantities: u, m0, m1, w00, w01, w11, th
#define JAC_NP 6       // derivative planes (1 .. 6)

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
            // grad_geom, dec0 at the record's row in the full frame: sigma (its row stays zero where the floor 1/30 holds), phi
            // [degrees], rho; then the location through CD
            grad_geom(bd, rec.px, rec.py + (double)win_y0, sh, cphi, [&](int i, const double *Ti, const double *dT) {
                double v[3];
                grad_dw(Ti, dT, v);
                if (i < 3) {
                    double *r = M + (3 + i) * JAC_NQ + 3;
                    r[0] = c * v[0]; r[1] = c * v[1]; r[2] = c * v[2];
                } else {
                    double *l = (i == 3) ? lx : ly;
                    l[0] = v[0]; l[1] = v[1]; l[2] = v[2];
                }
            });
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

template <bool GAL>
__device__ __forceinline__ void jac_rows(const double *__restrict__ tab, const double *__restrict__ M, double c, int xi,
                                         int ya, int y1, int ystep, double *__restrict__ o /* at (row ya, column xi) */,
                                         int64_t nx, int64_t area) {
    const double x = (double)xi;
    for (int yi = ya; yi < y1; yi += ystep, o += (int64_t)ystep * nx) {
        double q[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        grad_pixel<false>(tab, nullptr, GAL ? K_GAL : K_PSF, GAL, x, (double)yi, q);
        const double u = q[0], m0 = q[1], m1 = q[2], w00 = q[3], w01 = q[4], w11 = q[5], th = q[6];
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
    __shared__ double tab[GRAD_TAB];
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
    if (lane < K) grad_tab_fill(bd, *rp, gal, lane, tab);
    if (lane == 63) jac_matrix(*bd, *rp, gal, type[jb.src], shape + 4 * (int64_t)jb.src, win_y0, c, M);
    __syncthreads();
    const int xi = jb.x0 + (lane & (sw - 1));
    if (xi >= ob.y) return;
    const int ystep = 64 / sw, ya = jb.y0 + lane / sw;
    double *o = out + offsets[jb.src] + (int64_t)(ya - ob.z) * nx + (xi - ob.x);
    if (gal) jac_rows<true>(tab, M, c, xi, ya, jb.y1, ystep, o, nx, area);
    else jac_rows<false>(tab, M, c, xi, ya, jb.y1, ystep, o, nx, area);
}
