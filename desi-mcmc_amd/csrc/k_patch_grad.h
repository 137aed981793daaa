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
// and not five as long as their longest.  Lanes below K build the component table in LDS with grad_src_body's arithmetic
// (k_grad.h: A and A' with the theta factor apart, the mean, the precision, var_k; no drop threshold); the part's pixels are
// lane-strided as in grad_box; per pixel K direct exponentials, the seven quantities u; m0, m1; w00, w01, w11; th, the residual
// from the datum and seven FMAs.  In MODE 0 a pixel with z == 0 is not evaluated at all (r = 0 there, and most pixels of a faint
// source's box hold no photon).  wave_sum closes the sums; one lane writes GRAD_NS doubles.  Fixed order, no atomics: the bits
// depend on the inputs alone.
//
// k_patch_grad_chain: one thread per proposal; adds the parts in part order and the bands in band order, and takes the sums to
// the public coordinates.  The chain rule is k_grad_chain's, restated here (k_grad.h stays as it is); the record-type rules
// above replace its `rec.type < 0: continue`.  It writes the 7 + B layout: slot 0 (the value) is left to the host.
#pragma once
#include "k_grad.h"

#define PGRAD_PARTS 4

template <int MODE, bool GAL, typename TZ>
__device__ __forceinline__ void pgrad_rows(const double *__restrict__ tab, int x0, int ya, int nx, int n, const TZ *__restrict__ zd,
                                           const double *__restrict__ zn, int64_t zpitch, double counts, double eps, int lane,
                                           double acc[7]) {
    const double *tA = tab, *tB = tab + K_GAL, *tmx = tab + 2 * K_GAL, *tmy = tab + 3 * K_GAL, *tqa = tab + 4 * K_GAL,
                 *tqb = tab + 5 * K_GAL, *tqc = tab + 6 * K_GAL, *tvar = tab + 7 * K_GAL;
    const int K = GAL ? K_GAL : K_PSF;
    for (int i = lane; i < n; i += 64) {
        const int yy = i / nx, xx = i - yy * nx;
        const int64_t zi = (int64_t)yy * zpitch + xx;
        const double z = zd ? (double)zd[zi] : zn[zi];
        if (MODE == 0 && z == 0.0) continue;                  // r = 0: the pixel contributes exactly nothing
        const double x = (double)(x0 + xx), y = (double)(ya + yy);
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
        const double m = counts * u;
        double r;
        if (MODE == 0) r = (m > 0.0) ? z / m : 0.0;
        else if (MODE == 2) r = (m > 0.0) ? z / m - 1.0 : 0.0;
        else r = z / (m + eps) - 1.0;
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

// TZ: the patch data's element type, as k_patch_ll's -- double for a caller's patches and for nelec, int for the resident split
template <int MODE, typename TZ>
__global__ void __launch_bounds__(64)
k_patch_grad(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs,
             const int *__restrict__ owner /* P, or nullptr = 0 */, const int4 *__restrict__ pbox /* NB*B: x0, x1, y0, y1 */,
             const int64_t *__restrict__ offsets /* NB*B+1 */, const TZ *__restrict__ data,
             const double *__restrict__ nelec /* used when data == nullptr */, int H, int W,
             double *__restrict__ sums /* P*B*PGRAD_PARTS*GRAD_NS */) {
    __shared__ double tab[8 * K_GAL];      // 8 rows of K_GAL doubles: A, B, mx, my, qa, qb, qc, var (k_stamp_jac's layout)
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
#pragma unroll
    for (int i = 0; i < 7; i++) acc[i] = wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; i++) out[i] = acc[i];
        out[7] = 0.0;
    }
}

// ---- chain rule to the public coordinates, one thread per proposal -------------------------------------------------------
// <G, dW> for dW = dT T^T + T dT^T with G = (G00, G01, G11) the entry-wise gradient of a symmetric W: w01 enters C_k in both
// off-diagonal places, so it carries 2 G01 (k_grad.h's contract_dw)
__device__ __forceinline__ double pgrad_dw(const double G[3], const double T[4], const double dT[4]) {
    const double d00 = 2.0 * (dT[0] * T[0] + dT[1] * T[1]);
    const double d01 = dT[0] * T[2] + dT[1] * T[3] + T[0] * dT[2] + T[1] * dT[3];
    const double d11 = 2.0 * (dT[2] * T[2] + dT[3] * T[3]);
    return G[0] * d00 + 2.0 * G[1] * d01 + G[2] * d11;
}
__device__ __forceinline__ void pgrad_m2mul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] + a[1] * b[2]; o[1] = a[0] * b[1] + a[1] * b[3];
    o[2] = a[2] * b[0] + a[3] * b[2]; o[3] = a[2] * b[1] + a[3] * b[3];
}

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
        const double c = counts[p * B + b];
        double gpx = c * q[1], gpy = c * q[2];
        const double cphi = cos(bd.phi[1] / 180.0 * PI_D);
        if (gal) {
            const double G[3] = {c * q[3], c * q[4], c * q[5]};
            gsh[0] += c * q[6];                              // theta: both profiles, the theta factor kept apart
            if (t == 2) {
                gsh[1] += G[0];
                gsh[2] += 2.0 * G[1];
                gsh[3] += G[2];
            } else {
                // W = Tinv Tinv^T, Tinv = D Gm, D = CD^-1, Gm = re [[cp, sp rho], [-sp, cp rho]] (k_prep; phi in degrees).
                // cd_at_pixel's CD = [[ups0, ups1] cos(dec0) / cos(phi1), [ups2, ups3]] with dec0 the pixel's declination:
                // affine in (px, py), so d CD / d px = -sin(dec0) (pi/180) ups2 / cos(phi1) [[ups0, ups1], [0, 0]] (ups3 for py)
                const double sig = shape[4 * p + 1], phs = shape[4 * p + 2], rho = shape[4 * p + 3];
                const double dec0 = bd.ups[2] * (rec.px - bd.rho[0]) + bd.ups[3] * (rec.py - bd.rho[1]) + bd.phi[1];
                const double dr = dec0 * (PI_D / 180.0);
                const double cosd = cos(dr), sind = sin(dr);
                const double CD[4] = {bd.ups[0] * cosd / cphi, bd.ups[1] * cosd / cphi, bd.ups[2], bd.ups[3]};
                const double cdet = CD[0] * CD[3] - CD[1] * CD[2];
                const double D[4] = {CD[3] / cdet, -CD[1] / cdet, -CD[2] / cdet, CD[0] / cdet};
                const double phi = (90.0 - phs) * PI_D / 180.0;
                const double re = fmax(1.0 / 30, sig) / 3600.0;
                const double cp = cos(phi), sn = sin(phi);
                const double Gm[4] = {re * cp, re * sn * rho, -re * sn, re * cp * rho};
                double Ti[4], dT[4], tmp[4], tmp2[4];
                pgrad_m2mul(D, Gm, Ti);
                // sigma: Tinv is proportional to re; zero where the floor 1/30 holds
                if (sig > 1.0 / 30) {
                    const double k = 1.0 / sig;
                    for (int i = 0; i < 4; i++) dT[i] = Ti[i] * k;
                    gsh[1] += pgrad_dw(G, Ti, dT);
                }
                // phi [degrees]: d phi / d phi_s = -pi / 180
                {
                    const double f = -PI_D / 180.0;
                    const double dG[4] = {-re * sn * f, re * cp * rho * f, -re * cp * f, -re * sn * rho * f};
                    pgrad_m2mul(D, dG, dT);
                    gsh[2] += pgrad_dw(G, Ti, dT);
                }
                // rho
                {
                    const double dG[4] = {0.0, re * sn, 0.0, re * cp};
                    pgrad_m2mul(D, dG, dT);
                    gsh[3] += pgrad_dw(G, Ti, dT);
                }
                // location through CD: dTinv = dD Gm = -D dCD D Gm = -D dCD Tinv
                const double f = -sind * (PI_D / 180.0) / cphi;
                for (int ax = 0; ax < 2; ax++) {
                    const double a = f * bd.ups[2 + ax];
                    const double dCD[4] = {a * bd.ups[0], a * bd.ups[1], 0.0, 0.0};
                    pgrad_m2mul(dCD, Ti, tmp);
                    pgrad_m2mul(D, tmp, tmp2);
                    for (int i = 0; i < 4; i++) dT[i] = -tmp2[i];
                    const double gl = pgrad_dw(G, Ti, dT);
                    if (ax == 0) gpx += gl; else gpy += gl;
                }
            }
        }
        // equa2pixel: px = ups_inv0 (ra - phi0) cos(phi1) + ups_inv1 (dec - phi1) + rho0, and py likewise
        gra += (gpx * bd.ups_inv[0] + gpy * bd.ups_inv[2]) * cphi;
        gdec += gpx * bd.ups_inv[1] + gpy * bd.ups_inv[3];
    }
    o[0] = 0.0;
    o[1] = gra; o[2] = gdec;
    for (int i = 0; i < 4; i++) o[3 + i] = gsh[i];
}
