// k_patch_grad_nz.h -- the mode-0 gradient sums of k_patch_grad.h, taken at a patch's photon list instead of over its pixels
//
// Definition.  k_patch_grad<0, int> on a resident split's patch skips every pixel with z == 0 (r = z / m is 0 there), so its
// seven sums run over exactly the pixels of the patch's photon list (k_nz_compact, k_split.h: the pixels with z != 0, as
// (x | y << 16, z)).  pgrad_nz_sums forms the same seven sums over that list -- the same terms in another order, with every
// lane on a photon -- and writes k_patch_grad's layout, sums[(job * PGRAD_PARTS + part) * GRAD_NS + i]:
//     i = 0: sum r u;   1, 2: sum r m0, sum r m1;   3, 4, 5: sum r w00, sum r w01, sum r w11;   6: sum r th;   7: 0
// with r = z / (counts u) where counts u > 0, else 0 (no 0 / 0: every output is finite whenever the value is).
// k_patch_grad_chain reads them as it reads the dense kernel's: the record-type rules, the chain rule and the - wsum_b of
// the counts entry stay where they are.
//
// Jobs that write eight zeros, at their first instructions: owner < 0 (the HMC launch covers every chain, running or not), an
// empty patch in the band, type -3 (the overlap-test miss: only the mass term, which the chain adds), an empty list, and a
// part the dealing rule gives no trip.  Types -1 / -2 (own box empty) render their kind, as in the dense kernel.
//
// Dealing.  One wave per (proposal, band, part).  A list's trips are PGNZ_TRIP photons each.  A list of at most
// PGNZ_DEAL_PHOTONS photons is taken whole by part 0; a longer one is dealt trip t -> part t mod PGRAD_PARTS.  The rule reads
// the list's length alone: the bits depend on the inputs only, and a proposal scored alone returns the bits of its row in a
// batch of 10 000.  A lane adds its photons of its trips in trip order, wave_sum closes the sums, k_patch_grad_chain adds the
// parts in part order.  No atomics.
// (The threshold: a block's set-up -- record, tables, the pair decomposition -- is ~700 instructions, a galaxy's trip
// 42 x 2 x ~27 + the exponentials, a star's a tenth of that.  Below four trips the set-up repeated on three more waves buys
// little on a full device; above, a 10 000-photon galaxy patch would be one wave's work for the whole launch.)
//
// Nothing is dropped (k_patch_grad.h's reasoning): every component at every photon; CEL_OPT_TAIL_LOG[_SOURCE] is not read.
//
// Arithmetic.  Exponentials by the 256-entry table and its cubic (exp_tab256_p3: 1.4083e-13 relative, tests/test_primitives.py).
// Coordinates are taken relative to the SOURCE (X = x - px): a component's centre seen from there is the band's mux, muy.
//   general form (stars; a galaxy whose pair decomposition is not sound on every lane): per component and photon
//       d = (X - ux, Y - uy), pd = Prec d, e = exp(-1/2 d.pd), g = A e;  u += g;  m += g pd;
//       galaxy: w += 1/2 var g (pd pd^T - Prec), th += B e                    (pgrad_rows' terms)
//   rotated form (galaxies): the basis of nz_trip_gal (k_patch_ll.h), M_k^T W M_k = I, M_k^T P_k M_k = diag(l1, l2).  With
//       a = M_k^T (x - centre_k), s_i = 1 / (v_j + l_i), t_i = a_i s_i:  pd = M_k t and Prec = M_k diag(s) M_k^T, so
//       e = exp(-1/2 (a1 t1 + a2 t2)), g = A e;  u += g;  th += B e;  T += g t;
//       X11 += 1/2 v g (t1^2 - s1),  X12 += 1/2 v g t1 t2,  X22 += 1/2 v g (t2^2 - s2)
//     per component, and ONCE per (PSF component, photon):  m += M_k T,  w += M_k X M_k^T  (nine products of M_k's entries, from
//     the table).  a1, a2 are formed once per (PSF component, photon) as well.
// A lane takes PGNZ_TRIP / 64 photons per trip, so a component's constants are read from LDS once for all of them (the value
// kernel found the reads, not the arithmetic, to bind with one photon per lane).
#pragma once
#include "k_patch_grad.h"
#include "k_patch_ll.h"

#define PGNZ_TRIP 128              // photons per trip: two per lane
#define PGNZ_DEAL_PHOTONS 512      // a list LONGER than this is dealt to PGRAD_PARTS parts, trip t -> part t mod PGRAD_PARTS

// per component (8 doubles apart):   general A B ux uy qa qb qc hv     rotated  s1 s2 gs1 gs2 A B hv -
//   (qa qb qc, gs1 gs2: times -1/2 * 256 / ln 2 where they feed the exponent; hv = var / 2)
// per PSF component (16 doubles apart, rotated form): a1 = k[0] + k[1] X + k[2] Y, a2 = k[3] + k[4] X + k[5] Y;
//   k[6..8]: w00's weights of X11 X12 X22, k[9..11]: w01's, k[12..14]: w11's
#define PGNZ_LOAD(P, L, n, i0, lane, px, py, X, Y, z)                                  \
    _Pragma("unroll") for (int p = 0; p < P; p++) {                                    \
        const int i = (i0) + 64 * p + (lane);                                          \
        const NzEntry en = (L)[min(i, (n) - 1)];                                       \
        X[p] = (double)(en.xy & 0xffff) - (px);                                        \
        Y[p] = (double)((unsigned)en.xy >> 16) - (py);                                 \
        z[p] = (i < (n)) ? (double)en.z : 0.0;                                         \
    }

template <int P, bool GAL>
__device__ __forceinline__ void pgnz_trip_quad(const NzEntry *__restrict__ L, int n, int i0, int lane, int K,
                                               const double *__restrict__ tc, const double *__restrict__ et,
                                               double px, double py, double counts, double acc[7]) {
    double X[P], Y[P], z[P], u[P], m0[P], m1[P], w00[P], w01[P], w11[P], th[P];
    PGNZ_LOAD(P, L, n, i0, lane, px, py, X, Y, z)
#pragma unroll
    for (int p = 0; p < P; p++) u[p] = m0[p] = m1[p] = w00[p] = w01[p] = w11[p] = th[p] = 0.0;
#pragma nounroll
    for (int k = 0; k < K; k++) {
        asm volatile("" ::: "memory");
        const double *c = tc + 8 * k;
        const double A = c[0], B = c[1], ux = c[2], uy = c[3], qa = c[4], qb = c[5], qc = c[6], hv = c[7];
#pragma unroll
        for (int p = 0; p < P; p++) {
            const double dx = X[p] - ux, dy = Y[p] - uy;
            const double pdx = fma(qa, dx, qb * dy), pdy = fma(qb, dx, qc * dy);
            const double e = exp_tab256_p3((-0.5 * EXP_SCALE256) * fma(dx, pdx, dy * pdy), et);
            const double g = A * e;
            u[p] += g;
            m0[p] = fma(g, pdx, m0[p]);
            m1[p] = fma(g, pdy, m1[p]);
            if (GAL) {
                const double hg = hv * g;
                w00[p] = fma(hg, fma(pdx, pdx, -qa), w00[p]);
                w01[p] = fma(hg, fma(pdx, pdy, -qb), w01[p]);
                w11[p] = fma(hg, fma(pdy, pdy, -qc), w11[p]);
                th[p] = fma(B, e, th[p]);
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
        const double m = counts * u[p];
        const double r = (z[p] != 0.0 && m > 0.0) ? z[p] / m : 0.0;
        acc[0] = fma(r, u[p], acc[0]);
        acc[1] = fma(r, m0[p], acc[1]);
        acc[2] = fma(r, m1[p], acc[2]);
        if (GAL) {
            acc[3] = fma(r, w00[p], acc[3]);
            acc[4] = fma(r, w01[p], acc[4]);
            acc[5] = fma(r, w11[p], acc[5]);
            acc[6] = fma(r, th[p], acc[6]);
        }
    }
}

template <int P>
__device__ __forceinline__ void pgnz_trip_rot(const NzEntry *__restrict__ L, int n, int i0, int lane,
                                              const double *__restrict__ tk, const double *__restrict__ tc,
                                              const double *__restrict__ et, double px, double py, double counts, double acc[7]) {
    double X[P], Y[P], z[P], u[P], m0[P], m1[P], w00[P], w01[P], w11[P], th[P];
    PGNZ_LOAD(P, L, n, i0, lane, px, py, X, Y, z)
#pragma unroll
    for (int p = 0; p < P; p++) u[p] = m0[p] = m1[p] = w00[p] = w01[p] = w11[p] = th[p] = 0.0;
    // (rolled loops with their table reads inside, as in nz_trip_gal: unrolled, the table lands in registers that do not exist)
#pragma nounroll
    for (int k = 0; k < K_PSF; k++) {
        asm volatile("" ::: "memory");
        const double *g = tk + 16 * k;
        double a1[P], a2[P], r1[P], r2[P], T1[P], T2[P], X11[P], X12[P], X22[P];
        {
            const double p0 = g[0], p1 = g[1], p2 = g[2], q0 = g[3], q1 = g[4], q2 = g[5];
#pragma unroll
            for (int p = 0; p < P; p++) {
                a1[p] = fma(p1, X[p], fma(p2, Y[p], p0));
                a2[p] = fma(q1, X[p], fma(q2, Y[p], q0));
                r1[p] = a1[p] * a1[p];
                r2[p] = a2[p] * a2[p];
                T1[p] = T2[p] = X11[p] = X12[p] = X22[p] = 0.0;
            }
        }
#pragma nounroll
        for (int j = 0; j < K_PROF; j++) {
            asm volatile("" ::: "memory");
            const double *c = tc + 8 * (k * K_PROF + j);
            const double s1 = c[0], s2 = c[1], gs1 = c[2], gs2 = c[3], A = c[4], B = c[5], hv = c[6];
#pragma unroll
            for (int p = 0; p < P; p++) {
                const double e = exp_tab256_p3(fma(gs1, r1[p], gs2 * r2[p]), et);
                const double gg = A * e;
                const double t1 = a1[p] * s1, t2 = a2[p] * s2;
                const double hg = hv * gg;
                u[p] += gg;
                th[p] = fma(B, e, th[p]);
                T1[p] = fma(gg, t1, T1[p]);
                T2[p] = fma(gg, t2, T2[p]);
                X11[p] = fma(hg, fma(t1, t1, -s1), X11[p]);
                X12[p] = fma(hg, t1 * t2, X12[p]);
                X22[p] = fma(hg, fma(t2, t2, -s2), X22[p]);
            }
        }
        // back to (m0, m1) and (w00, w01, w11): M_k = [[p1, q1], [p2, q2]]
        {
            const double p1 = g[1], p2 = g[2], q1 = g[4], q2 = g[5];
#pragma unroll
            for (int p = 0; p < P; p++) {
                m0[p] += fma(p1, T1[p], q1 * T2[p]);
                m1[p] += fma(p2, T1[p], q2 * T2[p]);
            }
            const double c0 = g[6], c1 = g[7], c2 = g[8];
#pragma unroll
            for (int p = 0; p < P; p++) w00[p] += fma(c0, X11[p], fma(c1, X12[p], c2 * X22[p]));
            const double d0 = g[9], d1 = g[10], d2 = g[11];
#pragma unroll
            for (int p = 0; p < P; p++) w01[p] += fma(d0, X11[p], fma(d1, X12[p], d2 * X22[p]));
            const double e0 = g[12], e1 = g[13], e2 = g[14];
#pragma unroll
            for (int p = 0; p < P; p++) w11[p] += fma(e0, X11[p], fma(e1, X12[p], e2 * X22[p]));
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
        const double m = counts * u[p];
        const double r = (z[p] != 0.0 && m > 0.0) ? z[p] / m : 0.0;
        acc[0] = fma(r, u[p], acc[0]);
        acc[1] = fma(r, m0[p], acc[1]);
        acc[2] = fma(r, m1[p], acc[2]);
        acc[3] = fma(r, w00[p], acc[3]);
        acc[4] = fma(r, w01[p], acc[4]);
        acc[5] = fma(r, w11[p], acc[5]);
        acc[6] = fma(r, th[p], acc[6]);
    }
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
pgrad_nz_sums(const BandDev *__restrict__ bands, int B, int64_t P, const SrcRec *__restrict__ recs,
              const int *__restrict__ owner /* P, or nullptr = 0 */, const int4 *__restrict__ pbox /* NB*B: x0, x1, y0, y1 */,
              const int64_t *__restrict__ nzoff /* NB*B+1 */, const NzEntry *__restrict__ nzlist,
              double *__restrict__ sums /* P*B*PGRAD_PARTS*GRAD_NS */) {
    __shared__ double et[256];                 // 2^(j/256) (exp_tab256_p3)
    __shared__ double tc[8 * K_GAL];
    __shared__ double tk[16 * K_PSF];
    const int lane = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)PGRAD_PARTS);
    const int64_t job = (int64_t)(blockIdx.x / (unsigned)PGRAD_PARTS);
    const int b = (int)(job % B);
    const int64_t p = job / B;
    double *out = sums + (job * PGRAD_PARTS + part) * GRAD_NS;
    const int own = owner ? owner[p] : 0;
    int n = 0;
    const NzEntry *L = nzlist;
    if (own >= 0) {
        const int64_t ob = (int64_t)own * B + b;
        const int4 bx = pbox[ob];
        if (bx.y - bx.x > 0 && bx.w - bx.z > 0) {
            const int64_t o0 = nzoff[ob];
            n = (int)(nzoff[ob + 1] - o0);
            L += o0;
        }
    }
    const bool dealt = n > PGNZ_DEAL_PHOTONS;
    // the part's trips, from the list's length alone: none for parts 1.. of a list taken whole, or behind a dealt list's last trip
    const int ntrip = (n + PGNZ_TRIP - 1) / PGNZ_TRIP;
    const bool idle = n <= 0 || (dealt ? part >= ntrip : part != 0);
    RecU rec{};
    if (!idle) rec = rec_unpack(rec_fetch(recs + (int64_t)b * P, (int)p, lane));
    if (idle || rec.type == -3) {
        if (lane < GRAD_NS) out[lane] = 0.0;
        return;
    }
    const bool gal = (rec.type == 1 || rec.type == -2);  // -1 renders as a star, -2 as a galaxy, on the imposed limits
    const int K = gal ? K_GAL : K_PSF;
    const BandDev *bd = bands + b;
    exp_tab256_fill(et, lane, exp2((double)lane * (1.0 / 64.0)));
    bool rot_ok = true;
    double row[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // this lane's component, general form
    double rr[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // ... rotated form
    double rk[16];
#pragma unroll
    for (int i = 0; i < 16; i++) rk[i] = 0.0;
    if (lane < K) {
        // grad_tab_fill's quantities (k_grad_common.h: A = theta_k A' with the theta factor kept apart, B = d A / d theta), kept as
        // this kernel's own copy: reciprocals by Newton steps, centres seen from the source, the record in registers
        const int kk = gal ? lane / K_PROF : lane;
        double cxx = bd->cxx[kk], cxy = bd->cxy[kk], cyy = bd->cyy[kk], wt = bd->w[kk];
        const double ux = bd->mux[kk], uy = bd->muy[kk];           // the component's centre seen from the source
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
        double inv, rsq;
        rcp_rsqrt(det, inv, rsq);
        const double a1 = wt * (0.5 / PI_D) * rsq;
        row[0] = tf * a1; row[1] = sg * a1; row[2] = ux; row[3] = uy;
        row[4] = cyy * inv; row[5] = -cxy * inv; row[6] = cxx * inv; row[7] = 0.5 * var;
        if (gal) {
            // the pair (W, P_k) diagonalised, as k_patch_ll_nz does it: W = L L^T, C = L^-1 P_k L^-T, one Jacobi rotation of C
            const double pxx = bd->cxx[kk], pxy = bd->cxy[kk], pyy = bd->cyy[kk];
            const double ia = rsqrt64(rec.w00), l21 = rec.w01 * ia, d22 = rec.w11 - l21 * l21;
            const double ic = rsqrt64(d22), ib = -l21 * ia * ic;
            const double C11 = ia * ia * pxx, C12 = ia * (ib * pxx + ic * pxy);
            const double C22 = ib * ib * pxx + 2.0 * ib * ic * pxy + ic * ic * pyy;
            double cs = 1.0, sn = 0.0, lam1 = C11, lam2 = C22;
            if (C12 != 0.0) {
                const double tau = (C22 - C11) / (2.0 * C12);
                const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                cs = rsqrt64(1.0 + t * t); sn = t * cs;
                lam1 = C11 - t * C12; lam2 = C22 + t * C12;
            }
            const double d1 = var + lam1, d2 = var + lam2;
            const double s1 = rcp64(d1), s2 = rcp64(d2);
            const double al1 = cs * ia - sn * ib, be1 = -sn * ic, al2 = sn * ia + cs * ib, be2 = cs * ic;
            const double g0 = -(al1 * ux + be1 * uy), g3 = -(al2 * ux + be2 * uy);
            rr[0] = s1; rr[1] = s2; rr[2] = (-0.5 * EXP_SCALE256) * s1; rr[3] = (-0.5 * EXP_SCALE256) * s2;
            rr[4] = row[0]; rr[5] = row[1]; rr[6] = 0.5 * var;
            rk[0] = g0; rk[1] = al1; rk[2] = be1; rk[3] = g3; rk[4] = al2; rk[5] = be2;
            rk[6] = al1 * al1; rk[7] = 2.0 * al1 * al2; rk[8] = al2 * al2;
            rk[9] = al1 * be1; rk[10] = al1 * be2 + al2 * be1; rk[11] = al2 * be2;
            rk[12] = be1 * be1; rk[13] = 2.0 * be1 * be2; rk[14] = be2 * be2;
            rot_ok = (rec.w00 > 0.0) && (d22 > 0.0) && (d1 > 0.0) && (d2 > 0.0) && (s1 == s1) && (s2 == s2) && (fabs(s1) < 1e300) &&
                     (fabs(s2) < 1e300) && (g0 == g0) && (g3 == g3) && (fabs(g0) < 1e300) && (fabs(g3) < 1e300);
        }
    }
    // a galaxy whose decomposition is sound on every lane takes the rotated form; any other the general quadratic form
    const bool rot = gal && (__ballot(lane < K && !rot_ok) == 0ull);
    if (lane < K) {
#pragma unroll
        for (int i = 0; i < 8; i++) tc[8 * lane + i] = rot ? rr[i] : row[i];
        if (rot && lane % K_PROF == 0) {
#pragma unroll
            for (int i = 0; i < 16; i++) tk[16 * (lane / K_PROF) + i] = rk[i];
        }
    }
    __syncthreads();
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double counts = rec.scale;
    int t = 0;
    for (int i0 = 0; i0 < n; i0 += PGNZ_TRIP, t++) {
        if (dealt && (t % PGRAD_PARTS) != part) continue;
        const bool two = (n - i0) > 64;
        if (rot) {
            if (two) pgnz_trip_rot<2>(L, n, i0, lane, tk, tc, et, rec.px, rec.py, counts, acc);
            else pgnz_trip_rot<1>(L, n, i0, lane, tk, tc, et, rec.px, rec.py, counts, acc);
        } else if (gal) {
            if (two) pgnz_trip_quad<2, true>(L, n, i0, lane, K, tc, et, rec.px, rec.py, counts, acc);
            else pgnz_trip_quad<1, true>(L, n, i0, lane, K, tc, et, rec.px, rec.py, counts, acc);
        } else {
            if (two) pgnz_trip_quad<2, false>(L, n, i0, lane, K, tc, et, rec.px, rec.py, counts, acc);
            else pgnz_trip_quad<1, false>(L, n, i0, lane, K, tc, et, rec.px, rec.py, counts, acc);
        }
    }
    grad_store_sums(acc, lane, out);
}
