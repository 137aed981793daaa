// k_comps.h -- the component cache: what a (band, source) record's components are on EVERY tile, built once per record generation
//
// The general render sets a galaxy record up on every tile its box touches (8.2 tiles at the benchmark field), and a part of
// that set-up depends on nothing but the record and the band's PSF table: the 42 covariances, their determinants, the Newton
// reciprocal and reciprocal square root, the inverse covariance, the amplitude, the mean, the row-to-row ratio exp(-qc) and
// log |A| for the drop threshold.  k_comps runs exactly that arithmetic -- the same functions on the same exp2(lane / 64)
// table -- once per record, one wave per record, lane k = component k, and stores the results; k_render_hwc (k_render_hw.h)
// loads them where the plain kernel computes them.  Nothing that depends on the sky level, the drop threshold, the tile or
// the kernel choice is in a row.  Who vouches for the rows: RecordStamps::comps_of_records (field_state.h).
//
// Layout.  One row per (band, source) record, record n = b * S + s, COMP_ROW doubles each: seven fields of K_GAL doubles,
// struct-of-arrays (lane k's load of one field is 8 bytes beside lane k + 1's: 336 contiguous bytes per field), then K_GAL
// floats.  2 520 bytes per record -- B * S rows: 134 MB at the benchmark field; a star's row holds its three PSF components
// and zeros behind them (a star that the star pass refuses reaches the general path with the bits it has today).
#pragma once
#include "k_render.h"

#define COMP_F64 7                                        // A, mx, my, qa, qb, qc, eq
#define COMP_ROW (COMP_F64 * K_GAL + K_GAL / 2)           // doubles per row: the floats take K_GAL / 2 of them
static_assert(K_GAL % 2 == 0, "a row's floats fill whole doubles");

struct CompRow {      // lane k's share of a row
    double A, mx, my, qa, qb, qc;     // as make_comp_lc leaves them (qa, qb, qc WITHOUT the factor EXP_SCALE: the drop test reads them)
    double eq;                        // comp_eq(qc)
    float logA;                       // comp_log_amp(A)
};

// the two pieces of the set-up that follow make_comp_lc, written once: the render's plain path and k_comps call the same
// expressions (the compiler contracts t - rint(t) inside exp_tab64 into one fma with the product -qc * EXP_SCALE, in both)
__device__ __forceinline__ double comp_eq(double qc, const double *__restrict__ et) { return exp_tab64(-qc * EXP_SCALE, et); }
__device__ __forceinline__ float comp_log_amp(double A) { return __logf((float)fabs(A)); }

__device__ __forceinline__ CompRow comp_row_load(const double *__restrict__ row, int lane) {
    CompRow r;
    r.A = row[lane]; r.mx = row[K_GAL + lane]; r.my = row[2 * K_GAL + lane];
    r.qa = row[3 * K_GAL + lane]; r.qb = row[4 * K_GAL + lane]; r.qc = row[5 * K_GAL + lane];
    r.eq = row[6 * K_GAL + lane];
    r.logA = reinterpret_cast<const float *>(row + COMP_F64 * K_GAL)[lane];
    return r;
}

#define COMPS_WAVES 4
// n_rec = B * S records (recs[b * S + s], as k_prep stores them); comps: n_rec rows
__global__ void __launch_bounds__(64 * COMPS_WAVES)
k_comps(const BandDev *__restrict__ bands, const SrcRec *__restrict__ recs, int64_t S, int64_t n_rec, double *__restrict__ comps) {
    __shared__ double et[64];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) et[lane] = exp2((double)lane * (1.0 / 64.0));
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * COMPS_WAVES + (threadIdx.x >> 6);
    if (n >= n_rec) return;
    const BandDev *bd = bands + n / S;
    const LaneConst lc = lane_consts(lane, bd);
    const RecU rec = rec_unpack(reinterpret_cast<const int *>(recs + n)[lane & 31]);
    const int K = (rec.type == 0) ? K_PSF : K_GAL;
    if (lane >= K_GAL) return;
    CompRow r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.f};
    if (lane < K) {
        const Comp c = make_comp_lc(lc, rec);
        r.A = c.A; r.mx = c.mx; r.my = c.my; r.qa = c.qa; r.qb = c.qb; r.qc = c.qc;
        r.eq = comp_eq(c.qc, et);
        r.logA = comp_log_amp(c.A);
    }
    double *row = comps + n * COMP_ROW;
    row[lane] = r.A; row[K_GAL + lane] = r.mx; row[2 * K_GAL + lane] = r.my;
    row[3 * K_GAL + lane] = r.qa; row[4 * K_GAL + lane] = r.qb; row[5 * K_GAL + lane] = r.qc;
    row[6 * K_GAL + lane] = r.eq;
    reinterpret_cast<float *>(row + COMP_F64 * K_GAL)[lane] = r.logA;
}
