// k_moments.h -- the zeroth, first and second moments of every source's photons in the resident split (cel_slice_sample, param = CEL_SLICE_MOMENTS)
//
// Definition.  Per (source s, band b) job i = s B + b, with z the photons the split gave s at a pixel of its patch and
// dx = x - x0, dy = y - y0 counted from the low corner of the patch's box (d_sbox; the box cel_samples_fetch reports):
//     mom[6 i ..] = N, Sx, Sy, Sxx, Sxy, Syy = sum z, sum z dx, sum z dy, sum z dx dx, sum z dx dy, sum z dy dy
// in int64.  Integer sums: EXACT and independent of the order, of the route and of the dealing while they fit (the range: the
// header).  A job without a patch leaves its row as the host zeroed it.
//
// Two routes, the same integers.  A patch whose photon list stands and is selected (k_nz_layout's mode, the rule the conditional
// likelihoods follow; `nzmode` == nullptr: no lists) is summed over its list entries (x | y << 16, z): 8 bytes per photon.
// Every other patch is summed over its dense int32 pixels: 4 bytes per pixel, most of them zero.
//
// One wave per (job, part).  A job whose box holds at most MOM_SPLIT_PIXELS pixels is taken whole by part 0, which stores its
// row; a larger one is dealt to MOM_PARTS blocks -- contiguous shares of the rows (dense) or of the list -- that add their
// sums into the zeroed row with 64-bit integer atomics (global_atomic_add_x2).  The rule reads the box alone, so both routes
// deal the same jobs; integer addition makes the deal invisible.  (The threshold: a 64 x 64 patch is 16 KB, 64 loads per lane
// with MOM_FLIGHT of them in flight -- one wave's latency chain of eight round trips, and a catalogue has thousands of such
// jobs to fill the device with; a 256 x 256 patch of a bright galaxy would be a chain of 128 on one wave while the launch
// waits for it, and is 32 on each of four.)
//
// Dense route: the lanes are laid over `rp` whole rows of `cw` columns (cw = the power of two that holds the row, 64 at the
// most; rp = 64 / cw), so lane -> (row, column) is a shift and a mask once per wave, and the walk adds rp to the row: no lane
// divides per pixel.  A row of more than 64 columns is walked in chunks of 64.  MOM_FLIGHT row steps are loaded together
// (unconditional loads at clamped addresses, k_nz_compact's way) and summed afterwards.  A 1-pixel-wide patch takes 64 rows a
// step; consecutive rows are contiguous in memory, so a step's loads are one segment whatever the width.
//
// Arithmetic: z is an int32 and dx, dy < 2^12, so dx dx, dx dy, dy dy fit an int32 and each term is one v_mad_i64_i32 into the
// lane's int64 partial sum: five of them and an add per pixel, against a 4-byte load -- bandwidth-bound at every fill.
// The wave closes with the shuffle tree of wave_sum.  No LDS, no scratch.
#pragma once
#include "k_render.h"

#define MOM_PARTS 4
#define MOM_SPLIT_PIXELS CEL_MOMENTS_SPLIT_PIXELS   // a box of MORE pixels than this is dealt to MOM_PARTS blocks (celeste_hip.h)
#define MOM_FLIGHT 8             // row steps (dense) or list entries (lists) a lane has in flight

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__device__ __forceinline__ void mom_add(long long acc[6], int z, int dx, int dy) {
    acc[0] += z;
    acc[1] += (long long)z * dx;
    acc[2] += (long long)z * dy;
    acc[3] += (long long)z * (dx * dx);
    acc[4] += (long long)z * (dx * dy);
    acc[5] += (long long)z * (dy * dy);
}

__global__ void __launch_bounds__(64)
k_moments(int64_t n /* S*B jobs */, const int4 *__restrict__ sbox /* x0, x1, y0, y1 */, const int64_t *__restrict__ soff,
          const int *__restrict__ samp, const int *__restrict__ nzmode /* nullptr: every job densely */,
          const int64_t *__restrict__ nzoff, const NzEntry *__restrict__ list, long long *__restrict__ mom /* n * 6, zeroed */) {
    const int64_t i = (int64_t)blockIdx.x / MOM_PARTS;
    const int part = (int)(blockIdx.x - i * MOM_PARTS);
    if (i >= n) return;
    const int4 bx = sbox[i];
    const int nx = bx.y - bx.x, ny = bx.w - bx.z;
    if (nx <= 0 || ny <= 0) return;
    const bool dealt = (int64_t)nx * ny > MOM_SPLIT_PIXELS;
    if (!dealt && part != 0) return;
    const int lane = threadIdx.x;
    long long acc[6] = {0, 0, 0, 0, 0, 0};
    if (nzmode && nzmode[i]) {
        const int64_t l0 = nzoff[i], cnt = nzoff[i + 1] - l0;
        // a dealt list: part p takes entries [p cnt / MOM_PARTS, (p + 1) cnt / MOM_PARTS)
        const int64_t lo = dealt ? (cnt * part) / MOM_PARTS : 0, hi = dealt ? (cnt * (part + 1)) / MOM_PARTS : cnt;
        const NzEntry *L = list + l0;
        for (int64_t k0 = lo; k0 < hi; k0 += 64 * MOM_FLIGHT) {
            NzEntry en[MOM_FLIGHT];
#pragma unroll
            for (int j = 0; j < MOM_FLIGHT; j++) en[j] = L[min(k0 + 64 * j + lane, hi - 1)];
#pragma unroll
            for (int j = 0; j < MOM_FLIGHT; j++) {
                const int z = (k0 + 64 * j + lane < hi) ? en[j].z : 0;
                mom_add(acc, z, (en[j].xy & 0xffff) - bx.x, (int)((unsigned)en[j].xy >> 16) - bx.z);
            }
        }
    } else {
        // a dealt patch: part p takes rows [p ny / MOM_PARTS, (p + 1) ny / MOM_PARTS)
        const int r0 = dealt ? (int)(((int64_t)ny * part) / MOM_PARTS) : 0, r1 = dealt ? (int)(((int64_t)ny * (part + 1)) / MOM_PARTS) : ny;
        if (r1 > r0) {
            int sh = 6;                                            // cw = 1 << sh: the smallest power of two >= nx, at most 64
            while (sh > 0 && (1 << (sh - 1)) >= nx) sh--;
            const int cw = 1 << sh, rp = 64 >> sh;
            const int sub = lane >> sh, cl = lane & (cw - 1);
            const int *p = samp + soff[i];
            for (int xc = 0; xc < nx; xc += cw) {                   // (one trip unless the row has more than 64 columns)
                const int x = xc + cl;
                const int xq = min(x, nx - 1);
                for (int y0 = r0 + sub; y0 - sub < r1; y0 += rp * MOM_FLIGHT) {
                    int z[MOM_FLIGHT];
#pragma unroll
                    for (int j = 0; j < MOM_FLIGHT; j++) z[j] = p[(int64_t)min(y0 + j * rp, r1 - 1) * nx + xq];
#pragma unroll
                    for (int j = 0; j < MOM_FLIGHT; j++) {
                        const int y = y0 + j * rp;
                        mom_add(acc, (x < nx && y < r1) ? z[j] : 0, x, y);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = wave_sum_i64(acc[k]);
    if (lane == 0) {
        long long *out = mom + 6 * i;
        if (dealt) {
#pragma unroll
            for (int k = 0; k < 6; k++) atomicAdd((unsigned long long *)out + k, (unsigned long long)acc[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 6; k++) out[k] = acc[k];
        }
    }
}
