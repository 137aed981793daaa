// k_mask.h -- the Poisson term of a MASKED image set, as a pass of its own
//
// A NaN in nelec marks a pixel that was not observed (cel_images_set_nelec): it contributes to no sum.  The render kernels
// know nothing of this -- there are seven forms of them and the headline kernel's epilogue is tuned to the instruction -- so
// on a masked set render_impl renders the model image WITHOUT the fused Poisson term and this kernel then streams nelec and
// lambda once (16 B per pixel, no LDS) into one partial per render tile of the set's own tile geometry, which k_reduce adds
// in its fixed order exactly as it adds the render kernels' partials (row windows and owned rows included).
//
// One wave per tile.  A lane owns one column of the tile (64 / TW rows per wave instruction) and walks its rows in
// order, MLL_CH at a time: every load of a chunk is issued before the first use, at addresses CLAMPED into the frame so that
// none of them stands under a condition (the compiler then counts what is outstanding, see hw_epilogue); whether a pixel
// counts is decided on the loaded values.  Additions: the lane's rows in order, then wave_sum's shuffle tree -- at most
// 64 + 6 per partial, the same bits on every run.  log() is the library's, not the render's table: 1 ulp.
#pragma once

#define MLL_CH 16       // loads of each plane a lane has in flight (2 x 16 x 8 B x 64 lanes = 16 KB per wave)

__global__ void __launch_bounds__(64)
k_masked_ll(const double *__restrict__ nelec, const double *__restrict__ lambda, int H, int W, int TW, int TH, int ntx, int nty,
            double *__restrict__ partials /* B * ntx * nty */) {
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int per_band = ntx * nty;
    const int b = tile / per_band;
    const int t = tile - b * per_band;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int X0 = tx * TW, Y0 = ty * TH;
    const int rstep = 64 / TW;                              // TW is 16, 32 or 64: rows per wave instruction
    const int xi = X0 + (lane & (TW - 1)), ysub = lane / TW;
    const int nr = TH / rstep;                              // rows per lane: 32 or 64
    const int64_t col = (int64_t)b * H * W + min(xi, W - 1);
    double part = 0.0;
    for (int r0 = 0; r0 < nr && Y0 + r0 * rstep < H; r0 += MLL_CH) {     // (wave-uniform)
        double ne[MLL_CH], la[MLL_CH];
#pragma unroll
        for (int r = 0; r < MLL_CH; r++) {
            const int64_t idx = col + (int64_t)min(Y0 + (r0 + r) * rstep + ysub, H - 1) * W;
            ne[r] = nelec[idx];
            la[r] = lambda[idx];
        }
#pragma unroll
        for (int r = 0; r < MLL_CH; r++) {
            const bool in = (xi < W) && (Y0 + (r0 + r) * rstep + ysub < H);
            const double v = ne[r] * log(la[r]) - la[r];
            part += (in && ne[r] == ne[r]) ? v : 0.0;
        }
    }
    part = wave_sum(part);
    if (lane == 0) partials[tile] = part;
}
