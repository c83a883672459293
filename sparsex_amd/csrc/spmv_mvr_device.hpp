// spmv_mvr_device.hpp -- device code of the multi-vector product on ROW-MAJOR (interleaved) blocks,
// csx_spmv_mv_kernel<MvrArgs, ...> (spmv_mvr_kernels.hip, spmv_mvr_f32_kernels.hip): the K-vector composition of
// the pieces of spmv_device.hpp for an x whose entry (column c, vector j) lies at x[c * ldx + j].  The K doubles a
// lane needs of column c are contiguous -- one or two cache lines for K = 8 where the column-major composition
// gathers K of them.
//
// Overloads unit_passes of spmv_device.hpp on the argument struct, so that run_units, run_pass and run_pair
// -- the pass kinds, widths and the pairing of two passes of one shape -- are the ones every interpreter
// kernel uses; and stage_xwin and write_rows of spmv_mv_device.hpp, so that the body around them, mv_body, is the
// column-major kernels'.
#pragma once

#include "spmv_mv_device.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// the K doubles of one column (row-major x: K consecutive doubles at xp).  `x16`: xp is 16-byte aligned
// (MvrArgs::x16: the group's first element and ldx * 8 both are), so that they come two per load.
template <int K>
__device__ __forceinline__ void load_xk(const double *xp, bool x16, double (&x)[K])
{
    if (K >= 2 && x16) {
        const double2 *xp2 = reinterpret_cast<const double2 *>(xp);
#pragma unroll
        for (int p = 0; p < K / 2; ++p) {
            const double2 xx = xp2[p];
            x[2 * p] = xx.x;
            x[2 * p + 1] = xx.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) x[j] = xp[j];
    }
}

// ... from the staged window (LDS; entry (i, j) at win[i * K + j], behind K * copies * n_rows doubles: 16-byte
// aligned for every even K)
template <int K>
__device__ __forceinline__ void load_xk_lds(const double *wp, double (&x)[K])
{
    if (K >= 2) {
        const double2 *wp2 = reinterpret_cast<const double2 *>(wp);
#pragma unroll
        for (int p = 0; p < K / 2; ++p) {
            const double2 xx = wp2[p];
            x[2 * p] = xx.x;
            x[2 * p + 1] = xx.y;
        }
    } else {
        x[0] = wp[0];
    }
}

// value w of the lane's W (PassValues keeps them as they were loaded: pairs, an odd last one alone)
template <int W, class V>
__device__ __forceinline__ double pass_value(const PassValues<W, V> &v, int w)
{
    if ((W & 1) && w == W - 1) return (double) v.v1;
    return (double) ((w & 1) ? v.v2[w / 2].y : v.v2[w / 2].x);
}

// K vectors, row-major: index and values once; then column by column of the lane's W the K doubles of that
// column and K fused multiply-adds into K accumulators -- for every vector the chain of dot() in column order,
// which is what makes a column bit-identical to the single-vector product where the tiles are kept per
// wavefront --; then per vector the add to ITS y tile (vector j at tile + j * n_rows: consecutive rows of one
// vector in consecutive LDS banks, as in the column-major kernels; the write-out transposes).  `win`: the
// staged x window, xwin_len x K doubles, where MvrArgs::stage says so.
template <int W, int B, int G, int K, class V = double>
__device__ __forceinline__ void unit_passes(const MvrArgs &a, const SpxRowBlock &rb, const SpxPass (&ps)[B],
                                            double *tile, const double *win, int lane)
{
    bool active[B];
    uint32_t l[B];
    uint2 q[B];
    uint32_t goff[B][G ? W : 1];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        active[b] = (uint32_t) lane < (uint32_t) ps[b].nseg;
        l[b] = active[b] ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0
        SPX_LOAD_INDEX(W, G, a, rb, ps[b], active[b], l[b], lane, q[b], goff[b]);
    }
    PassValues<W, V> v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) v[b] = load_values<W, V>(a, rb, ps[b], l[b]);
    const bool staged = G == 2 && a.stage;
    const int n_rows = rb.n_rows;
    int row[B];
    double acc[B][K];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        int len;
        uint32_t col;
        if (G) {
            row[b] = (int) SPX_SEGROW_ROW(q[b].x);
            len = (int) SPX_SEGROW_LEN(q[b].x);
            col = G == 2 ? rb.xwin_base : rb.cbase;
        } else {
            const UnitOrigin o = unit_origin(q[b].y, ps[b].seg0 + l[b], ps[b].elem0);
            row[b] = o.row;
            col = q[b].x + (uint32_t) o.dcol;
            len = W;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) acc[b][j] = 0.0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            double x[K];
            if (G && staged) load_xk_lds<K>(win + (size_t) goff[b][G ? w : 0] * K, x);
            else if (G) load_xk<K>(a.x + (size_t) (col + goff[b][G ? w : 0]) * a.ldx, a.x16 != 0, x);
            else load_xk<K>(a.x + (size_t) (col + (uint32_t) w) * a.ldx, a.x16 != 0, x);
            const double vw = pass_value<W, V>(v[b], w);
            // (a piece shorter than the pass is padded: nothing is multiplied there)
#pragma unroll
            for (int j = 0; j < K; ++j) acc[b][j] = fma(vw, (!G || w < len) ? x[j] : 0.0, acc[b][j]);
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double *tj = tile + j * n_rows;
        if (G == 1 && rb.n_rows == 1) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < B; ++b) t += active[b] ? acc[b][j] : 0.0;
            wave_add(tj, t, lane);
        } else {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (active[b]) atomicAdd(&tj[row[b]], acc[b][j]);
        }
    }
}

// ---- the two layout-dependent pieces of mv_body (spmv_mv_device.hpp) for row-major blocks ----------------------

// the x window: rows xwin_base .. xwin_base + xwin_len - 1 of X, K doubles of each (entry (i, j) at win[i * K + j]):
// one run where ldx == K
template <int K, int BLOCK_THREADS>
__device__ __forceinline__ void stage_xwin(const MvrArgs &a, const SpxRowBlock &rb, double *win)
{
    const int xk = (int) rb.xwin_len * K;
    const double *xw = a.x + (size_t) rb.xwin_base * a.ldx;
    for (int e = threadIdx.x; e < xk; e += BLOCK_THREADS) win[e] = xw[(size_t) (e / K) * a.ldx + (e % K)];
}

// the owned rows: entry e of the row-block's n_rows x K piece of Y, in memory order (the tiles are vector-major:
// transposed here); no diagonal term (general streams only)
template <int K, int BLOCK_THREADS, bool ACCUM, class V>
__device__ __forceinline__ void write_rows(const MvrArgs &a, uint32_t row0, int n_rows, const double *tile)
{
    const int tiles = K * n_rows;
    if (ACCUM) {
        for (int e = threadIdx.x; e < tiles; e += BLOCK_THREADS) {
            const int i = e / K, j = e % K;
            atomicAdd(&a.y[((size_t) row0 + i) * a.ldy + j], a.alpha * tile[j * n_rows + i]);
        }
    } else {
        for (int e = threadIdx.x; e < tiles; e += BLOCK_THREADS) {
            const int i = e / K, j = e % K;
            double *yp = a.y + ((size_t) row0 + i) * a.ldy + j;
            double t = tile[j * n_rows + i];
            t *= a.alpha;
            if (a.beta != 0.0) t += a.beta * *yp;
            *yp = t;
        }
    }
}

}  // namespace spx
