// spmv_mvr_device.hpp -- device code of the multi-vector product on ROW-MAJOR (interleaved) blocks,
// csx_spmv_mvr_kernel (spmv_mvr_kernels.hip): the K-vector composition of the pieces of spmv_device.hpp for
// an x whose entry (column c, vector j) lies at x[c * ldx + j].  The K doubles a lane needs of column c are
// contiguous -- one or two cache lines for K = 8 where the column-major composition gathers K of them.
//
// Overloads unit_passes of spmv_device.hpp on the argument struct, so that run_units, run_pass and run_pair
// -- the pass kinds, widths and the pairing of two passes of one shape -- are the ones every interpreter
// kernel uses.
#pragma once

#include "spmv_device.hpp"
#include "spmv_launch.hpp"

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

// ---- the body of csx_spmv_mvr_kernel and its kin (spmv_mvr_kernels.hip, spmv_mvr_f32_kernels.hip) ----------------

// One workgroup owns one row-block: LDS holds COPIES x K y tiles (copy c, vector j at (c * K + j) * n_rows),
// then the x window (xwin_len x K doubles, row-major) where it is staged.
// V: the type of the stream's values (float: a.values points at the float twin, spx.gpu.values_f32); x, the
// window, the tiles, products, sums and the write-out are fp64 whatever V is.
template <int K, int WAVES, bool ACCUM, bool DET, class V = double>
__device__ __forceinline__ void mvr_body(const MvrArgs &a, const XcdSplit &xs, double *lds)
{
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    SpxPass p0 = passes[wave];
    SpxPass p1 = passes[wave + WAVES];                   // (the table is padded by one stride)
    const int n_rows = rb.n_rows;
    constexpr int COPIES = DET ? WAVES : 1;
    const int tiles = K * n_rows;                        // doubles per copy
    double *tile = lds + (DET ? wave * tiles : 0);
    for (int i = threadIdx.x; i < COPIES * tiles; i += BLOCK_THREADS) lds[i] = 0.0;
    double *win = lds + COPIES * tiles;
    if (a.stage) {
        // rows xwin_base .. xwin_base + xwin_len - 1 of X, K doubles of each: one run where ldx == K
        const int xk = (int) rb.xwin_len * K;
        const double *xw = a.x + (size_t) rb.xwin_base * a.ldx;
        for (int e = threadIdx.x; e < xk; e += BLOCK_THREADS) win[e] = xw[(size_t) (e / K) * a.ldx + (e % K)];
    }
    __syncthreads();

    // wave w takes passes w, w + WAVES, ..., two at a time when they have the same shape
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += 2 * WAVES) {
        const bool two = t + WAVES < n_pass;
        if (two) {
            if (same_shape(p0, p1)) {
                run_pair<K, V>(a, rb, {p0, p1}, tile, win, lane);
            } else {
                run_pass<K, V>(a, rb, p0, tile, win, lane);
                run_pass<K, V>(a, rb, p1, tile, win, lane);
            }
        } else {
            run_pass<K, V>(a, rb, p0, tile, win, lane);
        }
        if (t + 2 * WAVES < n_pass) {
            p0 = passes[t + 2 * WAVES];
            p1 = passes[t + 3 * WAVES];
        }
    }
    __syncthreads();
    if (DET) {
        // the wavefronts' copies, summed in wavefront order into the first one
        for (int i = threadIdx.x; i < tiles; i += BLOCK_THREADS) {
            double t = lds[i];
#pragma unroll
            for (int w = 1; w < COPIES; ++w) t += lds[w * tiles + i];
            lds[i] = t;
        }
        __syncthreads();
        tile = lds;
    }

    // ---- write the owned rows: entry e of the row-block's n_rows x K piece of Y, in memory order ----------
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x < K) a.carry[(size_t) threadIdx.x * a.n_carry + rb.carry_slot] = tile[threadIdx.x * n_rows];
    } else if (ACCUM) {
        for (int e = threadIdx.x; e < tiles; e += BLOCK_THREADS) {
            const int i = e / K, j = e % K;
            atomicAdd(&a.y[((size_t) rb.row0 + i) * a.ldy + j], a.alpha * tile[j * n_rows + i]);
        }
    } else {
        for (int e = threadIdx.x; e < tiles; e += BLOCK_THREADS) {
            const int i = e / K, j = e % K;
            double *yp = a.y + ((size_t) rb.row0 + i) * a.ldy + j;
            double t = tile[j * n_rows + i];
            t *= a.alpha;
            if (a.beta != 0.0) t += a.beta * *yp;
            *yp = t;
        }
    }
}

}  // namespace spx
