// spmv_mv_device.hpp -- the body of the multi-vector kernels that own one row-block per workgroup, for both
// layouts of X and Y and both value types: csx_spmv_mv_kernel (spmv_mv_instances.hpp) as instantiated by
// spmv_mv_kernels.hip and spmv_mv_f32_kernels.hip (column-major blocks, MvArgs) and by spmv_mvr_kernels.hip and
// spmv_mvr_f32_kernels.hip (row-major blocks, MvrArgs).  Here: the body and the two pieces of it that depend on
// the layout -- staging the x window and writing the owned rows -- for MvArgs; spmv_mvr_device.hpp overloads the
// two for MvrArgs, as it overloads unit_passes.
#pragma once

#include "spmv_device.hpp"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// column-major x: the K windows of xwin_len doubles, vector j's at win + j * xwin_len
template <int K, int BLOCK_THREADS>
__device__ __forceinline__ void stage_xwin(const MvArgs &a, const SpxRowBlock &rb, double *win)
{
    const int xw = rb.xwin_len;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double *xs_j = a.x + (size_t) j * a.ldx + rb.xwin_base;
        for (int i = threadIdx.x; i < xw; i += BLOCK_THREADS) win[j * xw + i] = xs_j[i];
    }
}

// column-major y: the owned rows vector by vector, coalesced; ACCUM: added with global atomics on top of
// csx_scale_kernel, else stored with the diagonal term (symmetric, fused) and beta * y.  The diagonal has no float
// twin and is rounded to V in registers, so that the product is that of the matrix whose every stored entry is
// rounded (spmv_body does the same).
// (row0 and n_rows as values, not the row-block's header by reference: with the header the row-major accum K = 8
// instances came out with two instructions of the write-out in another order -- profiles/r17/REFACTOR.md)
template <int K, int BLOCK_THREADS, bool ACCUM, class V>
__device__ __forceinline__ void write_rows(const MvArgs &a, uint32_t row0, int n_rows, const double *tile)
{
    if (ACCUM) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) j * a.ldy + row0 + i], a.alpha * tile[j * n_rows + i]);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xj = a.x + (size_t) j * a.ldx;
            double *yj = a.y + (size_t) j * a.ldy;
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) {
                const size_t g = (size_t) row0 + i;
                double t = tile[j * n_rows + i];
                if (a.dvalues) t += stored_as<V>(a.dvalues[g]) * xj[g];
                t *= a.alpha;
                if (a.beta != 0.0) t += a.beta * yj[g];
                yj[g] = t;
            }
        }
    }
}

// One workgroup owns one row-block: LDS holds COPIES x K y tiles (copy c, vector j at
// (c * K + j) * n_rows), then the x window(s) where they are staged (Args::stage; layout: stage_xwin).
// ACCUM (SPX_RB_ACCUM): the tiles are added to Y with global atomics on top of the scale kernel.
// DET: a copy of the tiles per wavefront, summed in wavefront order.
// V: the type of the stream's values (float: a.values points at the float twin, spx.gpu.values_f32).  Vectors,
// windows, tiles, products, sums and the write-out are fp64 whatever V is.
// Args: MvArgs or MvrArgs; it picks the composition of the passes (unit_passes, through run_pass and run_pair),
// stage_xwin and write_rows.
template <int K, int WAVES, bool ACCUM, bool DET, class V, class Args>
__device__ __forceinline__ void mv_body(const Args &a, const XcdSplit &xs, double *lds)
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
    if (a.stage) stage_xwin<K, BLOCK_THREADS>(a, rb, win);
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

    // a row split over several row-blocks leaves its K partials in the carry slot, else the owned rows go to Y
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x < K) a.carry[(size_t) threadIdx.x * a.n_carry + rb.carry_slot] = tile[threadIdx.x * n_rows];
    } else {
        write_rows<K, BLOCK_THREADS, ACCUM, V>(a, rb.row0, n_rows, tile);
    }
}

}  // namespace spx
