// spmv_mv_device.hpp -- the body of the column-major multi-vector kernels: csx_spmv_mv_kernel and its kin
// (spmv_mv_kernels.hip, values read as doubles) and their float forms (spmv_mv_f32_kernels.hip, values read
// from the float twin, spx.gpu.values_f32).  A header so that the two sets of instances are translation units
// of their own.
#pragma once

#include "spmv_device.hpp"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// One workgroup owns one row-block: LDS holds COPIES x K y tiles (copy c, vector j at
// (c * K + j) * n_rows), then the K x windows where they are staged.
// ACCUM (SPX_RB_ACCUM): the tiles are added to Y with global atomics on top of csx_scale_kernel.
// V: the type of the stream's values (float: a.values points at the float twin).  Vectors, windows, tiles,
// products and sums are fp64 whatever V is; the diagonal has no twin and is rounded to V in registers, so that
// the product is that of the matrix whose every stored entry is rounded (spmv_body does the same).
template <int K, int WAVES, bool ACCUM, bool DET, class V = double>
__device__ __forceinline__ void mv_body(const MvArgs &a, const XcdSplit &xs, double *lds)
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
        const int xw = rb.xwin_len;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xs_j = a.x + (size_t) j * a.ldx + rb.xwin_base;
            for (int i = threadIdx.x; i < xw; i += BLOCK_THREADS) win[j * xw + i] = xs_j[i];
        }
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

    // ---------------- write the owned rows of every vector ------------------------------------
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x < K) a.carry[(size_t) threadIdx.x * a.n_carry + rb.carry_slot] = tile[threadIdx.x * n_rows];
    } else if (ACCUM) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) j * a.ldy + rb.row0 + i], a.alpha * tile[j * n_rows + i]);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xj = a.x + (size_t) j * a.ldx;
            double *yj = a.y + (size_t) j * a.ldy;
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) {
                const size_t g = (size_t) rb.row0 + i;
                double t = tile[j * n_rows + i];
                if (a.dvalues) t += stored_as<V>(a.dvalues[g]) * xj[g];
                t *= a.alpha;
                if (a.beta != 0.0) t += a.beta * yj[g];
                yj[g] = t;
            }
        }
    }
}

}  // namespace spx
