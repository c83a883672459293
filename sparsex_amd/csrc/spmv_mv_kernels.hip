// spmv_mv_kernels.hip -- the multi-vector product Y <- alpha*A*X + beta*Y for gfx950: K vectors per pass
// over the stream (K = 2, 4 or 8; one vector is the single-vector kernels' business).  The host side is
// device_spmm (device_runtime.cpp).
//
// The interpreter of spmv_device.hpp with its vector-count parameter K, over the PLAIN stream (passes,
// descs): a lane loads its descriptor or its gather offsets and its W values once, then for every vector j of
// the group gathers X_j[col .. col + W - 1], multiplies with the values it holds in registers and adds one
// partial sum to the y tile of vector j in LDS.  The write-out is per vector, coalesced.  The steps around the
// row-block launches (scale, symmetric init, fix-up) are the kernels of spmv_kernels.hip with gridDim.y = K.
// X and Y are column-major blocks: vector j of X at x + j * ldx, of Y at y + j * ldy.
//
// DET (spx.gpu.deterministic, or the launch tuner's tile per wavefront): a copy of the K tiles per
// wavefront, the passes taken by the wavefronts in the order and pairs of csx_spmv_det_kernel, the
// copies summed in wavefront order: every column is bit-identical to the single-vector product.
#include "spmv_device.hpp"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// One workgroup owns one row-block: LDS holds COPIES x K y tiles (copy c, vector j at
// (c * K + j) * n_rows), then the K x windows where they are staged.
// ACCUM (SPX_RB_ACCUM): the tiles are added to Y with global atomics on top of csx_scale_kernel.
template <int K, int WAVES, bool ACCUM, bool DET>
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
                run_pair<K>(a, rb, {p0, p1}, tile, win, lane);
            } else {
                run_pass<K>(a, rb, p0, tile, win, lane);
                run_pass<K>(a, rb, p1, tile, win, lane);
            }
        } else {
            run_pass<K>(a, rb, p0, tile, win, lane);
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
                if (a.dvalues) t += a.dvalues[g] * xj[g];
                t *= a.alpha;
                if (a.beta != 0.0) t += a.beta * yj[g];
                yj[g] = t;
            }
        }
    }
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles, then the K x windows
    mv_body<K, WAVES, false, false>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_accum_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    mv_body<K, WAVES, true, false>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_det_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles per wavefront, then the K x windows
    mv_body<K, WAVES, false, true>(a, xs, lds_dyn);
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*MvKernel)(MvArgs, XcdSplit);

template <int K, int WAVES>
static MvKernel mv_kernel(MvFamily family)
{
    switch (family) {
    case MvFamily::accum: return csx_spmv_mv_accum_kernel<K, WAVES>;
    case MvFamily::det: return csx_spmv_mv_det_kernel<K, WAVES>;
    case MvFamily::plain: break;
    }
    return csx_spmv_mv_kernel<K, WAVES>;
}

template <int K>
static MvKernel mv_kernel_w(MvFamily family, int waves)
{
    return waves == 2 ? mv_kernel<K, 2>(family) : waves == 8 ? mv_kernel<K, 8>(family) : mv_kernel<K, 4>(family);
}

static MvKernel mv_kernel_kw(MvFamily family, int K, int waves)
{
    return K == 8 ? mv_kernel_w<8>(family, waves) : K == 4 ? mv_kernel_w<4>(family, waves) : mv_kernel_w<2>(family, waves);
}

void launch_spmv_mv(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                    const XcdSplit &xs)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    hipLaunchKernelGGL(mv_kernel_kw(family, K, w), dim3(blocks), dim3(64 * w), lds_bytes, static_cast<hipStream_t>(stream),
                       a, xs);
}

void spmv_mv_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    for (MvFamily f : {MvFamily::plain, MvFamily::accum, MvFamily::det})
        for (int K : {2, 4, 8})
            for (int w : {2, 4, 8})
                (void) hipFuncSetAttribute(reinterpret_cast<const void *>(mv_kernel_kw(f, K, w)),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

}  // namespace spx
