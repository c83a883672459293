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
// (mv_body, the body of the kernels below and of their float forms in spmv_mv_f32_kernels.hip: spmv_mv_device.hpp)
#include "spmv_mv_device.hpp"

namespace spx {

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
