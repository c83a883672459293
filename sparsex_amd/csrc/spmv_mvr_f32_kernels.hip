// spmv_mvr_f32_kernels.hip -- the float forms of the kernels of spmv_mvr_kernels.hip: the multi-vector product
// Y <- alpha*fl32(A)*X + beta*Y on ROW-MAJOR (interleaved) blocks, K = 1, 2, 4 or 8 vectors per pass over the
// plain stream of a general tune, with the values read from the float twin (spx.gpu.values_f32):
// MvrArgs::values POINTS AT FLOATS, element for element the array of doubles.  The host side is
// device_spmm_rm_f32 (device_runtime.cpp).
//
// mvr_body with V = float and nothing else changed: the values widen in registers; x, the staged window, the
// tiles, the fused multiply-adds, the sums and the write-out are fp64; LDS, staging, family and wavefronts are
// those of the handle's fp64 row-major product.  The scale and fix-up steps around the row-block launches read
// no values (general streams have no diagonal array) and are the fp64 product's: csx_scale_rm_kernel,
// csx_fixup_rm_kernel.
//
// A translation unit of its own: the build stays parallel, and the fp64 object is the one it was.
#include "spmv_mvr_device.hpp"

namespace spx {

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mvr_f32_kernel(MvrArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles, then the x window
    mvr_body<K, WAVES, false, false, float>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mvr_accum_f32_kernel(MvrArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    mvr_body<K, WAVES, true, false, float>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mvr_det_f32_kernel(MvrArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles per wavefront, then the x window
    mvr_body<K, WAVES, false, true, float>(a, xs, lds_dyn);
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*MvrKernel)(MvrArgs, XcdSplit);

template <int K, int WAVES>
static MvrKernel mvr_f32_kernel(MvFamily family)
{
    switch (family) {
    case MvFamily::accum: return csx_spmv_mvr_accum_f32_kernel<K, WAVES>;
    case MvFamily::det: return csx_spmv_mvr_det_f32_kernel<K, WAVES>;
    case MvFamily::plain: break;
    }
    return csx_spmv_mvr_f32_kernel<K, WAVES>;
}

template <int K>
static MvrKernel mvr_f32_kernel_w(MvFamily family, int waves)
{
    return waves == 2 ? mvr_f32_kernel<K, 2>(family) : waves == 8 ? mvr_f32_kernel<K, 8>(family)
                                                                  : mvr_f32_kernel<K, 4>(family);
}

static MvrKernel mvr_f32_kernel_kw(MvFamily family, int K, int waves)
{
    return K == 8 ? mvr_f32_kernel_w<8>(family, waves) : K == 4 ? mvr_f32_kernel_w<4>(family, waves)
         : K == 2 ? mvr_f32_kernel_w<2>(family, waves) : mvr_f32_kernel_w<1>(family, waves);
}

void launch_spmv_mvr_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream,
                         const MvrArgs &a, const XcdSplit &xs)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    hipLaunchKernelGGL(mvr_f32_kernel_kw(family, K, w), dim3(blocks), dim3(64 * w), lds_bytes,
                       static_cast<hipStream_t>(stream), a, xs);
}

void spmv_mvr_f32_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    for (MvFamily f : {MvFamily::plain, MvFamily::accum, MvFamily::det})
        for (int K : {1, 2, 4, 8})
            for (int w : {2, 4, 8})
                (void) hipFuncSetAttribute(reinterpret_cast<const void *>(mvr_f32_kernel_kw(f, K, w)),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

}  // namespace spx
