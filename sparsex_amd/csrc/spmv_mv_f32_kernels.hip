// spmv_mv_f32_kernels.hip -- the float forms of the kernels of spmv_mv_kernels.hip: the multi-vector product
// Y <- alpha*fl32(A)*X + beta*Y on column-major blocks, K = 2, 4 or 8 vectors per pass over the stream, with the
// values read from the float twin (spx.gpu.values_f32): MvArgs::values POINTS AT FLOATS, element for element the
// array of doubles.  The host side is device_spmm_f32 (device_runtime.cpp).
//
// mv_body with V = float and nothing else changed: the values widen in registers, the vectors, the x windows
// in LDS, the tiles, the fused multiply-adds, the sums and the write-out are fp64, and LDS, staging, family and
// wavefronts are those of the handle's fp64 block product.  A diagonal added at the write-out (symmetric
// streams under spx.gpu.sym_once=false) has no twin and is rounded in registers.  Every column is the product
// csx_spmv_f32_kernel gives for it, bit for bit where the tiles are kept per wavefront (DET).
//
// A translation unit of its own: the build stays parallel, and the fp64 object is the one it was.
#include "spmv_mv_device.hpp"

namespace spx {

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_f32_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles, then the K x windows
    mv_body<K, WAVES, false, false, float>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_accum_f32_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    mv_body<K, WAVES, true, false, float>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_det_f32_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles per wavefront, then the K x windows
    mv_body<K, WAVES, false, true, float>(a, xs, lds_dyn);
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*MvKernel)(MvArgs, XcdSplit);

template <int K, int WAVES>
static MvKernel mv_f32_kernel(MvFamily family)
{
    switch (family) {
    case MvFamily::accum: return csx_spmv_mv_accum_f32_kernel<K, WAVES>;
    case MvFamily::det: return csx_spmv_mv_det_f32_kernel<K, WAVES>;
    case MvFamily::plain: break;
    }
    return csx_spmv_mv_f32_kernel<K, WAVES>;
}

template <int K>
static MvKernel mv_f32_kernel_w(MvFamily family, int waves)
{
    return waves == 2 ? mv_f32_kernel<K, 2>(family) : waves == 8 ? mv_f32_kernel<K, 8>(family) : mv_f32_kernel<K, 4>(family);
}

static MvKernel mv_f32_kernel_kw(MvFamily family, int K, int waves)
{
    return K == 8 ? mv_f32_kernel_w<8>(family, waves) : K == 4 ? mv_f32_kernel_w<4>(family, waves)
                                                               : mv_f32_kernel_w<2>(family, waves);
}

void launch_spmv_mv_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                        const XcdSplit &xs)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    hipLaunchKernelGGL(mv_f32_kernel_kw(family, K, w), dim3(blocks), dim3(64 * w), lds_bytes,
                       static_cast<hipStream_t>(stream), a, xs);
}

void spmv_mv_f32_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    for (MvFamily f : {MvFamily::plain, MvFamily::accum, MvFamily::det})
        for (int K : {2, 4, 8})
            for (int w : {2, 4, 8})
                (void) hipFuncSetAttribute(reinterpret_cast<const void *>(mv_f32_kernel_kw(f, K, w)),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

}  // namespace spx
