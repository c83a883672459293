// spmv_mvr_f32_kernels.hip -- the float forms of the kernels of spmv_mvr_kernels.hip: the multi-vector product
// Y <- alpha*fl32(A)*X + beta*Y on ROW-MAJOR (interleaved) blocks, K = 1, 2, 4 or 8 vectors per pass over the
// plain stream of a general tune, with the values read from the float twin (spx.gpu.values_f32):
// MvrArgs::values POINTS AT FLOATS, element for element the array of doubles.  The host side is
// device_spmm_rm_f32 (device_runtime.cpp).
//
// mv_body over MvrArgs with V = float and nothing else changed: the values widen in registers; x, the staged window, the
// tiles, the fused multiply-adds, the sums and the write-out are fp64; LDS, staging, family and wavefronts are
// those of the handle's fp64 row-major product.  The scale and fix-up steps around the row-block launches read
// no values (general streams have no diagonal array) and are the fp64 product's: csx_scale_rm_kernel,
// csx_fixup_rm_kernel.
//
// A translation unit of its own: the build stays parallel, and the fp64 object is the one it was.
#include "spmv_mvr_device.hpp"
#include "spmv_mv_instances.hpp"

namespace spx {

using Instances = MvInstances<MvrArgs, float, 1, 2, 4, 8>;     // csx_spmv_mv_kernel<MvrArgs, float, family, K, waves>

void launch_spmv_mvr_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream,
                         const MvrArgs &a, const XcdSplit &xs)
{
    Instances::launch(family, K, waves, blocks, lds_bytes, stream, a, xs);
}

void spmv_mvr_f32_allow_lds(size_t bytes) { Instances::allow_lds(bytes); }

}  // namespace spx
