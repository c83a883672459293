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
#include "spmv_mv_instances.hpp"

namespace spx {

using Instances = MvInstances<MvArgs, float, 2, 4, 8>;     // csx_spmv_mv_kernel<MvArgs, float, family, K, waves>

void launch_spmv_mv_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                        const XcdSplit &xs)
{
    Instances::launch(family, K, waves, blocks, lds_bytes, stream, a, xs);
}

void spmv_mv_f32_allow_lds(size_t bytes) { Instances::allow_lds(bytes); }

}  // namespace spx
