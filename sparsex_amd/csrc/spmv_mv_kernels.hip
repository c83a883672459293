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
// (mv_body: spmv_mv_device.hpp; the kernel template over it, csx_spmv_mv_kernel<MvArgs, double, family, K, waves>,
// and the table of its instances: spmv_mv_instances.hpp)
#include "spmv_mv_instances.hpp"

namespace spx {

using Instances = MvInstances<MvArgs, double, 2, 4, 8>;

void launch_spmv_mv(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                    const XcdSplit &xs)
{
    Instances::launch(family, K, waves, blocks, lds_bytes, stream, a, xs);
}

void spmv_mv_allow_lds(size_t bytes) { Instances::allow_lds(bytes); }

}  // namespace spx
