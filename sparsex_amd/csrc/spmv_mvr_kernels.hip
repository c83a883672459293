// spmv_mvr_kernels.hip -- the multi-vector product Y <- alpha*A*X + beta*Y for gfx950 on ROW-MAJOR
// (interleaved) blocks: entry (i, j) of X at x[i * ldx + j], of Y at y[i * ldy + j]; K vectors per pass over
// the stream, K = 1, 2, 4 or 8 (one vector too: a remainder vector of such a block is still strided, which the
// single-vector kernels cannot read).  The host side is device_spmm_rm (device_runtime.cpp).
//
// The kernel of spmv_mv_kernels.hip with the K-vector composition of spmv_mvr_device.hpp: the same row-blocks,
// pass order and pairing, K-wide carry and LDS budget, over the PLAIN stream (passes, descs) of a general
// tune.  What differs is where x and y lie: a lane loads the K contiguous doubles of each of its columns, the
// staged x window is one copy of xwin_len consecutive rows of X, and the write-out walks the row-block's
// n_rows x K entries of Y in memory order.
//
// The y tiles in LDS stay vector-major (vector j's rows at j * n_rows, the layout of mv_body) and are
// transposed at the write-out: in a unit pass neighbouring lanes mostly own neighbouring rows, so the adds of
// one vector (one ds_add_f64 per pass and vector) fall into consecutive banks, where tile[row * K + j] would
// put the lanes 8 * K bytes apart (K = 8: every lane on one of four bank groups).  The adds run once per row
// segment, the write-out once per row, so the conflicts are put where they are paid least often.  Only this
// layout was built; the reasoning, not a measurement of both, decided (profiles/r15/MATMAT_RM.md).
//
// DET: as in spmv_mv_kernels.hip -- a copy of the K tiles per wavefront, summed in wavefront order: every
// column is bit-identical to the single-vector product.
// (mv_body: spmv_mv_device.hpp; the kernel template over it, csx_spmv_mv_kernel<MvrArgs, double, family, K, waves>,
// and the table of its instances: spmv_mv_instances.hpp)
#include "spmv_mvr_device.hpp"
#include "spmv_mv_instances.hpp"

#include <cstddef>
#include <cstdint>

namespace spx {

// ---- the steps around the row-block launches, interleaved forms of csx_scale_kernel and csx_fixup_kernel ----

// column slices in one launch, first step: y <- beta * y on the K vectors of the rows [lo, hi); one thread per
// entry, never the padding behind a row's K
__global__ void csx_scale_rm_kernel(double *y, size_t ldy, size_t lo, size_t n, uint32_t K, double beta)
{
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * K) return;
    double *yp = y + (lo + e / K) * ldy + e % K;
    *yp = beta == 0.0 ? 0.0 : beta * *yp;
}

// rows split over several row-blocks: sum their partials (vector j's at carry + j * n_carry; blockIdx.y: j)
__global__ void csx_fixup_rm_kernel(const SpxSharedRow *shared, uint32_t n_shared, const double *carry, uint32_t n_carry,
                                    double *y, size_t ldy, double alpha, double beta)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_shared) return;
    const size_t j = blockIdx.y;
    const SpxSharedRow sr = shared[i];
    const double *cj = carry + j * n_carry;
    double *yp = y + (size_t) sr.row * ldy + j;
    double s = 0.0;
    for (uint32_t k = 0; k < sr.n_slots; ++k) s += cj[sr.first_slot + k];
    *yp = (beta == 0.0) ? alpha * s : alpha * s + beta * *yp;
}

// ---- launchers ------------------------------------------------------------------------------

using Instances = MvInstances<MvrArgs, double, 1, 2, 4, 8>;

void launch_spmv_mvr(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvrArgs &a,
                     const XcdSplit &xs)
{
    Instances::launch(family, K, waves, blocks, lds_bytes, stream, a, xs);
}

void spmv_mvr_allow_lds(size_t bytes) { Instances::allow_lds(bytes); }

void launch_scale_rm(void *stream, int nvec, double *y, size_t ldy, size_t lo, size_t hi, double beta)
{
    const size_t t = 256, n = (hi - lo) * (size_t) nvec;
    hipLaunchKernelGGL(csx_scale_rm_kernel, dim3((unsigned) ((n + t - 1) / t)), dim3((unsigned) t), 0,
                       static_cast<hipStream_t>(stream), y, ldy, lo, hi - lo, (uint32_t) nvec, beta);
}

void launch_fixup_rm(void *stream, int nvec, const SpxSharedRow *shared, uint32_t n_shared, const double *carry,
                     uint32_t n_carry, double *y, size_t ldy, double alpha, double beta)
{
    hipLaunchKernelGGL(csx_fixup_rm_kernel, dim3((n_shared + 63) / 64, (unsigned) nvec), dim3(64), 0,
                       static_cast<hipStream_t>(stream), shared, n_shared, carry, n_carry, y, ldy, alpha, beta);
}

}  // namespace spx
