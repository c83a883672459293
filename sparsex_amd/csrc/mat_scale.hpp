// mat_scale.hpp -- row / column norms and diagonal scaling of the host copy of a general stream (host-only
// matrices, spx.rt.host_only): what csx_norms_kernel and csx_scale_values_kernel (scale_kernels.hip) do in HBM,
// on the host threads through the one walk over the stream (stream_walk.hpp).
#pragma once

#include "gpu_emit.hpp"

#include <cstddef>

namespace spx {

// kind: 0 sum of |a|, 1 sum of a^2, 2 max of |a| (spx_hip_mat_norms).  rows[own_lo, own_hi) and cols[0, ncols) are
// written (+0.0 where nothing is stored), either may be null; per-thread partial results, joined at the end.
void host_mat_norms(const GpuStream &s, int kind, size_t nrows, size_t ncols, size_t own_lo, size_t own_hi,
                    double *rows, double *cols, unsigned nthreads);

// values[p] <- fl(fl(dr[r] * values[p]) * dc[c]) for every stored element (a null vector: its product is not
// formed); positions without an element keep their bits
void host_mat_scale(GpuStream &s, size_t nrows, size_t ncols, const double *dr, const double *dc, unsigned nthreads);

}  // namespace spx
