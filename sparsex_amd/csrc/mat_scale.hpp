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

// The same on the host copy of a SYMMETRIC stream (csx_sym_norms_kernel, csx_sym_scale_kernel of
// sym_scale_kernels.hip).  host_mat_sym_norms writes all n elements of out: a value held once (tiles, read-once
// segments) counts for its row and its column, a value held twice for the row of each copy, the diagonal array for
// the own rows [own_lo, own_hi), the thin mirror list for its rows.  host_mat_sym_scale: values[p] <-
// fl(fl(d[max(r,c)] * values[p]) * d[min(r,c)]), the diagonal array and the mirror list alike.  A position with
// row == column (the zero of a block that closes over the diagonal) is neither counted nor written, and a +-0 of a
// tile pass keeps its bits.
void host_mat_sym_norms(const GpuStream &s, int kind, size_t n, size_t own_lo, size_t own_hi, double *out, unsigned nthreads);
void host_mat_sym_scale(GpuStream &s, size_t n, size_t own_lo, size_t own_hi, const double *d, unsigned nthreads);

}  // namespace spx
