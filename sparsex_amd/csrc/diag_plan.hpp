// diag_plan.hpp -- where the diagonal of a tuned matrix lies (spx_hip_mat_diag_plan, spx_hip_mat_get_diag): per
// own row the position in the descriptor stream's value array that holds a(i, i), found by ONE walk over the
// stream (stream_walk.hpp, the walk of the values plan) instead of one stream_locate -- a row-block decode -- per
// row.  Reading the diagonal is then a gather: csx_gather_diag_kernel (refresh_kernels.hip) in HBM, a loop over
// the host copy of a host-only matrix.
//
// The reference hands out single entries only (spx_mat_get_entry, src/api/matvec.c:340-374); a Jacobi
// preconditioner needs all of the diagonal, in the numbering of the products' vectors, from the values as they
// are NOW -- after spx_hip_mat_set_values they may exist only in HBM.
//
// A symmetric stream keeps its diagonal in an array of its own (GpuStream::dvalues): nothing to plan.
#pragma once

#include "gpu_emit.hpp"

#include <cstdint>
#include <vector>

namespace spx {

constexpr uint32_t DIAG_PLAN_NONE = 0xffffffffu;       // a row without a stored diagonal entry: it reads +0.0

struct DiagPlan {
    std::vector<uint32_t> pos;   // general: per own row (own_lo + i) the position in GpuStream::values, or DIAG_PLAN_NONE;
                                 // symmetric: empty
    size_t own_lo = 0, n_rows = 0;
    uint64_t n_present = 0;      // own rows with a stored diagonal entry (symmetric: not counted, 0)
    bool symmetric = false;
};

// The stream may be the index-only copy a matrix in HBM keeps on the host: `n_values` is the length of its value array.
struct DiagPlanInput {
    const GpuStream *stream = nullptr;
    size_t n_values = 0;
    size_t nrows = 0, ncols = 0;
    bool symmetric = false;
    size_t own_lo = 0, own_hi = 0;
};

// Throws FatalError when a diagonal entry is stored at two positions, when the stream points outside its value
// array, or when the value array has 2^32 - 1 positions or more (a position would not fit the plan).
void build_diag_plan(const DiagPlanInput &in, DiagPlan &plan, unsigned nthreads);

// d[own_lo + i] for the plan's own rows from the host copy of a stream WITH values: a(i, i), +0.0 where none is
// stored; symmetric: the stream's diagonal array.  The rest of d is left alone.
void read_diag_host(const DiagPlan &plan, const GpuStream &s, val_t *d);

}  // namespace spx
