// values_plan.hpp -- new values for a tuned matrix whose pattern stays (spx_hip_mat_values_plan,
// spx_hip_mat_set_values): a one-time plan "position in the descriptor stream <- index in the caller's CSR
// value array", built by ONE walk over the stream (every pass kind, the thin mirror list, the diagonal array)
// with one binary search per stored element in the caller's CSR row.
//
// The reference offers spx_mat_set_entry only (src/api/matvec.c:376-407); an outer loop that changes every
// value -- Newton steps, time steps, interior-point iterations -- would pay a row-block decode per nonzero
// there, or a new tune.  Applying the plan is a gather: refresh_kernels.hip in HBM, apply_values_plan on the
// host copy of a host-only matrix.
#pragma once

#include "gpu_emit.hpp"

#include <cstdint>
#include <vector>

namespace spx {

constexpr uint32_t VALUES_PLAN_NONE = 0xffffffffu;     // a position without a source: it keeps its bits

struct ValuesPlan {
    // per position of GpuStream::values / mirror_val / per own row (dvalues[own_lo + i]): the CSR index
    // (0-based position in the caller's value array) or VALUES_PLAN_NONE
    std::vector<uint32_t> src_values, src_mirror, src_diag;
    size_t own_lo = 0;           // src_diag[i] belongs to row own_lo + i
    size_t csr_nnz = 0;          // entries the caller's value array must hold
    uint64_t n_sources = 0;      // CSR entries the stream holds at least once
    uint64_t n_dest = 0;         // positions with a source, over the three arrays
};

// What the plan is built from.  The stream may be the index-only copy a matrix keeps on the host (no values):
// `n_values` is the length of its value array.  `perm`: the matrix' permutation (caller's row -> tuned row) or
// null.  The CSR arrays hold rows [csr_row_base, csr_row_base + csr_rows) of the caller's numbering (the whole
// matrix, or the slice an input with spx.rt.row_offset was loaded from); `base` is their indexing, 0 or 1.
struct ValuesPlanInput {
    const GpuStream *stream = nullptr;
    size_t n_values = 0;
    size_t nrows = 0, ncols = 0;
    bool symmetric = false;
    size_t own_lo = 0, own_hi = 0;
    const int32_t *perm = nullptr;
    const idx_t *rowptr = nullptr, *colind = nullptr;
    int base = 0;
    size_t csr_row_base = 0, csr_rows = 0;
};

// Throws FatalError naming the first offending (row, column) -- caller's numbering, the arrays' indexing -- when
// the CSR pattern is not the tuned one: an entry this process owns without a destination, a stored element
// without a source, a row with a repeated column.
void build_values_plan(const ValuesPlanInput &in, ValuesPlan &plan, unsigned nthreads);

// dst[i] = csr_values[src[i]] for every position with a source, on the host threads
void apply_values_plan(const ValuesPlan &plan, const val_t *csr_values, GpuStream &s, unsigned nthreads);

// 128 bits over the bit patterns of every position with a source, in order: what a host-only matrix keeps of the
// values it held before its first bulk update, to know when an update has put exactly those back (its encoded
// partitions, which no update touches, are then true again)
struct ValuesDigest {
    uint64_t a = 0, b = 0;
    bool operator==(const ValuesDigest &o) const { return a == o.a && b == o.b; }
};
ValuesDigest values_plan_digest(const ValuesPlan &plan, const GpuStream &s, unsigned nthreads);

}  // namespace spx
