// diag_plan.cpp -- see diag_plan.hpp.
#include "diag_plan.hpp"

#include "stream_walk.hpp"

#include <atomic>
#include <string>

namespace spx {

void build_diag_plan(const DiagPlanInput &in, DiagPlan &plan, unsigned nthreads)
{
    plan.pos.clear();
    plan.own_lo = in.own_lo;
    plan.n_rows = in.own_hi > in.own_lo ? in.own_hi - in.own_lo : 0;
    plan.n_present = 0;
    plan.symmetric = in.symmetric;
    if (in.symmetric) return;            // (the diagonal has an array of its own)
    if (in.n_values >= (size_t) DIAG_PLAN_NONE) throw FatalError("diagonal plan: more positions than a 32-bit index counts");
    plan.pos.assign(plan.n_rows, DIAG_PLAN_NONE);
    // (row-blocks are walked concurrently, and the column slices of spx.gpu.col_phases put a row into several)
    uint32_t *pos = plan.pos.data();
    std::atomic<int64_t> twice(-1);
    for_each_stored_value(*in.stream, nthreads, [&](size_t at, int64_t row, int64_t col, bool) {
        if (row != col) return;
        if (row < 0 || (size_t) row >= in.nrows || (size_t) col >= in.ncols || at >= in.n_values)
            throw FatalError("diagonal plan: the descriptor stream points outside the matrix");
        if ((size_t) row < in.own_lo || (size_t) row >= in.own_hi) return;
        uint32_t none = DIAG_PLAN_NONE;
        if (!__atomic_compare_exchange_n(pos + ((size_t) row - in.own_lo), &none, (uint32_t) at, false, __ATOMIC_RELAXED,
                                         __ATOMIC_RELAXED))
            twice.store(row);
    });
    if (twice.load() >= 0) {
        const int64_t row = twice.load();
        plan.pos.clear();
        throw FatalError("diagonal plan: the stream holds the diagonal entry of row " + std::to_string(row) + " at two positions");
    }
    for (uint32_t p : plan.pos) plan.n_present += p != DIAG_PLAN_NONE ? 1 : 0;
}

void read_diag_host(const DiagPlan &plan, const GpuStream &s, val_t *d)
{
    if (plan.symmetric) {
        if (plan.own_lo + plan.n_rows > s.dvalues.size()) throw FatalError("diagonal plan: not the plan of this stream");
        for (size_t i = 0; i < plan.n_rows; ++i) d[plan.own_lo + i] = s.dvalues[plan.own_lo + i];
        return;
    }
    if (plan.pos.size() != plan.n_rows) throw FatalError("diagonal plan: not the plan of this stream");
    for (size_t i = 0; i < plan.n_rows; ++i) {
        const uint32_t p = plan.pos[i];
        if (p != DIAG_PLAN_NONE && p >= s.values.size()) throw FatalError("diagonal plan: not the plan of this stream");
        d[plan.own_lo + i] = p == DIAG_PLAN_NONE ? 0.0 : s.values[p];
    }
}

}  // namespace spx
