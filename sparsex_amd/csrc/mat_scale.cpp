// mat_scale.cpp -- see mat_scale.hpp
#include "mat_scale.hpp"

#include "stream_walk.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

namespace spx {

namespace {

// the partial results of one host thread: nrows + ncols doubles, found again through a thread-local pointer that
// is valid for one call (`epoch`)
struct ThreadPartial {
    uint64_t epoch = 0;
    double *buf = nullptr;
};
thread_local ThreadPartial tl_partial;
std::atomic<uint64_t> next_epoch(1);

inline double join(int kind, double s, double t) { return kind == 2 ? (t > s ? t : s) : s + t; }

}  // namespace

void host_mat_norms(const GpuStream &s, int kind, size_t nrows, size_t ncols, size_t own_lo, size_t own_hi,
                    double *rows, double *cols, unsigned nthreads)
{
    const uint64_t epoch = next_epoch.fetch_add(1);
    const size_t len = nrows + ncols;
    std::mutex mtx;
    std::vector<std::unique_ptr<std::vector<double>>> partials;
    for_each_stored_value(s, nthreads, [&](size_t pos, int64_t r, int64_t c, bool) {
        ThreadPartial &tp = tl_partial;
        if (tp.epoch != epoch) {
            std::lock_guard<std::mutex> lk(mtx);
            partials.emplace_back(new std::vector<double>(len ? len : 1, 0.0));
            tp.buf = partials.back()->data();
            tp.epoch = epoch;
        }
        if (r < 0 || (size_t) r >= nrows || c < 0 || (size_t) c >= ncols) throw FatalError("norms: an element outside the matrix");
        const double v = s.values[pos];
        const double t = kind == 1 ? v * v : std::fabs(v);
        if (rows) tp.buf[r] = join(kind, tp.buf[r], t);
        if (cols) tp.buf[nrows + (size_t) c] = join(kind, tp.buf[nrows + (size_t) c], t);
    });
    tl_partial = ThreadPartial();
    if (rows)
        parallel_for(own_hi > own_lo ? own_hi - own_lo : 0, nthreads > 1 && own_hi - own_lo > 4096 ? nthreads : 1, [&](size_t i) {
            double acc = 0.0;
            for (const auto &p : partials) acc = join(kind, acc, (*p)[own_lo + i]);
            rows[own_lo + i] = acc;
        });
    if (cols)
        parallel_for(ncols, nthreads > 1 && ncols > 4096 ? nthreads : 1, [&](size_t i) {
            double acc = 0.0;
            for (const auto &p : partials) acc = join(kind, acc, (*p)[nrows + i]);
            cols[i] = acc;
        });
}

void host_mat_scale(GpuStream &s, size_t nrows, size_t ncols, const double *dr, const double *dc, unsigned nthreads)
{
    // (two IEEE multiplications in this order: nothing is added behind them, so nothing can be contracted)
    double *values = s.values.data();
    for_each_stored_value(s, nthreads, [&](size_t pos, int64_t r, int64_t c, bool) {
        if (r < 0 || (size_t) r >= nrows || c < 0 || (size_t) c >= ncols) throw FatalError("scale: an element outside the matrix");
        double t = values[pos];
        if (dr) t = dr[r] * t;
        if (dc) t = t * dc[c];
        values[pos] = t;
    });
}

void host_mat_sym_norms(const GpuStream &s, int kind, size_t n, size_t own_lo, size_t own_hi, double *out, unsigned nthreads)
{
    const uint64_t epoch = next_epoch.fetch_add(1);
    std::mutex mtx;
    std::vector<std::unique_ptr<std::vector<double>>> partials;
    auto term = [kind](double v) { return kind == 1 ? v * v : std::fabs(v); };
    for_each_stored_value_of_pass(s, nthreads, [&](size_t pos, int64_t r, int64_t c, bool, uint8_t pass) {
        ThreadPartial &tp = tl_partial;
        if (tp.epoch != epoch) {
            std::lock_guard<std::mutex> lk(mtx);
            partials.emplace_back(new std::vector<double>(n ? n : 1, 0.0));
            tp.buf = partials.back()->data();
            tp.epoch = epoch;
        }
        if (r < 0 || (size_t) r >= n || c < 0 || (size_t) c >= n) throw FatalError("sym_norms: an element outside the matrix");
        if (r == c) return;
        const double t = term(s.values[pos]);
        tp.buf[r] = join(kind, tp.buf[r], t);
        if (pass == SPX_PASS_SYMTILE || pass == SPX_PASS_SYMSEG) tp.buf[c] = join(kind, tp.buf[c], t);
    });
    tl_partial = ThreadPartial();
    parallel_for(n, nthreads > 1 && n > 4096 ? nthreads : 1, [&](size_t i) {
        double acc = 0.0;
        for (const auto &p : partials) acc = join(kind, acc, (*p)[i]);
        if (i >= own_lo && i < own_hi && i < s.dvalues.size()) acc = join(kind, acc, term(s.dvalues[i]));
        out[i] = acc;
    });
    for (size_t t = 0; t < s.mirror_rows.size(); ++t) {
        const size_t r = s.mirror_rows[t];
        if (r >= n) throw FatalError("sym_norms: a mirror row outside the matrix");
        for (uint32_t k = s.mirror_ptr[t]; k < s.mirror_ptr[t + 1]; ++k) out[r] = join(kind, out[r], term(s.mirror_val[k]));
    }
}

void host_mat_sym_scale(GpuStream &s, size_t n, size_t own_lo, size_t own_hi, const double *d, unsigned nthreads)
{
    // (two IEEE multiplications, the factor of the larger index first: a mirror image gets the bits of its lower copy)
    for (size_t t = 0; t < s.mirror_rows.size(); ++t) {
        if (s.mirror_rows[t] >= n) throw FatalError("sym_scale: a mirror row outside the matrix");
        for (uint32_t k = s.mirror_ptr[t]; k < s.mirror_ptr[t + 1]; ++k)
            if (s.mirror_col[k] >= n) throw FatalError("sym_scale: a mirror column outside the matrix");
    }
    double *values = s.values.data();
    for_each_stored_value_of_pass(s, nthreads, [&](size_t pos, int64_t r, int64_t c, bool, uint8_t pass) {
        if (r < 0 || (size_t) r >= n || c < 0 || (size_t) c >= n) throw FatalError("sym_scale: an element outside the matrix");
        if (r == c) return;
        const double a = values[pos];
        if (pass == SPX_PASS_SYMTILE && a == 0.0) return;
        const double t = d[std::max(r, c)] * a;
        values[pos] = t * d[std::min(r, c)];
    });
    for (size_t i = own_lo; i < own_hi && i < s.dvalues.size(); ++i) {
        const double t = d[i] * s.dvalues[i];
        s.dvalues[i] = t * d[i];
    }
    for (size_t t = 0; t < s.mirror_rows.size(); ++t) {
        const size_t r = s.mirror_rows[t];
        for (uint32_t k = s.mirror_ptr[t]; k < s.mirror_ptr[t + 1]; ++k) {
            const size_t c = s.mirror_col[k];
            const double u = d[std::max(r, c)] * s.mirror_val[k];
            s.mirror_val[k] = u * d[std::min(r, c)];
        }
    }
}

}  // namespace spx
