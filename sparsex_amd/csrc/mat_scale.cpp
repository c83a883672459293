// mat_scale.cpp -- see mat_scale.hpp
#include "mat_scale.hpp"

#include "stream_walk.hpp"

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

}  // namespace spx
