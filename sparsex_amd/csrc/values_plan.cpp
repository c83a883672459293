// values_plan.cpp -- see values_plan.hpp.
#include "values_plan.hpp"

#include "stream_walk.hpp"
#include "threads.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

namespace spx {

namespace {

constexpr uint32_t NONE = VALUES_PLAN_NONE;

// The caller's CSR arrays, looked up by (row, column) of the caller's numbering, 0-based.
struct CsrLookup {
    const idx_t *rowptr = nullptr, *colind = nullptr;
    int64_t base = 0;
    int64_t row_base = 0, rows = 0;
    // rows whose columns do not ascend: the positions of every row sorted by column (identity for the rows
    // that ascend); empty where every row ascends
    std::vector<uint32_t> order;

    size_t row_begin(int64_t lr) const { return (size_t)((int64_t) rowptr[lr] - base); }
    size_t row_end(int64_t lr) const { return (size_t)((int64_t) rowptr[lr + 1] - base); }

    uint32_t find(int64_t row, int64_t col) const
    {
        const int64_t lr = row - row_base;
        if (lr < 0 || lr >= rows) return NONE;
        size_t lo = row_begin(lr), hi = row_end(lr);
        const size_t end = hi;
        const int64_t key = col + base;
        if (order.empty()) {
            while (lo < hi) {
                const size_t mid = (lo + hi) / 2;
                if ((int64_t) colind[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            return lo < end && (int64_t) colind[lo] == key ? (uint32_t) lo : NONE;
        }
        while (lo < hi) {
            const size_t mid = (lo + hi) / 2;
            if ((int64_t) colind[order[mid]] < key) lo = mid + 1;
            else hi = mid;
        }
        return lo < end && (int64_t) colind[order[lo]] == key ? order[lo] : NONE;
    }
};

// the first offender by (row, column) of all the threads found
struct Offender {
    std::mutex mtx;
    bool any = false;
    int64_t row = 0, col = 0;
    std::string what;
    void report(int64_t r, int64_t c, const char *w)
    {
        std::lock_guard<std::mutex> lk(mtx);
        if (any && (row < r || (row == r && col <= c))) return;
        any = true;
        row = r;
        col = c;
        what = w;
    }
};

inline void count_hit(std::vector<uint8_t> &hits, uint32_t k)
{
    // (row-blocks are walked concurrently and a symmetric entry has up to three copies in different ones)
    uint8_t *p = &hits[k];
    if (__atomic_load_n(p, __ATOMIC_RELAXED) < 255) __atomic_fetch_add(p, (uint8_t) 1, __ATOMIC_RELAXED);
}

}  // namespace

void build_values_plan(const ValuesPlanInput &in, ValuesPlan &plan, unsigned nthreads)
{
    const GpuStream &s = *in.stream;
    const int64_t base = in.base;
    const size_t rows = in.csr_rows;
    // 1. the arrays themselves: row pointers ascending from the index base, columns inside the matrix
    if ((int64_t) in.rowptr[0] != base) throw FatalError("values plan: rowptr does not start at the index base");
    for (size_t r = 0; r < rows; ++r)
        if (in.rowptr[r + 1] < in.rowptr[r]) throw FatalError("values plan: rowptr is not ascending");
    const size_t nnz = (size_t)((int64_t) in.rowptr[rows] - base);
    if (nnz >= (size_t) NONE) throw FatalError("values plan: more entries than a 32-bit index counts");
    CsrLookup csr;
    csr.rowptr = in.rowptr;
    csr.colind = in.colind;
    csr.base = base;
    csr.row_base = (int64_t) in.csr_row_base;
    csr.rows = (int64_t) rows;
    // permutation: caller's row -> tuned row, and back
    std::vector<int32_t> pinv;
    if (in.perm) {
        pinv.assign(in.nrows, -1);
        for (size_t r = 0; r < in.nrows; ++r) {
            const int32_t t = in.perm[r];
            if (t < 0 || (size_t) t >= in.nrows || pinv[(size_t) t] >= 0) throw FatalError("values plan: bad permutation");
            pinv[(size_t) t] = (int32_t) r;
        }
    }
    auto to_caller = [&](int64_t t) { return in.perm ? (int64_t) pinv[(size_t) t] : t; };
    auto to_tuned = [&](int64_t r) { return in.perm ? (int64_t) in.perm[(size_t) r] : r; };
    Offender bad;
    auto fail_if_any = [&]() {
        if (!bad.any) return;
        throw FatalError("values plan: " + bad.what + " at (row " + std::to_string(bad.row + base) + ", column " +
                         std::to_string(bad.col + base) + ") -- not the pattern this matrix was tuned from");
    };
    constexpr size_t ROW_CHUNK = 1024;
    const size_t n_row_chunks = (rows + ROW_CHUNK - 1) / ROW_CHUNK;
    // 2. rows in any order the loader accepts: the unsorted ones get their positions sorted by column
    {
        std::vector<char> unsorted_chunk(n_row_chunks, 0);
        parallel_for(n_row_chunks, nthreads, [&](size_t c) {
            for (size_t r = c * ROW_CHUNK; r < std::min(rows, (c + 1) * ROW_CHUNK); ++r) {
                const size_t a = csr.row_begin((int64_t) r), b = csr.row_end((int64_t) r);
                for (size_t k = a; k < b; ++k) {
                    const int64_t col = (int64_t) in.colind[k] - base;
                    if (col < 0 || (size_t) col >= in.ncols) {
                        bad.report((int64_t)(r + in.csr_row_base), col, "a column outside the matrix");
                        return;
                    }
                    if (k > a && in.colind[k] <= in.colind[k - 1]) unsorted_chunk[c] = 1;
                }
            }
        });
        fail_if_any();
        bool any_unsorted = false;
        for (char u : unsorted_chunk) any_unsorted = any_unsorted || u;
        if (any_unsorted) {
            csr.order.resize(nnz);
            parallel_for(n_row_chunks, nthreads, [&](size_t c) {
                for (size_t r = c * ROW_CHUNK; r < std::min(rows, (c + 1) * ROW_CHUNK); ++r) {
                    const size_t a = csr.row_begin((int64_t) r), b = csr.row_end((int64_t) r);
                    for (size_t k = a; k < b; ++k) csr.order[k] = (uint32_t) k;
                    if (!unsorted_chunk[c]) continue;
                    std::sort(csr.order.begin() + a, csr.order.begin() + b,
                              [&](uint32_t x, uint32_t y) { return in.colind[x] < in.colind[y]; });
                    for (size_t k = a + 1; k < b; ++k)
                        if (in.colind[csr.order[k]] == in.colind[csr.order[k - 1]])
                            bad.report((int64_t)(r + in.csr_row_base), (int64_t) in.colind[csr.order[k]] - base,
                                       "a repeated column");
                }
            });
            fail_if_any();
        }
    }
    // 3. one walk over the stream: (position, row, column) of every stored element -> its CSR index
    plan.src_values.assign(in.n_values, NONE);
    plan.src_mirror.assign(s.mirror_col.size(), NONE);
    plan.src_diag.assign(in.symmetric ? in.own_hi - in.own_lo : 0, NONE);
    plan.own_lo = in.own_lo;
    plan.csr_nnz = nnz;
    std::vector<uint8_t> hits(nnz, 0);
    // the CSR index a stored element (tuned row, tuned column) takes its value from.  A symmetric stream holds the
    // entries on and below the diagonal of the tuned numbering (and mirror images of them): the position the tune
    // read, else the transposed one.
    auto source = [&](int64_t trow, int64_t tcol) -> uint32_t {
        if (in.symmetric && tcol > trow) std::swap(trow, tcol);
        const int64_t r = to_caller(trow), c = to_caller(tcol);
        uint32_t k = csr.find(r, c);
        if (k == NONE && in.symmetric && r != c) k = csr.find(c, r);
        return k;
    };
    auto place = [&](std::vector<uint32_t> &dst, size_t pos, int64_t trow, int64_t tcol, bool may_be_absent) {
        if (trow < 0 || (size_t) trow >= in.nrows || tcol < 0 || (size_t) tcol >= in.ncols || pos >= dst.size())
            throw FatalError("values plan: the descriptor stream points outside the matrix");
        // (a symmetric stream keeps the diagonal in its own array: where a dense block of the lower triangle and
        // its mirror image closes over the diagonal, the cell on it is a zero the tune put there and stays one)
        if (in.symmetric && trow == tcol && &dst == &plan.src_values) return;
        const uint32_t k = source(trow, tcol);
        if (k == NONE) {
            if (!may_be_absent) bad.report(to_caller(trow), to_caller(tcol), "the tuned matrix holds an entry the CSR arrays lack");
            return;
        }
        dst[pos] = k;
        count_hit(hits, k);
    };
    for_each_stored_value(s, nthreads, [&](size_t pos, int64_t trow, int64_t tcol, bool may_be_absent) {
        place(plan.src_values, pos, trow, tcol, may_be_absent);
    });
    // ... the thin mirror list of a symmetric slice: entry k of row t is the mirror image of (column, row)
    for (size_t t = 0; t < s.mirror_rows.size(); ++t)
        for (uint32_t k = s.mirror_ptr[t]; k < s.mirror_ptr[t + 1]; ++k)
            place(plan.src_mirror, k, (int64_t) s.mirror_rows[t], (int64_t) s.mirror_col[k], false);
    // ... and the diagonal array (a row without a diagonal entry keeps its zero)
    if (in.symmetric) {
        constexpr size_t DCHUNK = 4096;
        const size_t nd = plan.src_diag.size();
        parallel_for((nd + DCHUNK - 1) / DCHUNK, nthreads, [&](size_t c) {
            for (size_t i = c * DCHUNK; i < std::min(nd, (c + 1) * DCHUNK); ++i)
                place(plan.src_diag, i, (int64_t)(in.own_lo + i), (int64_t)(in.own_lo + i), true);
        });
    }
    fail_if_any();
    // 4. every CSR entry this process owns has a destination.  General: the entries of its own rows.  Symmetric:
    //    those on and below the diagonal of the tuned numbering (an entry above it counts where its transposed
    //    position is absent: the stream would have had to take it from there).
    std::vector<uint64_t> sources_of(n_row_chunks, 0);
    parallel_for(n_row_chunks, nthreads, [&](size_t c) {
        uint64_t n = 0;
        for (size_t lr = c * ROW_CHUNK; lr < std::min(rows, (c + 1) * ROW_CHUNK); ++lr) {
            const int64_t r = (int64_t)(lr + in.csr_row_base);
            if ((size_t) r >= in.nrows) {
                bad.report(r, 0, "a row outside the matrix");
                return;
            }
            const int64_t tr = to_tuned(r);
            for (size_t k = csr.row_begin((int64_t) lr); k < csr.row_end((int64_t) lr); ++k) {
                if (hits[k]) {
                    ++n;
                    continue;
                }
                const int64_t col = (int64_t) in.colind[k] - base;
                bool owned;
                if (!in.symmetric) {
                    owned = (size_t) tr >= in.own_lo && (size_t) tr < in.own_hi;
                } else {
                    const int64_t tc = to_tuned(col);
                    const int64_t lower_row = std::max(tr, tc);
                    owned = (size_t) lower_row >= in.own_lo && (size_t) lower_row < in.own_hi &&
                            (tr >= tc || csr.find(col, r) == NONE);
                }
                if (owned) bad.report(r, col, "the CSR arrays hold an entry the tuned matrix lacks");
            }
        }
        sources_of[c] = n;
    });
    fail_if_any();
    plan.n_sources = 0;
    for (uint64_t n : sources_of) plan.n_sources += n;
    plan.n_dest = 0;
    for (const std::vector<uint32_t> *v : {&plan.src_values, &plan.src_mirror, &plan.src_diag})
        for (uint32_t k : *v) plan.n_dest += k != NONE ? 1 : 0;
}

namespace {

void apply_one(const std::vector<uint32_t> &src, const val_t *csr_values, val_t *dst, unsigned nthreads)
{
    constexpr size_t CHUNK = (size_t) 1 << 16;
    const size_t n = src.size();
    parallel_for((n + CHUNK - 1) / CHUNK, nthreads, [&](size_t c) {
        for (size_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); ++i)
            if (src[i] != NONE) dst[i] = csr_values[src[i]];
    });
}

}  // namespace

void apply_values_plan(const ValuesPlan &plan, const val_t *csr_values, GpuStream &s, unsigned nthreads)
{
    if (plan.src_values.size() != s.values.size() || plan.src_mirror.size() != s.mirror_val.size() ||
        (!plan.src_diag.empty() && plan.own_lo + plan.src_diag.size() > s.dvalues.size()))
        throw FatalError("values plan: not the plan of this stream");
    apply_one(plan.src_values, csr_values, s.values.data(), nthreads);
    apply_one(plan.src_mirror, csr_values, s.mirror_val.data(), nthreads);
    if (!plan.src_diag.empty()) apply_one(plan.src_diag, csr_values, s.dvalues.data() + plan.own_lo, nthreads);
}

namespace {

inline void digest_step(ValuesDigest &d, uint64_t v)
{
    d.a = (d.a ^ v) * 0x100000001B3ull;                              // FNV-1a over 64-bit words
    uint64_t x = d.b + v + 0x9E3779B97F4A7C15ull;                    // ... and a splitmix round: two unrelated mixes
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    d.b = x ^ (x >> 31);
}

void digest_one(ValuesDigest &d, const std::vector<uint32_t> &src, const val_t *vals, unsigned nthreads)
{
    constexpr size_t CHUNK = (size_t) 1 << 16;
    const size_t n = src.size(), chunks = (n + CHUNK - 1) / CHUNK;
    std::vector<ValuesDigest> part(chunks);
    parallel_for(chunks, nthreads, [&](size_t c) {
        ValuesDigest h;
        h.a = 0xCBF29CE484222325ull;
        for (size_t i = c * CHUNK; i < std::min(n, (c + 1) * CHUNK); ++i) {
            if (src[i] == NONE) continue;
            uint64_t bits;
            std::memcpy(&bits, vals + i, sizeof(bits));
            digest_step(h, bits);
        }
        part[c] = h;
    });
    for (const ValuesDigest &h : part) {           // (in order: the digest does not depend on the threads)
        digest_step(d, h.a);
        digest_step(d, h.b);
    }
}

}  // namespace

ValuesDigest values_plan_digest(const ValuesPlan &plan, const GpuStream &s, unsigned nthreads)
{
    if (plan.src_values.size() != s.values.size() || plan.src_mirror.size() != s.mirror_val.size() ||
        (!plan.src_diag.empty() && plan.own_lo + plan.src_diag.size() > s.dvalues.size()))
        throw FatalError("values plan: not the plan of this stream");
    ValuesDigest d;
    digest_one(d, plan.src_values, s.values.data(), nthreads);
    digest_one(d, plan.src_mirror, s.mirror_val.data(), nthreads);
    if (!plan.src_diag.empty()) digest_one(d, plan.src_diag, s.dvalues.data() + plan.own_lo, nthreads);
    return d;
}

}  // namespace spx
