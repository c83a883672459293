// stream_walk.hpp -- ONE walk over the row-block descriptor stream that names every position of its value array:
// visit(position, tuned row, tuned column, may_be_absent) for every stored element of every pass kind, row-blocks
// in chunks on the host threads.  Shared by the plan of a bulk value update (values_plan.cpp: position <- CSR
// index) and the plan of the diagonal (diag_plan.cpp: row -> position), so that the two cannot drift apart.  It
// reads index arrays only: the index-only host copy of a matrix in HBM serves as well as a full stream.
#pragma once

#include "stream_lanes.hpp"
#include "threads.hpp"

#include <algorithm>

namespace spx {

// `visit` is called concurrently for different row-blocks.  may_be_absent: a cell of an 8x8 tile, which the
// matrix need not hold (it stays the zero the tune put there); every other position visited is a real element
// (pass padding and lanes beyond a piece's length are not visited).  Rows and columns are NOT checked against
// the matrix: a caller that indexes by them does.
// for_each_stored_value_of_pass: the same walk, which also reports the kind of the pass that holds the position
// (SPX_PASS_*): on a symmetric stream SPX_PASS_SYMTILE and SPX_PASS_SYMSEG hold an entry ONCE, for its row and its
// column; every other kind holds one copy of an entry stored twice (mat_scale.cpp).
template <typename Visit>
void for_each_stored_value_of_pass(const GpuStream &s, unsigned nthreads, Visit visit)
{
    constexpr size_t RB_CHUNK = 16;
    const size_t n_rb = s.rbs.size();
    parallel_for((n_rb + RB_CHUNK - 1) / RB_CHUNK, nthreads, [&](size_t c) {
        for (size_t i = c * RB_CHUNK; i < std::min(n_rb, (c + 1) * RB_CHUNK); ++i) {
            const SpxRowBlock &rb = s.rbs[i];
            for (uint32_t t = 0; t < rb.n_pass; ++t) {
                const SpxPass &ps = s.passes[(size_t) rb.pass_off + t];
                const uint32_t nseg = ps.nseg, W = ps.width;
                const size_t vbase = (size_t) rb.val_off + ps.val_off;
                for (uint32_t l = 0; l < nseg; ++l) {
                    if (is_gather(ps)) {
                        // (lanes beyond a piece's length are padding)
                        const uint32_t sr = s.segrows[(size_t) rb.seg_off + ps.seg0 + l];
                        const int64_t row = (int64_t) rb.row0 + SPX_SEGROW_ROW(sr);
                        for (uint32_t w = 0; w < W && w < SPX_SEGROW_LEN(sr); ++w)
                            visit(vbase + spx_pass_value_index(l, w, nseg, W), row,
                                  gather_col(s, rb, ps, (size_t) ps.elem0 + l + (size_t) w * nseg), false, ps.kind);
                    } else if (ps.kind == SPX_PASS_SYMTILE) {
                        // (a cell of a tile that the matrix does not hold stays the zero the tune put there)
                        int64_t r, c0;
                        tile_lane(s, rb, ps, l, r, c0);
                        for (uint32_t w = 0; w < 8; ++w)
                            visit(vbase + spx_pass_value_index(l, w, nseg, 8), (int64_t) rb.row0 + r, c0 + w, true, ps.kind);
                    } else {
                        int64_t r, c0;
                        unit_lane(s, rb, ps, l, r, c0);
                        for (uint32_t w = 0; w < W; ++w)
                            visit(vbase + spx_pass_value_index(l, w, nseg, W), (int64_t) rb.row0 + r, c0 + w, false, ps.kind);
                    }
                }
            }
        }
    });
}

template <typename Visit>
void for_each_stored_value(const GpuStream &s, unsigned nthreads, Visit visit)
{
    for_each_stored_value_of_pass(s, nthreads, [&](size_t pos, int64_t row, int64_t col, bool may_be_absent, uint8_t) {
        visit(pos, row, col, may_be_absent);
    });
}

}  // namespace spx
