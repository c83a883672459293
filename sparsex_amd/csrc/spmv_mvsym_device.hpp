// spmv_mvsym_device.hpp -- device code of the read-once symmetric passes (SPX_PASS_SYMTILE,
// SPX_PASS_SYMSEG; gpu_format.h) for K vectors at once, used by csx_spmv_mvsym_kernel
// (spmv_mvsym_kernels.hip).  The K-vector forms of symtile_pass and symseg_passes of
// spmv_sym_device.hpp: a lane loads its descriptor, its slot entry and its values ONCE and then, vector
// by vector, does what the single-vector pass does -- the row sum into the y tile of that vector, the
// transposed products into its slots.
//
// LDS layout the passes assume: vector j keeps {slots, y tile} at lds + j * core, core = n_slots + n_rows
// of the row-block; `lds` below is the first vector's slots and `tile` its y tile (lds + n_slots).
// Column-major blocks: vector j of X at a.x + j * a.ldx, of Y at a.y + j * a.ldy.
#pragma once

#include "spmv_sym_device.hpp"

namespace spx {

// Vectors whose x loads go out together, for a pass of width W: the loads of one vector are a dependent round
// trip (x comes through L2), and K copies of a row-block's slots and y tile leave a CU few wavefronts to hide it
// behind -- so as many vectors at once as about 40 doubles of registers hold (W + 1 each): all K for the short
// segments of a stencil, four for tiles.  (Two at a time: syn-nlpkkt e240 1447 us per vector at K = 4,
// profiles/r10/MATMAT_SYM.md.)
template <int K, int W>
struct MvSymBatch {
    static constexpr int J = K * (W + 1) <= 40 ? K : (K >= 4 && 4 * (W + 1) <= 40 ? 4 : 2);
    static_assert(K % J == 0, "whole batches");
};

// A pass of symmetric tiles for K vectors.  `x16`: every vector's x is 16-byte aligned (x and ldx * 8 both
// are), so that the eight x values of a tile -- tiles start on columns that are multiples of eight -- come as
// four 16-byte loads; with an odd ldx every second vector is 8-byte aligned only and all of them load singly.
template <int K>
__device__ __forceinline__ void mvsym_tile_pass(const MvSymArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                                double *lds, double *tile, int core, bool x16, int lane)
{
    constexpr int J = MvSymBatch<K, 8>::J;
    const uint32_t nseg = ps.nseg;
    const bool active = (uint32_t) lane < nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;
    // the lane's tile descriptor: {col0, row0 | slot << 9}
    const uint2 q = ld_stream(reinterpret_cast<const uint2 *>(a.descs + rb.desc_off + ps.rank0 + (l >> 3)));
    const double *vals = a.values + rb.val_off + ps.val_off;
    double v[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const double2 vv = ld_stream(reinterpret_cast<const double2 *>(vals + (uint32_t) p * 2u * nseg + l * 2u));
        v[2 * p] = vv.x;
        v[2 * p + 1] = vv.y;
    }
    const int i = (int) (l & 7u);
    const int row = (int) (ps.elem0 + (q.y & 511u)) + i;
    const uint32_t slot = q.y >> 9;
    for (int j0 = 0; j0 < K; j0 += J) {
        double xr[J], xc[J][8];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            const double *xj = a.x + (size_t) (j0 + jj) * a.ldx;
            xr[jj] = xj[rb.row0 + (uint32_t) row];
            const double *xp = xj + q.x;
            if (x16) {
                const double2 *xp2 = reinterpret_cast<const double2 *>(xp);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const double2 xx = xp2[p];
                    xc[jj][2 * p] = xx.x;
                    xc[jj][2 * p + 1] = xx.y;
                }
            } else {
#pragma unroll
                for (int w = 0; w < 8; ++w) xc[jj][w] = xp[w];
            }
        }
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            double t = 0.0, p8[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                t = fma(v[w], xc[jj][w], t);
                // (idle lanes are whole idle tiles and the exchange stays inside a tile's eight lanes: symtile_pass)
                p8[w] = v[w] * xr[jj];
            }
            // the column sums, one per lane, by the three-step exchange of symtile_pass
            double p4[4];
            {
                const bool hi = (i & 4) != 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const double send = hi ? p8[w] : p8[w + 4];
                    const double keep = hi ? p8[w + 4] : p8[w];
                    p4[w] = keep + xchg4(send);
                }
            }
            double p2[2];
            {
                const bool hi = (i & 2) != 0;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const double send = hi ? p4[w] : p4[w + 2];
                    const double keep = hi ? p4[w + 2] : p4[w];
                    p2[w] = keep + xchg2(send);
                }
            }
            double cs;
            {
                const bool hi = (i & 1) != 0;
                const double send = hi ? p2[0] : p2[1];
                const double keep = hi ? p2[1] : p2[0];
                cs = keep + xchg1(send);
            }
            if (active) {
                const int at = (j0 + jj) * core;
                atomicAdd(&tile[at + row], t);
                atomicAdd(&lds[at + (int) slot + i], cs);
            }
        }
    }
}

// A pass of read-once row segments of width W for K vectors.  A segment without a slot adds its
// transposed products straight to y_j with global atomics, scaled by alpha.
template <int W, int K>
__device__ __forceinline__ void mvsym_seg_pass(const MvSymArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                               double *lds, double *tile, int core, int lane)
{
    constexpr int J = MvSymBatch<K, W>::J;
    const uint32_t nseg = ps.nseg;
    const bool active = (uint32_t) lane < nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;
    uint2 q;
    uint32_t slot0;
    if (ps.flags & SPX_PASSF_INLINE) {
        // (the pass' only descriptor came with its header)
        q.x = (uint32_t) ps.mask;
        q.y = (uint32_t) (ps.mask >> 32);
        slot0 = a.descs[rb.desc_off + (uint32_t) ps.rank0 + 1u].col0;
    } else {
        // (two entries per unit: the descriptor, then its slot)
        const uint32_t rank = (uint32_t) ps.rank0 + 2u * (active ? starts_upto(ps.mask, lane) : 0u);
        q = ld_stream(reinterpret_cast<const uint2 *>(a.descs + rb.desc_off + rank));
        slot0 = a.descs[rb.desc_off + rank + 1u].col0;
    }
    double v[W];
    {
        const double *vals = a.values + rb.val_off + ps.val_off;
#pragma unroll
        for (int p = 0; p < W / 2; ++p) {
            const double2 vv = ld_stream(reinterpret_cast<const double2 *>(vals + (uint32_t) p * 2u * nseg + l * 2u));
            v[2 * p] = vv.x;
            v[2 * p + 1] = vv.y;
        }
        if (W & 1) v[W - 1] = ld_stream(vals + (uint32_t) (W / 2) * 2u * nseg + l);
    }
    const UnitOrigin o = unit_origin(q.y, ps.seg0 + l, ps.elem0);
    const int row = o.row;
    const uint32_t col = q.x + (uint32_t) o.dcol;
    for (int j0 = 0; j0 < K; j0 += J) {
        double xr[J], x[J][W];
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            const double *xj = a.x + (size_t) (j0 + jj) * a.ldx;
            xr[jj] = xj[rb.row0 + (uint32_t) row];
#pragma unroll
            for (int w = 0; w < W; ++w) x[jj][w] = xj[col + (uint32_t) w];
        }
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) t = fma(v[w], x[jj][w], t);
            if (!active) continue;
            const int at = (j0 + jj) * core;
            atomicAdd(&tile[at + row], t);
            if (slot0 != SPX_NO_SLOT) {
                double *sl = lds + at + (int) slot0 + o.dcol;
#pragma unroll
                for (int w = 0; w < W; ++w) atomicAdd(&sl[w], v[w] * xr[jj]);
            } else {
                double *yp = a.y + (size_t) (j0 + jj) * a.ldy + col;
#pragma unroll
                for (int w = 0; w < W; ++w) atomicAdd(&yp[w], a.alpha * (v[w] * xr[jj]));
            }
        }
    }
}

template <int K>
__device__ __forceinline__ void run_mvsym_seg(const MvSymArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                              double *lds, double *tile, int core, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 2: mvsym_seg_pass<2, K>(a, rb, ps, lds, tile, core, lane); break;
    case 3: mvsym_seg_pass<3, K>(a, rb, ps, lds, tile, core, lane); break;
    case 4: mvsym_seg_pass<4, K>(a, rb, ps, lds, tile, core, lane); break;
    case 5: mvsym_seg_pass<5, K>(a, rb, ps, lds, tile, core, lane); break;
    case 6: mvsym_seg_pass<6, K>(a, rb, ps, lds, tile, core, lane); break;
    case 7: mvsym_seg_pass<7, K>(a, rb, ps, lds, tile, core, lane); break;
    default: mvsym_seg_pass<8, K>(a, rb, ps, lds, tile, core, lane); break;
    }
}

}  // namespace spx
