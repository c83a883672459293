// stream_lanes.hpp -- the lane decoders of the row-block descriptor stream (gpu_format.h): which row and which
// columns lane l of a pass covers.  Shared by the walks of stream_index.cpp (random access, validation, halo and
// conflict rows) and of values_plan.cpp (the plan of a bulk value update), so that the two cannot drift apart.
#pragma once

#include "gpu_emit.hpp"

#include <cstring>

namespace spx {

inline uint32_t popcount_upto(uint64_t mask, uint32_t lane)
{
    // set bits in lanes 1..lane (bit 0 is never set)
    const uint64_t m = lane >= 63 ? mask : (mask & ((2ull << lane) - 1ull));
    return (uint32_t) __builtin_popcountll(m);
}

// row (relative to the row-block) and first column of lane l of a unit pass
inline void unit_lane(const GpuStream &s, const SpxRowBlock &rb, const SpxPass &ps, uint32_t l,
                      int64_t &row, int64_t &col, uint32_t *slot = nullptr)
{
    // (read-once symmetric segments: two entries per unit, the second holds the slot)
    const uint32_t stride = ps.kind == SPX_PASS_SYMSEG ? 2u : 1u;
    const uint32_t rank = (uint32_t) ps.rank0 + stride * popcount_upto(spx_pass_mask(&ps), l);
    const SpxUnitDesc &d = s.descs[(size_t) rb.desc_off + rank];
    if (slot) *slot = stride == 2 ? s.descs[(size_t) rb.desc_off + rank + 1].col0 : SPX_NO_SLOT;
    const uint32_t bits = d.bits;
    const int sidx = (int) ((ps.seg0 + l - ((bits >> 9) & 8191u)) & 0xffffu);
    const uint32_t kind = (bits >> 22) & 7u;
    const int step = (int) (bits >> 25);
    const int drow = kind == SPX_KIND_BLOCK ? 1 : (kind >= SPX_KIND_VERT ? step : 0);
    const int dcol = (kind == SPX_KIND_HORIZ || kind == SPX_KIND_DIAG)
                         ? step : (kind == SPX_KIND_ADIAG ? -step : 0);
    row = (int64_t) ps.elem0 + (int64_t) (bits & 511u) + (int64_t) sidx * drow;
    col = (int64_t) d.col0 + (int64_t) sidx * dcol;
    if (slot && *slot != SPX_NO_SLOT) *slot = (uint32_t)((int64_t) *slot + (int64_t) sidx * dcol);
}

// row (relative to the row-block) and first column of lane l of a pass of 8x8 tiles (SPX_PASS_SYMTILE): lanes
// 8t .. 8t + 7 are the rows of tile t, every lane covers the tile's eight columns
inline void tile_lane(const GpuStream &s, const SpxRowBlock &rb, const SpxPass &ps, uint32_t l,
                      int64_t &row, int64_t &col)
{
    const SpxUnitDesc &d = s.descs[(size_t) rb.desc_off + ps.rank0 + (l >> 3)];
    row = (int64_t) ps.elem0 + (int64_t) (d.bits & 511u) + (l & 7u);
    col = (int64_t) d.col0;
}

// column of leftover e of a gather pass (through L2, or from the x window)
inline int64_t gather_col(const GpuStream &s, const SpxRowBlock &rb, const SpxPass &ps, size_t e)
{
    if (ps.kind == SPX_PASS_GATHER_LDS) {
        uint16_t v;
        std::memcpy(&v, s.cidx.data() + ((size_t) rb.cidx_off + rb.near_off) * 16u + e * 2, 2);
        return (int64_t) rb.xwin_base + v;
    }
    const uint8_t *c = s.cidx.data() + (size_t) rb.cidx_off * 16u;
    if (rb.cidx_width == 4) {
        uint32_t v;
        std::memcpy(&v, c + e * 4, 4);
        return (int64_t) rb.cbase + v;
    }
    uint16_t v;
    std::memcpy(&v, c + e * 2, 2);
    if (rb.cidx_width == 3) return (int64_t) rb.cbase + (v | ((uint32_t) c[(size_t) rb.hi_off * 16u + e] << 16));
    return (int64_t) rb.cbase + v;
}

inline bool is_gather(const SpxPass &ps)
{
    return ps.kind == SPX_PASS_GATHER || ps.kind == SPX_PASS_GATHER_LDS;
}

}  // namespace spx
