// spmv_device.hpp -- device code shared by the kernels of the CSX interpreter (spmv_kernels.hip: the
// general and the symmetric kernels; spmv_mv_kernels.hip: K vectors per pass over the stream;
// spmv_xw_kernels.hip: the general kernel with the unit windows of x in LDS): the pieces of a pass -- one
// lane per row segment, values interleaved, x gathered through L2 or read from the row-block's LDS
// window -- and their composition for one vector and for K.  The kernel arguments and the launchers:
// spmv_launch.hpp.
//
// Semantics restated from the reference's SpMV templates (src/templates/csx_spmv_tmpl.c:66-101 and the
// per-unit bodies delta/horiz/vert/diag/rdiag/block_row/block_col _tmpl.c).
#pragma once

#include "gpu_format.h"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// Loads of the matrix stream (values, descriptors): plain loads.  (Marking them non-temporal, so that
// they would not push x out of the L2, measured slower on every workload: profiles/r03/ablation.md
// section 4, profiles/r05/xw_nontemporal_raw.md; the experiment hook is gone, the record stays.)
typedef double spx_d2_t __attribute__((ext_vector_type(2)));
// two doubles at any 8-byte aligned address as ONE load (global_load_dwordx4 needs no 16-byte
// alignment on gfx9): the x of a row segment comes in pairs wherever its first column lies
typedef double spx_d2u_t __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ double2 ld_stream(const double2 *p) { return *p; }
__device__ __forceinline__ double ld_stream(const double *p) { return *p; }
__device__ __forceinline__ uint2 ld_stream(const uint2 *p) { return *p; }
// (the float twin of the values, spx.gpu.values_f32: the same loads at half the width)
typedef float spx_f2u_t __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ float2 ld_stream(const float2 *p) { return *p; }
__device__ __forceinline__ float ld_stream(const float *p) { return *p; }
// The type of the stream's values, V: double, or float for the products that read the float twin
// (csx_spmv_f32_kernel and its kin: StreamArgs::values then POINTS AT FLOATS, element for element the array
// of doubles).  Values widen in registers; every product and sum is fp64 whatever V is.
template <class V> struct ValueVec;
template <> struct ValueVec<double> { typedef double2 pair; typedef spx_d2u_t pair_u; };
template <> struct ValueVec<float> { typedef float2 pair; typedef spx_f2u_t pair_u; };
// a value that has no twin (the diagonal and the thin mirror list of a symmetric stream: at most one per row), as
// the product with values of type V sees it: rounded to V in registers, to nearest even
template <class V>
__device__ __forceinline__ double stored_as(double d) { return (double) (V) d; }
#define SPX_LD_INDEX(expr) (expr)

// set bits of `mask` in lanes 1..lane (bit 0 is never set by the emitter)
__device__ __forceinline__ uint32_t starts_upto(uint64_t mask, int lane)
{
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
    return below + (uint32_t)((mask >> lane) & 1ull);
}

// ---- the pieces of a pass of the plain stream, one pass at a time ------------------------------------
// A pass of width W gives lane l one row segment of W consecutive columns (unit pass), or a piece of one
// row's leftover nonzeros, each with a column offset of its own (gather pass, G: SPX_PASS_GATHER 1,
// SPX_PASS_GATHER_LDS 2).  The single-vector and the K-vector interpreter below are compositions of these.

template <int W, class V = double>
struct PassValues {
    typename ValueVec<V>::pair v2[W / 2 > 0 ? W / 2 : 1];
    V v1;
};

// The index load of pass `ps` into q (uint2) and goff (uint32_t[G ? W : 1]).  G: the lane's row comes from the
// row-block's u16 rows (q.x) and the column offsets of its nonzeros from cidx (element-major [W][nseg]; 16, 24
// or 32 bits wide; G == 2: u16 offsets into the row-block's x window); else q is the lane's unit descriptor
// {first column, bits}, found by ranking the pass' segment-start mask, or the header's copy of the pass'
// only one.  `l`: the lane, 0 for idle ones (they shadow lane 0).
// (A macro, expanded in the two compositions below: as a function -- with a struct or with q and goff by
// reference, returning by value, templated on the arguments or on plain pointers, for one pass or for all B
// -- it cost every K-vector kernel three to seven VGPRs and with them a wavefront per SIMD:
// profiles/r08/REFACTOR.md.)
#define SPX_LOAD_INDEX(W, G, a, rb, ps, active, l, lane, q, goff)                                                      \
    do {                                                                                                               \
        const uint32_t nseg_ = (ps).nseg;                                                                              \
        if (G) {                                                                                                       \
            (q).x = SPX_LD_INDEX((a).segrows[(rb).seg_off + (ps).seg0 + (l)]);                                         \
            const uint8_t *cidx = (a).cidx + ((size_t) (rb).cidx_off + (G == 2 ? (rb).near_off : 0u)) * 16u;           \
            const uint32_t e0 = (ps).elem0 + (l);                                                                      \
            if (G == 1 && (rb).cidx_width == 4) {                                                                      \
                _Pragma("unroll")                                                                                      \
                for (int w = 0; w < W; ++w)                                                                            \
                    (goff)[w] = SPX_LD_INDEX(reinterpret_cast<const uint32_t *>(cidx)[e0 + (uint32_t) w * nseg_]);     \
            } else if (G == 1 && (rb).cidx_width == 3) {                                                               \
                /* 24-bit offsets: the low halves, then (array of its own) the high bytes */                           \
                const uint8_t *hi = cidx + (size_t) (rb).hi_off * 16u;                                                 \
                _Pragma("unroll")                                                                                      \
                for (int w = 0; w < W; ++w) {                                                                          \
                    const uint32_t e = e0 + (uint32_t) w * nseg_;                                                      \
                    (goff)[w] = (uint32_t) SPX_LD_INDEX(reinterpret_cast<const uint16_t *>(cidx)[e]) |                 \
                                ((uint32_t) SPX_LD_INDEX(hi[e]) << 16);                                                \
                }                                                                                                      \
            } else {                                                                                                   \
                _Pragma("unroll")                                                                                      \
                for (int w = 0; w < W; ++w)                                                                            \
                    (goff)[w] = SPX_LD_INDEX(reinterpret_cast<const uint16_t *>(cidx)[e0 + (uint32_t) w * nseg_]);     \
            }                                                                                                          \
        } else if ((ps).flags & SPX_PASSF_INLINE) {                                                                    \
            /* the pass' only descriptor came with its header (wave-uniform, in SGPRs) */                              \
            (q).x = (uint32_t) (ps).mask;                                                                              \
            (q).y = (uint32_t) ((ps).mask >> 32);                                                                      \
        } else {                                                                                                       \
            const uint64_t mk = ((ps).flags & SPX_PASSF_INLINE) ? 0ull : (ps).mask;                                    \
            const uint32_t rank = (uint32_t) (ps).rank0 + ((active) ? starts_upto(mk, lane) : 0u);                     \
            (q) = ld_stream(reinterpret_cast<const uint2 *>((a).descs + (rb).desc_off + rank));                        \
        }                                                                                                              \
    } while (0)

// the value load: interleaved pairs, 16 bytes per lane and load (floats: 8)
template <int W, class V = double>
__device__ __forceinline__ PassValues<W, V> load_values(const StreamArgs &a, const SpxRowBlock &rb, const SpxPass &ps, uint32_t l)
{
    PassValues<W, V> v;
    const uint32_t nseg = ps.nseg;
    const V *vals = reinterpret_cast<const V *>(a.values) + rb.val_off + ps.val_off;
#pragma unroll
    for (int p = 0; p < W / 2; ++p)
        v.v2[p] = ld_stream(reinterpret_cast<const typename ValueVec<V>::pair *>(vals + (uint32_t) p * 2u * nseg + l * 2u));
    if (W & 1) v.v1 = ld_stream(vals + (uint32_t) (W / 2) * 2u * nseg + l);
    return v;
}

// the value store (csx_scale_values_kernel): what load_values read, back to where it lay -- 16 bytes per lane and
// pair (floats: 8).  `values`: the array of doubles, or its float twin.  `len` (a piece of a gather pass): the
// positions len .. W - 1 of the lane are padding and keep their bits
template <int W, class V = double>
__device__ __forceinline__ void store_values(V *values, const SpxRowBlock &rb, const SpxPass &ps, uint32_t l,
                                             const PassValues<W, V> &v, int len = W)
{
    const uint32_t nseg = ps.nseg;
    V *vals = values + rb.val_off + ps.val_off;
#pragma unroll
    for (int p = 0; p < W / 2; ++p) {
        V *dst = vals + (uint32_t) p * 2u * nseg + l * 2u;
        if (2 * p + 1 < len) *reinterpret_cast<typename ValueVec<V>::pair *>(dst) = v.v2[p];
        else if (2 * p < len) dst[0] = v.v2[p].x;
    }
    if ((W & 1) && W - 1 < len) vals[(uint32_t) (W / 2) * 2u * nseg + l] = v.v1;
}

// the values of a pass as doubles (V = double: as they are): the members load_values wrote, W / 2 pairs and the
// odd last one
template <int W, class V>
__device__ __forceinline__ PassValues<W> widened(const PassValues<W, V> &v)
{
    PassValues<W> d;
#pragma unroll
    for (int p = 0; p < W / 2; ++p) {
        d.v2[p].x = (double) v.v2[p].x;
        d.v2[p].y = (double) v.v2[p].y;
    }
    if (W & 1) d.v1 = (double) v.v1;
    return d;
}

// descriptor bits -> where segment `seg` of the row-block (only its low 16 bits count) lies: its row in the
// row-block (`row0`: the first row of the pass' part of it, SpxPass::elem0) and its first column, as an
// offset from the unit's first column
struct UnitOrigin {
    int row, dcol;
};
__device__ __forceinline__ UnitOrigin unit_origin(uint32_t bits, uint32_t seg, uint32_t row0)
{
    // segment index inside its unit, then its row / first column
    const int s = (int) ((seg - ((bits >> 9) & 8191u)) & 0xffffu);
    const uint32_t kind = (bits >> 22) & 7u;
    const int step = (int) (bits >> 25);
    const int drow = kind == SPX_KIND_BLOCK ? 1 : (kind >= SPX_KIND_VERT ? step : 0);
    const int dcol = (kind == SPX_KIND_HORIZ || kind == SPX_KIND_DIAG)
                         ? step : (kind == SPX_KIND_ADIAG ? -step : 0);
    UnitOrigin o;
    o.row = (int) (row0 + (bits & 511u)) + s * drow;
    o.dcol = s * dcol;
    return o;
}

// x of a gather pass, from memory or from a staged window (`xp`: what the offsets count from)
// (a piece shorter than the pass is padded: nothing is multiplied there)
template <int W, int N>
__device__ __forceinline__ void gather_x(const double *xp, const uint32_t (&goff)[N], int len, double (&x)[W])
{
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const double xv = xp[goff[N == W ? w : 0]];          // (N == 1 < W: a unit pass, never gathered)
        x[w] = w < len ? xv : 0.0;
    }
}

// x of a unit pass: W consecutive doubles from xp on.
// The x loads cost address-unit issue slots like the value loads do: they come in pairs
// at any alignment, W / 2 + (W & 1) load instructions instead of W.  (One full-width load
// per diagonal stack with the other W - 1 columns taken from the neighbouring lanes by
// DPP shifts was built and measured slower: profiles/r03/ablation.md section 6.)
template <int W>
__device__ __forceinline__ void load_x(const double *xp, double (&x)[W])
{
    if (W >= 2) {
        const spx_d2u_t *xp2 = reinterpret_cast<const spx_d2u_t *>(xp);
#pragma unroll
        for (int p = 0; p < W / 2; ++p) {
            const spx_d2u_t xx = xp2[p];
            x[2 * p] = xx.x;
            x[2 * p + 1] = xx.y;
        }
        if (W & 1) x[W - 1] = xp[W - 1];
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = xp[w];
    }
}

// the lane's partial sum: W fused multiply-adds, in column order
template <int W, class V>
__device__ __forceinline__ double dot(const PassValues<W, V> &v, const double (&x)[W])
{
    double t = 0.0;
#pragma unroll
    for (int p = 0; p < W / 2; ++p) {
        t = fma((double) v.v2[p].x, x[2 * p], t);
        t = fma((double) v.v2[p].y, x[2 * p + 1], t);
    }
    if (W & 1) t = fma((double) v.v1, x[W - 1], t);
    return t;
}

// a chunk of one over-long row (a gather pass of a row-block of one row): every lane targets the same
// element of the tile, so the wavefront sums what its lanes hold and adds once
__device__ __forceinline__ void wave_add(double *p, double t, int lane)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
    if (lane == 0) atomicAdd(p, t);
}

// ---- the interpreter: B passes of the same width at once ---------------------------------------------
// All index loads go out first, then all value loads, then the x gathers: one memory round trip per stage
// for the whole batch instead of one per pass.  `win`: the row-block's x window in LDS (SPX_PASS_GATHER_LDS).

// one vector.  (Row, x and dot product pass by pass: decoding all passes first and then applying them, the
// K-vector order below, costs the single-vector kernels five to eight VGPRs: profiles/r08/REFACTOR.md.)
template <int W, int B, int G, int K = 1, class V = double>
__device__ __forceinline__ void unit_passes(const KernelArgs &a, const SpxRowBlock &rb,
                                            const SpxPass (&ps)[B], double *tile,
                                            const double *win, int lane)
{
    bool active[B];
    uint32_t l[B];
    uint2 q[B];
    uint32_t goff[B][G ? W : 1];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        active[b] = (uint32_t) lane < (uint32_t) ps[b].nseg;
        l[b] = active[b] ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0
        SPX_LOAD_INDEX(W, G, a, rb, ps[b], active[b], l[b], lane, q[b], goff[b]);
    }
    PassValues<W, V> v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) v[b] = load_values<W, V>(a, rb, ps[b], l[b]);
    int row[B];
    double acc[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        double x[W];
        if (G == 2) {
            row[b] = (int) SPX_SEGROW_ROW(q[b].x);
            gather_x(win, goff[b], (int) SPX_SEGROW_LEN(q[b].x), x);
        } else if (G) {
            row[b] = (int) SPX_SEGROW_ROW(q[b].x);
            gather_x(a.x + rb.cbase, goff[b], (int) SPX_SEGROW_LEN(q[b].x), x);
        } else {
            const UnitOrigin o = unit_origin(q[b].y, ps[b].seg0 + l[b], ps[b].elem0);
            row[b] = o.row;
            load_x(a.x + (q[b].x + (uint32_t) o.dcol), x);
        }
        acc[b] = dot<W, V>(v[b], x);
    }
    if (G == 1 && rb.n_rows == 1) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) t += active[b] ? acc[b] : 0.0;
        wave_add(tile, t, lane);
        return;
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
        if (active[b]) atomicAdd(&tile[row[b]], acc[b]);
}

// K vectors (column-major: vector j of x at a.x + j * a.ldx): index and values once, then for every vector
// its x, the dot products and the adds to ITS y tile (vector j at tile + j * n_rows).  `win`: the K staged x
// windows (vector j at win + j * xwin_len) where MvArgs::stage says so, else the SPX_PASS_GATHER_LDS offsets
// gather through L2 relative to xwin_base.  V: the type of the values, as in the single-vector composition.
template <int W, int B, int G, int K, class V = double>
__device__ __forceinline__ void unit_passes(const MvArgs &a, const SpxRowBlock &rb, const SpxPass (&ps)[B],
                                            double *tile, const double *win, int lane)
{
    bool active[B];
    uint32_t l[B];
    uint2 q[B];
    uint32_t goff[B][G ? W : 1];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        active[b] = (uint32_t) lane < (uint32_t) ps[b].nseg;
        l[b] = active[b] ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0
        SPX_LOAD_INDEX(W, G, a, rb, ps[b], active[b], l[b], lane, q[b], goff[b]);
    }
    // (widened once, in front of the K vectors: every vector multiplies with the same doubles)
    PassValues<W> v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) v[b] = widened<W, V>(load_values<W, V>(a, rb, ps[b], l[b]));
    // the lane's row and where its x lies: the same for every vector of the group
    int row[B], len[B];
    uint32_t col[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if (G) {
            row[b] = (int) SPX_SEGROW_ROW(q[b].x);
            len[b] = (int) SPX_SEGROW_LEN(q[b].x);
            col[b] = G == 2 ? rb.xwin_base : rb.cbase;
        } else {
            const UnitOrigin o = unit_origin(q[b].y, ps[b].seg0 + l[b], ps[b].elem0);
            row[b] = o.row;
            col[b] = q[b].x + (uint32_t) o.dcol;
            len[b] = W;
        }
    }
    const bool staged = G == 2 && a.stage;
    const int n_rows = rb.n_rows;
    for (int j = 0; j < K; ++j) {
        const double *xj = a.x + (size_t) j * a.ldx;
        double acc[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            double x[W];
            if (G && staged) {
                const double *wj = win + (size_t) j * rb.xwin_len;
                gather_x(wj, goff[b], len[b], x);
            } else if (G) {
                const double *xp = xj + col[b];
                gather_x(xp, goff[b], len[b], x);
            } else {
                const double *xp = xj + col[b];
                load_x(xp, x);
            }
            // (dot() written out: called here, in any form, it costs the K = 8 kernels 35 more SGPR spills,
            // 92 -> 127 -- profiles/r08/REFACTOR.md)
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < W / 2; ++p) {
                t = fma(v[b].v2[p].x, x[2 * p], t);
                t = fma(v[b].v2[p].y, x[2 * p + 1], t);
            }
            if (W & 1) t = fma(v[b].v1, x[W - 1], t);
            acc[b] = t;
        }
        double *tj = tile + j * n_rows;
        if (G == 1 && rb.n_rows == 1) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < B; ++b) t += active[b] ? acc[b] : 0.0;
            wave_add(tj, t, lane);
        } else {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (active[b]) atomicAdd(&tj[row[b]], acc[b]);
        }
    }
}

// B passes of one kind, by their width (wave-uniform)
template <int B, int G, int K = 1, class V = double, class Args>
__device__ __forceinline__ void run_units(const Args &a, const SpxRowBlock &rb,
                                          const SpxPass (&ps)[B], double *tile, const double *win,
                                          int lane)
{
    switch (ps[0].width) {         // wave-uniform
    case 1: unit_passes<1, B, G, K, V>(a, rb, ps, tile, win, lane); break;
    case 2: unit_passes<2, B, G, K, V>(a, rb, ps, tile, win, lane); break;
    case 3: unit_passes<3, B, G, K, V>(a, rb, ps, tile, win, lane); break;
    case 4: unit_passes<4, B, G, K, V>(a, rb, ps, tile, win, lane); break;
    case 5: unit_passes<5, 1, G, K, V>(a, rb, {ps[0]}, tile, win, lane);
            if (B > 1) unit_passes<5, 1, G, K, V>(a, rb, {ps[B - 1]}, tile, win, lane);
            break;
    case 6: unit_passes<6, 1, G, K, V>(a, rb, {ps[0]}, tile, win, lane);
            if (B > 1) unit_passes<6, 1, G, K, V>(a, rb, {ps[B - 1]}, tile, win, lane);
            break;
    case 7: unit_passes<7, 1, G, K, V>(a, rb, {ps[0]}, tile, win, lane);
            if (B > 1) unit_passes<7, 1, G, K, V>(a, rb, {ps[B - 1]}, tile, win, lane);
            break;
    default: unit_passes<8, 1, G, K, V>(a, rb, {ps[0]}, tile, win, lane);
            if (B > 1) unit_passes<8, 1, G, K, V>(a, rb, {ps[B - 1]}, tile, win, lane);
            break;
    }
}

// one pass on its own
template <int K = 1, class V = double, class Args>
__device__ __forceinline__ void run_pass(const Args &a, const SpxRowBlock &rb,
                                         const SpxPass &ps, double *tile, const double *win, int lane)
{
    if (ps.kind == SPX_PASS_GATHER) run_units<1, 1, K, V>(a, rb, {ps}, tile, win, lane);
    else if (ps.kind == SPX_PASS_GATHER_LDS) run_units<1, 2, K, V>(a, rb, {ps}, tile, win, lane);
    else run_units<1, 0, K, V>(a, rb, {ps}, tile, win, lane);
}

// a wavefront's round of two passes, side by side when they have the same shape (they mostly do: passes
// are sorted by width), so that their loads overlap
__device__ __forceinline__ bool same_shape(const SpxPass &p0, const SpxPass &p1)
{
    return p0.kind == p1.kind && p0.width == p1.width;
}
template <int K = 1, class V = double, class Args>
__device__ __forceinline__ void run_pair(const Args &a, const SpxRowBlock &rb, const SpxPass (&ps)[2],
                                         double *tile, const double *win, int lane)
{
    if (ps[0].kind == SPX_PASS_GATHER) run_units<2, 1, K, V>(a, rb, ps, tile, win, lane);
    else if (ps[0].kind == SPX_PASS_GATHER_LDS) run_units<2, 2, K, V>(a, rb, ps, tile, win, lane);
    else run_units<2, 0, K, V>(a, rb, ps, tile, win, lane);
}

// ---- pass headers as six dwords (the pipelined kernels: spmv_xw_kernels.hip, spmv_sx_kernels.hip) ----
// Read through the constant address space -- the stream is never written while a product runs, and only so
// does the compiler keep fetching them with scalar loads once a kernel contains LDS DMA -- and as whole
// dwords: a byte field read on its own becomes a VECTOR byte load (gfx950 has no scalar one).
typedef const __attribute__((address_space(4))) uint32_t *spx_const_words_t;
struct PassWords {
    uint32_t w[6];
    __device__ __forceinline__ uint64_t mask() const { return (uint64_t) w[0] | ((uint64_t) w[1] << 32); }
    __device__ __forceinline__ uint32_t val_off() const { return w[2]; }
    __device__ __forceinline__ uint32_t rank0() const { return w[3] & 0xffffu; }
    __device__ __forceinline__ uint32_t seg0() const { return w[3] >> 16; }
    __device__ __forceinline__ uint32_t nseg() const { return w[4] & 0xffu; }
    __device__ __forceinline__ uint32_t width() const { return (w[4] >> 8) & 0xffu; }
    __device__ __forceinline__ uint32_t kind() const { return (w[4] >> 16) & 0xffu; }
    __device__ __forceinline__ uint32_t flags() const { return w[4] >> 24; }
    __device__ __forceinline__ SpxPass pass() const
    {
        SpxPass ps;
        ps.mask = mask(); ps.val_off = w[2]; ps.rank0 = (uint16_t) rank0(); ps.seg0 = (uint16_t) seg0();
        ps.nseg = (uint8_t) nseg(); ps.width = (uint8_t) width(); ps.kind = (uint8_t) kind();
        ps.flags = (uint8_t) flags(); ps.elem0 = w[5];
        return ps;
    }
};
static_assert(sizeof(SpxPass) == 24 && offsetof(SpxPass, val_off) == 8 && offsetof(SpxPass, rank0) == 12 &&
              offsetof(SpxPass, seg0) == 14 && offsetof(SpxPass, nseg) == 16 && offsetof(SpxPass, width) == 17 &&
              offsetof(SpxPass, kind) == 18 && offsetof(SpxPass, flags) == 19 && offsetof(SpxPass, elem0) == 20,
              "PassWords mirrors SpxPass");
__device__ __forceinline__ PassWords load_pass(spx_const_words_t passes, int index)
{
    const spx_const_words_t p = passes + 6 * index;
    PassWords h;
#pragma unroll
    for (int k = 0; k < 6; ++k) h.w[k] = p[k];
    return h;
}

// the pass headers of the row-block in LDS (the workgroup copies them there in its prologue: one coalesced
// load instead of a scalar load from memory per pass and wavefront): entry `index` as six dwords, the same
// for every lane, then into SGPRs
__device__ __forceinline__ PassWords lds_pass(const uint32_t *hdr, int index)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(hdr + 6 * index);
    const uint2 a = p[0], b = p[1], c = p[2];
    PassWords h;
    h.w[0] = (uint32_t) __builtin_amdgcn_readfirstlane((int) a.x);
    h.w[1] = (uint32_t) __builtin_amdgcn_readfirstlane((int) a.y);
    h.w[2] = (uint32_t) __builtin_amdgcn_readfirstlane((int) b.x);
    h.w[3] = (uint32_t) __builtin_amdgcn_readfirstlane((int) b.y);
    h.w[4] = (uint32_t) __builtin_amdgcn_readfirstlane((int) c.x);
    h.w[5] = (uint32_t) __builtin_amdgcn_readfirstlane((int) c.y);
    return h;
}

// a pass that is not there (the second half of a round at the end of a wavefront's list): the first
// one's addresses, no lanes
__device__ __forceinline__ PassWords no_pass(const PassWords &like)
{
    PassWords h = like;
    h.w[4] &= ~0xffu;
    return h;
}

#define SPX_KERNEL_PARAMS                                                                        \
    const SpxRowBlock *rbs_, const SpxPass *passes_, uint32_t n_rb_, uint32_t pass_stride_,      \
    XcdSplit xcd_split, const double *values_, const SpxUnitDesc *descs_, \
    const uint8_t *cidx_, const uint16_t *segrows_, const double *x_, double *y_,               \
    double *carry_, const double *dvalues_, double *spill_, const uint32_t *slot_col_,         \
    double alpha_, double beta_, const double *dvalues_priv_, double beta_priv_
#define SPX_KERNEL_ARGS(a)                                                                       \
    KernelArgs a;                                                                                \
    a.rbs = rbs_; a.passes = passes_; a.n_rb = n_rb_; a.pass_stride = pass_stride_;              \
    a.values = values_; a.descs = descs_; a.cidx = cidx_; a.segrows = segrows_; a.x = x_;        \
    a.y = y_; a.carry = carry_; a.dvalues = dvalues_; a.spill = spill_; a.slot_col = slot_col_;  \
    a.alpha = alpha_; a.dvalues_priv = dvalues_priv_; a.beta_priv = beta_priv_;                  \
    a.beta = beta_; a.xw_tab = nullptr

}  // namespace spx
