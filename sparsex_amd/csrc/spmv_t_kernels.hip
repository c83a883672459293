// spmv_t_kernels.hip -- the transposed product of the general path, y <- y + alpha * A^T * x, over the stream
// that the forward kernels walk (csx_spmv_t_kernel; launched by device_spmv_trans in device_runtime.cpp on top
// of a pass that put beta * y there).
//
// Every stored nonzero a(r,c) contributes alpha * a * x[r] to y[c]: the scatter direction of the reference's
// symmetric bodies (src/templates/csx_sym_spmv_tmpl.c:60-106, `y[col] += value * x[row]`) applied to a general
// matrix.  A lane of a pass knows its row, its columns and its values exactly as in the forward product; what
// changes is that x is read by ROW -- the row-block's rows of x, times alpha, sit in LDS -- and that the W
// products of a lane go to W different elements of y, which other workgroups add to as well:
//  * XW launches (the device copy holds a window plan, xwindows.hpp): a unit pass of a row-block with unit
//    windows adds into those windows in LDS (ds_add_f64), and the workgroup hands every window to y once,
//    coalesced, with global atomics -- the atomic bytes of such a row-block are its staged doubles, not its
//    nonzeros;
//  * everything else -- unit passes of row-blocks without windows, gather passes -- adds to y with one global
//    atomic per nonzero.
// No y tile, no carry (there is no row sum: SPX_RB_SHARED row-blocks need nothing special), no write-out.
#include "spmv_device.hpp"

#include <cstddef>
#include <cstdint>

namespace spx {

// One pass.  G as in SPX_LOAD_INDEX (0: unit pass, 1: SPX_PASS_GATHER, 2: SPX_PASS_GATHER_LDS); LDS: the unit
// pass adds into the row-block's unit windows (its descriptors hold window offsets).  `xt`: alpha * x of the
// row-block's rows; `xw`: the unit windows.
template <int W, int G, bool LDS>
__device__ __forceinline__ void trans_pass(const TransArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                           const double *xt, double *xw, int lane)
{
    const bool active = (uint32_t) lane < (uint32_t) ps.nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0 (and add nothing)
    uint2 q;
    uint32_t goff[G ? W : 1];
    SPX_LOAD_INDEX(W, G, a, rb, ps, active, l, lane, q, goff);
    const PassValues<W> v = load_values<W>(a, rb, ps, l);
    int row, len = W;
    uint32_t col = 0;
    if (G) {
        row = (int) SPX_SEGROW_ROW(q.x);
        len = (int) SPX_SEGROW_LEN(q.x);
    } else {
        const UnitOrigin o = unit_origin(q.y, ps.seg0 + l, ps.elem0);
        row = o.row;
        col = q.x + (uint32_t) o.dcol;
    }
    const double xr = xt[row];
    double p[W];
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        p[2 * k] = v.v2[k].x * xr;
        p[2 * k + 1] = v.v2[k].y * xr;
    }
    if (W & 1) p[W - 1] = v.v1 * xr;
    if (!active) return;
    if (G) {
        // (a piece shorter than the pass is padded: nothing is added there)
        double *yp = a.y + (G == 2 ? rb.xwin_base : rb.cbase);
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < len) atomicAdd(&yp[goff[w]], p[w]);
    } else if (LDS) {
        double *dst = xw + (int) col;
#pragma unroll
        for (int w = 0; w < W; ++w) atomicAdd(&dst[w], p[w]);
    } else {
        double *yp = a.y + col;
#pragma unroll
        for (int w = 0; w < W; ++w) atomicAdd(&yp[w], p[w]);
    }
}

template <int G, bool LDS>
__device__ __forceinline__ void trans_width(const TransArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                            const double *xt, double *xw, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 1: trans_pass<1, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 2: trans_pass<2, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 3: trans_pass<3, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 4: trans_pass<4, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 5: trans_pass<5, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 6: trans_pass<6, G, LDS>(a, rb, ps, xt, xw, lane); break;
    case 7: trans_pass<7, G, LDS>(a, rb, ps, xt, xw, lane); break;
    default: trans_pass<8, G, LDS>(a, rb, ps, xt, xw, lane); break;
    }
}

// One workgroup per row-block, in the XCD-aware order of the forward kernels; wavefront w takes the passes
// w, w + WAVES, ...  XW: the launch reads the pass headers, descriptors and window table of the window plan.
// LDS: alpha * x of the row-block's rows, then (on an even offset) its unit windows.
template <int WAVES, bool XW>
__device__ __forceinline__ void spmv_body_t(const TransArgs &a, const XcdSplit &xs, double *lds)
{
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    const int n_rows = rb.n_rows;
    double *xt = lds;
    {
        const double *xsrc = a.x + rb.row0;
        for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) xt[i] = a.alpha * xsrc[i];
    }
    double *xw = lds + ((n_rows + 1) & ~1);
    // (entry 0 of the row-block's table: {pass range of the forward pipeline, doubles of unit windows})
    const XwEntry *tab = XW ? a.xw_tab + (size_t) rb_idx * XW_TAB : nullptr;
    const uint32_t xw_total = XW ? tab[0].off_len : 0u;
    if (XW)
        for (uint32_t i = threadIdx.x; i < xw_total; i += BLOCK_THREADS) xw[i] = 0.0;
    __syncthreads();

    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += WAVES) {
        const SpxPass ps = passes[t];
        if (ps.kind == SPX_PASS_GATHER) trans_width<1, false>(a, rb, ps, xt, xw, lane);
        else if (ps.kind == SPX_PASS_GATHER_LDS) trans_width<2, false>(a, rb, ps, xt, xw, lane);
        else if (XW && (ps.flags & SPX_PASSF_XLDS)) trans_width<0, true>(a, rb, ps, xt, xw, lane);
        else trans_width<0, false>(a, rb, ps, xt, xw, lane);
    }
    if (!XW) return;
    __syncthreads();

    // every window goes to y once: consecutive lanes, consecutive doubles
    for (uint32_t k = 0; k < XW_MAX; ++k) {
        const XwEntry e = tab[XW_RANGES + k];
        const uint32_t len = e.off_len >> 16, off = e.off_len & 0xffffu;
        if (len == 0) break;
        double *yp = a.y + e.base;
        for (uint32_t i = threadIdx.x; i < len; i += BLOCK_THREADS) atomicAdd(&yp[i], xw[off + i]);
    }
}

template <int WAVES, bool XW>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_t_kernel(TransArgs a, XcdSplit xcd_split)
{
    extern __shared__ double lds_dyn[];      // alpha * x of the row-block's rows, the unit windows
    spmv_body_t<WAVES, XW>(a, xcd_split, lds_dyn);
}

void launch_spmv_t(bool windows, int waves, unsigned blocks, size_t lds_bytes, void *stream_, const TransArgs &a,
                   const XcdSplit &xs)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
#define SPX_LAUNCH_T(W, X) hipLaunchKernelGGL((csx_spmv_t_kernel<W, X>), dim3(blocks), dim3(64 * W), lds_bytes, stream, a, xs)
    if (windows) {
        if (waves == 2) SPX_LAUNCH_T(2, true);
        else if (waves == 8) SPX_LAUNCH_T(8, true);
        else SPX_LAUNCH_T(4, true);
    } else {
        if (waves == 2) SPX_LAUNCH_T(2, false);
        else if (waves == 8) SPX_LAUNCH_T(8, false);
        else SPX_LAUNCH_T(4, false);
    }
#undef SPX_LAUNCH_T
}

// row-blocks whose windows need more than the default 64 KB of dynamic LDS
void spmv_t_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(&csx_spmv_t_kernel<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b);
    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(&csx_spmv_t_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b);
    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(&csx_spmv_t_kernel<8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

}  // namespace spx
