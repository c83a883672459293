// scale_kernels.hip -- the matrix where it lies, one pass over the stream of a general tune: diagonal scaling in
// place, A <- D_r * A * D_c (csx_scale_values_kernel), and row / column norms (csx_norms_kernel); launched by
// device_mat_scale and device_mat_norms in device_runtime.cpp.
//
// Both walk the stream as the transposed product does (spmv_body_t, spmv_t_kernels.hip): a lane of a pass knows its
// row, its columns and its values; one workgroup per row-block in the XCD-aware order, wavefront w takes the passes
// w, w + WAVES, ...; the plain pass headers and descriptors, so that every column slice and every row slice is
// covered by the launches of the forward product.  PETSc's MatDiagonalScale / MatGetRowMaxAbs / MatGetColumnNorms
// on a format that has neither a row pointer nor a column array.
#include "spmv_device.hpp"

#include <cstddef>
#include <cstdint>

namespace spx {

// ---- diagonal scaling --------------------------------------------------------------------------------------
// The arithmetic is fixed: fl(fl(dr[r] * a) * dc[c]), two IEEE multiplications in this order (there is no sum
// behind them that could take one in as an fma); a null vector's product is not formed.
template <bool DR, bool DC>
__device__ __forceinline__ double scaled(double a, double r, double c)
{
    double t = a;
    if (DR) t = r * t;
    if (DC) t = t * c;
    return t;
}

// One pass.  G as in SPX_LOAD_INDEX.  `rt`: dr of the row-block's rows (DR).  Idle lanes shadow lane 0 and store
// nothing; the positions len .. W - 1 of a gather piece and the padding of a pass keep their bits.
template <int W, int G, bool DR, bool DC>
__device__ __forceinline__ void scale_pass(const ScaleArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                           const double *rt, int lane)
{
    const bool active = (uint32_t) lane < (uint32_t) ps.nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0 (and store nothing)
    uint2 q;
    uint32_t goff[G ? W : 1];
    SPX_LOAD_INDEX(W, G, a, rb, ps, active, l, lane, q, goff);
    PassValues<W> v = load_values<W>(a, rb, ps, l);
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
    const double r = DR ? rt[row] : 1.0;
    double c[W];
    if (DC) {
        if (G) gather_x(a.dc + (G == 2 ? rb.xwin_base : rb.cbase), goff, len, c);
        else load_x(a.dc + col, c);
    }
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        v.v2[k].x = scaled<DR, DC>(v.v2[k].x, r, DC ? c[2 * k] : 1.0);
        v.v2[k].y = scaled<DR, DC>(v.v2[k].y, r, DC ? c[2 * k + 1] : 1.0);
    }
    if (W & 1) v.v1 = scaled<DR, DC>(v.v1, r, DC ? c[W - 1] : 1.0);
    if (!active) return;
    store_values<W>(a.values_rw, rb, ps, l, v, len);
    if (a.values_f32) {       // (kernel-uniform) the twin's layout is the doubles', element for element
        PassValues<W, float> f;
#pragma unroll
        for (int k = 0; k < W / 2; ++k) {
            f.v2[k].x = (float) v.v2[k].x;        // round to nearest even, as csx_narrow_values_kernel narrows
            f.v2[k].y = (float) v.v2[k].y;
        }
        if (W & 1) f.v1 = (float) v.v1;
        store_values<W, float>(a.values_f32, rb, ps, l, f, len);
    }
}

template <int G, bool DR, bool DC>
__device__ __forceinline__ void scale_width(const ScaleArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                            const double *rt, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 1: scale_pass<1, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 2: scale_pass<2, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 3: scale_pass<3, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 4: scale_pass<4, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 5: scale_pass<5, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 6: scale_pass<6, G, DR, DC>(a, rb, ps, rt, lane); break;
    case 7: scale_pass<7, G, DR, DC>(a, rb, ps, rt, lane); break;
    default: scale_pass<8, G, DR, DC>(a, rb, ps, rt, lane); break;
    }
}

// LDS: dr of the row-block's rows (DR)
template <int WAVES, bool DR, bool DC>
__global__ __launch_bounds__(64 * WAVES)
void csx_scale_values_kernel(ScaleArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    double *rt = lds_dyn;
    if (DR) {
        const int n_rows = rb.n_rows;
        const double *src = a.dr + rb.row0;
        for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) rt[i] = src[i];
        __syncthreads();
    }
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += WAVES) {
        const SpxPass ps = passes[t];
        if (ps.kind == SPX_PASS_GATHER) scale_width<1, DR, DC>(a, rb, ps, rt, lane);
        else if (ps.kind == SPX_PASS_GATHER_LDS) scale_width<2, DR, DC>(a, rb, ps, rt, lane);
        else scale_width<0, DR, DC>(a, rb, ps, rt, lane);
    }
}

void launch_scale_values(int waves, unsigned blocks, size_t lds_bytes, void *stream_, const ScaleArgs &a, const XcdSplit &xs)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool dr = a.dr != nullptr, dc = a.dc != nullptr;
#define SPX_LAUNCH_S(W, R, C) hipLaunchKernelGGL((csx_scale_values_kernel<W, R, C>), dim3(blocks), dim3(64 * W), lds_bytes, stream, a, xs)
#define SPX_LAUNCH_SW(W)                       \
    do {                                       \
        if (dr && dc) SPX_LAUNCH_S(W, true, true);    \
        else if (dr) SPX_LAUNCH_S(W, true, false);    \
        else SPX_LAUNCH_S(W, false, true);            \
    } while (0)
    if (waves == 2) SPX_LAUNCH_SW(2);
    else if (waves == 8) SPX_LAUNCH_SW(8);
    else SPX_LAUNCH_SW(4);
#undef SPX_LAUNCH_SW
#undef SPX_LAUNCH_S
}

// ---- norms -----------------------------------------------------------------------------------------------------
// what one stored value contributes, and how two contributions combine.  The maximum of non-negative doubles is
// the unsigned maximum of their bit patterns.
template <int KIND>
__device__ __forceinline__ double norm_term(double v)
{
    return KIND == NORM_SUM_SQ ? v * v : fabs(v);
}
template <int KIND>
__device__ __forceinline__ double norm_join(double s, double t)
{
    return KIND == NORM_MAX_ABS ? fmax(s, t) : s + t;
}
template <int KIND>
__device__ __forceinline__ void norm_atomic(double *p, double t)
{
    if (KIND == NORM_MAX_ABS)
        atomicMax(reinterpret_cast<unsigned long long *>(p), (unsigned long long) __double_as_longlong(t));
    else
        atomicAdd(p, t);
}

// One pass: the lane's W terms join into one for its row (`tile`: the row-block's rows in LDS, where a.rows is given) and go
// one by one to their columns (a.cols, or null).  Padding is never read into a result: idle lanes and the positions
// len .. W - 1 of a gather piece contribute nothing.
template <int KIND, int W, int G>
__device__ __forceinline__ void norms_pass(const NormArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                           double *tile, int lane)
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
    double t[W];
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        t[2 * k] = norm_term<KIND>(v.v2[k].x);
        t[2 * k + 1] = norm_term<KIND>(v.v2[k].y);
    }
    if (W & 1) t[W - 1] = norm_term<KIND>(v.v1);
    if (!active) return;
    if (a.rows) {
        double s = t[0];                  // (a piece holds at least one element)
#pragma unroll
        for (int w = 1; w < W; ++w)
            if (w < len) s = norm_join<KIND>(s, t[w]);
        norm_atomic<KIND>(&tile[row], s);
    }
    if (a.cols) {
        if (G) {
            double *cp = a.cols + (G == 2 ? rb.xwin_base : rb.cbase);
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < len) norm_atomic<KIND>(&cp[goff[w]], t[w]);
        } else {
            double *cp = a.cols + col;
#pragma unroll
            for (int w = 0; w < W; ++w) norm_atomic<KIND>(&cp[w], t[w]);
        }
    }
}

template <int KIND, int G>
__device__ __forceinline__ void norms_width(const NormArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                            double *tile, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 1: norms_pass<KIND, 1, G>(a, rb, ps, tile, lane); break;
    case 2: norms_pass<KIND, 2, G>(a, rb, ps, tile, lane); break;
    case 3: norms_pass<KIND, 3, G>(a, rb, ps, tile, lane); break;
    case 4: norms_pass<KIND, 4, G>(a, rb, ps, tile, lane); break;
    case 5: norms_pass<KIND, 5, G>(a, rb, ps, tile, lane); break;
    case 6: norms_pass<KIND, 6, G>(a, rb, ps, tile, lane); break;
    case 7: norms_pass<KIND, 7, G>(a, rb, ps, tile, lane); break;
    default: norms_pass<KIND, 8, G>(a, rb, ps, tile, lane); break;
    }
}

// LDS: the results of the row-block's rows (where a.rows is given).  They go to a.rows with global atomics, on
// top of the zero fill of the own rows: several row-blocks may hold parts of one row (SPX_RB_SHARED, the column
// slices of spx.gpu.col_phases).
template <int KIND, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_norms_kernel(NormArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    const int n_rows = rb.n_rows;
    double *tile = lds_dyn;
    if (a.rows) {       // (kernel-uniform)
        for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) tile[i] = 0.0;
        __syncthreads();
    }
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += WAVES) {
        const SpxPass ps = passes[t];
        if (ps.kind == SPX_PASS_GATHER) norms_width<KIND, 1>(a, rb, ps, tile, lane);
        else if (ps.kind == SPX_PASS_GATHER_LDS) norms_width<KIND, 2>(a, rb, ps, tile, lane);
        else norms_width<KIND, 0>(a, rb, ps, tile, lane);
    }
    if (!a.rows) return;
    __syncthreads();
    double *dst = a.rows + rb.row0;
    for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) norm_atomic<KIND>(&dst[i], tile[i]);
}

void launch_norms(int kind, int waves, unsigned blocks, size_t lds_bytes, void *stream_, const NormArgs &a, const XcdSplit &xs)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
#define SPX_LAUNCH_N(K, W) hipLaunchKernelGGL((csx_norms_kernel<K, W>), dim3(blocks), dim3(64 * W), lds_bytes, stream, a, xs)
#define SPX_LAUNCH_NW(K)                   \
    do {                                   \
        if (waves == 2) SPX_LAUNCH_N(K, 2);       \
        else if (waves == 8) SPX_LAUNCH_N(K, 8);  \
        else SPX_LAUNCH_N(K, 4);                  \
    } while (0)
    if (kind == NORM_SUM_ABS) SPX_LAUNCH_NW(NORM_SUM_ABS);
    else if (kind == NORM_SUM_SQ) SPX_LAUNCH_NW(NORM_SUM_SQ);
    else SPX_LAUNCH_NW(NORM_MAX_ABS);
#undef SPX_LAUNCH_NW
#undef SPX_LAUNCH_N
}

}  // namespace spx
