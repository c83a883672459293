// spmv_mv_kernels.hip -- the multi-vector product Y <- alpha*A*X + beta*Y for gfx950: K vectors per pass
// over the stream (K = 2, 4 or 8; one vector is the single-vector kernels' business).  The host side is
// device_spmm (device_runtime.cpp).
//
// The same interpreter as spmv_body (spmv_kernels.hip) over the PLAIN stream (passes, descs): a lane loads
// its descriptor or its gather offsets and its W values once, then for every vector j of the group gathers
// X_j[col .. col + W - 1], multiplies with the values it holds in registers and adds one partial sum to the
// y tile of vector j in LDS.  The write-out is per vector, coalesced, in the single-vector expression order.
// X and Y are column-major blocks: vector j of X at x + j * ldx, of Y at y + j * ldy.
//
// DET (spx.gpu.deterministic, or the launch tuner's tile per wavefront): a copy of the K tiles per
// wavefront, the passes taken by the wavefronts in the same order and pairs as csx_spmv_det_kernel, the
// copies summed in wavefront order: every column is bit-identical to the single-vector product.
#include "spmv_device.hpp"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// B passes of width W (unit_passes in spmv_device.hpp) for the K vectors of the group.  `tile`: the K y tiles
// of this wavefront (vector j at tile + j * n_rows); `win`: the K staged x windows (vector j at
// win + j * xwin_len) where MvArgs::stage says so, else the SPX_PASS_GATHER_LDS offsets gather through L2
// relative to xwin_base.
template <int W, int B, int G, int K>
__device__ __forceinline__ void mv_unit_passes(const MvArgs &a, const SpxRowBlock &rb, const SpxPass (&ps)[B],
                                               double *tile, int n_rows, const double *win, int lane)
{
    bool active[B];
    uint32_t l[B], nseg[B];
    uint2 q[B];
    uint32_t goff[B][G ? W : 1];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        nseg[b] = ps[b].nseg;
        active[b] = (uint32_t) lane < nseg[b];
        l[b] = active[b] ? (uint32_t) lane : 0u;         // idle lanes shadow lane 0
        if (G) {
            q[b].x = a.segrows[rb.seg_off + ps[b].seg0 + l[b]];
            const uint8_t *cidx = a.cidx + ((size_t) rb.cidx_off + (G == 2 ? rb.near_off : 0u)) * 16u;
            const uint32_t e0 = ps[b].elem0 + l[b];
            if (G == 1 && rb.cidx_width == 4) {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    goff[b][w] = reinterpret_cast<const uint32_t *>(cidx)[e0 + (uint32_t) w * nseg[b]];
            } else if (G == 1 && rb.cidx_width == 3) {
                const uint8_t *hi = cidx + (size_t) rb.hi_off * 16u;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t e = e0 + (uint32_t) w * nseg[b];
                    goff[b][w] = (uint32_t) reinterpret_cast<const uint16_t *>(cidx)[e] | ((uint32_t) hi[e] << 16);
                }
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    goff[b][w] = reinterpret_cast<const uint16_t *>(cidx)[e0 + (uint32_t) w * nseg[b]];
            }
        } else if (ps[b].flags & SPX_PASSF_INLINE) {
            q[b].x = (uint32_t) ps[b].mask;
            q[b].y = (uint32_t) (ps[b].mask >> 32);
        } else {
            const uint32_t rank = (uint32_t) ps[b].rank0 + (active[b] ? starts_upto(ps[b].mask, lane) : 0u);
            q[b] = ld_stream(reinterpret_cast<const uint2 *>(a.descs + rb.desc_off + rank));
        }
    }
    double2 v2[B][W / 2 > 0 ? W / 2 : 1];
    double v1[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const double *vals = a.values + rb.val_off + ps[b].val_off;
#pragma unroll
        for (int p = 0; p < W / 2; ++p)
            v2[b][p] = ld_stream(reinterpret_cast<const double2 *>(vals + (uint32_t) p * 2u * nseg[b] + l[b] * 2u));
        if (W & 1) v1[b] = ld_stream(vals + (uint32_t) (W / 2) * 2u * nseg[b] + l[b]);
    }
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
            const uint32_t bits = q[b].y;
            const int s = (int) ((ps[b].seg0 + l[b] - ((bits >> 9) & 8191u)) & 0xffffu);
            const uint32_t kind = (bits >> 22) & 7u;
            const int step = (int) (bits >> 25);
            const int drow = kind == SPX_KIND_BLOCK ? 1 : (kind >= SPX_KIND_VERT ? step : 0);
            const int dcol = (kind == SPX_KIND_HORIZ || kind == SPX_KIND_DIAG)
                                 ? step : (kind == SPX_KIND_ADIAG ? -step : 0);
            row[b] = (int) (ps[b].elem0 + (bits & 511u)) + s * drow;
            col[b] = q[b].x + (uint32_t) (s * dcol);
            len[b] = W;
        }
    }
    const bool staged = G == 2 && a.stage;
    for (int j = 0; j < K; ++j) {
        const double *xj = a.x + (size_t) j * a.ldx;
        double acc[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            double x[W];
            if (G && staged) {
                const double *wj = win + (size_t) j * rb.xwin_len;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const double xv = wj[goff[b][w]];
                    x[w] = w < len[b] ? xv : 0.0;
                }
            } else if (G) {
                const double *xp = xj + col[b];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const double xv = xp[goff[b][w]];
                    x[w] = w < len[b] ? xv : 0.0;
                }
            } else {
                const double *xp = xj + col[b];
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
                    x[0] = xp[0];
                }
            }
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < W / 2; ++p) {
                t = fma(v2[b][p].x, x[2 * p], t);
                t = fma(v2[b][p].y, x[2 * p + 1], t);
            }
            if (W & 1) t = fma(v1[b], x[W - 1], t);
            acc[b] = t;
        }
        double *tj = tile + j * n_rows;
        if (G == 1 && rb.n_rows == 1) {
            // a chunk of one over-long row: every lane targets tile_j[0]
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < B; ++b) t += active[b] ? acc[b] : 0.0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d);
            if (lane == 0) atomicAdd(&tj[0], t);
        } else {
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (active[b]) atomicAdd(&tj[row[b]], acc[b]);
        }
    }
}

template <int B, int G, int K>
__device__ __forceinline__ void mv_run_units(const MvArgs &a, const SpxRowBlock &rb, const SpxPass (&ps)[B],
                                             double *tile, int n_rows, const double *win, int lane)
{
    switch (ps[0].width) {         // wave-uniform; the same split as run_units
    case 1: mv_unit_passes<1, B, G, K>(a, rb, ps, tile, n_rows, win, lane); break;
    case 2: mv_unit_passes<2, B, G, K>(a, rb, ps, tile, n_rows, win, lane); break;
    case 3: mv_unit_passes<3, B, G, K>(a, rb, ps, tile, n_rows, win, lane); break;
    case 4: mv_unit_passes<4, B, G, K>(a, rb, ps, tile, n_rows, win, lane); break;
    case 5: mv_unit_passes<5, 1, G, K>(a, rb, {ps[0]}, tile, n_rows, win, lane);
            if (B > 1) mv_unit_passes<5, 1, G, K>(a, rb, {ps[B - 1]}, tile, n_rows, win, lane);
            break;
    case 6: mv_unit_passes<6, 1, G, K>(a, rb, {ps[0]}, tile, n_rows, win, lane);
            if (B > 1) mv_unit_passes<6, 1, G, K>(a, rb, {ps[B - 1]}, tile, n_rows, win, lane);
            break;
    case 7: mv_unit_passes<7, 1, G, K>(a, rb, {ps[0]}, tile, n_rows, win, lane);
            if (B > 1) mv_unit_passes<7, 1, G, K>(a, rb, {ps[B - 1]}, tile, n_rows, win, lane);
            break;
    default: mv_unit_passes<8, 1, G, K>(a, rb, {ps[0]}, tile, n_rows, win, lane);
            if (B > 1) mv_unit_passes<8, 1, G, K>(a, rb, {ps[B - 1]}, tile, n_rows, win, lane);
            break;
    }
}

template <int K>
__device__ __forceinline__ void mv_run_pass(const MvArgs &a, const SpxRowBlock &rb, const SpxPass &ps, double *tile,
                                            int n_rows, const double *win, int lane)
{
    if (ps.kind == SPX_PASS_GATHER) mv_run_units<1, 1, K>(a, rb, {ps}, tile, n_rows, win, lane);
    else if (ps.kind == SPX_PASS_GATHER_LDS) mv_run_units<1, 2, K>(a, rb, {ps}, tile, n_rows, win, lane);
    else mv_run_units<1, 0, K>(a, rb, {ps}, tile, n_rows, win, lane);
}

// One workgroup owns one row-block, as in spmv_body: LDS holds COPIES x K y tiles (copy c, vector j at
// (c * K + j) * n_rows), then the K x windows where they are staged.
// ACCUM (SPX_RB_ACCUM): the tiles are added to Y with global atomics on top of csx_mv_scale_kernel.
template <int K, int WAVES, bool ACCUM, bool DET>
__device__ __forceinline__ void mv_body(const MvArgs &a, const XcdSplit &xs, double *lds)
{
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    SpxPass p0 = passes[wave];
    SpxPass p1 = passes[wave + WAVES];                   // (the table is padded by one stride)
    const int n_rows = rb.n_rows;
    constexpr int COPIES = DET ? WAVES : 1;
    const int tiles = K * n_rows;                        // doubles per copy
    double *tile = lds + (DET ? wave * tiles : 0);
    for (int i = threadIdx.x; i < COPIES * tiles; i += BLOCK_THREADS) lds[i] = 0.0;
    double *win = lds + COPIES * tiles;
    if (a.stage) {
        const int xw = rb.xwin_len;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xs_j = a.x + (size_t) j * a.ldx + rb.xwin_base;
            for (int i = threadIdx.x; i < xw; i += BLOCK_THREADS) win[j * xw + i] = xs_j[i];
        }
    }
    __syncthreads();

    // wave w takes passes w, w + WAVES, ..., two at a time when they have the same shape (spmv_body's order)
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += 2 * WAVES) {
        const bool two = t + WAVES < n_pass;
        if (two) {
            if (p0.kind == p1.kind && p0.width == p1.width) {
                if (p0.kind == SPX_PASS_GATHER) mv_run_units<2, 1, K>(a, rb, {p0, p1}, tile, n_rows, win, lane);
                else if (p0.kind == SPX_PASS_GATHER_LDS) mv_run_units<2, 2, K>(a, rb, {p0, p1}, tile, n_rows, win, lane);
                else mv_run_units<2, 0, K>(a, rb, {p0, p1}, tile, n_rows, win, lane);
            } else {
                mv_run_pass<K>(a, rb, p0, tile, n_rows, win, lane);
                mv_run_pass<K>(a, rb, p1, tile, n_rows, win, lane);
            }
        } else {
            mv_run_pass<K>(a, rb, p0, tile, n_rows, win, lane);
        }
        if (t + 2 * WAVES < n_pass) {
            p0 = passes[t + 2 * WAVES];
            p1 = passes[t + 3 * WAVES];
        }
    }
    __syncthreads();
    if (DET) {
        // the wavefronts' copies, summed in wavefront order into the first one
        for (int i = threadIdx.x; i < tiles; i += BLOCK_THREADS) {
            double t = lds[i];
#pragma unroll
            for (int w = 1; w < COPIES; ++w) t += lds[w * tiles + i];
            lds[i] = t;
        }
        __syncthreads();
        tile = lds;
    }

    // ---------------- write the owned rows of every vector ------------------------------------
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x < K) a.carry[(size_t) threadIdx.x * a.n_carry + rb.carry_slot] = tile[threadIdx.x * n_rows];
    } else if (ACCUM) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) j * a.ldy + rb.row0 + i], a.alpha * tile[j * n_rows + i]);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xj = a.x + (size_t) j * a.ldx;
            double *yj = a.y + (size_t) j * a.ldy;
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) {
                const size_t g = (size_t) rb.row0 + i;
                double t = tile[j * n_rows + i];
                if (a.dvalues) t += a.dvalues[g] * xj[g];
                t *= a.alpha;
                if (a.beta != 0.0) t += a.beta * yj[g];
                yj[g] = t;
            }
        }
    }
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles, then the K x windows
    mv_body<K, WAVES, false, false>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_accum_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    mv_body<K, WAVES, true, false>(a, xs, lds_dyn);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_det_kernel(MvArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K y tiles per wavefront, then the K x windows
    mv_body<K, WAVES, false, true>(a, xs, lds_dyn);
}

// ---- the K-column forms of the steps around the row-block launches (blockIdx.y: the vector) ----------------

// rows split over several row-blocks: sum their partials (csx_fixup_kernel per vector)
__global__ void csx_mv_fixup_kernel(const SpxSharedRow *shared, uint32_t n_shared, const double *carry, uint32_t n_carry,
                                    double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                                    const double *x, size_t ldx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_shared) return;
    const size_t j = blockIdx.y;
    const SpxSharedRow sr = shared[i];
    const double *cj = carry + j * n_carry;
    double *yj = y + j * ldy;
    double s = dvalues ? dvalues[sr.row] * x[j * ldx + sr.row] : 0.0;
    for (uint32_t k = 0; k < sr.n_slots; ++k) s += cj[sr.first_slot + k];
    yj[sr.row] = (beta == 0.0) ? alpha * s : alpha * s + beta * yj[sr.row];
}

// column slices in one launch, first step: Y <- beta * Y on the rows [lo, hi)
__global__ void csx_mv_scale_kernel(double *y, size_t ldy, size_t lo, size_t hi, double beta)
{
    const size_t i = lo + (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    double *yj = y + (size_t) blockIdx.y * ldy;
    if (i < hi) yj[i] = beta == 0.0 ? 0.0 : beta * yj[i];
}

// symmetric path, first step: Y <- beta*Y + alpha*diag(A)*X on the owned rows, 0 elsewhere
__global__ void csx_mv_sym_init_kernel(double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                                       size_t first, size_t nrows, size_t own_lo, size_t own_hi, double alpha, double beta)
{
    const size_t i = first + (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    double *yj = y + (size_t) blockIdx.y * ldy;
    double v = 0.0;
    if (i >= own_lo && i < own_hi) {
        v = alpha * dvalues[i] * x[(size_t) blockIdx.y * ldx + i];
        if (beta != 0.0) v += beta * yj[i];
    }
    yj[i] = v;
}

// symmetric slice: the thin mirror image on rows of other processes (csx_sym_mirror_rows_kernel per vector)
__global__ void csx_mv_sym_mirror_rows_kernel(const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                                              const double *val, const double *x, size_t ldx, double *y, size_t ldy,
                                              double alpha, uint32_t n)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double *xj = x + (size_t) blockIdx.y * ldx;
    double s = 0.0;
    for (uint32_t k = ptr[t]; k < ptr[t + 1]; ++k) s = fma(val[k], xj[col[k]], s);
    y[(size_t) blockIdx.y * ldy + rows[t]] = alpha * s;
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*MvKernel)(MvArgs, XcdSplit);

template <int K, int WAVES>
static MvKernel mv_kernel(MvFamily family)
{
    switch (family) {
    case MvFamily::accum: return csx_spmv_mv_accum_kernel<K, WAVES>;
    case MvFamily::det: return csx_spmv_mv_det_kernel<K, WAVES>;
    case MvFamily::plain: break;
    }
    return csx_spmv_mv_kernel<K, WAVES>;
}

template <int K>
static MvKernel mv_kernel_w(MvFamily family, int waves)
{
    return waves == 2 ? mv_kernel<K, 2>(family) : waves == 8 ? mv_kernel<K, 8>(family) : mv_kernel<K, 4>(family);
}

static MvKernel mv_kernel_kw(MvFamily family, int K, int waves)
{
    return K == 8 ? mv_kernel_w<8>(family, waves) : K == 4 ? mv_kernel_w<4>(family, waves) : mv_kernel_w<2>(family, waves);
}

void launch_spmv_mv(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                    const XcdSplit &xs)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    hipLaunchKernelGGL(mv_kernel_kw(family, K, w), dim3(blocks), dim3(64 * w), lds_bytes, static_cast<hipStream_t>(stream),
                       a, xs);
}

void spmv_mv_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    for (MvFamily f : {MvFamily::plain, MvFamily::accum, MvFamily::det})
        for (int K : {2, 4, 8})
            for (int w : {2, 4, 8})
                (void) hipFuncSetAttribute(reinterpret_cast<const void *>(mv_kernel_kw(f, K, w)),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

void launch_mv_fixup(void *stream, int nvec, const SpxSharedRow *shared, uint32_t n_shared, const double *carry,
                     uint32_t n_carry, double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                     const double *x, size_t ldx)
{
    hipLaunchKernelGGL(csx_mv_fixup_kernel, dim3((n_shared + 63) / 64, (unsigned) nvec), dim3(64), 0,
                       static_cast<hipStream_t>(stream), shared, n_shared, carry, n_carry, y, ldy, alpha, beta, dvalues,
                       x, ldx);
}

void launch_mv_scale(void *stream, int nvec, double *y, size_t ldy, size_t lo, size_t hi, double beta)
{
    const int t = 256;
    hipLaunchKernelGGL(csx_mv_scale_kernel, dim3((unsigned)((hi - lo + t - 1) / t), (unsigned) nvec), dim3(t), 0,
                       static_cast<hipStream_t>(stream), y, ldy, lo, hi, beta);
}

void launch_mv_sym_init(void *stream, int nvec, double *y, size_t ldy, const double *x, size_t ldx,
                        const double *dvalues, size_t lo, size_t hi, size_t own_lo, size_t own_hi, double alpha,
                        double beta)
{
    const int t = 256;
    hipLaunchKernelGGL(csx_mv_sym_init_kernel, dim3((unsigned)((hi - lo + t - 1) / t), (unsigned) nvec), dim3(t), 0,
                       static_cast<hipStream_t>(stream), y, ldy, x, ldx, dvalues, lo, hi, own_lo, own_hi, alpha, beta);
}

void launch_mv_sym_mirror_rows(void *stream, int nvec, const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                               const double *val, const double *x, size_t ldx, double *y, size_t ldy, double alpha,
                               uint32_t n)
{
    hipLaunchKernelGGL(csx_mv_sym_mirror_rows_kernel, dim3((n + 255) / 256, (unsigned) nvec), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rows, ptr, col, val, x, ldx, y, ldy, alpha, n);
}

}  // namespace spx
