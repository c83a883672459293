// sym_scale_kernels.hip -- the matrix where it lies, one pass over the stream of a SYMMETRIC tune: the scaling that
// keeps it symmetric, A <- D * A * D in place (csx_sym_scale_kernel), and the norms of its rows, which are those of
// its columns (csx_sym_norms_kernel); launched by device_mat_sym_scale and device_mat_sym_norms in
// device_runtime.cpp.
//
// Launch shape of scale_kernels.hip: one workgroup per row-block in the XCD-aware order, wavefront w takes the
// passes w, w + WAVES, ...; the PLAIN pass headers and descriptors, whatever kernel family the product runs.  A
// symmetric stream holds an off-diagonal entry either twice -- the lower copy and its mirror image, in unit and
// gather passes (or the thin mirror list of a row slice) -- or ONCE, in a pass of 8x8 tiles (SPX_PASS_SYMTILE) or
// of read-once row segments (SPX_PASS_SYMSEG), decoded here as spmv_sym_device.hpp decodes them.  The diagonal
// lies in an array of its own (dvalues); a position of a pass with row == column is the zero a dense block holds
// where it closes over the diagonal, and an exact zero inside a tile pass is a cell the matrix need not hold:
// neither is counted or rewritten.
#include "spmv_sym_device.hpp"

#include <cstddef>
#include <cstdint>

namespace spx {

// which kind of pass a lane decodes: a unit pass, the two gather passes (G of SPX_LOAD_INDEX), tiles, read-once
// row segments
enum : int { SYM_UNIT = 0, SYM_GATHER = 1, SYM_GATHER_LDS = 2, SYM_TILE = 3, SYM_SEG = 4 };

// what a lane of a pass covers: its row inside the row-block, the length of its piece, its first column (the W
// columns follow each other) or its W column offsets (gather passes, from `cbase`), and, read-once segments, the
// slot of its first column (SPX_NO_SLOT: none)
template <int W, int P>
struct SymLane {
    int row, len;
    uint32_t col, slot;
    uint32_t goff[(P == SYM_GATHER || P == SYM_GATHER_LDS) ? W : 1];
};

template <int W, int P, class Args>
__device__ __forceinline__ SymLane<W, P> sym_lane(const Args &a, const SpxRowBlock &rb, const SpxPass &ps, bool active,
                                                  uint32_t l, int lane)
{
    SymLane<W, P> s;
    s.len = W;
    s.col = 0;
    s.slot = SPX_NO_SLOT;
    if (P == SYM_GATHER || P == SYM_GATHER_LDS) {
        uint2 q;
        if (P == SYM_GATHER) SPX_LOAD_INDEX(W, 1, a, rb, ps, active, l, lane, q, s.goff);
        else SPX_LOAD_INDEX(W, 2, a, rb, ps, active, l, lane, q, s.goff);
        s.row = (int) SPX_SEGROW_ROW(q.x);
        s.len = (int) SPX_SEGROW_LEN(q.x);
        s.col = P == SYM_GATHER_LDS ? rb.xwin_base : rb.cbase;
    } else if (P == SYM_TILE) {
        // the tile's descriptor {col0, row0 | slot << 9}; lanes 8t .. 8t + 7 are the rows of tile t
        const uint2 q = *reinterpret_cast<const uint2 *>(a.descs + rb.desc_off + ps.rank0 + (l >> 3));
        s.row = (int) (ps.elem0 + (q.y & 511u)) + (int) (l & 7u);
        s.col = q.x;
        s.slot = q.y >> 9;
    } else if (P == SYM_SEG) {
        // two descriptors per unit, the second holds the slot of segment 0's first column
        uint2 q;
        uint32_t slot0;
        if (ps.flags & SPX_PASSF_INLINE) {
            q.x = (uint32_t) ps.mask;
            q.y = (uint32_t) (ps.mask >> 32);
            slot0 = a.descs[rb.desc_off + (uint32_t) ps.rank0 + 1u].col0;
        } else {
            const uint32_t rank = (uint32_t) ps.rank0 + 2u * (active ? starts_upto(ps.mask, lane) : 0u);
            q = ld_stream(reinterpret_cast<const uint2 *>(a.descs + rb.desc_off + rank));
            slot0 = a.descs[rb.desc_off + rank + 1u].col0;
        }
        const UnitOrigin o = unit_origin(q.y, ps.seg0 + l, ps.elem0);
        s.row = o.row;
        s.col = q.x + (uint32_t) o.dcol;
        s.slot = slot0 != SPX_NO_SLOT ? slot0 + (uint32_t) o.dcol : SPX_NO_SLOT;
    } else {
        uint2 q;
        SPX_LOAD_INDEX(W, 0, a, rb, ps, active, l, lane, q, s.goff);
        const UnitOrigin o = unit_origin(q.y, ps.seg0 + l, ps.elem0);
        s.row = o.row;
        s.col = q.x + (uint32_t) o.dcol;
    }
    return s;
}

template <int W, int P>
__device__ __forceinline__ uint32_t sym_column(const SymLane<W, P> &s, int w)
{
    return (P == SYM_GATHER || P == SYM_GATHER_LDS) ? s.col + s.goff[w] : s.col + (uint32_t) w;
}

template <int W>
__device__ __forceinline__ void unpack(const PassValues<W> &v, double (&x)[W])
{
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        x[2 * k] = v.v2[k].x;
        x[2 * k + 1] = v.v2[k].y;
    }
    if (W & 1) x[W - 1] = v.v1;
}

// ---- D * A * D ---------------------------------------------------------------------------------------------
// The arithmetic is fixed: fl(fl(d[max(r,c)] * a) * d[min(r,c)]), two IEEE multiplications in this order (there is
// no sum behind them that could take one in as an fma), so that a mirror image gets the bits of its lower copy.
// `rt`: d of the row-block's rows.  Idle lanes shadow lane 0 and store nothing; the positions len .. W - 1 of a
// gather piece and the padding of a pass keep their bits; a position on the diagonal and a zero of a tile are
// stored back as they were read.
template <int W, int P>
__device__ __forceinline__ void sym_scale_pass(const SymScaleArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                               const double *rt, int lane)
{
    const bool active = (uint32_t) lane < (uint32_t) ps.nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;
    const SymLane<W, P> s = sym_lane<W, P>(a, rb, ps, active, l, lane);
    PassValues<W> v = load_values<W>(a, rb, ps, l);
    double c[W];
    if (P == SYM_GATHER || P == SYM_GATHER_LDS) gather_x(a.d + s.col, s.goff, s.len, c);
    else load_x(a.d + s.col, c);
    const double r = rt[s.row];
    const uint32_t grow = rb.row0 + (uint32_t) s.row;
    double x[W];
    unpack<W>(v, x);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t col = sym_column<W, P>(s, w);
        const bool lower = grow >= col;
        const double t = ((lower ? r : c[w]) * x[w]) * (lower ? c[w] : r);
        const bool keep = col == grow || (P == SYM_TILE && x[w] == 0.0);
        x[w] = keep ? x[w] : t;
    }
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        v.v2[k].x = x[2 * k];
        v.v2[k].y = x[2 * k + 1];
    }
    if (W & 1) v.v1 = x[W - 1];
    if (!active) return;
    store_values<W>(a.values_rw, rb, ps, l, v, s.len);
    if (a.values_f32) {       // (kernel-uniform) the twin's layout is the doubles', element for element
        PassValues<W, float> f;
#pragma unroll
        for (int k = 0; k < W / 2; ++k) {
            f.v2[k].x = (float) v.v2[k].x;        // round to nearest even, as csx_narrow_values_kernel narrows
            f.v2[k].y = (float) v.v2[k].y;
        }
        if (W & 1) f.v1 = (float) v.v1;
        store_values<W, float>(a.values_f32, rb, ps, l, f, s.len);
    }
}

template <int P>
__device__ __forceinline__ void sym_scale_width(const SymScaleArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                                const double *rt, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 1: sym_scale_pass<1, P>(a, rb, ps, rt, lane); break;
    case 2: sym_scale_pass<2, P>(a, rb, ps, rt, lane); break;
    case 3: sym_scale_pass<3, P>(a, rb, ps, rt, lane); break;
    case 4: sym_scale_pass<4, P>(a, rb, ps, rt, lane); break;
    case 5: sym_scale_pass<5, P>(a, rb, ps, rt, lane); break;
    case 6: sym_scale_pass<6, P>(a, rb, ps, rt, lane); break;
    case 7: sym_scale_pass<7, P>(a, rb, ps, rt, lane); break;
    default: sym_scale_pass<8, P>(a, rb, ps, rt, lane); break;
    }
}

// LDS: d of the row-block's rows
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_sym_scale_kernel(SymScaleArgs a, XcdSplit xs)
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
    {
        const int n_rows = rb.n_rows;
        const double *src = a.d + rb.row0;
        for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) rt[i] = src[i];
        __syncthreads();
    }
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += WAVES) {
        const SpxPass ps = passes[t];
        if (ps.kind == SPX_PASS_SYMTILE) sym_scale_pass<8, SYM_TILE>(a, rb, ps, rt, lane);
        else if (ps.kind == SPX_PASS_SYMSEG) sym_scale_width<SYM_SEG>(a, rb, ps, rt, lane);
        else if (ps.kind == SPX_PASS_GATHER) sym_scale_width<SYM_GATHER>(a, rb, ps, rt, lane);
        else if (ps.kind == SPX_PASS_GATHER_LDS) sym_scale_width<SYM_GATHER_LDS>(a, rb, ps, rt, lane);
        else sym_scale_width<SYM_UNIT>(a, rb, ps, rt, lane);
    }
}

// what has no place in the row-blocks: the diagonal of the own rows, a(i,i) <- fl(fl(d[i] * a) * d[i]), and the thin
// mirror list of a row slice, entry k of row t at (mirror_rows[t], mirror_col[k]) above the diagonal.  Thread i < n_own
// takes own row i, thread n_own + t mirror row t.
__global__ void csx_sym_scale_rest_kernel(double *dvalues, size_t own_lo, size_t n_own, const uint32_t *mrows,
                                          const uint32_t *mptr, const uint32_t *mcol, double *mval, uint32_t n_mirror,
                                          const double *d)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_own) {
        const double di = d[own_lo + i];
        dvalues[own_lo + i] = (di * dvalues[own_lo + i]) * di;
    } else if (i - n_own < n_mirror) {
        const uint32_t t = (uint32_t) (i - n_own);
        const double dr = d[mrows[t]];
        for (uint32_t k = mptr[t]; k < mptr[t + 1]; ++k) {
            const uint32_t c = mcol[k];
            const double dc = d[c];
            const bool lower = mrows[t] >= c;
            mval[k] = ((lower ? dr : dc) * mval[k]) * (lower ? dc : dr);
        }
    }
}

void launch_sym_scale(int waves, unsigned blocks, size_t lds_bytes, void *stream_, const SymScaleArgs &a, const XcdSplit &xs)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (waves == 2) hipLaunchKernelGGL((csx_sym_scale_kernel<2>), dim3(blocks), dim3(128), lds_bytes, stream, a, xs);
    else if (waves == 8) hipLaunchKernelGGL((csx_sym_scale_kernel<8>), dim3(blocks), dim3(512), lds_bytes, stream, a, xs);
    else hipLaunchKernelGGL((csx_sym_scale_kernel<4>), dim3(blocks), dim3(256), lds_bytes, stream, a, xs);
}

void launch_sym_scale_rest(void *stream, double *dvalues, size_t own_lo, size_t n_own, const uint32_t *mrows,
                           const uint32_t *mptr, const uint32_t *mcol, double *mval, uint32_t n_mirror, const double *d)
{
    const size_t n = n_own + n_mirror;
    if (!n) return;
    hipLaunchKernelGGL(csx_sym_scale_rest_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), dvalues, own_lo, n_own, mrows, mptr, mcol, mval, n_mirror, d);
}

// ---- norms -----------------------------------------------------------------------------------------------------
// what one stored value contributes, and how two contributions combine.  The maximum of non-negative doubles is
// the unsigned maximum of their bit patterns (in LDS: ds_max_u64).
template <int KIND>
__device__ __forceinline__ double sym_term(double v)
{
    return KIND == NORM_SUM_SQ ? v * v : fabs(v);
}
template <int KIND>
__device__ __forceinline__ double sym_join(double s, double t)
{
    return KIND == NORM_MAX_ABS ? fmax(s, t) : s + t;
}
template <int KIND>
__device__ __forceinline__ void sym_atomic(double *p, double t)
{
    if (KIND == NORM_MAX_ABS)
        atomicMax(reinterpret_cast<unsigned long long *>(p), (unsigned long long) __double_as_longlong(t));
    else
        atomicAdd(p, t);
}

// One pass.  `lds`: the row-block's transposed-sum slots, then (slot n_slots + i is own row i) its rows.  The
// lane's W terms join into one for its row.  A value that the stream holds once also counts for its column: in the
// column's slot -- a tile's eight lanes first join their columns in registers, as the product does, so that each
// adds one of them -- or, a read-once segment without slots, straight in `out`.  A value stored twice counts for
// the row of each copy and needs nothing more: no global atomic per stored value.  Padding is never read into a
// result, a position on the diagonal contributes nothing (the diagonal array is joined in by the init pass).
template <int KIND, int W, int P>
__device__ __forceinline__ void sym_norms_pass(const SymNormArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                               double *lds, int lane)
{
    const bool active = (uint32_t) lane < (uint32_t) ps.nseg;
    const uint32_t l = active ? (uint32_t) lane : 0u;
    const SymLane<W, P> s = sym_lane<W, P>(a, rb, ps, active, l, lane);
    const PassValues<W> v = load_values<W>(a, rb, ps, l);
    const uint32_t grow = rb.row0 + (uint32_t) s.row;
    double x[W], t[W];
    unpack<W>(v, x);
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const bool counts = w < s.len && sym_column<W, P>(s, w) != grow;
        t[w] = counts ? sym_term<KIND>(x[w]) : 0.0;
        sum = sym_join<KIND>(sum, t[w]);
    }
    double *tile = lds + rb.n_slots;
    if (P == SYM_TILE) {
        // (W == 8) the columns of the tile over its eight lanes: exchanges with lane ^ 4, ^ 2, ^ 1, after which lane i
        // of the tile holds column i.  Whole idle tiles shadow tile 0 among themselves and are kept from adding.
        const int i = (int) (l & 7u);
        double p4[4], p2[2], cs;
        {
            const bool hi = (i & 4) != 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const double send = hi ? t[w] : t[(w + 4) % W];
                const double keep = hi ? t[(w + 4) % W] : t[w];
                p4[w] = sym_join<KIND>(keep, xchg4(send));
            }
        }
        {
            const bool hi = (i & 2) != 0;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const double send = hi ? p4[w] : p4[w + 2];
                const double keep = hi ? p4[w + 2] : p4[w];
                p2[w] = sym_join<KIND>(keep, xchg2(send));
            }
        }
        {
            const bool hi = (i & 1) != 0;
            const double send = hi ? p2[0] : p2[1];
            const double keep = hi ? p2[1] : p2[0];
            cs = sym_join<KIND>(keep, xchg1(send));
        }
        if (active) {
            sym_atomic<KIND>(&tile[s.row], sum);
            sym_atomic<KIND>(&lds[s.slot + (uint32_t) i], cs);
        }
        return;
    }
    if (!active) return;
    sym_atomic<KIND>(&tile[s.row], sum);
    if (P == SYM_SEG) {
        // (two branches, so that the slot side keeps its address space: ds_add_f64 / ds_max_u64, not flat atomics)
        if (s.slot != SPX_NO_SLOT) {
            double *sl = lds + s.slot;
#pragma unroll
            for (int w = 0; w < W; ++w) sym_atomic<KIND>(&sl[w], t[w]);
        } else {
            double *op = a.out + s.col;
#pragma unroll
            for (int w = 0; w < W; ++w) sym_atomic<KIND>(&op[w], t[w]);
        }
    }
}

template <int KIND, int P>
__device__ __forceinline__ void sym_norms_width(const SymNormArgs &a, const SpxRowBlock &rb, const SpxPass &ps,
                                                double *lds, int lane)
{
    switch (ps.width) {            // wave-uniform
    case 1: sym_norms_pass<KIND, 1, P>(a, rb, ps, lds, lane); break;
    case 2: sym_norms_pass<KIND, 2, P>(a, rb, ps, lds, lane); break;
    case 3: sym_norms_pass<KIND, 3, P>(a, rb, ps, lds, lane); break;
    case 4: sym_norms_pass<KIND, 4, P>(a, rb, ps, lds, lane); break;
    case 5: sym_norms_pass<KIND, 5, P>(a, rb, ps, lds, lane); break;
    case 6: sym_norms_pass<KIND, 6, P>(a, rb, ps, lds, lane); break;
    case 7: sym_norms_pass<KIND, 7, P>(a, rb, ps, lds, lane); break;
    default: sym_norms_pass<KIND, 8, P>(a, rb, ps, lds, lane); break;
    }
}

// LDS: the row-block's n_slots transposed-sum slots, then its n_rows rows.  Both go to `out` with global atomics
// on top of the init pass, one per row and one per slot: the rows at row0 + i, slot i at column
// slot_col[spill_off / 8 + i / 8] + i % 8.
template <int KIND, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_sym_norms_kernel(SymNormArgs a, XcdSplit xs)
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
    const int n_rows = rb.n_rows, n_slots = rb.n_slots;
    for (int i = threadIdx.x; i < n_slots + n_rows; i += BLOCK_THREADS) lds_dyn[i] = 0.0;
    __syncthreads();
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += WAVES) {
        const SpxPass ps = passes[t];
        if (ps.kind == SPX_PASS_SYMTILE) sym_norms_pass<KIND, 8, SYM_TILE>(a, rb, ps, lds_dyn, lane);
        else if (ps.kind == SPX_PASS_SYMSEG) sym_norms_width<KIND, SYM_SEG>(a, rb, ps, lds_dyn, lane);
        else if (ps.kind == SPX_PASS_GATHER) sym_norms_width<KIND, SYM_GATHER>(a, rb, ps, lds_dyn, lane);
        else if (ps.kind == SPX_PASS_GATHER_LDS) sym_norms_width<KIND, SYM_GATHER_LDS>(a, rb, ps, lds_dyn, lane);
        else sym_norms_width<KIND, SYM_UNIT>(a, rb, ps, lds_dyn, lane);
    }
    __syncthreads();
    double *dst = a.out + rb.row0;
    for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) sym_atomic<KIND>(&dst[i], lds_dyn[n_slots + i]);
    if (n_slots) {
        const uint32_t *gcol = a.slot_col + (rb.spill_off >> 3);
        for (int i = threadIdx.x; i < n_slots; i += BLOCK_THREADS)
            sym_atomic<KIND>(&a.out[(size_t) gcol[i >> 3] + (i & 7)], lds_dyn[i]);
    }
}

// the init pass: out[i] = the term of the diagonal on the own rows, +0.0 on every other element of the n
template <int KIND>
__global__ void csx_sym_norms_init_kernel(double *out, size_t n, const double *dvalues, size_t own_lo, size_t own_hi)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (i >= own_lo && i < own_hi) ? sym_term<KIND>(dvalues[i]) : 0.0;
}

// the thin mirror list of a row slice: every entry counts for its row (a row of another process)
template <int KIND>
__global__ void csx_sym_norms_mirror_kernel(double *out, const uint32_t *mrows, const uint32_t *mptr, const double *mval,
                                            uint32_t n_mirror)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_mirror) return;
    double s = 0.0;
    for (uint32_t k = mptr[t]; k < mptr[t + 1]; ++k) s = sym_join<KIND>(s, sym_term<KIND>(mval[k]));
    sym_atomic<KIND>(&out[mrows[t]], s);
}

template <int KIND>
static void sym_norms_launches(int waves, unsigned blocks, size_t lds_bytes, hipStream_t stream, const SymNormArgs &a,
                               const XcdSplit &xs)
{
    if (waves == 2) hipLaunchKernelGGL((csx_sym_norms_kernel<KIND, 2>), dim3(blocks), dim3(128), lds_bytes, stream, a, xs);
    else if (waves == 8) hipLaunchKernelGGL((csx_sym_norms_kernel<KIND, 8>), dim3(blocks), dim3(512), lds_bytes, stream, a, xs);
    else hipLaunchKernelGGL((csx_sym_norms_kernel<KIND, 4>), dim3(blocks), dim3(256), lds_bytes, stream, a, xs);
}

void launch_sym_norms(int kind, int waves, unsigned blocks, size_t lds_bytes, void *stream_, const SymNormArgs &a,
                      const XcdSplit &xs)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (kind == NORM_SUM_ABS) sym_norms_launches<NORM_SUM_ABS>(waves, blocks, lds_bytes, stream, a, xs);
    else if (kind == NORM_SUM_SQ) sym_norms_launches<NORM_SUM_SQ>(waves, blocks, lds_bytes, stream, a, xs);
    else sym_norms_launches<NORM_MAX_ABS>(waves, blocks, lds_bytes, stream, a, xs);
}

void launch_sym_norms_init(int kind, void *stream_, double *out, size_t n, const double *dvalues, size_t own_lo,
                           size_t own_hi, const uint32_t *mrows, const uint32_t *mptr, const double *mval, uint32_t n_mirror)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 g((unsigned) ((n + 255) / 256)), gm((n_mirror + 255) / 256), b(256);
#define SPX_LAUNCH_I(K)                                                                                              \
    do {                                                                                                             \
        if (n) hipLaunchKernelGGL(csx_sym_norms_init_kernel<K>, g, b, 0, stream, out, n, dvalues, own_lo, own_hi);   \
        if (n_mirror) hipLaunchKernelGGL(csx_sym_norms_mirror_kernel<K>, gm, b, 0, stream, out, mrows, mptr, mval, n_mirror); \
    } while (0)
    if (kind == NORM_SUM_ABS) SPX_LAUNCH_I(NORM_SUM_ABS);
    else if (kind == NORM_SUM_SQ) SPX_LAUNCH_I(NORM_SUM_SQ);
    else SPX_LAUNCH_I(NORM_MAX_ABS);
#undef SPX_LAUNCH_I
}

// dynamic LDS beyond the default 64 KB (wide row-blocks: 8192 slots + 2048 rows); on the current device, so every
// upload that needs it asks, as with spmv_allow_lds
void sym_norms_allow_lds(size_t bytes)
{
#define SPX_ALLOW(K, W) \
    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(csx_sym_norms_kernel<K, W>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes)
    SPX_ALLOW(NORM_SUM_ABS, 2); SPX_ALLOW(NORM_SUM_ABS, 4); SPX_ALLOW(NORM_SUM_ABS, 8);
    SPX_ALLOW(NORM_SUM_SQ, 2); SPX_ALLOW(NORM_SUM_SQ, 4); SPX_ALLOW(NORM_SUM_SQ, 8);
    SPX_ALLOW(NORM_MAX_ABS, 2); SPX_ALLOW(NORM_MAX_ABS, 4); SPX_ALLOW(NORM_MAX_ABS, 8);
#undef SPX_ALLOW
}

}  // namespace spx
