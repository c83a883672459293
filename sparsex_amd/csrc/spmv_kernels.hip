// spmv_kernels.hip -- the CSX interpreter for gfx950 (MI355X): its kernels and their launchers
// (spmv_launch.hpp).  The host side -- upload, the choice of kernel, the host-vector path -- is
// device_runtime.cpp.
//
// One workgroup walks one row-block of the descriptor stream (gpu_format.h).
// A pass is 64 row segments of equal width, one per lane: contiguous 16-byte
// per-lane reads of the interleaved values, the pass' segment-start mask
// ranked with mbcnt to find each lane's unit descriptor, strided decode of
// (row, first column), x gathered through L2, W fused multiply-adds per lane,
// one LDS add per lane into the row-block's y tile, and one coalesced write
// of the owned rows of y.  Leftover nonzeros (CSX delta units) run through the
// same code as gather passes: a lane owns up to 8 leftovers of one row, each
// with its own column offset.
//
// Semantics restated from the reference's SpMV templates
// (src/templates/csx_spmv_tmpl.c:66-101 and the per-unit bodies
// delta/horiz/vert/diag/rdiag/block_row/block_col _tmpl.c; symmetric:
// csx_sym_spmv_tmpl.c:60-106): every stored nonzero a(r,c) contributes
// alpha*a*x[c] to y[r]; on the symmetric path the stream also holds the mirror
// image of every stored unit, so a(r,c) contributes alpha*a*x[r] to y[c] too.
#include "hip_check.hpp"
#include "spmv_device.hpp"
#include "spmv_launch.hpp"
#include "spmv_sym_device.hpp"
#include "spx_abl.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

// One workgroup owns one row-block; its wavefronts take the passes in turn
// (wave w: passes w, w+4, ...) and accumulate into one y tile in LDS, which
// is written out (y = alpha*tile + beta*y) at the end.
// SYM: the symmetric variant with tiles (dynamic LDS: the row-block's
// transposed-sum slots in front of its y tile; the sums of columns owned by
// other row-blocks are spilled for csx_symfix_kernel).
// ATOMIC (symmetric tiles only): the row-block hands everything over with
// global_atomic_add_f64 -- its own rows (csx_sym_init_kernel has put beta*y and the
// diagonal term there) and, in aligned groups of eight, the transposed sums of
// the columns in front of it -- instead of spilling them for a second kernel.
//
// DET (spx.gpu.deterministic): every wavefront adds into a y tile (and slots) of its
// own, and the copies are summed in wavefront order before the write-out -- the
// only thing in this library whose order of additions is not fixed is the LDS adds
// of different wavefronts of a workgroup into the shared tile.
//
// V: the type of the values the passes load -- double, or float for the products on the
// float twin of the value array (spx.gpu.values_f32; a.values then points at floats).  Same loads at half the
// width, same element offsets, widened in registers: the FMAs, the tile and the write-out are fp64 either way.
// The diagonal of a symmetric stream has no twin: the float forms read its doubles and round them in registers
// (stored_as<V>), so that the product is that of the matrix whose EVERY stored entry is rounded to float.
template <bool SYM, bool ATOMIC, int WAVES_PER_BLOCK, bool DET = false, bool SEGS = false, bool TILES = true,
          class V = double>
__device__ __forceinline__ void spmv_body(const KernelArgs &a, const XcdSplit &xs,
                                          double *lds)
{
    constexpr int BLOCK_THREADS = 64 * WAVES_PER_BLOCK;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware order: workgroup b runs on XCD b % 8 and takes that XCD's next row-block
    // (the grid is 8 x the longest of the eight lists)
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    // the pass headers sit at a fixed stride, so the wave's first two are
    // fetched together with the row-block header, not after it
    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    SpxPass p0 = passes[wave];
    SpxPass p1 = passes[wave + WAVES_PER_BLOCK];         // (the table is padded by one stride)
    const int n_rows = rb.n_rows;
    const int n_slots = SYM ? (int) rb.n_slots : 0;
    const int core = n_slots + n_rows;                       // doubles per copy of slots + y tile
    constexpr int COPIES = DET ? WAVES_PER_BLOCK : 1;
    double *mine = lds + (DET ? wave * core : 0);            // this wavefront's slots, then its y tile
    double *tile = mine + n_slots;
    for (int i = threadIdx.x; i < COPIES * core; i += BLOCK_THREADS) lds[i] = 0.0;
    // the row-block's x window (leftovers whose columns lie close together gather
    // from LDS): staged once, coalesced
    double *win = lds + COPIES * core;
    {
        const int xw = rb.xwin_len;
        const double *xs = a.x + rb.xwin_base;
        for (int i = threadIdx.x; i < xw; i += BLOCK_THREADS) win[i] = xs[i];
    }
    // atomic hand-over: the first columns of the slot groups are fetched now, into LDS behind
    // the window, so that the hand-over at the end does not start with a load from memory
    // (a dependent L2/HBM round trip per 256 slots, at a point where the workgroup has
    // nothing else in flight)
    uint32_t *gcol_lds = reinterpret_cast<uint32_t *>(win + rb.xwin_len);
    if (ATOMIC) {
        const uint32_t *gcol = a.slot_col + (rb.spill_off >> 3);
        for (int i = threadIdx.x; i < (n_slots >> 3); i += BLOCK_THREADS) gcol_lds[i] = gcol[i];
    }
    __syncthreads();

    // wave w takes passes w, w + W, ..., two at a time when they have the same shape (they mostly
    // do: passes are sorted by width), so that their loads overlap
    const int n_pass = rb.n_pass;
    int t = wave;
    // (symmetric tiles: the tile passes at the head of the wavefront's list, one round trip each)
    if (SYM && TILES && !abl::sym_no_tile_run) symtile_run<WAVES_PER_BLOCK, V>(a, rb, passes, n_pass, t, p0, p1, mine, tile, lane);
    for (; t < n_pass; t += 2 * WAVES_PER_BLOCK) {
        const bool two = t + WAVES_PER_BLOCK < n_pass;
        if (SEGS && (p0.kind == SPX_PASS_SYMSEG || (two && p1.kind == SPX_PASS_SYMSEG))) {
            // read-once row segments (atomic hand-over only); whatever shares the round runs on its own
            if (two && p0.kind == SPX_PASS_SYMSEG && p1.kind == SPX_PASS_SYMSEG &&
                run_symseg2<V>(a, rb, p0, p1, mine, tile, lane)) {
                // (both done)
            } else {
                if (p0.kind == SPX_PASS_SYMSEG) run_symseg<V>(a, rb, p0, mine, tile, lane);
                else if (TILES && p0.kind == SPX_PASS_SYMTILE) symtile_pass<V>(a, rb, p0, mine, tile, lane);
                else run_pass<1, V>(a, rb, p0, tile, win, lane);
                if (two) {
                    if (p1.kind == SPX_PASS_SYMSEG) run_symseg<V>(a, rb, p1, mine, tile, lane);
                    else if (TILES && p1.kind == SPX_PASS_SYMTILE) symtile_pass<V>(a, rb, p1, mine, tile, lane);
                    else run_pass<1, V>(a, rb, p1, tile, win, lane);
                }
            }
        } else if (SYM && TILES && p0.kind == SPX_PASS_SYMTILE) {
            symtile_pass<V>(a, rb, p0, mine, tile, lane);
            if (two) {
                if (p1.kind == SPX_PASS_SYMTILE) symtile_pass<V>(a, rb, p1, mine, tile, lane);
                else run_pass<1, V>(a, rb, p1, tile, win, lane);
            }
        } else if (two) {
            if (same_shape(p0, p1)) {
                run_pair<1, V>(a, rb, {p0, p1}, tile, win, lane);
            } else {
                run_pass<1, V>(a, rb, p0, tile, win, lane);
                if (SYM && TILES && p1.kind == SPX_PASS_SYMTILE) symtile_pass<V>(a, rb, p1, mine, tile, lane);
                else run_pass<1, V>(a, rb, p1, tile, win, lane);
            }
        } else {
            run_pass<1, V>(a, rb, p0, tile, win, lane);
        }
        if (t + 2 * WAVES_PER_BLOCK < n_pass) {
            p0 = passes[t + 2 * WAVES_PER_BLOCK];
            p1 = passes[t + 3 * WAVES_PER_BLOCK];
        }
    }
    __syncthreads();
    if (DET) {
        // the wavefronts' copies, summed in wavefront order into the first one
        for (int i = threadIdx.x; i < core; i += BLOCK_THREADS) {
            double t = lds[i];
#pragma unroll
            for (int w = 1; w < COPIES; ++w) t += lds[w * core + i];
            lds[i] = t;
        }
        __syncthreads();
        tile = lds + n_slots;
    }

    // ---------------- write the owned rows ------------------------------------------------
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x == 0) a.carry[rb.carry_slot] = tile[0];
    } else if (ATOMIC) {
        if (abl::sym_no_own) {
            // (experiment build: the own rows stay where they are)
        } else if ((rb.flags & SPX_RB_PRIVATE) && a.dvalues_priv) {
            // nobody else adds to these rows (mark_private_rowblocks): stored, with the diagonal
            // term and beta * y; the init pass leaves them out
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) {
                const size_t g = (size_t) rb.row0 + i;
                double t = a.alpha * (tile[i] + stored_as<V>(a.dvalues_priv[g]) * a.x[g]);
                if (a.beta_priv != 0.0) t += a.beta_priv * a.y[g];
                a.y[g] = t;
            }
        } else {
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) rb.row0 + i], a.alpha * tile[i]);
        }
        if (!abl::sym_no_handover)
            for (int i = threadIdx.x; i < n_slots; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) gcol_lds[i >> 3] + (i & 7)], a.alpha * lds[i]);
    } else {
        for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS) {
            const size_t g = (size_t) rb.row0 + i;
            double t = tile[i];
            if (a.dvalues) t += stored_as<V>(a.dvalues[g]) * a.x[g];
            t *= a.alpha;
            if (a.beta != 0.0) t += a.beta * a.y[g];
            a.y[g] = t;
        }
    }
    if (SYM && !ATOMIC)
        for (int i = threadIdx.x; i < n_slots; i += BLOCK_THREADS) a.spill[rb.spill_off + i] = lds[i];
}


// (Individual scalar arguments, most urgent first, where the K-vector kernels take their MvArgs as one
// struct: these kernels are tuned to the register and to the order in which their arguments arrive, so the
// stream pointers that the two share (StreamArgs) are filled in one place on the host and spread here.
// Preloading them into SGPRs
// at wave launch -- hipcc -mllvm -amdgpu-kernarg-preload-count=16 -- was
// measured: it removes the kernarg fetch in front of the first real load but
// costs more at dispatch, cant 7.5 -> 8.0 us; not used.)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];      // y tile, then the x window
    spmv_body<false, false, WAVES>(a, xcd_split, lds_dyn);
}

// general path, column slices in one launch (SPX_RB_ACCUM): every row-block adds its y tile to
// y with global atomics (lanes of consecutive rows: 64-byte groups), on top of csx_scale_kernel
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_accum_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<false, true, WAVES>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, false, WAVES>(a, xcd_split, lds_dyn);
}

// the atomic hand-over kernel for streams that also hold read-once row segments
// (SPX_PASS_SYMSEG): a kernel of its own so that the tile-only one keeps its registers
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symseg_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES, false, true>(a, xcd_split, lds_dyn);
}

// ... and the same for streams with such segments and no tiles at all (a stencil matrix)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symseg_notile_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES, false, true, false>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_det_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];      // a y tile per wavefront, then the x window
    spmv_body<false, false, WAVES, true>(a, xcd_split, lds_dyn);
}

// ---- the general forms on the float twin of the values (spx_hip_matvec_kernel_f32) ----------------------
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<false, false, WAVES, false, false, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_accum_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<false, true, WAVES, false, false, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_det_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<false, false, WAVES, true, false, true, float>(a, xcd_split, lds_dyn);
}

// ---- ... and the symmetric forms: the stored triangle read once as floats, the diagonal rounded at the write-out
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, false, WAVES, false, false, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_atomic_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES, false, false, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symseg_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES, false, true, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symseg_notile_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES, false, true, false, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_det_f32_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, false, WAVES, true, false, true, float>(a, xcd_split, lds_dyn);
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_det_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, false, WAVES, true>(a, xcd_split, lds_dyn);
}

// (forcing eight wavefronts per SIMD on this kernel -- amdgpu_waves_per_eu(8, 8): 64 VGPRs and
// 32 B of scratch instead of 70 -- was measured on syn-nd24k: 25.5 -> 30.5 us; not used)
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_symtile_atomic_kernel(SPX_KERNEL_PARAMS)
{
    SPX_KERNEL_ARGS(a);
    extern __shared__ double lds_dyn[];
    spmv_body<true, true, WAVES>(a, xcd_split, lds_dyn);
}

// symmetric tiles, second step: every row collects the transposed sums that
// other row-blocks spilled for it (fixed order: deterministic).  A wavefront
// takes eight consecutive rows, lanes (g, r) = (lane >> 3, lane & 7): row r's
// entries g, g+8, ...  The eight columns of a tile are eight consecutive rows
// here with consecutive slots, so the eight lanes of a g read one 64-byte line.
// (Measured: one thread per row 16.4 us, this 9.1 us, a workgroup per eight
// rows 9.6 us on syn-nd24k -- the kernel is bound by its ~300 k scattered
// line requests, not by the depth of its loop.)
__global__ __launch_bounds__(256)
void csx_symfix_kernel(const uint32_t *fix_ptr, const uint32_t *fix_idx,
                       const double *spill, double *y, double alpha, uint32_t nrows)
{
    const uint32_t lane = threadIdx.x & 63u;
    // XCD-aware: workgroup b runs on XCD b % 8; each XCD takes one contiguous
    // eighth of the rows, so that the two halves of a 128-byte spill line (the
    // slots of two neighbouring tile columns) are asked for by the same L2
    const uint32_t blk = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const uint32_t row = (blk * 4u + (threadIdx.x >> 6)) * 8u + (lane & 7u);
    const uint32_t g = lane >> 3;
    double s = 0.0;
    if (row < nrows) {
        const uint32_t e = fix_ptr[row + 1];
        for (uint32_t k = fix_ptr[row] + g; k < e; k += 8u) s += spill[fix_idx[k]];
    }
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0 && row < nrows && s != 0.0) y[row] += alpha * s;
}

// ---- the steps around the row-block launches, for gridDim.y vectors at once (blockIdx.y: the vector; vector j
// of x at x + j * ldx, of y at y + j * ldy) ------------------------------------------------------------------

// rows split over several row-blocks: sum their partials (vector j's at carry + j * n_carry)
// (V, here and in the two steps of the symmetric path below: double, or float for the product on the float twin
// of the values -- the diagonal and the thin mirror list have no twin and are rounded in registers, stored_as<V>)
template <class V>
__device__ __forceinline__ void fixup_body(const SpxSharedRow *shared, uint32_t n_shared, const double *carry, uint32_t n_carry,
                                           double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                                           const double *x, size_t ldx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_shared) return;
    const size_t j = blockIdx.y;
    const SpxSharedRow sr = shared[i];
    const double *cj = carry + j * n_carry;
    double *yj = y + j * ldy;
    double s = dvalues ? stored_as<V>(dvalues[sr.row]) * x[j * ldx + sr.row] : 0.0;
    for (uint32_t k = 0; k < sr.n_slots; ++k) s += cj[sr.first_slot + k];
    yj[sr.row] = (beta == 0.0) ? alpha * s : alpha * s + beta * yj[sr.row];
}
__global__ void csx_fixup_kernel(const SpxSharedRow *shared, uint32_t n_shared, const double *carry, uint32_t n_carry,
                                 double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                                 const double *x, size_t ldx)
{
    fixup_body<double>(shared, n_shared, carry, n_carry, y, ldy, alpha, beta, dvalues, x, ldx);
}
__global__ void csx_fixup_f32_kernel(const SpxSharedRow *shared, uint32_t n_shared, const double *carry, uint32_t n_carry,
                                     double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                                     const double *x, size_t ldx)
{
    fixup_body<float>(shared, n_shared, carry, n_carry, y, ldy, alpha, beta, dvalues, x, ldx);
}

// column slices in one launch, first step: y <- beta * y on the rows [lo, hi)
__global__ void csx_scale_kernel(double *y, size_t ldy, size_t lo, size_t hi, double beta)
{
    const size_t i = lo + (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    double *yj = y + (size_t) blockIdx.y * ldy;
    if (i < hi) yj[i] = beta == 0.0 ? 0.0 : beta * yj[i];
}

// symmetric path, first step: y <- beta*y + alpha*diag(A)*x on the owned
// rows, 0 elsewhere (the main kernel then accumulates; on several GPUs the
// per-GPU vectors are summed afterwards)
template <class V>
__device__ __forceinline__ void sym_init_body(double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                                              size_t first, size_t nrows, size_t own_lo, size_t own_hi, double alpha, double beta)
{
    const size_t i = first + (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    double *yj = y + (size_t) blockIdx.y * ldy;
    double v = 0.0;
    if (i >= own_lo && i < own_hi) {
        v = alpha * stored_as<V>(dvalues[i]) * x[(size_t) blockIdx.y * ldx + i];
        if (beta != 0.0) v += beta * yj[i];
    }
    yj[i] = v;
}
__global__ void csx_sym_init_kernel(double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                                    size_t first, size_t nrows, size_t own_lo, size_t own_hi, double alpha, double beta)
{
    sym_init_body<double>(y, ldy, x, ldx, dvalues, first, nrows, own_lo, own_hi, alpha, beta);
}
__global__ void csx_sym_init_f32_kernel(double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                                        size_t first, size_t nrows, size_t own_lo, size_t own_hi, double alpha, double beta)
{
    sym_init_body<float>(y, ldy, x, ldx, dvalues, first, nrows, own_lo, own_hi, alpha, beta);
}

// symmetric slice: the thinly spread part of the mirror image on rows of other
// processes (GpuStream::mirror_*): one thread per such row, its few nonzeros in
// fixed order.  The rows are distinct and no row-block touches them.
template <class V>
__device__ __forceinline__ void sym_mirror_rows_body(const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                                                     const double *val, const double *x, size_t ldx, double *y, size_t ldy,
                                                     double alpha, uint32_t n)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double *xj = x + (size_t) blockIdx.y * ldx;
    double s = 0.0;
    for (uint32_t k = ptr[t]; k < ptr[t + 1]; ++k) s = fma(stored_as<V>(val[k]), xj[col[k]], s);
    y[(size_t) blockIdx.y * ldy + rows[t]] = alpha * s;          // (nothing else adds to these rows: no need to clear them first)
}
__global__ void csx_sym_mirror_rows_kernel(const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                                           const double *val, const double *x, size_t ldx, double *y, size_t ldy,
                                           double alpha, uint32_t n)
{
    sym_mirror_rows_body<double>(rows, ptr, col, val, x, ldx, y, ldy, alpha, n);
}
__global__ void csx_sym_mirror_rows_f32_kernel(const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                                               const double *val, const double *x, size_t ldx, double *y, size_t ldy,
                                               double alpha, uint32_t n)
{
    sym_mirror_rows_body<float>(rows, ptr, col, val, x, ldx, y, ldy, alpha, n);
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*SpmvKernel)(SPX_KERNEL_PARAMS);

template <int WAVES>
static SpmvKernel spmv_kernel(SpmvFamily family)
{
    switch (family) {
    case SpmvFamily::accum: return csx_spmv_accum_kernel<WAVES>;
    case SpmvFamily::symtile: return csx_spmv_symtile_kernel<WAVES>;
    case SpmvFamily::symtile_atomic: return csx_spmv_symtile_atomic_kernel<WAVES>;
    case SpmvFamily::symseg: return csx_spmv_symseg_kernel<WAVES>;
    case SpmvFamily::symseg_notile: return csx_spmv_symseg_notile_kernel<WAVES>;
    case SpmvFamily::det: return csx_spmv_det_kernel<WAVES>;
    case SpmvFamily::symtile_det: return csx_spmv_symtile_det_kernel<WAVES>;
    case SpmvFamily::plain: break;
    }
    return csx_spmv_kernel<WAVES>;
}

// the float twin's kernel of a family
template <int WAVES>
static SpmvKernel spmv_f32_kernel(SpmvFamily family)
{
    switch (family) {
    case SpmvFamily::accum: return csx_spmv_accum_f32_kernel<WAVES>;
    case SpmvFamily::symtile: return csx_spmv_symtile_f32_kernel<WAVES>;
    case SpmvFamily::symtile_atomic: return csx_spmv_symtile_atomic_f32_kernel<WAVES>;
    case SpmvFamily::symseg: return csx_spmv_symseg_f32_kernel<WAVES>;
    case SpmvFamily::symseg_notile: return csx_spmv_symseg_notile_f32_kernel<WAVES>;
    case SpmvFamily::det: return csx_spmv_det_f32_kernel<WAVES>;
    case SpmvFamily::symtile_det: return csx_spmv_symtile_det_f32_kernel<WAVES>;
    case SpmvFamily::plain: break;
    }
    return csx_spmv_f32_kernel<WAVES>;
}

void launch_spmv(SpmvFamily family, int waves, unsigned blocks, size_t lds_bytes, void *stream, const KernelArgs &a,
                 const XcdSplit &xs, bool f32)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    const SpmvKernel k = f32 ? (w == 2 ? spmv_f32_kernel<2>(family) : w == 8 ? spmv_f32_kernel<8>(family) : spmv_f32_kernel<4>(family))
                             : (w == 2 ? spmv_kernel<2>(family) : w == 8 ? spmv_kernel<8>(family) : spmv_kernel<4>(family));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * w), lds_bytes, static_cast<hipStream_t>(stream), a.rbs, a.passes,
                       a.n_rb, a.pass_stride, xs, a.values, a.descs, a.cidx, a.segrows, a.x, a.y, a.carry, a.dvalues,
                       a.spill, a.slot_col, a.alpha, a.beta, a.dvalues_priv, a.beta_priv);
}

void spmv_allow_lds(SpmvFamily family, size_t bytes)
{
    const int b = (int) bytes;
    for (SpmvKernel k : {spmv_kernel<2>(family), spmv_kernel<4>(family), spmv_kernel<8>(family)})
        (void) hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, b);
    for (SpmvKernel k : {spmv_f32_kernel<2>(family), spmv_f32_kernel<4>(family), spmv_f32_kernel<8>(family)})
        (void) hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

void launch_sym_init(void *stream, int nvec, double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                     size_t lo, size_t hi, size_t own_lo, size_t own_hi, double alpha, double beta, bool f32)
{
    const int t = 256;
    hipLaunchKernelGGL(f32 ? csx_sym_init_f32_kernel : csx_sym_init_kernel, dim3((unsigned)((hi - lo + t - 1) / t), (unsigned) nvec), dim3(t), 0,
                       static_cast<hipStream_t>(stream), y, ldy, x, ldx, dvalues, lo, hi, own_lo, own_hi, alpha, beta);
}

void launch_sym_mirror_rows(void *stream, int nvec, const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                            const double *val, const double *x, size_t ldx, double *y, size_t ldy, double alpha,
                            uint32_t n, bool f32)
{
    hipLaunchKernelGGL(f32 ? csx_sym_mirror_rows_f32_kernel : csx_sym_mirror_rows_kernel, dim3((n + 255) / 256, (unsigned) nvec), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rows, ptr, col, val, x, ldx, y, ldy, alpha, n);
}

void launch_scale(void *stream, int nvec, double *y, size_t ldy, size_t lo, size_t hi, double beta)
{
    const int t = 256;
    hipLaunchKernelGGL(csx_scale_kernel, dim3((unsigned)((hi - lo + t - 1) / t), (unsigned) nvec), dim3(t), 0,
                       static_cast<hipStream_t>(stream), y, ldy, lo, hi, beta);
}

void launch_fixup(void *stream, int nvec, const SpxSharedRow *shared, uint32_t n_shared, const double *carry,
                  uint32_t n_carry, double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                  const double *x, size_t ldx, bool f32)
{
    hipLaunchKernelGGL(f32 ? csx_fixup_f32_kernel : csx_fixup_kernel, dim3((n_shared + 63) / 64, (unsigned) nvec), dim3(64), 0,
                       static_cast<hipStream_t>(stream), shared, n_shared, carry, n_carry, y, ldy, alpha, beta, dvalues,
                       x, ldx);
}

// (four wavefronts of eight rows per workgroup; a multiple of eight workgroups, one share per XCD)
void launch_symfix(void *stream, const uint32_t *fix_ptr, const uint32_t *fix_idx, const double *spill, double *y,
                   double alpha, size_t nrows)
{
    hipLaunchKernelGGL(csx_symfix_kernel, dim3((unsigned)((((nrows + 31) / 32) + 7) & ~(size_t) 7)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), fix_ptr, fix_idx, spill, y, alpha, (uint32_t) nrows);
}

}  // namespace spx
