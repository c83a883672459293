// spmv_mvsym_kernels.hip -- the multi-vector product Y <- alpha*A*X + beta*Y on symmetric streams whose
// values are read once and used twice (SPX_PASS_SYMTILE, SPX_PASS_SYMSEG), for gfx950: K = 2, 4 or 8 vectors
// per pass over the stream (spx.gpu.sym_matmat; the host side is device_spmm, device_runtime.cpp).
//
// The K-vector form of the atomic hand-over kernels of spmv_kernels.hip (csx_spmv_symtile_atomic_kernel,
// csx_spmv_symseg_kernel), over the PLAIN pass table: one workgroup per row-block, LDS holds K copies of
// {transposed-sum slots, y tile}, a lane loads its descriptor and its values once and serves the K vectors in
// turn (spmv_mvsym_device.hpp; the ordinary passes of such a stream -- what is held with its mirror image, the
// leftovers -- through run_pass<K> / run_pair<K> of spmv_device.hpp).  Everything is handed over with global
// atomics on top of csx_sym_init_kernel, which has put beta * y and the diagonal term into every vector: the
// own rows, then the slots in aligned groups of eight columns.  The store shortcut of SPX_RB_PRIVATE
// row-blocks is the single-vector product's (device_product restricts it to K == 1).
#include "spmv_mvsym_device.hpp"
#include "spmv_launch.hpp"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace spx {

__device__ __forceinline__ bool read_once_pass(const SpxPass &p)
{
    return p.kind == SPX_PASS_SYMTILE || p.kind == SPX_PASS_SYMSEG;
}

// one pass on its own, whatever its kind (`rbk`: the row-block as the ordinary passes are to see it, mvsym_body)
template <int K>
__device__ __forceinline__ void mvsym_one(const MvSymArgs &a, const SpxRowBlock &rb, const SpxRowBlock &rbk, const SpxPass &p,
                                          double *lds, double *tile, const double *win, int core, bool x16, int lane)
{
    if (p.kind == SPX_PASS_SYMTILE) mvsym_tile_pass<K>(a, rb, p, lds, tile, core, x16, lane);
    else if (p.kind == SPX_PASS_SYMSEG) run_mvsym_seg<K>(a, rb, p, lds, tile, core, lane);
    else run_pass<K>(static_cast<const MvArgs &>(a), rbk, p, tile, win, lane);
}

// LDS: vector j's slots and y tile at j * (n_slots + n_rows), then the K x windows where they are staged
// (MvArgs::stage), then the first columns of the row-block's slot groups.
template <int K, int WAVES>
__device__ __forceinline__ void mvsym_body(const MvSymArgs &a, const XcdSplit &xs, double *lds)
{
    constexpr int BLOCK_THREADS = 64 * WAVES;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware order: workgroup b runs on XCD b % 8 and takes that XCD's next row-block
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t rb_idx = xs.first[xcd] + (blockIdx.x >> 3);
    if (rb_idx >= xs.first[xcd + 1u]) return;

    const SpxPass *passes = a.passes + (size_t) rb_idx * a.pass_stride;
    const SpxRowBlock rb = a.rbs[rb_idx];
    SpxPass p0 = passes[wave];
    SpxPass p1 = passes[wave + WAVES];                   // (the table is padded by one stride)
    const int n_rows = rb.n_rows;
    const int n_slots = rb.n_slots;
    const int core = n_slots + n_rows;                   // doubles per vector
    for (int i = threadIdx.x; i < K * core; i += BLOCK_THREADS) lds[i] = 0.0;
    double *win = lds + K * core;
    const int xw = a.stage ? (int) rb.xwin_len : 0;
    if (xw) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double *xs_j = a.x + (size_t) j * a.ldx + rb.xwin_base;
            for (int i = threadIdx.x; i < xw; i += BLOCK_THREADS) win[j * xw + i] = xs_j[i];
        }
    }
    // the first columns of the slot groups, fetched now: the hand-over at the end does not start with a
    // load from memory
    uint32_t *gcol_lds = reinterpret_cast<uint32_t *>(win + K * xw);
    {
        const uint32_t *gcol = a.slot_col + (rb.spill_off >> 3);
        for (int i = threadIdx.x; i < (n_slots >> 3); i += BLOCK_THREADS) gcol_lds[i] = gcol[i];
    }
    __syncthreads();

    // The ordinary passes add to vector j's tile at tile + j * (rows of the row-block they are given): a copy
    // of the header whose rows are the whole of {slots, y tile} gives them this kernel's layout.  (A row-block
    // of one row with slots would lose the wavefront-wide sum of its gather passes, not its result.)
    SpxRowBlock rbk = rb;
    rbk.n_rows = (uint16_t) core;
    double *tile = lds + n_slots;
    const bool x16 = ((reinterpret_cast<uintptr_t>(a.x) | (uintptr_t) (a.ldx * sizeof(double))) & 15u) == 0;
    const MvArgs &am = a;

    // wave w takes passes w, w + WAVES, ..., ordinary ones two at a time when they have the same shape
    const int n_pass = rb.n_pass;
    for (int t = wave; t < n_pass; t += 2 * WAVES) {
        const bool two = t + WAVES < n_pass;
        if (two && !read_once_pass(p0) && same_shape(p0, p1)) {
            run_pair<K>(am, rbk, {p0, p1}, tile, win, lane);
        } else {
            mvsym_one<K>(a, rb, rbk, p0, lds, tile, win, core, x16, lane);
            if (two) mvsym_one<K>(a, rb, rbk, p1, lds, tile, win, core, x16, lane);
        }
        if (t + 2 * WAVES < n_pass) {
            p0 = passes[t + 2 * WAVES];
            p1 = passes[t + 3 * WAVES];
        }
    }
    __syncthreads();

    // ---------------- hand over: the owned rows of every vector, then its slots --------------------
    if (rb.flags & SPX_RB_SHARED) {
        if (threadIdx.x < K) a.carry[(size_t) threadIdx.x * a.n_carry + rb.carry_slot] = tile[threadIdx.x * core];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j)
            for (int i = threadIdx.x; i < n_rows; i += BLOCK_THREADS)
                atomicAdd(&a.y[(size_t) j * a.ldy + rb.row0 + i], a.alpha * tile[j * core + i]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        for (int i = threadIdx.x; i < n_slots; i += BLOCK_THREADS)
            atomicAdd(&a.y[(size_t) j * a.ldy + gcol_lds[i >> 3] + (i & 7)], a.alpha * lds[j * core + i]);
}

template <int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mvsym_kernel(MvSymArgs a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];      // K x {slots, y tile}, the K x windows, the slot groups' columns
    mvsym_body<K, WAVES>(a, xs, lds_dyn);
}

// ---- launchers ------------------------------------------------------------------------------

typedef void (*MvSymKernel)(MvSymArgs, XcdSplit);

template <int K>
static MvSymKernel mvsym_kernel_w(int waves)
{
    return waves == 2 ? csx_spmv_mvsym_kernel<K, 2> : waves == 8 ? csx_spmv_mvsym_kernel<K, 8> : csx_spmv_mvsym_kernel<K, 4>;
}

static MvSymKernel mvsym_kernel_kw(int K, int waves)
{
    return K == 8 ? mvsym_kernel_w<8>(waves) : K == 4 ? mvsym_kernel_w<4>(waves) : mvsym_kernel_w<2>(waves);
}

void launch_spmv_mvsym(int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvSymArgs &a,
                       const XcdSplit &xs)
{
    const int w = (waves == 2 || waves == 8) ? waves : 4;
    hipLaunchKernelGGL(mvsym_kernel_kw(K, w), dim3(blocks), dim3(64 * w), lds_bytes, static_cast<hipStream_t>(stream), a, xs);
}

void spmv_mvsym_allow_lds(size_t bytes)
{
    const int b = (int) bytes;
    for (int K : {2, 4, 8})
        for (int w : {2, 4, 8})
            (void) hipFuncSetAttribute(reinterpret_cast<const void *>(mvsym_kernel_kw(K, w)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, b);
}

}  // namespace spx
