// spmv_launch.hpp -- what host code needs to launch the CSX interpreter: the kernel arguments, the
// XCD-aware row-block order, the kernel families and the launchers of the eleven interpreter translation
// units (spmv_kernels.hip, spmv_xw_kernels.hip, spmv_sx_kernels.hip, spmv_t_kernels.hip, spmv_mv_kernels.hip,
// spmv_mv_f32_kernels.hip, spmv_mvr_kernels.hip, spmv_mvr_f32_kernels.hip, spmv_mvsym_kernels.hip,
// scale_kernels.hip, sym_scale_kernels.hip).  Plain C++: no HIP header, so that the host runtime
// (device_runtime.cpp) is compiled by the host compiler.
#pragma once

#include "gpu_format.h"
#include "xwindows.hpp"

#include <cstddef>
#include <cstdint>

namespace spx {

// the stream of a matrix on the device: what every kernel that walks row-blocks reads, whatever it multiplies with.
// (The K-vector kernels take their arguments as one struct, and the order of its fields decides how they
// arrive in SGPRs: with pass_stride in here, in front of x, the K = 8 kernels spilled 215 SGPRs where they
// spill 92 -- profiles/r08/REFACTOR.md.  So it stays where each struct had it.)
struct StreamArgs {
    const SpxRowBlock *rbs;
    const SpxPass *passes;
    const double *values;
    const SpxUnitDesc *descs;
    const uint8_t *cidx;
    const uint16_t *segrows;
};

// the single-vector kernels
struct KernelArgs : StreamArgs {
    const double *x;
    double *y;
    double *carry;
    const double *dvalues;   // symmetric, fused: diagonal added at the write-out (else null)
    double *spill;           // symmetric tiles: transposed sums of columns owned by other row-blocks
    const uint32_t *slot_col;  // ... or (atomic hand-over) the first column of every group of eight slots
    double alpha, beta;
    const double *dvalues_priv;   // atomic hand-over: diagonal for the row-blocks that store their rows
    double beta_priv;             // ... and the caller's beta for them (beta above is 1 after the init pass)
    uint32_t n_rb;
    uint32_t pass_stride;    // pass headers of row-block i start at passes[i * pass_stride]
    const XwEntry *xw_tab;   // unit windows of x (xwindows.hpp): XW_MAX entries per row-block, or null
};

// XCD-aware order of the row-blocks: workgroup b runs on XCD b % 8; XCD x walks the row-blocks
// [first[x], first[x + 1]) in turn, a contiguous part of the matrix that holds an eighth of its
// VALUES (not of its row-blocks: a symmetric KKT matrix keeps its stored triangle in the second
// half of its rows, and an eighth of the row-blocks by count left five XCDs without work)
struct XcdSplit {
    uint32_t first[9];
};

// wavefronts per workgroup: the kernels exist for 2, 4 and 8 (spx.gpu.waves, or
// measured at tune time: small matrices like 2, leftover-heavy ones 8)
constexpr int MAX_WAVES_PER_BLOCK = 8;

// The kernels of spmv_kernels.hip that walk the row-blocks (one template, spmv_body, in eight forms)
enum class SpmvFamily {
    plain,            // csx_spmv_kernel: general path
    accum,            // csx_spmv_accum_kernel: column slices in one launch, y tiles added with atomics
    symtile,          // csx_spmv_symtile_kernel: symmetric tiles, sums spilled for csx_symfix_kernel
    symtile_atomic,   // csx_spmv_symtile_atomic_kernel: ... handed over with global atomics
    symseg,           // csx_spmv_symseg_kernel: ... and read-once row segments
    symseg_notile,    // csx_spmv_symseg_notile_kernel: read-once row segments, no tiles
    det,              // csx_spmv_det_kernel: a y tile per wavefront
    symtile_det,      // csx_spmv_symtile_det_kernel: symmetric tiles, a copy of slots + y tile per wavefront
};

// spmv_kernels.hip (`waves`: 2, 4 or 8, anything else runs as 4; `stream`: a hipStream_t)
// `f32` (every family; launch_spmv_sx and launch_spmv_xw as well): the kernel that reads the float twin of the values
// (spx.gpu.values_f32) -- a.values then points at that array of floats, element for element the doubles'.  The
// steps around a symmetric product take the flag too: the diagonal and the thin mirror list have no twin, and
// the float product rounds their doubles in registers
void launch_spmv(SpmvFamily family, int waves, unsigned blocks, size_t lds_bytes, void *stream, const KernelArgs &a,
                 const XcdSplit &xs, bool f32 = false);
void spmv_allow_lds(SpmvFamily family, size_t bytes);      // dynamic LDS beyond the default 64 KB
// the steps around the row-block launches, for `nvec` vectors at once (gridDim.y; vector j of x at x + j * ldx,
// of y at y + j * ldy, its carry slots at carry + j * n_carry)
void launch_sym_init(void *stream, int nvec, double *y, size_t ldy, const double *x, size_t ldx, const double *dvalues,
                     size_t lo, size_t hi, size_t own_lo, size_t own_hi, double alpha, double beta, bool f32 = false);
void launch_sym_mirror_rows(void *stream, int nvec, const uint32_t *rows, const uint32_t *ptr, const uint32_t *col,
                            const double *val, const double *x, size_t ldx, double *y, size_t ldy, double alpha,
                            uint32_t n, bool f32 = false);
void launch_scale(void *stream, int nvec, double *y, size_t ldy, size_t lo, size_t hi, double beta);
void launch_fixup(void *stream, int nvec, const SpxSharedRow *shared, uint32_t n_shared, const double *carry,
                  uint32_t n_carry, double *y, size_t ldy, double alpha, double beta, const double *dvalues,
                  const double *x, size_t ldx, bool f32 = false);
void launch_symfix(void *stream, const uint32_t *fix_ptr, const uint32_t *fix_idx, const double *spill, double *y,
                   double alpha, size_t nrows);

// spmv_sx_kernels.hip
void launch_spmv_sx(int waves, unsigned blocks, size_t lds_bytes, void *stream, const KernelArgs &a, const XcdSplit &xs,
                    const uint32_t *sx_tab, bool f32 = false);
size_t spmv_sx_header_bytes(uint32_t pass_stride);
void spmv_sx_allow_lds(size_t bytes);

// spmv_xw_kernels.hip
void launch_spmv_xw(int waves, unsigned blocks, size_t lds_bytes, void *stream, const KernelArgs &a, const XcdSplit &xs,
                    bool f32 = false);
void spmv_xw_allow_lds(size_t bytes);

// spmv_t_kernels.hip: the transposed product of a general stream, y += alpha * A^T * x (every launch adds: the
// caller has put beta * y there).  x: the rows of the matrix (global row numbers), y: its columns.
struct TransArgs : StreamArgs {
    const double *x;
    double *y;
    double alpha;
    uint32_t pass_stride;
    const XwEntry *xw_tab;   // `windows` launches: the table of the window plan; passes and descs are the plan's too
};
// `windows`: unit passes with SPX_PASSF_XLDS accumulate in the row-block's unit windows in LDS, which go to y once
// (lds_bytes: the most rows of a row-block, rounded up to even, plus its unit windows); else one atomic per nonzero
// (lds_bytes: the most rows of a row-block)
void launch_spmv_t(bool windows, int waves, unsigned blocks, size_t lds_bytes, void *stream, const TransArgs &a,
                   const XcdSplit &xs);
void spmv_t_allow_lds(size_t bytes);

// scale_kernels.hip: one pass over a general stream where it lies, as csx_spmv_t_kernel walks it (the PLAIN pass
// headers and descriptors, one launch per entry of the matrix' XCD splits).
// csx_scale_values_kernel: a(r,c) <- fl(fl(dr[r] * a) * dc[c]) in place (a null vector: its product is not formed),
// and the float twin of the values, where there is one, rewritten by the same lane.  lds_bytes: the most rows of a
// row-block (dr of its rows).
struct ScaleArgs : StreamArgs {
    const double *dr, *dc;   // nrows / ncols doubles, either may be null
    double *values_rw;       // StreamArgs::values, to be written
    float *values_f32;       // its float twin, or null
    uint32_t pass_stride;
};
void launch_scale_values(int waves, unsigned blocks, size_t lds_bytes, void *stream, const ScaleArgs &a, const XcdSplit &xs);
// csx_norms_kernel<KIND>: rows[r] (+)= |a(r,c)|, a(r,c)^2 or max |a(r,c)| over the stored entries of row r, cols[c]
// the same over column c; both through atomics, on top of a pass that zero-filled them; either may be null.
// lds_bytes: the most rows of a row-block (its rows' results), also where rows is null.
constexpr int NORM_SUM_ABS = 0, NORM_SUM_SQ = 1, NORM_MAX_ABS = 2;
struct NormArgs : StreamArgs {
    double *rows, *cols;
    uint32_t pass_stride;
};
void launch_norms(int kind, int waves, unsigned blocks, size_t lds_bytes, void *stream, const NormArgs &a, const XcdSplit &xs);

// sym_scale_kernels.hip: the same for a SYMMETRIC stream -- tiles, read-once segments, lower copies and mirror
// images; the plain pass headers and descriptors, one launch per entry of the matrix' XCD splits.
// csx_sym_scale_kernel: a(r,c) <- fl(fl(d[max(r,c)] * a) * d[min(r,c)]) in place and in the float twin, where there
// is one.  lds_bytes: the most rows of a row-block (d of its rows).  launch_sym_scale_rest: the diagonal array of
// the own rows [own_lo, own_lo + n_own) and the thin mirror list (n_mirror rows), which have no twin.
struct SymScaleArgs : StreamArgs {
    const double *d;         // nrows doubles
    double *values_rw;       // StreamArgs::values, to be written
    float *values_f32;       // its float twin, or null
    uint32_t pass_stride;
};
void launch_sym_scale(int waves, unsigned blocks, size_t lds_bytes, void *stream, const SymScaleArgs &a, const XcdSplit &xs);
void launch_sym_scale_rest(void *stream, double *dvalues, size_t own_lo, size_t n_own, const uint32_t *mrows,
                           const uint32_t *mptr, const uint32_t *mcol, double *mval, uint32_t n_mirror, const double *d);
// csx_sym_norms_kernel<KIND>: out[i] (+)= the terms of row i of the full matrix.  A value stored once counts for
// its row and, through the row-block's transposed-sum slots in LDS, for its column; a value stored twice for the
// row of each copy.  Atomics on top of launch_sym_norms_init, which writes all n elements of `out`: the term of the
// diagonal on the own rows, zero elsewhere, and then joins in the thin mirror list.  lds_bytes: the most slots +
// rows of a row-block (sym_norms_allow_lds: beyond the default 64 KB).
struct SymNormArgs : StreamArgs {
    double *out;
    const uint32_t *slot_col;  // the first column of every group of eight transposed-sum slots
    uint32_t pass_stride;
};
void launch_sym_norms(int kind, int waves, unsigned blocks, size_t lds_bytes, void *stream, const SymNormArgs &a,
                      const XcdSplit &xs);
void launch_sym_norms_init(int kind, void *stream, double *out, size_t n, const double *dvalues, size_t own_lo,
                           size_t own_hi, const uint32_t *mrows, const uint32_t *mptr, const double *mval, uint32_t n_mirror);
void sym_norms_allow_lds(size_t bytes);

// spmv_mv_kernels.hip: the multi-vector product, K = 2, 4 or 8 vectors per pass over the plain stream.
// Column-major blocks: vector j of X at x + j * ldx, of Y at y + j * ldy.
struct MvArgs : StreamArgs {
    const double *x;
    double *y;
    size_t ldx, ldy;
    double *carry;             // SPX_RB_SHARED: vector j's partial of slot s at carry[j * n_carry + s]
    const double *dvalues;     // symmetric, fused: diagonal added at the write-out (else null)
    double alpha, beta;
    uint32_t n_carry;
    uint32_t pass_stride;
    uint32_t stage;            // 1: the K x windows of a row-block are staged in LDS behind the K y tiles
};
// the families of csx_spmv_mv_kernel<Args, V, family, K, waves> (spmv_mv_instances.hpp): one kernel template for
// both layouts (Args: MvArgs, or MvrArgs below) and both value types (V: double, or float for the twin)
enum class MvFamily {
    plain,     // K y tiles per workgroup
    accum,     // column slices in one launch, tiles added with atomics
    det,       // K y tiles per wavefront, summed in wavefront order
};
void launch_spmv_mv(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                    const XcdSplit &xs);
void spmv_mv_allow_lds(size_t bytes);
// spmv_mv_f32_kernels.hip: the same kernels reading the float twin of the values (spx.gpu.values_f32) -- a.values
// then points at that array of floats; everything else, a.dvalues included, as above
void launch_spmv_mv_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvArgs &a,
                        const XcdSplit &xs);
void spmv_mv_f32_allow_lds(size_t bytes);

// spmv_mvr_kernels.hip: the multi-vector product on ROW-MAJOR (interleaved) blocks, K = 1, 2, 4 or 8 vectors per
// pass over the plain stream of a general tune: entry (i, j) of X at x[i * ldx + j], of Y at y[i * ldy + j]; x
// and y point at the group's first vector.  The fields of MvArgs with that meaning of ldx and ldy (dvalues is
// not read: symmetric streams are column-major business); `stage`: the x window of a row-block, xwin_len x K
// doubles, is staged in LDS behind the K y tiles.
struct MvrArgs : MvArgs {
    uint32_t x16;              // 1: x and ldx * 8 are multiples of 16 -- the K doubles of a column load in pairs
};
void launch_spmv_mvr(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvrArgs &a,
                     const XcdSplit &xs);
void spmv_mvr_allow_lds(size_t bytes);
// spmv_mvr_f32_kernels.hip: the same kernels reading the float twin of the values (a.values points at the floats)
void launch_spmv_mvr_f32(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream,
                         const MvrArgs &a, const XcdSplit &xs);
void spmv_mvr_f32_allow_lds(size_t bytes);
// the steps around its row-block launches: y <- beta * y on the nvec vectors of the rows [lo, hi) (never the
// padding behind them), and the sum of the carry slots (vector j's at carry + j * n_carry) of rows split over
// several row-blocks
void launch_scale_rm(void *stream, int nvec, double *y, size_t ldy, size_t lo, size_t hi, double beta);
void launch_fixup_rm(void *stream, int nvec, const SpxSharedRow *shared, uint32_t n_shared, const double *carry,
                     uint32_t n_carry, double *y, size_t ldy, double alpha, double beta);

// spmv_mvsym_kernels.hip: the multi-vector product on symmetric streams with read-once passes
// (SPX_PASS_SYMTILE, SPX_PASS_SYMSEG; spx.gpu.sym_matmat), atomic hand-over, over the plain pass table.
// (slot_col behind the fields of MvArgs: their order decides how they arrive in SGPRs, see StreamArgs)
struct MvSymArgs : MvArgs {
    const uint32_t *slot_col;  // the first column of every group of eight transposed-sum slots
};
void launch_spmv_mvsym(int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const MvSymArgs &a,
                       const XcdSplit &xs);
void spmv_mvsym_allow_lds(size_t bytes);

// refresh_kernels.hip: dst[i] = src[map[i]] for the n positions of a value array of the stream, where map[i] is
// not 0xffffffff (values_plan.hpp).  `map` holds n rounded up to a multiple of four entries, the padding without a
// source.  Enqueues on `stream`, nothing else.
// `dst_f32` (or null): the float twin of dst, which gets the same values rounded to nearest in the same pass
// (both 16-byte aligned then).
void launch_refresh_values(void *stream, double *dst, const uint32_t *map, const double *src, size_t n,
                           float *dst_f32 = nullptr);
// the diagonal of a tuned matrix (diag_plan.hpp): dst[i] = values[pos[i]], +0.0 where pos[i] is 0xffffffff, for
// i < n; pos == null: dst[i] = values[i] (the diagonal array of a symmetric stream).  `pos` is 16-byte aligned
// and holds n entries, `dst` any 8-byte aligned address.  Enqueues on `stream`, nothing else.
void launch_gather_diag(void *stream, double *dst, const uint32_t *pos, const double *values, size_t n);
// dst[i] = (float) src[i] for i < n, round to nearest even; n a multiple of four, both arrays 16-byte aligned
void launch_narrow_values(void *stream, float *dst, const double *src, size_t n);

}  // namespace spx
