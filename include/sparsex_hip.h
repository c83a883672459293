/*
 * sparsex_hip.h -- additive extensions of the MI355X build of the SparseX C API.
 *
 * Nothing here changes a signature of <sparsex/sparsex.h>.  The entry points
 * let a caller (a) keep x and y resident in HBM between calls, which is how
 * an iterative solver should drive the library on a GPU, (b) inspect the
 * row-block descriptor stream's size, and (c) export a tuned partition in the
 * reference's own CSX byte format (ctl / values / id_map / rows_info of
 * include/sparsex/internals/Csx.hpp:29-53 in the reference tree) so that the
 * reference's SpMV code, or a parity oracle, can consume it.
 *
 * Extra option mnemonics understood by spx_option_set() in this build:
 *   spx.rt.host_only        "true": spx_mat_tune() only preprocesses (no GPU
 *                           needed); spx_matvec_*() on such a matrix fail
 *   spx.rt.device           HIP device ordinal (default: current device)
 *   spx.rt.gpu_rank/world   this process owns partitions
 *                           [rank*P/world, (rank+1)*P/world), P = spx.rt.nr_threads
 *   spx.rt.row_offset,      the input holds rows [offset, offset + its rows) of a
 *   spx.rt.global_rows      matrix with global_rows rows (0: the input is the matrix)
 *   spx.gpu.rowblock_elems  target nonzeros per row-block (default 0 = auto:
 *                           nnz/1280 clamped to [1024, 4096]; 8192 beyond 64 M)
 *   spx.gpu.waves           wavefronts per workgroup of the SpMV kernel: 2, 4 or 8;
 *                           0 (default): spx_mat_tune() measures a few launch
 *                           configurations on the device and keeps the fastest.  (The multi-vector kernel of
 *                           spx.gpu.sym_matmat runs eight where its LDS leaves a compute unit room for fewer than
 *                           four workgroups, whatever is set or measured here.)
 *   spx.gpu.rowblock_rows   max rows per row-block (default 512; up to 2048: planned row-blocks of
 *                           at most 512 rows are then joined up to the target size -- for matrices
 *                           with a few nonzeros per row; measured on syn-webbase: 38.8 us with 512,
 *                           40.9 with 1024, so not the default)
 *   spx.gpu.stack_segments  "false": one descriptor per CSX unit piece instead
 *                           of merging equal row segments of consecutive rows
 *   spx.gpu.recut_linear    "false": vertical / diagonal / strided units always run one
 *                           nonzero per lane, even where they line up along rows
 *   spx.gpu.col_phases      general path: the stream as a sum of K column slices, A = A_0 + A_1 + ..., each a run of
 *                           row-blocks of its own, so that a workgroup only gathers from 1 / K of x (a slice that
 *                           fits the 4 MB of L2 of an XCD).  "c2" | "c4" | "c8": all slices in ONE launch, slice k on
 *                           its own group of 8 / K XCDs, every row-block adding its y tile on top of a beta * y pass
 *                           (global atomics: not with spx.gpu.deterministic); "2" .. "8": the slices launched one
 *                           after the other (slice k > 0 adds to y; measured slower than the plain stream:
 *                           every launch has a ~10 us critical path); "1": off; "auto" (default): for
 *                           leftover-dominated matrices whose x exceeds 6 MB, two and four concurrent slices
 *                           are measured against the plain stream at tune time and the fastest stays
 *                           (syn-webbase: 38.7 us plain, 32.6 us with two slices; profiles/r03/ablation.md)
 *   spx.gpu.band_order      "true": row-blocks are launched strip by strip across the planes of a stencil
 *                           instead of in row order (measured 4-7 % slower on the KKT stand-in: off)
 *   spx.gpu.inline_desc     "false": unit passes whose lanes share one descriptor load it like any other
 *                           (default: it travels in the pass header, SPX_PASSF_INLINE: one dependent round trip
 *                           per pass instead of two; 4-5 % on the KKT stand-in)
 *   spx.gpu.keep_units      "false": ... even those none of whose nonzeros has a neighbour along
 *                           its row (default: such a unit stays one descriptor -- the main diagonal
 *                           of a KKT system -- instead of a leftover nonzero per row)
 *   spx.gpu.wave_tiles      a y tile per wavefront instead of one per workgroup: "true",
 *                           "false", "auto" (default: spx_mat_tune() measures it)
 *   spx.gpu.deterministic   "true": bit-identical repeated products (wave tiles, the
 *                           symmetric tiles' sums through the fixed-order lists)
 *   spx.gpu.sym_spill       symmetric tiles' transposed sums: "lists" (second kernel,
 *                           fixed order), "atomic" (global atomics), "auto" (measured)
 *   spx.gpu.sym_segments    symmetric path: runs of consecutive columns of the lower triangle
 *                           (spx.gpu.sym_segment_min or more of them, default 2; with 3 syn-nlpkkt
 *                           takes 0.880 instead of 0.836 ms) are read once and used for both triangles
 *                           ("true"), their mirror image is stored instead ("false"), or
 *                           "auto" (default): read once where at least half of the triangle
 *                           lies in such runs and the triangle has 16 M nonzeros or more (a
 *                           smaller matrix stays in the Infinity Cache, where reading it
 *                           twice is cheaper than the extra atomics); implies the atomic
 *                           hand-over
 *   spx.gpu.sym_wide_rows   rows of a row-block that holds such segments: consecutive row-blocks
 *                           (512 rows at most each) go side by side into one with a common y
 *                           tile and common slots, so that a column several of them reach is
 *                           handed to y once (default 1024, at most 2048; measured on syn-nlpkkt,
 *                           734 M nonzeros: 512 0.842 ms, 1024 0.826 ms, 2048 0.92 ms)
 *   spx.gpu.sym_matmat      symmetric path with tiles or read-once segments: "false" (default) | "true" -- the
 *                           read-once passes serve groups of vectors (spx_hip_matmat_kernel reads the stored triangle
 *                           once per group, csx_spmv_mvsym_kernel).  Read where the device copy is built (spx_mat_tune,
 *                           spx_mat_restore; not part of a saved matrix).  At tune time it makes spx.gpu.sym_spill=auto
 *                           "atomic" without a measurement and spx.gpu.sym_wide_rows at most 512, so that K copies of a
 *                           row-block's slots and y tile fit the LDS; an explicit "lists", spx.gpu.deterministic=true or
 *                           spx.gpu.wave_tiles=true keep their meaning and the group stays 1.  General matrices and
 *                           spx.gpu.sym_once=false ignore it; any other value fails spx_mat_tune
 *   spx.gpu.sym_pipeline    symmetric path, streams of read-once segments: "auto" (default: measured at tune time) |
 *                           "true" | "false" -- passes whose lanes all belong to one unit carry their geometry in a
 *                           device-side copy of their header, so that values and x are requested in one round trip
 *                           and the passes run as a two-stage pipeline (csx_spmv_sx_kernel; the bench matrix 1.00 ->
 *                           0.91 ms, edges 100-180 10-17 % faster: profiles/r06/NOTES.md)
 *   spx.gpu.sym_pure_passes "true" (default): a long run of equal read-once segments (40 and more) fills passes of its
 *                           own, i.e. passes with ONE descriptor -- what the pipeline above feeds on; "false": passes
 *                           are filled regardless of units, as before round 6
 *   spx.gpu.sym_segment_max widest segment a longer run of columns is cut into (default 8; with 4 every segment could
 *                           ride the pipeline, measured slower: syn-kkt2f 122 -> 135 us, profiles/r06/segment_max_raw.md)
 *   spx.gpu.arena           "true": every array of a tuned matrix in ONE HBM allocation (2 MB-aligned pieces)
 *                           instead of one allocation each (default; the arena was built to test whether
 *                           placement explains the run-to-run spread: it does not, profiles/r04/spread.md)
 *   spx.rt.dist_reorder     the whole matrix given to every process of a multi-GPU job (spx.rt.gpu_world > 1):
 *                           "rcm" | "rcm_owner" renumber the unknowns in front of the nonzero-balanced cut
 *                           (spx_hip_dist_reorder below; spx_mat_get_perm returns the permutation); "none" (default)
 *   spx.rt.dist_chunks      SPX_DIST_OVERLAP: parts the own product is cut into (default 4; 1: no rounds planned --
 *                           on every process or on none: planning the rounds is collective; the counts may differ)
 *   spx.gpu.x_window        "false": leftovers never gather from an LDS window of x
 *   spx.gpu.unit_windows    general path: "auto" (default: measured at tune time) | "true" | "false" -- the columns a
 *                           row-block's unit passes read are staged in LDS once per workgroup and the unit passes run
 *                           as a software pipeline (csx_spmv_xw_kernel); spx.gpu.unit_window_doubles (3072): most
 *                           doubles of x a row-block may stage (row-blocks that need more gather through L2);
 *                           spx.gpu.unit_window_gap (16): column intervals closer than this are staged as one
 *   spx.gpu.trans_windows   transposed product of a general matrix (spx_hip_matvec_trans_kernel): "auto" (default: where
 *                           the window plan stages fewer doubles than it serves nonzeros) | "true" | "false" -- unit passes
 *                           accumulate in the row-block's unit windows in LDS, which are added to y once, instead of one
 *                           atomic add per nonzero; read by spx_mat_tune / spx_mat_restore, not saved with the matrix
 *   spx.gpu.values_f32      "false" (default) | "true" | "all".  "true": a general tune keeps a float copy of the stream's
 *                           values in HBM next to the doubles (half of value_bytes, an allocation of its own, also with
 *                           spx.gpu.arena), built on the device once the launch tuner has settled, for
 *                           spx_hip_matvec_kernel_f32; symmetric tunes ignore it.  "all": general tunes as under "true",
 *                           and symmetric tunes keep the copy of their stream's values too (the stored triangle, read
 *                           once as floats; the diagonal and a slice's thin mirror list get no copy and are rounded in
 *                           registers).  Any other value fails the tune; read by spx_mat_tune / spx_mat_restore, not
 *                           saved with the matrix
 *   spx.vec.device          "false" (default) | "true" (also: env SPX_VEC_DEVICE through spx_options_set_from_env):
 *                           vectors the library allocates itself (spx_vec_create, spx_vec_create_random; page-locked)
 *                           keep x's HBM copy between spx_matvec_* calls, reused while no spx_vec_* call has changed
 *                           the vector.  OPT-IN because struct vector_struct is public: a client that writes through
 *                           v->elements must call spx_hip_vec_touch(v) afterwards (a sampled fingerprint of the
 *                           contents is a second net only: a rewritten vector is seen, one poked element may not be).
 *                           Views of user buffers (spx_vec_create_from_buff, both modes) always travel
 *   spx.vec.register        "auto" (default) | "false": the buffer of a view (spx_vec_create_from_buff) of 32 MB or
 *                           more is page-locked where it lies (hipHostRegister) at the view's first spx_matvec_*, and
 *                           released by spx_vec_destroy; it then travels like a vector of the library's own instead
 *                           of through staging memory.  Invisible to the client (it keeps writing through its own
 *                           pointer); a buffer that cannot be locked is staged.  The buffer must outlive the view
 *                           (as src/api/matvec.c:780-815 assumes)
 *   spx.rt.dist_chunks      at most 64 parts (larger values are clamped)
 *   spx.rt.host_parts       spx_matvec_* on host vectors of 32 MB or more: the number of parts the product runs in
 *                           while y travels back (and x up) part by part; "0" (default): 24 where x goes up by need
 *                           (16 on symmetric streams), else 8; at most 64.  Read at every call
 *   spx.gpu.sym_once        "false": symmetric path reads lower triangle and mirror
 *                           image (default: dense 8x8 tiles are read once)
 *   spx.gpu.sym_remine      "false": symmetric path mirrors unit by unit
 *                           instead of re-cutting the upper triangle
 *   spx.rt.keep_encoded     "false": drop the encoded partitions after the
 *                           upload (no get/set entry, no CSX export)
 *   spx.matrix.onedim_blocks  "true" enables br1/bc1 (MatrixOneDimBlocks,
 *                           no mnemonic in the reference: Runtime.cpp:60)
 */
#ifndef SPARSEX_HIP_H
#define SPARSEX_HIP_H

#include <sparsex/sparsex.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device-resident SpMV -------------------------------------------------
 * Replaces, for GPU-resident vectors, the host-vector entry points
 * spx_matvec_mult / spx_matvec_kernel (reference src/api/matvec.c:551-620).
 * x_dev: ncols doubles, y_dev: nrows doubles, both HBM pointers on the
 * matrix's device.  `stream` is a hipStream_t (NULL = default stream); the
 * call only enqueues work (so loops of these calls can be captured into a
 * hipGraph by stream capture).  With several processes (spx.rt.gpu_world > 1)
 * only the rows of this process' partitions are written on the general path;
 * on the symmetric path y_dev receives this process' partial vector, to be
 * summed over processes by the caller (RCCL all-reduce) -- or use the exchange plan
 * of spx_hip_mat_dist_attach / spx_hip_matvec_dist below, which moves only the
 * entries that have to travel.
 * A matrix handle is single-stream: products of the SAME matrix must not overlap in
 * time (they share its scratch: the partial sums of over-long rows, the spill array
 * of the symmetric tiles, the exchange buffers); different matrices are independent.
 * The calling thread's current HIP device must be the matrix's device (checked).
 * spx_mat_set_entry() on a tuned matrix patches the value where it lives, in HBM, after a
 * hipDeviceSynchronize() -- one per batch of edits, not per entry (the first edit after a product was
 * enqueued waits; it fails, value untouched, while a stream of the device is being captured):
 * products still in flight finish with the old value; a captured
 * graph replayed later reads the new one.
 * Once an exchange plan is attached (spx_hip_mat_dist_attach), the plain entry points above
 * write only the rows this process owns or adds to, [first conflict row, last owned row):
 * the rest of y_dev is left as it is (it is nobody's business any more).  Inside that range the
 * owned rows and the conflict rows hold this process' partial vector; a row in front of the owned
 * ones that the process does not add to is either cleared to 0 or left as it is.
 * A cut may leave a process a single row (or hand it rows without a nonzero below the diagonal):
 * such a slice tunes, multiplies and attaches like any other.
 */
spx_error_t spx_hip_matvec_mult(spx_value_t alpha, const spx_matrix_t *A,
                                const spx_value_t *x_dev, spx_value_t *y_dev,
                                void *stream);
spx_error_t spx_hip_matvec_kernel(spx_value_t alpha, const spx_matrix_t *A,
                                  const spx_value_t *x_dev, spx_value_t beta,
                                  spx_value_t *y_dev, void *stream);

/* ---- transposed product -------------------------------------------------------------
 * y <- alpha*A^T*x + beta*y on device memory, over the stream A was tuned into: no second tune, no second copy
 * of the matrix.  x_dev: nrows doubles, y_dev: ncols doubles, HBM pointers on the matrix's device; enqueues
 * only (hipGraph-capturable), allocates nothing.  _mult is _kernel with beta = 0; beta == 0 never reads y_dev.
 * A symmetric matrix (any tune, slice or attached) runs spx_hip_matvec_kernel: the same result, the same rows.
 * A general matrix adds every product a(r,c)*x[r] to y[c] with atomics -- in LDS first where its unit windows
 * allow (spx.gpu.trans_windows = true | false | auto, read by spx_mat_tune / spx_mat_restore, not saved), then
 * in memory: the result lies within the fp64 bound of the product but is NOT bit-reproducible, and
 * spx.gpu.deterministic does not cover this call.  A general row slice (spx.rt.gpu_world > 1) reads only its own
 * rows of the full-length x_dev (global row numbers) and leaves this process' partial vector over ALL columns in
 * y_dev, to be summed over processes by the caller.
 * SPX_FAILURE (through the error handler) for a NULL handle or pointer, overlapping x and y ranges, a host-only
 * matrix, the wrong current device, a general matrix with an exchange plan attached, and (_vec) vectors whose
 * sizes are not nrows / ncols.
 */
spx_error_t spx_hip_matvec_trans_mult(spx_value_t alpha, const spx_matrix_t *A,
                                      const spx_value_t *x_dev, spx_value_t *y_dev,
                                      void *stream);
spx_error_t spx_hip_matvec_trans_kernel(spx_value_t alpha, const spx_matrix_t *A,
                                        const spx_value_t *x_dev, spx_value_t beta,
                                        spx_value_t *y_dev, void *stream);
/* Diagnostic: how the transposed product of this matrix runs.  -1: no device copy (or a NULL handle);
 * 0: symmetric, the forward product runs; 1: one atomic add per nonzero; 2: unit windows accumulate in LDS and
 * go to y once each (row-blocks and passes without windows still add per nonzero). */
int spx_hip_matvec_trans_mode(const spx_matrix_t *A);

/* ---- product with a float copy of the values ------------------------------------------
 * y <- alpha*fl32(A)*x + beta*y on device memory, where fl32(A) holds A's stored entries rounded to float
 * (nearest even).  For solvers that multiply with a rounded matrix most of the time (the correction step of
 * iterative refinement, an inner or preconditioning Krylov solve) and with the exact one for the residual: both
 * products run on ONE handle -- the same pattern, tune, descriptor stream and launch configuration; the float copy
 * of the values (spx.gpu.values_f32=true at spx_mat_tune / spx_mat_restore for general matrices, =all for symmetric
 * ones as well) costs half of value_bytes of HBM and halves the value bytes a product reads.  Vectors stay fp64, every product and sum is
 * fp64: the kernels load floats, widen them in registers and run the fp64 kernels' operations in their order.
 * Semantics are those of spx_hip_matvec_kernel in every respect (rows written by a slice or an attached matrix,
 * beta == 0 never reads y_dev, enqueues only, allocates nothing, hipGraph-capturable, the handle's single-stream
 * rule -- the carry scratch is shared with the fp64 product --, counts as a product for spx_mat_set_entry's wait,
 * bit-identical repeats under spx.gpu.deterministic=true); it runs the kernel family and wavefronts the handle's
 * fp64 product runs.  Accuracy: within the fp64 bound of the exact product with fl32(A), hence within
 * 2^-24 * |alpha| * sum|a||x| plus that bound of the product with A.  Stored values beyond float's range become
 * +-inf in the copy, values below its normal range become subnormal or 0.
 * A symmetric handle (spx.gpu.values_f32=all): fl32(A) rounds EVERY stored entry -- the lower triangle of the
 * stream, mirror-image copies the stream stores (spx.gpu.sym_once=false), the diagonal, the thin mirror list of a
 * slice.  Only the stream's value array has a copy (4 bytes per value, as for general streams); the diagonal and
 * the mirror list, at most a value per row, are read as doubles and rounded in registers by the float product
 * alone.  Every read-once family has its float form (tiles with lists or atomics, read-once segments with and
 * without tiles, the pipelined kernel, the deterministic one): with the atomic hand-over the result lies within
 * the bound above and is not bit-reproducible, like the fp64 product's.
 * spx_hip_mat_set_values(_host) writes both arrays in the same pass, spx_mat_set_entry patches the float next
 * to the double; spx_mat_get_entry, spx_mat_save, export and every other product read the doubles, as without
 * the option.
 * SPX_FAILURE (through the error handler, nothing enqueued) for a NULL handle or pointer, overlapping x and y
 * ranges, the wrong current device, a host-only matrix, (_vec) vectors whose sizes are not ncols / nrows, and a
 * matrix WITHOUT a float copy -- tuned or restored without the option, or tuned as a symmetric one without
 * spx.gpu.values_f32=all; the message says which.  There is no silent fp64 fallback.
 * The two multi-vector products have float forms as well: spx_hip_matmat_kernel_f32 and
 * spx_hip_matmat_rm_kernel_f32, behind the fp64 multi-vector products below.
 * Not provided: a float form of the multi-vector product on read-once symmetric streams (spx.gpu.sym_matmat: such a
 * handle runs spx_hip_matmat_kernel_f32 column by column), of the transposed, parts and dist products
 * (spx_hip_matvec_trans_* on a symmetric handle keeps running the fp64 forward product), host vectors, and a launch
 * tune of their own for the float kernels (they run with the wavefronts and the family measured for the fp64
 * product).
 */
spx_error_t spx_hip_matvec_mult_f32(spx_value_t alpha, const spx_matrix_t *A, const spx_value_t *x_dev,
                                    spx_value_t *y_dev, void *stream);
spx_error_t spx_hip_matvec_kernel_f32(spx_value_t alpha, const spx_matrix_t *A, const spx_value_t *x_dev,
                                      spx_value_t beta, spx_value_t *y_dev, void *stream);
/* Bytes of HBM the float copy takes (4 per value of the stream, padding included); 0: no copy; -1: a NULL handle
 * or a matrix without a device copy. */
int64_t spx_hip_mat_values_f32_bytes(const spx_matrix_t *A);
/* Diagnostic (tools/f32_bench.py): seconds one run of the kernel that builds the copy takes on this matrix
 * (synchronous; rewrites the copy with what it holds); negative without a copy. */
double spx_hip_mat_values_f32_narrow_seconds(const spx_matrix_t *A);

/* ---- multi-vector product ----------------------------------------------------------
 * Y <- alpha*A*X + beta*Y for nvec vectors at once, on device memory.
 * Column-major blocks (BLAS convention): vector j of X is X_dev + j*ldx (ncols doubles, ldx >= ncols),
 * vector j of Y is Y_dev + j*ldy (nrows doubles, ldy >= nrows).  HBM pointers on the matrix's device;
 * enqueues only (hipGraph-capturable), like spx_hip_matvec_kernel.
 * Column j of the result is what spx_hip_matvec_kernel(alpha, A, X_dev + j*ldx, beta, Y_dev + j*ldy, stream)
 * writes: the same rows (row slices, an attached exchange plan), beta == 0 never reads Y, and with
 * spx.gpu.deterministic=true every column is bit-identical to that product.  The padding between columns is
 * never read or written; nvec == 0 does nothing.  SPX_FAILURE (through the error handler) for a NULL pointer
 * with nvec > 0, ldx < ncols, ldy < nrows, overlapping X and Y, a host-only matrix or the wrong current device.
 * One pass over the matrix' stream serves spx_hip_matmat_group(A) vectors (the values, descriptors and column
 * offsets are read once for all of them); streams with symmetric tiles or read-once segments (the default
 * symmetric tune) run one single-vector product per column -- exact, no faster -- unless they were tuned or
 * restored with spx.gpu.sym_matmat=true: then a pass over the stored triangle serves a group of 8, 4 or 2 vectors
 * wherever the transposed sums are handed over with global atomics and one tile per workgroup is kept (not with
 * spx.gpu.sym_spill=lists, spx.gpu.deterministic=true or spx.gpu.wave_tiles=true).  Such columns go through
 * atomics: within the fp64 bound of the product, not bit-reproducible.  Nothing is allocated.
 */
spx_error_t spx_hip_matmat_kernel(spx_value_t alpha, const spx_matrix_t *A, size_t nvec,
                                  const spx_value_t *X_dev, size_t ldx, spx_value_t beta,
                                  spx_value_t *Y_dev, size_t ldy, void *stream);
/* Diagnostic: how many vectors one pass over this matrix' stream serves (>= 2: the multi-vector
 * kernels run; 1: one product per vector), -1 for a matrix without a device copy.  A symmetric tune with tiles or
 * read-once segments: 1, or under spx.gpu.sym_matmat=true the widest of 8, 4, 2 of which that many copies of the
 * largest row-block's slots and y tile fit 80 KB of LDS (two workgroups per compute unit). */
int spx_hip_matmat_group(const spx_matrix_t *A);

/* ---- multi-vector product on row-major (interleaved) blocks ----------------------------
 * Y <- alpha*A*X + beta*Y for nvec vectors at once, on device memory, for the layout a torch tensor of shape
 * (ncols, nvec) or a PETSc-style dense block has: entry (i, j) of X is X_dev[i*ldx + j] (i < ncols, j < nvec,
 * ldx >= nvec), entry (i, j) of Y is Y_dev[i*ldy + j] (i < nrows, j < nvec, ldy >= nvec).  HBM pointers on the
 * matrix's device; the call only enqueues and allocates nothing (hipGraph-capturable), like
 * spx_hip_matvec_kernel, refuses a thread whose current device is not the matrix', and the handle stays
 * single-stream.
 * Column j of Y is what spx_hip_matvec_kernel writes for column j of X (taken as a contiguous vector): on a row
 * slice the same rows are written, beta == 0 never reads Y, and with spx.gpu.deterministic=true every column is
 * bit-identical to that product.  The positions j >= nvec of a row (the padding up to ldx / ldy) are never
 * multiplied and never written; nvec == 0 does nothing.  X and Y must not overlap.
 * General (non-symmetric) tunes only.  A symmetric handle is refused with a message that says so: the
 * single-vector kernels cannot read a strided x, so there is no per-column fallback (tune the matrix of a block
 * solver as general, or hand spx_hip_matmat_kernel column-major blocks).  A matrix with an exchange plan attached
 * (spx_hip_mat_dist_attach) is refused as well.
 * SPX_FAILURE (through the error handler, nothing enqueued) for these two, a NULL handle, a host-only matrix, a
 * NULL pointer with nvec > 0, ldx < nvec, ldy < nvec, overlapping X and Y, and the wrong current device.
 * One pass over the matrix' stream serves spx_hip_matmat_rm_group(A) vectors; a remainder runs as groups of 4, 2
 * and 1 (one vector of such a block is still strided: it has a kernel of its own).  A lane reads the nvec values of
 * a column of A's row as one contiguous run -- 16 bytes per load where X_dev + j0 and ldx*8 are multiples of 16
 * for the group's first vector j0, 8 bytes otherwise -- where the column-major product gathers one value per
 * vector.
 */
spx_error_t spx_hip_matmat_rm_kernel(spx_value_t alpha, const spx_matrix_t *A, size_t nvec,
                                     const spx_value_t *X_dev, size_t ldx, spx_value_t beta,
                                     spx_value_t *Y_dev, size_t ldy, void *stream);
/* Diagnostic: how many vectors one pass of spx_hip_matmat_rm_kernel over this matrix' stream serves: the widest
 * of 8, 4, 2, 1 of which that many y tiles of the largest row-block (per wavefront where the tune keeps a tile
 * per wavefront) fit 80 KB of LDS -- the rule of spx_hip_matmat_group.  0: a symmetric handle, which the
 * product refuses; -1: a matrix without a device copy. */
int spx_hip_matmat_rm_group(const spx_matrix_t *A);

/* ---- multi-vector products with the float copy of the values ----------------------------
 * Y <- alpha*fl32(A)*X + beta*Y for nvec vectors at once: spx_hip_matmat_kernel (column-major blocks) and
 * spx_hip_matmat_rm_kernel (row-major blocks) through kernels that read the float copy of the values
 * (spx.gpu.values_f32, see "product with a float copy of the values" above).  For a block solver with an inner
 * mixed-precision solve: one pass over the stream serves a group of vectors AND reads half the value bytes.
 * Column j of Y is what spx_hip_matvec_kernel_f32 writes for column j of X; everything else is the fp64 call's of
 * the same layout: the rows written on a row slice or (column-major) an attached matrix, beta == 0 never reads Y,
 * the padding is never read or written, nvec == 0 does nothing, X and Y must not overlap, the call only enqueues
 * and allocates nothing (hipGraph-capturable), the handle's single-stream rule (the carry scratch is shared with
 * the other products), it counts as a product for spx_mat_set_entry's wait, and with
 * spx.gpu.deterministic=true every column is bit-identical to spx_hip_matvec_kernel_f32's.  Vectors, the x
 * windows and y tiles in LDS, products and sums are fp64; the kernel family, wavefronts, LDS and staging are
 * those of the handle's fp64 multi-vector product.
 * Column-major groups: spx_hip_matmat_group_f32(A) vectors per pass -- spx_hip_matmat_group(A) on general tunes
 * and on symmetric ones without tiles or read-once segments (spx.gpu.sym_once=false: the diagonal is rounded in
 * registers); 1 on symmetric tunes with tiles or read-once segments, spx.gpu.sym_matmat=true included: one
 * spx_hip_matvec_kernel_f32 per column -- still fl32(A), exact, no faster.  The fp64 group kernel never runs.
 * Row-major groups: spx_hip_matmat_rm_group(A).
 * SPX_FAILURE (through the error handler, nothing enqueued, Y untouched): every refusal of the fp64 call of the
 * same layout (row-major: a symmetric handle and an attached matrix among them), and a handle WITHOUT a float copy;
 * the message says which option was missing.  There is no fp64 fallback.
 */
spx_error_t spx_hip_matmat_kernel_f32(spx_value_t alpha, const spx_matrix_t *A, size_t nvec,
                                      const spx_value_t *X_dev, size_t ldx, spx_value_t beta,
                                      spx_value_t *Y_dev, size_t ldy, void *stream);
spx_error_t spx_hip_matmat_rm_kernel_f32(spx_value_t alpha, const spx_matrix_t *A, size_t nvec,
                                         const spx_value_t *X_dev, size_t ldx, spx_value_t beta,
                                         spx_value_t *Y_dev, size_t ldy, void *stream);
/* Diagnostic: vectors per pass of spx_hip_matmat_kernel_f32 (see above); 0: no float copy; -1: a NULL handle or
 * a matrix without a device copy. */
int spx_hip_matmat_group_f32(const spx_matrix_t *A);

/* ---- device-resident vectors ---------------------------------------------------
 * HBM counterparts of the reference's host vector helpers (spx_vec_init,
 * spx_vec_scale, spx_vec_scale_add, spx_vec_add, spx_vec_sub, spx_vec_mul,
 * spx_vec_copy; reference src/api/matvec.c:838-931, src/internals/
 * Vector.cpp:206-394) so that a CG / GMRES iteration never leaves the GPU.
 * Same argument order and meaning as the host versions; every call enqueues on
 * `stream` (NULL = default stream) and returns immediately, except
 * spx_hip_vec_mul and the download, which synchronise the stream.  A solver
 * loop that must not stall (or that is captured into a hipGraph) keeps its
 * scalars in HBM instead: spx_hip_vec_mul_dev, spx_hip_vec_scale_add_ratio and
 * spx_hip_vec_cg_update below take and leave them there, and only enqueue.
 */
typedef struct spx_hip_vec spx_hip_vec_t;

/* spx.vec.device=true only: tells the library that the client wrote to v->elements directly (a vector from
 * spx_vec_create / spx_vec_create_random); the next spx_matvec_* uploads it again.  Harmless otherwise. */
void spx_hip_vec_touch(const spx_vector_t *v);
/* Diagnostic: how the vector's host memory travels.  0: through staging memory (pageable); 1: page-locked memory of the
 * library's own (spx_vec_create, spx_vec_create_random); 2: a client's buffer that the library page-locked in place
 * (spx.vec.register, from the view's first product on); 3: a client's buffer that was page-locked already. */
int spx_hip_vec_page_locked(const spx_vector_t *v);

spx_hip_vec_t *spx_hip_vec_create(size_t size);                 /* zero-filled        */
spx_hip_vec_t *spx_hip_vec_create_from_host(const spx_vector_t *v);
spx_error_t spx_hip_vec_destroy(spx_hip_vec_t *v);
spx_value_t *spx_hip_vec_data(spx_hip_vec_t *v);               /* HBM pointer        */
size_t spx_hip_vec_size(const spx_hip_vec_t *v);
spx_error_t spx_hip_vec_upload(spx_hip_vec_t *dst, const spx_vector_t *src, void *stream);
spx_error_t spx_hip_vec_download(const spx_hip_vec_t *src, spx_vector_t *dst, void *stream);
spx_error_t spx_hip_vec_init(spx_hip_vec_t *v, spx_value_t val, void *stream);
/* v2 <- num * v1 */
spx_error_t spx_hip_vec_scale(const spx_hip_vec_t *v1, spx_hip_vec_t *v2, spx_value_t num,
                              void *stream);
/* v3 <- v1 + num * v2 */
spx_error_t spx_hip_vec_scale_add(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2,
                                  spx_hip_vec_t *v3, spx_value_t num, void *stream);
/* v3 <- v1 + v2,  v3 <- v1 - v2 */
spx_error_t spx_hip_vec_add(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2,
                            spx_hip_vec_t *v3, void *stream);
spx_error_t spx_hip_vec_sub(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2,
                            spx_hip_vec_t *v3, void *stream);
/* *result <- v1 . v2   (deterministic two-stage reduction) */
spx_error_t spx_hip_vec_mul(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2,
                            spx_value_t *result, void *stream);
spx_error_t spx_hip_vec_copy(const spx_hip_vec_t *v1, spx_hip_vec_t *v2, void *stream);
/* ---- device scalars: a spx_value_t in HBM, given by pointer (typically an element of a small spx_hip_vec_t,
 * spx_hip_vec_data(s) + i).  The three calls below only enqueue: no allocation, no copy to the host, no
 * synchronisation; all are legal during stream capture.  A scalar may not lie inside a vector the call writes. */
/* *result_dev <- v1 . v2, the bits spx_hip_vec_mul returns (same grid, same partial sums, same order) */
spx_error_t spx_hip_vec_mul_dev(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2,
                                spx_value_t *result_dev, void *stream);
/* v3 <- v1 + c * v2,  c = scale * (*num_dev / *den_dev): what spx_hip_vec_scale_add gives for that host value.
 * den_dev == NULL: c = scale * *num_dev;  *den_dev == 0: c = 0.  v3 may be v1 or v2. */
spx_error_t spx_hip_vec_scale_add_ratio(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2, spx_hip_vec_t *v3,
                                        spx_value_t scale, const spx_value_t *num_dev,
                                        const spx_value_t *den_dev, void *stream);
/* One CG update in one pass over the vectors:  a = *rr_dev / *pap_dev (0 if *pap_dev == 0);
 *   x += a*p;  r -= a*ap;  rr_new = r.r (fixed order: reproducible; not the bits of spx_hip_vec_mul(r, r));
 *   *beta_dev = rr_new / *rr_dev (0 if *rr_dev == 0);  *rr_dev = rr_new.
 * x and r are what two spx_hip_vec_scale_add calls with a and -a give.  x, p, r, ap: four different vectors;
 * rr_dev, pap_dev, beta_dev: three different addresses.  With r = p = 0 the call changes nothing (no NaN). */
spx_error_t spx_hip_vec_cg_update(spx_hip_vec_t *x, const spx_hip_vec_t *p, spx_hip_vec_t *r,
                                  const spx_hip_vec_t *ap, spx_value_t *rr_dev,
                                  const spx_value_t *pap_dev, spx_value_t *beta_dev, void *stream);
/* ---- a diagonal preconditioner: elementwise helpers and the fused Jacobi-PCG step.  All four calls only enqueue
 * on `stream`: no allocation, no copy to the host, no synchronisation; all are legal during stream capture. */
/* v3 <- v1 .* v2 (one IEEE multiplication per element; v3 may be v1 or v2) */
spx_error_t spx_hip_vec_mul_elem(const spx_hip_vec_t *v1, const spx_hip_vec_t *v2, spx_hip_vec_t *v3, void *stream);
/* v2 <- 1 / v1 elementwise (IEEE division), if_zero where v1 is +-0; v2 may be v1.  With spx_hip_mat_get_diag_vec
 * in front of it: the Jacobi preconditioner of the matrix (rows without a diagonal entry get if_zero). */
spx_error_t spx_hip_vec_reciprocal(const spx_hip_vec_t *v1, spx_hip_vec_t *v2, spx_value_t if_zero, void *stream);
/* v2 <- 1 / sqrt(v1) elementwise (one IEEE square root, one IEEE division), if_zero where v1 is +-0; v2 may be v1.
 * Enqueue only, legal during stream capture.  Behind spx_hip_mat_norms(SPX_HIP_NORM_MAX_ABS): the factors of one
 * Ruiz equilibration sweep for spx_hip_mat_scale. */
spx_error_t spx_hip_vec_rsqrt(const spx_hip_vec_t *v1, spx_hip_vec_t *v2, spx_value_t if_zero, void *stream);
/* One preconditioned CG update in one pass over the vectors, minv any diagonal preconditioner:
 *   a = *rz_dev / *pap_dev (0 if *pap_dev == 0);  x += a*p;  r -= a*ap;
 *   z_i = minv_i * r_i (one rounded multiplication; z is not stored);
 *   rz_new = sum z_i*r_i;  rr_new = sum r_i*r_i   (both in a fixed order: reproducible)
 *   *beta_dev = rz_new / *rz_dev (0 if *rz_dev == 0);  *rz_dev = rz_new;  *rr_dev = rr_new.
 * x, r and *rr_dev get the bits spx_hip_vec_cg_update gives x, r and its rr for the same a.  p, ap and minv are
 * read only.  One iteration of Jacobi-PCG is a product (ap <- A p), spx_hip_vec_mul_dev(p, ap, pap_dev), this call
 * and spx_hip_vec_pcg_direction.  With *rz_dev = *pap_dev = 0 the call leaves x and r alone and writes
 * rz = z.r, rr = r.r and beta = 0: the start-up call, followed by spx_hip_vec_pcg_direction(p, r, minv, NULL).
 * With r = p = 0 nothing becomes NaN.
 * Refused with SPX_FAILURE through the error handler, nothing enqueued and every input untouched: vectors of
 * different sizes; x, p, r, ap, minv not five different vectors; rz_dev, pap_dev, beta_dev, rr_dev not four
 * different addresses; a scalar inside x or r; a NULL scalar or vector. */
spx_error_t spx_hip_vec_pcg_update(spx_hip_vec_t *x, const spx_hip_vec_t *p, spx_hip_vec_t *r, const spx_hip_vec_t *ap,
                                   const spx_hip_vec_t *minv, spx_value_t *rz_dev, const spx_value_t *pap_dev,
                                   spx_value_t *beta_dev, spx_value_t *rr_dev, void *stream);
/* p <- minv .* r + (*beta_dev) * p: the bits of spx_hip_vec_mul_elem(minv, r, z) followed by
 * spx_hip_vec_scale_add(z, p, p, *beta_dev), without z.  beta_dev == NULL: p <- minv .* r (the bits of z).
 * Refused as above: different sizes; p, r, minv not three different vectors; beta_dev inside p; a NULL vector. */
spx_error_t spx_hip_vec_pcg_direction(spx_hip_vec_t *p, const spx_hip_vec_t *r, const spx_hip_vec_t *minv,
                                      const spx_value_t *beta_dev, void *stream);
/* Diagnostic: a read stream with the stores of an SpMV in it. `src` is read in chunks of `chunk_doubles` (a
 * multiple of 2048), one per workgroup, workgroup b on XCD b % 8 as the SpMV kernels' row-blocks; every workgroup
 * then stores `write_doubles` doubles to its stretch of `dst` (dst->size >= chunks * write_doubles).  Timed by
 * the caller; what bench.py prints as roofline.measured_mixed_peak. */
spx_error_t spx_hip_probe_read_write(const spx_hip_vec_t *src, spx_hip_vec_t *dst, size_t chunk_doubles,
                                     size_t write_doubles, void *stream);
/* y <- alpha*A*x + beta*y on device vectors (spx_matvec_kernel, matvec.c:586-620) */
spx_error_t spx_hip_matvec_kernel_vec(spx_value_t alpha, const spx_matrix_t *A,
                                      const spx_hip_vec_t *x, spx_value_t beta,
                                      spx_hip_vec_t *y, void *stream);
/* y <- alpha*fl32(A)*x + beta*y on device vectors; see spx_hip_matvec_kernel_f32 */
spx_error_t spx_hip_matvec_kernel_f32_vec(spx_value_t alpha, const spx_matrix_t *A, const spx_hip_vec_t *x,
                                          spx_value_t beta, spx_hip_vec_t *y, void *stream);
/* y <- alpha*A^T*x + beta*y on device vectors (x: nrows, y: ncols elements); see spx_hip_matvec_trans_kernel */
spx_error_t spx_hip_matvec_trans_kernel_vec(spx_value_t alpha, const spx_matrix_t *A,
                                            const spx_hip_vec_t *x, spx_value_t beta,
                                            spx_hip_vec_t *y, void *stream);

/* ---- one process per GPU: row-partitioned matrices -------------------------------
 * The reference partitions the rows over the threads of one process
 * (include/sparsex/internals/SparseInternal.hpp:117-152); its symmetric kernel
 * lets every thread add into rows of the threads in front of it through local
 * buffers, and a conflict map says which entries have to be summed afterwards
 * (src/api/matvec.c:302-318, include/sparsex/internals/CsxBuild.hpp:400-451,
 * src/internals/Vector.cpp:291-299).  Here the "threads" are processes, one per
 * MI355X, and the map drives a point-to-point exchange over xGMI:
 *
 *   - every process tunes the rows it owns, either as a slice of the
 *     partitions of a matrix it was given in full (spx.rt.gpu_rank/gpu_world)
 *     or from just those rows (spx.rt.row_offset / spx.rt.global_rows: the
 *     input of spx_input_load_csr holds rows [offset, offset + nrows) of a
 *     matrix with global_rows rows; symmetric: the full rows, of which the part
 *     on and below the diagonal is kept);
 *   - spx_hip_mat_dist_attach() (collective) learns every process' row range,
 *     hands each process' conflict rows to their owners and builds the lists
 *     for the exchange;
 *   - spx_hip_matvec_dist() multiplies and completes the rows this process
 *     owns: general matrices need nothing from the others; symmetric ones send
 *     the sums they formed for rows in front of their own -- only those entries,
 *     packed -- to the owners, which add them in a fixed order.  With
 *     SPX_DIST_GATHER_Y the finished slices are then handed round so that every
 *     process holds all of y (what a solver needs as the next x).
 *
 * The exchange itself goes through a transport: RCCL over xGMI (built in;
 * librccl is loaded when the transport is created, so single-GPU users never
 * pay for it), or two callbacks of the caller's (the CPU tests run the same
 * plan over gloo).  Vectors are full length (ncols / global rows) on every
 * process, as in the reference, where every thread sees all of x.
 */
typedef struct spx_hip_transport {
    void *ctx;
    int rank, world;
    /* Per-peer exchange of 8-byte words in HOST memory; blocking; every
     * process calls it with matching counts (send_cnt[p] here = recv_cnt[me]
     * on p).  Offsets and counts are in words; entries for `rank` itself are
     * ignored.  Returns 0 on success. */
    int (*exchange_host)(void *ctx, const uint64_t *send, const size_t *send_off,
                         const size_t *send_cnt, uint64_t *recv, const size_t *recv_off,
                         const size_t *recv_cnt);
    /* The same for doubles in DEVICE memory, enqueued on `stream` (hipStream_t). */
    int (*exchange_device)(void *ctx, const spx_value_t *send, const size_t *send_off,
                           const size_t *send_cnt, spx_value_t *recv, const size_t *recv_off,
                           const size_t *recv_cnt, void *stream);
} spx_hip_transport_t;

#define SPX_RCCL_ID_BYTES 128
/* rank 0 creates the id and hands it to the others by whatever means the job
 * has (MPI, a file, torch.distributed); then every process creates its
 * transport -- collective, on the current HIP device. */
spx_error_t spx_hip_rccl_unique_id(void *id);
spx_hip_transport_t *spx_hip_transport_rccl(const void *id, int rank, int world);
void spx_hip_transport_destroy(spx_hip_transport_t *t);
/* The number of ranks the transport's RCCL communicator holds (ncclCommCount), or -1 for a transport that
 * was not made by spx_hip_transport_rccl or where librccl does not export the query. */
int spx_hip_transport_rccl_ranks(const spx_hip_transport_t *t);

/* Collective over the transport's processes; the matrix keeps a copy of *t
 * (the transport must outlive the matrix). */
spx_error_t spx_hip_mat_dist_attach(spx_matrix_t *A, const spx_hip_transport_t *t);

#define SPX_DIST_OWNED_ROWS 0   /* y[row_lo, row_hi) complete on return, the rest unspecified */
#define SPX_DIST_GATHER_Y   1   /* all of y complete on every process */
#define SPX_DIST_HALO_X     2   /* y[row_lo, row_hi) complete, and of the other processes' rows exactly the
                                   entries that THIS process' rows read as x (its halo, see
                                   spx_hip_mat_dist_halo): what an iteration x <- y needs here, nothing
                                   more.  Every owner packs the entries each of the others asked for at
                                   attach time and sends them pairwise; ignored with SPX_DIST_GATHER_Y */
#define SPX_DIST_OVERLAP    4   /* with SPX_DIST_HALO_X on the general path: the own product runs in
                                   spx.rt.dist_chunks launches over consecutive parts of the rows, and the
                                   halo entries of part k travel on a second stream while part k + 1 is
                                   computed; `stream` waits for the last round.  Same result; where the
                                   stream cannot be cut (or on the symmetric path, whose conflict rows are
                                   complete only after the whole product) the plain order is used */
/* y <- alpha*A*x + beta*y over all processes; device pointers of full length,
 * everything enqueued on `stream`.  Collective. */
spx_error_t spx_hip_matvec_dist(spx_value_t alpha, const spx_matrix_t *A,
                                const spx_value_t *x_dev, spx_value_t beta,
                                spx_value_t *y_dev, int flags, void *stream);

/* What the exchange of an attached matrix looks like (arrays owned by the matrix). */
typedef struct {
    int32_t rank, world;
    const spx_index_t *row_lo, *row_hi;     /* [world] rows of every process          */
    int64_t n_send;                         /* conflict rows of this process          */
    const spx_index_t *send_rows;           /* ascending, i.e. grouped by owner       */
    const size_t *send_off, *send_cnt;      /* [world] segment of every owner         */
    int64_t n_recv;                         /* entries this process receives          */
    const size_t *recv_off, *recv_cnt;      /* [world] segment of every sender        */
    int64_t n_fix_rows;                     /* own rows that receive something        */
    const spx_index_t *fix_rows;            /* [n_fix_rows] ascending                 */
    const uint32_t *fix_ptr, *fix_pos;      /* per such row: positions in the receive buffer */
    int32_t any_exchange;                   /* some process sends something           */
} spx_hip_dist_plan_t;
spx_error_t spx_hip_mat_dist_plan(const spx_matrix_t *A, spx_hip_dist_plan_t *plan);

/* Partition-aware numbering for a row-partitioned matrix.  Ranges of rows dealt by nonzeros follow the
 * order in which the application numbers its unknowns; where that order keeps coupled unknowns far
 * apart (a KKT matrix [H A^T; A D]: a range of state rows reads a whole range of multipliers), every
 * process needs a large part of the other processes' vectors.  spx_hip_dist_reorder() computes, from the
 * CSR pattern of the whole (square) matrix, a permutation perm[old] = new (0-based, `nrows` entries,
 * caller's array) after which the ranges couple mostly with themselves:
 *   SPX_DIST_REORDER_RCM        reverse Cuthill-McKee (the order spx_mat_tune(.., SPX_MAT_REORDER) uses)
 *   SPX_DIST_REORDER_RCM_OWNER  that order only decides WHICH of `world` ranges (equal nonzeros) a row
 *                               belongs to; inside a range the rows keep their original order, so the
 *                               substructures of the original numbering (runs, diagonals, blocks) survive
 * `flags`: SPX_DIST_PATTERN_SYMMETRIC promises that the pattern equals its transpose (it is then used
 * where it lies; otherwise A + A^T is built).  The caller applies the permutation to rows, columns and
 * vectors (P A P^T, spx_vec_reorder semantics), e.g. rank 0 computes it once and hands it to the others.
 * With the whole matrix given to every process (spx.rt.gpu_rank / gpu_world), the option
 * spx.rt.dist_reorder = none | rcm | rcm_owner makes spx_mat_tune() do all of this itself
 * (spx_mat_get_perm() returns the permutation).  Reference: its reordering is Rcm.hpp:85-121 on one
 * process; it has no partition-aware form. */
#define SPX_DIST_REORDER_RCM        1
#define SPX_DIST_REORDER_RCM_OWNER  2
#define SPX_DIST_PATTERN_SYMMETRIC  1
spx_error_t spx_hip_dist_reorder(const spx_index_t *rowptr, const spx_index_t *colind, spx_index_t nrows,
                                 int indexing /* SPX_INDEX_ZERO_BASED | SPX_INDEX_ONE_BASED */, int world,
                                 int mode, int flags, spx_index_t *perm);

/* The halo of x of an attached matrix (arrays owned by the matrix): the columns outside its
 * own rows that this process' stream reads (found by walking the stream itself), grouped by
 * owner, and the own rows the other processes asked for, grouped by the process that asked. */
typedef struct {
    int64_t n_recv;                         /* entries this process needs of the others        */
    const spx_index_t *recv_cols;           /* ascending, i.e. grouped by owner                */
    const size_t *recv_off, *recv_cnt;      /* [world] segment of every owner                  */
    int64_t n_send;                         /* own entries the others need (with repetitions)  */
    const spx_index_t *send_rows;           /* grouped by the process that asked, ascending    */
    const size_t *send_off, *send_cnt;      /* [world] segment of every such process           */
} spx_hip_dist_halo_t;
spx_error_t spx_hip_mat_dist_halo(const spx_matrix_t *A, spx_hip_dist_halo_t *halo);

/* y <- alpha*A*x + beta*y in `parts` launches over consecutive parts of the rows (equal work each),
 * one after the other on `stream`: what SPX_DIST_OVERLAP interleaves its rounds with, for a caller that
 * wants to interleave communication of its own (or to measure what cutting the launch costs).  General
 * path, plain streams; where the stream cannot be cut the product runs as one launch.  Returns the number
 * of launches through *launched (may be NULL). */
spx_error_t spx_hip_matvec_parts(spx_value_t alpha, const spx_matrix_t *A, const spx_value_t *x_dev,
                                 spx_value_t beta, spx_value_t *y_dev, int parts, void *stream, int *launched);

/* The rounds of the overlapped step (SPX_DIST_OVERLAP) of an attached matrix: round r moves, per
 * peer, the segment [off, off + cnt) of the halo send list (spx_hip_dist_halo_t::send_rows) out and
 * the segment of the halo receive list (recv_cols) in -- the entries that lie in part r of their
 * owner's rows.  Over all rounds every entry travels exactly once.  0 rounds: none planned
 * (spx.rt.dist_chunks <= 1). */
int spx_hip_mat_dist_rounds(const spx_matrix_t *A);
int spx_hip_mat_dist_parts(const spx_matrix_t *A);     /* launches THIS process' product is cut into (0: not cut) */
spx_error_t spx_hip_mat_dist_round(const spx_matrix_t *A, int round, const size_t **send_off, const size_t **send_cnt,
                                   const size_t **recv_off, const size_t **recv_cnt);

/* ---- introspection ---------------------------------------------------------- */
typedef struct {
    int64_t nnz;             /* logical nonzeros of the whole matrix            */
    int64_t nnz_stored;      /* values held by this process (lower+0 diag on sym) */
    int64_t n_unit_elems;    /* of those, inside substructure units             */
    int64_t n_delta_elems;   /* of those, in delta (leftover) regions           */
    int64_t n_units;         /* unit descriptors                                */
    int64_t n_rowblocks;
    int64_t n_shared_rows;   /* rows split over several row-blocks              */
    int64_t value_bytes;     /* values array incl. alignment padding            */
    int64_t index_bytes;     /* descriptors + start bits + column offsets + ... */
    int32_t nr_partitions;   /* P (all processes)                               */
    int32_t first_partition, last_partition;   /* owned: [first, last)          */
    int32_t row_lo, row_hi;  /* rows owned by this process: [lo, hi)            */
    int32_t symmetric;
    int32_t on_device;       /* 0 for host-only matrices                        */
    int32_t device;
    int32_t waves;           /* wavefronts per workgroup of the SpMV kernel      */
    int32_t sym_tiles;       /* symmetric path: the stream holds dense 8x8 tiles
                                that are read once (SPX_PASS_SYMTILE): 1 = their
                                transposed sums go through the spill lists and a
                                second kernel, 2 = straight into y (global atomics) */
    double  tune_seconds;    /* preprocessing (mining + encoding)               */
    double  emit_seconds;    /* descriptor stream + upload                      */
    int32_t wave_tiles;      /* 1: every wavefront of a workgroup adds into a y tile
                                of its own (summed in wavefront order)          */
    int32_t sym_segments;    /* the stream holds row segments of the lower triangle
                                that are read once and used twice (SPX_PASS_SYMSEG):
                                1 = next to dense tiles, 2 = and no tiles           */
    int32_t quad;            /* reserved (0): round 3's kernel variant with four narrow unit
                                passes side by side per wavefront is in use          */
    int32_t col_slices;      /* general path, spx.gpu.col_phases: K > 1 column slices in one
                                launch (a group of XCDs each), -K: launched in turn, else 1 */
    int32_t unit_windows;    /* general path, spx.gpu.unit_windows: 1 = the product stages the columns
                                its unit passes read in LDS (one set of windows per row-block) and
                                runs the unit passes as a software pipeline (csx_spmv_xw_kernel)   */
    int32_t unit_window_lds; /* ... bytes of LDS per workgroup of that kernel (0: no windows planned) */
    int64_t unit_window_elems;  /* ... nonzeros whose x comes from LDS (of n_unit_elems)            */
    int64_t unit_window_staged; /* ... doubles of x staged per product                              */
    int32_t sym_pipeline;    /* symmetric path, spx.gpu.sym_pipeline: 1 = the read-once passes that carry their
                                geometry in the header run pipelined, x requested with the values
                                (csx_spmv_sx_kernel)                                                  */
    int32_t reserved0;
    int64_t sym_pipeline_elems; /* ... nonzeros in such passes (of the nonzeros in read-once passes)    */
} spx_hip_info_t;

spx_error_t spx_hip_mat_info(const spx_matrix_t *A, spx_hip_info_t *info);

/* The unit windows of x (spx.gpu.unit_windows) planned from the matrix' descriptor stream with the given
 * budget (most doubles of x a row-block may stage in LDS) and gap (column intervals closer than this are
 * staged as one): what csx_spmv_xw_kernel is handed next to the stream -- for inspection and tests; works
 * on host-only matrices.  The arrays belong to the matrix and live until the next call or
 * spx_mat_destroy().  Layouts: sparsex_amd/csrc/xwindows.hpp. */
typedef struct {
    const uint32_t *tab;        /* n_rowblocks x 16 entries of {uint32, uint32}: 2 of pass ranges, 14 windows */
    const uint32_t *xdescs;     /* n_descs x {col0 or LDS offset, bits}                                       */
    const void *passes;         /* n_passes pass headers of 24 bytes (flag 2: the pass reads x from LDS)      */
    size_t n_rowblocks, n_descs, n_passes;
    size_t rowblocks_with_windows, rowblocks_with_units;
    uint64_t staged_doubles;    /* doubles of x staged per product                                            */
    uint64_t unit_elems, unit_elems_lds;   /* nonzeros in unit passes / in unit passes that read LDS          */
    uint32_t lds_doubles;       /* LDS of a launch, doubles: y tile + leftover window + unit windows          */
} spx_hip_xw_plan_t;
spx_error_t spx_hip_mat_unit_windows(spx_matrix_t *A, uint32_t budget, uint32_t gap, spx_hip_xw_plan_t *plan);

/* The device-side pass headers of the pipelined read-once kernel (spx.gpu.sym_pipeline), planned from the
 * matrix' descriptor stream: for inspection and tests; works on host-only matrices.  The arrays belong to the
 * matrix and live until the next call or spx_mat_destroy().  Layout of an SX header: sparsex_amd/csrc/sxplan.hpp. */
typedef struct {
    const void *passes;         /* n_passes pass headers of 24 bytes (flag 4: an SX header)                    */
    const uint32_t *n_sx;       /* per row-block: its passes [0, n_sx) are SX passes                            */
    size_t n_rowblocks, n_passes;
    size_t rowblocks_with_sx;
    uint64_t sym_elems, sx_elems;     /* nonzeros in read-once passes / of those, in SX passes                  */
    uint64_t sym_passes, sx_passes;
} spx_hip_sx_plan_t;
spx_error_t spx_hip_mat_sym_pipeline(spx_matrix_t *A, spx_hip_sx_plan_t *plan);

/* New values, same pattern: the outer loop of a Newton method, a time stepper or an interior-point solver keeps
 * the sparsity pattern and changes every value.  Instead of a new tune, or one spx_mat_set_entry per nonzero
 * (all the reference offers, src/api/matvec.c:376-407), the tuned stream is tied to the caller's CSR arrays
 * ONCE (spx_hip_mat_values_plan, host side) and every outer iteration gathers the new value array into the
 * stream in one bandwidth-bound pass (spx_hip_mat_set_values: csx_refresh_values_kernel).
 *
 *  - Which arrays: rowptr, colind and the value arrays are the ones given to spx_input_load_csr for this
 *    matrix -- the same rows (the slice's rows for an input loaded with spx.rt.row_offset, the whole matrix
 *    with spx.rt.gpu_rank/world), the same indexing (SPX_INDEX_ZERO_BASED / SPX_INDEX_ONE_BASED), columns of a
 *    row in any order the loader accepts.
 *  - A matrix tuned with SPX_MAT_REORDER or spx.rt.dist_reorder is addressed in the caller's numbering: the plan
 *    goes through the inverse of the matrix' permutation.
 *  - Symmetric matrices: the stream holds the entries on and below the diagonal of the tuned numbering; the plan
 *    takes each from exactly the CSR position the tune read, from the transposed position where that one is
 *    absent.  The caller's values must be symmetric.
 *  - Every stored copy is written: lower triangle, mirror image, the thin mirror list of a slice, the diagonal
 *    array, every column slice of spx.gpu.col_phases.
 *  - A process of a row-partitioned matrix plans the entries its own stream holds.
 *  - The plan fails with SPX_FAILURE through the error handler, the first offending (row, column) named, unless
 *    every CSR entry the process owns has at least one destination and every real position of the stream has a
 *    source: a pattern that is not the tuned one, a row with a repeated column, an entry the tune did not
 *    keep.  A failed call leaves no plan behind (the values stay as they are).
 *  - Positions without a source -- pass padding, lanes beyond a segment's length, absent cells of an 8x8 tile,
 *    the zero a dense block of a symmetric stream holds where it closes over the diagonal (the diagonal has an
 *    array of its own) -- hold, after any number of updates, exactly the bits the tune put there.
 *  - spx_hip_mat_set_values only enqueues on `stream` (a hipStream_t): no allocation, no wait, legal during
 *    stream capture.  It obeys the handle's single-stream rule: the stream orders it with the matrix' products.
 *    `values_dev` holds as many doubles as the planned CSR arrays hold entries, in HBM of the matrix' device.
 *  - It counts as "a product was enqueued since the last edit" for spx_mat_set_entry's wait-once rule; after it
 *    spx_mat_get_entry, spx_mat_set_entry, spx_mat_save and every product (forward, transposed, multi-vector,
 *    in parts, distributed) see the new values.
 *  - spx_hip_mat_set_values_host takes a host array and is synchronous: on a matrix in HBM the array goes up into
 *    a temporary buffer in pieces through page-locked staging, the kernel runs, the buffer is freed; on a
 *    host-only matrix (spx.rt.host_only) the host threads apply the plan to the host copy of the stream.
 *  - The values of the encoded partitions (spx_hip_mat_export_csx) are stale after a bulk update: from the first
 *    successful spx_hip_mat_set_values* on, spx_hip_mat_export_csx fails and says so -- it never hands out old
 *    values.  spx_hip_mat_export_units (the pattern) keeps working.  While they are stale spx_mat_set_entry leaves
 *    them alone and spx_mat_save writes the file without them: a matrix restored from it has none to export.  (A
 *    host-only matrix knows when spx_hip_mat_set_values_host has put back, bit for bit, the values it held before
 *    the first update: its partitions are true again, exported again and saved again.)
 *  - spx_hip_mat_values_plan leaves the calling thread's current device as it found it.
 *  - The plan is not part of a saved matrix: after spx_mat_restore it is built again from the CSR arrays (a
 *    restored matrix, which may hold no encoded partitions, works like a tuned one).  A second
 *    spx_hip_mat_values_plan replaces the first; spx_hip_mat_values_plan_drop and spx_mat_destroy release it.
 *  - spx_hip_mat_set_values* fail with SPX_FAILURE without a plan, with a NULL handle or pointer, when the
 *    calling thread's current device is not the matrix' one, and spx_hip_mat_set_values on a host-only matrix.
 *  - Cost: one uint32_t per stored value (spx_index_t is 32-bit, so a CSR index fits) in HBM and once more on the
 *    host -- about half of value_bytes, 3 GB on a matrix of 769 M nonzeros.  */
spx_error_t spx_hip_mat_values_plan(spx_matrix_t *A, const spx_index_t *rowptr, const spx_index_t *colind, int indexing);
spx_error_t spx_hip_mat_values_plan_drop(spx_matrix_t *A);
spx_error_t spx_hip_mat_set_values(spx_matrix_t *A, const spx_value_t *values_dev, void *stream);
spx_error_t spx_hip_mat_set_values_host(spx_matrix_t *A, const spx_value_t *values);
/* The plan, for inspection and tests: the arrays belong to the matrix and live until the next
 * spx_hip_mat_values_plan, spx_hip_mat_values_plan_drop or spx_mat_destroy(). */
typedef struct {
    const uint32_t *src_values;   /* per position of the stream's values: CSR index, or 0xffffffff (no source) */
    const uint32_t *src_mirror;   /* per entry of the thin mirror list of a symmetric slice                    */
    const uint32_t *src_diag;     /* symmetric: per own row, CSR index of its diagonal entry or 0xffffffff      */
    size_t n_values, n_mirror, n_diag;
    uint64_t n_sources;           /* CSR entries this process' stream holds at least once                      */
    uint64_t n_dest;              /* positions with a source, over the three arrays                            */
    uint64_t plan_bytes;          /* HBM the plan occupies (0 on a host-only matrix)                           */
} spx_hip_values_plan_t;
spx_error_t spx_hip_mat_values_plan_get(const spx_matrix_t *A, spx_hip_values_plan_t *plan);

/* The diagonal of a tuned matrix, for a Jacobi preconditioner (spx_hip_vec_reciprocal, spx_hip_vec_pcg_update):
 * read from the values as they are NOW -- after spx_hip_mat_set_values they may exist only in HBM -- and in the
 * numbering of the products' vectors, which is the tuned one under SPX_MAT_REORDER / spx.rt.dist_reorder.  The
 * reference hands out one entry per call (spx_mat_get_entry, src/api/matvec.c:340-374).
 *
 *  - spx_hip_mat_diag_plan (host side, once per tune or restore) finds in ONE walk over the descriptor stream,
 *    on all host threads, the position of a(i, i) in the stream's value array for every own row i, or 0xffffffff.
 *    It works on the index-only host copy of a matrix in HBM and on host-only matrices (spx.rt.host_only).  It
 *    fails with SPX_FAILURE through the error handler when a diagonal entry lies at two positions or the value
 *    array has 2^32 - 1 positions or more; a failed call leaves no plan behind, an earlier one included.
 *  - The position array goes to HBM once: 4 bytes per own row (plan_bytes; 0 on a host-only matrix).  The call
 *    leaves the calling thread's current device as it found it.
 *  - Symmetric matrices keep their diagonal in an array of its own in HBM: the plan call succeeds and plans
 *    nothing (pos == NULL, n_present == 0, plan_bytes == 0), and spx_hip_mat_get_diag* work without a plan call.
 *  - The plan is not part of a saved matrix: after spx_mat_restore it is built again.  A second
 *    spx_hip_mat_diag_plan replaces the first; spx_hip_mat_diag_plan_drop and spx_mat_destroy release it.
 *  - spx_hip_mat_get_diag enqueues ONE kernel (csx_gather_diag_kernel) on `stream` (a hipStream_t): no
 *    allocation, no wait, legal during stream capture.  It obeys the handle's single-stream rule: the stream
 *    orders it with spx_hip_mat_set_values and the matrix' products.  It counts as "a product was enqueued since
 *    the last edit" for spx_mat_set_entry's wait-once rule.
 *  - `d_dev` holds nrows doubles in HBM of the matrix' device, 8-byte aligned (16-byte stores are used where the
 *    address allows).  d[i] = a(i, i) for the own rows; +0.0 for a row without a stored diagonal entry and for a
 *    row i >= ncols of a rectangular matrix.  A row slice (spx.rt.gpu_rank/world, spx.rt.row_offset) or an
 *    attached matrix writes [row_lo, row_hi) and leaves the rest alone.
 *  - It reads the doubles where they live: it sees what spx_hip_mat_set_values* and spx_mat_set_entry wrote, with
 *    or without a float copy (spx.gpu.values_f32), in every column slice of spx.gpu.col_phases.
 *  - spx_hip_mat_get_diag_vec: the same into a device vector of nrows elements.
 *  - spx_hip_mat_get_diag_host is synchronous and takes a host array of nrows doubles: on a matrix in HBM through
 *    a temporary device buffer, on a host-only matrix from the host copy of the stream.
 *  - spx_hip_mat_get_diag* fail with SPX_FAILURE through the error handler, nothing enqueued and nothing written,
 *    with a NULL handle or pointer, on a general matrix without a plan ("no diagonal plan"), when the calling
 *    thread's current device is not the matrix' one, spx_hip_mat_get_diag[_vec] on a host-only matrix (use
 *    _host), and _vec with a vector whose size is not nrows. */
spx_error_t spx_hip_mat_diag_plan(spx_matrix_t *A);
spx_error_t spx_hip_mat_diag_plan_drop(spx_matrix_t *A);
spx_error_t spx_hip_mat_get_diag(const spx_matrix_t *A, spx_value_t *d_dev, void *stream);
spx_error_t spx_hip_mat_get_diag_vec(const spx_matrix_t *A, spx_hip_vec_t *d, void *stream);
spx_error_t spx_hip_mat_get_diag_host(const spx_matrix_t *A, spx_value_t *d);
/* The plan, for inspection and tests: the array belongs to the matrix and lives until the next
 * spx_hip_mat_diag_plan, spx_hip_mat_diag_plan_drop or spx_mat_destroy(). */
typedef struct {
    const uint32_t *pos;          /* per own row: position of a(i, i) in the stream's values, or 0xffffffff;
                                     NULL on a symmetric matrix                                              */
    size_t n_rows, row_lo;        /* own rows, the first of them                                             */
    uint64_t n_present;           /* own rows with a stored diagonal entry (symmetric: 0, nothing is planned) */
    uint64_t plan_bytes;          /* HBM the plan occupies (0 on host-only and symmetric matrices)           */
} spx_hip_diag_plan_t;
spx_error_t spx_hip_mat_diag_plan_get(const spx_matrix_t *A, spx_hip_diag_plan_t *plan);

/* Row and column norms and in-place diagonal scaling of a tuned matrix, A <- D_r * A * D_c: what a solver does
 * to a matrix before it iterates (PETSc: MatGetRowMaxAbs, MatGetColumnNorms, MatNorm, MatDiagonalScale), in ONE
 * pass over the stream where it lies -- no plan, no second copy of the matrix, no host round trip.  GENERAL tunes
 * (whole matrices, row slices, every spx.gpu.col_phases setting, unit windows, spx.gpu.deterministic, reordered
 * matrices, with or without the float copy of the values).
 *
 *  Vectors
 *  - They use the numbering of the products' vectors: the tuned one under SPX_MAT_REORDER / spx.rt.dist_reorder.
 *  - `rows` and `dr` hold nrows doubles, `cols` and `dc` hold ncols doubles; 8-byte aligned.  The _dev pointers
 *    lie in HBM of the matrix' device, the others in host memory.
 *  Row slices (spx.rt.gpu_rank/world, spx.rt.row_offset)
 *  - A row slice reads and writes [row_lo, row_hi) of `rows` and `dr` and leaves the rest alone.
 *  - It writes ALL of `cols` with this process' partial result; the caller all-reduces it: a sum for the two sum
 *    kinds, a maximum for the max kind.
 *  Results of spx_hip_mat_norms*
 *  - kind SPX_HIP_NORM_SUM_ABS: rows[r] = sum_c |a(r,c)|, cols[c] = sum_r |a(r,c)| (their maxima are ||A||_inf and
 *    ||A||_1); SPX_HIP_NORM_SUM_SQ: the sums of squares (the caller takes the root; their sum is ||A||_F^2);
 *    SPX_HIP_NORM_MAX_ABS: the largest |a(r,c)|.  Only stored entries count, padding is never read into a result.
 *  - A row or column with nothing stored gives +0.0.
 *  - The sum kinds are accumulated atomically: within the fp64 bound of a sum of n non-negative terms in any order
 *    (n * 2^-53 relative), not bit-reproducible.  The max kind is exact.
 *  - Either of rows / cols may be NULL: it is not computed.
 *  Scaling
 *  - The new value of a stored a(r,c) is fl(fl(dr[r] * a) * dc[c]): two IEEE multiplications in this order.  With
 *    dr or dc NULL that product is not formed at all.
 *  - spx_hip_mat_scale rewrites the doubles in HBM.  Every later product sees the new values -- forward,
 *    transposed, multi-vector, float, in parts -- and so do spx_hip_mat_get_diag*, spx_mat_get_entry /
 *    spx_mat_set_entry and spx_mat_save.  The float copy (spx.gpu.values_f32) is rewritten in the same call, each
 *    new double rounded to nearest even.
 *  - Positions of the value array that hold no entry (pass padding, lanes beyond a piece's length) keep their bits.
 *  - Diagonal and values plans stay valid; a later spx_hip_mat_set_values* simply overwrites with what the caller
 *    hands over (a Newton code calls set_values, then scale, every outer iteration).
 *  Encoded partitions
 *  - They go stale exactly as after spx_hip_mat_set_values: spx_hip_mat_export_csx then fails and says so,
 *    spx_hip_mat_export_units keeps working, spx_mat_save writes the file without them.  (A host-only matrix with a
 *    values plan knows when a scaling has put back, bit for bit, the values held before the first update.)
 *  Calling rules
 *  - spx_hip_mat_norms and spx_hip_mat_scale only enqueue on `stream` (a hipStream_t): no allocation, no wait;
 *    both are legal during stream capture, obey the handle's single-stream rule and count as "a product was
 *    enqueued since the last edit" for spx_mat_set_entry's wait-once rule.
 *  - The _host forms are synchronous: on a matrix in HBM through temporary device buffers, on a host-only matrix
 *    (spx.rt.host_only) on the host threads over the host copy of the stream.
 *  Failures: SPX_FAILURE through the error handler, nothing enqueued and nothing written, with a NULL handle, a
 *  `kind` out of range, both outputs NULL, both scale vectors NULL, a calling thread whose current device is not
 *  the matrix' one, a device form on a host-only matrix, a matrix tuned as a symmetric one (served by spx_hip_mat_sym_norms
 *  / spx_hip_mat_sym_scale below), and a matrix with an exchange plan attached (spx_hip_mat_dist_attach). */
#define SPX_HIP_NORM_SUM_ABS 0   /* rows: sum_c |a(r,c)|   cols: sum_r |a(r,c)|  */
#define SPX_HIP_NORM_SUM_SQ  1   /* sums of squares (the caller takes the root)   */
#define SPX_HIP_NORM_MAX_ABS 2
spx_error_t spx_hip_mat_norms(const spx_matrix_t *A, int kind, spx_value_t *rows_dev, spx_value_t *cols_dev, void *stream);
spx_error_t spx_hip_mat_norms_host(const spx_matrix_t *A, int kind, spx_value_t *rows, spx_value_t *cols);
spx_error_t spx_hip_mat_scale(spx_matrix_t *A, const spx_value_t *dr_dev, const spx_value_t *dc_dev, void *stream);
spx_error_t spx_hip_mat_scale_host(spx_matrix_t *A, const spx_value_t *dr, const spx_value_t *dc);

/* Norms and the scaling D * A * D of a matrix tuned as a symmetric one, where it lies: the read-once tiles and
 * segments, the lower copies and mirror images, the diagonal array and the thin mirror list of a row slice, whatever
 * kernel family the product runs (whole matrices, row slices, reordered matrices, spx.gpu.deterministic, with or
 * without the float copy spx.gpu.values_f32=all).  A symmetric matrix has ONE norm vector -- the norm of row i is
 * that of column i -- and only the scaling with the same vector on both sides keeps it symmetric.
 *
 *  Vectors
 *  - `out` and `d` hold nrows doubles in the numbering of the products' vectors (the tuned one under
 *    SPX_MAT_REORDER / spx.rt.dist_reorder), 8-byte aligned; the _dev pointers lie in HBM of the matrix' device.
 *  Norms
 *  - out[i] is the norm of row i of the full matrix, which is also that of column i; `kind` as above.
 *  - Only stored entries count.  An off-diagonal entry that the stream holds once (read-once tile or segment)
 *    counts for its row and for its column; an entry that it holds twice (lower copy and mirror image) counts once
 *    per copy, for that copy's row; the diagonal counts for its row.  A row with nothing stored gives +0.0.
 *  - The max kind is exact.  The sum kinds are accumulated atomically: within n * 2^-53 relative, not
 *    bit-reproducible.
 *  Scaling
 *  - The new value of a stored a(r,c) is fl(fl(d[max(r,c)] * a) * d[min(r,c)]): two IEEE multiplications, the
 *    factor of the larger index first.  For the stored lower triangle that is spx_hip_mat_scale(A, d, d)'s
 *    fl(fl(d[r] * a) * d[c]); a mirror image gets the bits of its lower copy, so the stored matrix stays symmetric
 *    bit for bit.  The diagonal becomes fl(fl(d[i] * a) * d[i]).
 *  - The float copy (spx.gpu.values_f32=all) is rewritten in the same call, each new double rounded to nearest
 *    even; the diagonal array and the thin mirror list have no float twin and stay doubles.
 *  - Scaling by powers of two is exact and undone by their reciprocals.
 *  - Not written: pass padding, lanes beyond a gather piece, a position of a row-block pass with row == column
 *    (the zero a block holds where it closes over the diagonal; it is not counted either), and a +-0 inside a pass
 *    of 8x8 tiles (a cell the matrix need not hold): they keep their bits.
 *  Row slices (spx.rt.gpu_rank/world, spx.rt.row_offset, no exchange plan)
 *  - The process accounts for the lower triangle and the diagonal of its own rows; the mirror image of those
 *    entries lands on rows in front of the slice.  spx_hip_mat_sym_norms* therefore writes ALL nrows elements of
 *    `out` with this process' partial result, zero where it holds nothing, and the caller all-reduces: a sum for
 *    the two sum kinds, a maximum for the max kind.
 *  - spx_hip_mat_sym_scale* reads `d` wherever its entries reach, that is over all of [0, row_hi).  Every process
 *    scales with the same `d`.
 *  Everything else as for spx_hip_mat_norms / spx_hip_mat_scale
 *  - The device forms only enqueue on `stream`: no allocation, no wait, legal during stream capture; the
 *    single-stream rule holds and they count as "a product was enqueued since the last edit".
 *  - The _host forms are synchronous; on a host-only matrix they work on the host copy of the stream.
 *  - Later products, spx_hip_mat_get_diag*, spx_mat_get_entry and spx_mat_save see the scaled matrix; values and
 *    diagonal plans stay valid; the encoded partitions go stale exactly as after spx_hip_mat_set_values, with the
 *    same digest rule on a host-only matrix with a values plan.
 *  Failures: SPX_FAILURE through the error handler, nothing enqueued and nothing written, with a NULL handle, a
 *  matrix tuned as a general one (spx_hip_mat_norms / spx_hip_mat_scale(A, d, d) serve it), a matrix with an exchange
 *  plan attached, a device form on a host-only matrix, a calling thread whose current device is not the matrix'
 *  one, a `kind` out of range and a NULL vector. */
spx_error_t spx_hip_mat_sym_norms(const spx_matrix_t *A, int kind, spx_value_t *out_dev, void *stream);
spx_error_t spx_hip_mat_sym_norms_host(const spx_matrix_t *A, int kind, spx_value_t *out);
spx_error_t spx_hip_mat_sym_scale(spx_matrix_t *A, const spx_value_t *d_dev, void *stream);
spx_error_t spx_hip_mat_sym_scale_host(spx_matrix_t *A, const spx_value_t *d);

/* The same for a caller compiled against another revision of this header: at most `size` bytes
 * (the caller's sizeof(spx_hip_info_t)) are written -- the struct only ever grows at its end.
 * spx_hip_mat_info() writes sizeof(spx_hip_info_t) of THIS header; SPX_HIP_ABI_VERSION changes
 * whenever the struct grows (round 3 added quad and col_slices: version 3; round 5 the four
 * unit_window fields: version 4; round 6 the sym_pipeline fields: version 5). */
#define SPX_HIP_ABI_VERSION 5
spx_error_t spx_hip_mat_info_sized(const spx_matrix_t *A, void *info, size_t size);
int spx_hip_abi_version(void);

/* Diagnostic: the number of parts the last spx_matvec_mult / spx_matvec_kernel on HOST vectors ran in (a large y
 * travels back part by part behind the product; 0: the product ran in one piece). */
int spx_hip_mat_host_parts(const spx_matrix_t *A);
/* ... and, where x of that call went up piece by piece in the order the parts needed it (general streams; the part
 * that needs the fewest pieces not yet on the device runs first, so that x on its way up and finished rows of y on
 * their way back share the link), the order the parts ran in: up to `cap` part numbers are written, the number of
 * parts is returned; 0 when x went up as a whole or not at all (resident since the last call). */
int spx_hip_mat_host_order(const spx_matrix_t *A, int32_t *order, int cap);
/* Inspection (host side; works on a matrix tuned with spx.rt.host_only=true): which pieces of x -- of `piece`
 * elements each, at most 64 of them -- every row-block of the stream reads: bit p of mask[i] for the columns
 * [p * piece, (p + 1) * piece), a superset; row0 / n_rows: the row-block's rows.  Any of the arrays may be NULL; up
 * to `cap` entries are written, the number of row-blocks is returned (-1: error).  The plan behind
 * spx_hip_mat_host_order is made of these. */
int64_t spx_hip_mat_x_pieces(spx_matrix_t *A, size_t piece, uint64_t *mask, uint32_t *row0, uint32_t *n_rows, size_t cap);

/* ---- export in the reference's CSX layout --------------------------------------
 * `part` is a global partition number owned by this process.  The arrays
 * stay owned by the matrix and live until spx_mat_destroy().
 */
typedef struct {
    const spx_value_t *values;   /* nnz values in unit order                    */
    const uint8_t *ctl;          /* ctl byte stream                              */
    int64_t ctl_size;
    spx_index_t nnz, ncols, nrows, row_start;
    int32_t row_jumps;           /* 1 if any unit carries a row jump             */
    int32_t full_colind;         /* 1: 32-bit absolute columns, 0: varint jumps  */
    long id_map[64];             /* slot -> pattern id, -1 terminated            */
    const spx_index_t *rows_info;/* nrows x {rowptr, valptr, span}               */
    const spx_value_t *dvalues;  /* symmetric: nrows diagonal values, else NULL  */
} spx_csx_export_t;

spx_error_t spx_hip_mat_export_csx(const spx_matrix_t *A, int part,
                                   spx_csx_export_t *out);

/* One record per unit of a partition after preprocessing, in row-major anchor
 * order: {type, delta, size, row, col} (1-based coordinates inside the
 * partition; type 0 = single leftover nonzero).  Returns the number of
 * records; fills at most `cap` of them. */
typedef struct {
    int32_t type, delta, size, row, col;
} spx_unit_record_t;

int64_t spx_hip_mat_export_units(const spx_matrix_t *A, int part,
                                 spx_unit_record_t *recs, int64_t cap);

/* The preprocessing log of the last spx_mat_tune() of this matrix (statistics
 * per round, chosen encodings); NUL-terminated, owned by the matrix. */
const char *spx_hip_mat_tune_log(const spx_matrix_t *A);

/* The coordinate maps between iteration orders used by the preprocessor
 * (reference include/sparsex/internals/Xform.hpp:37-248): transforms the
 * 1-based (*row, *col) from order `from` to order `to` (EncType numbering:
 * 1 h, 2 v, 3 d, 4 ad, 5..12 br1..8, 13..20 bc1..8).  Exposed for tests. */
void spx_hip_xform(int from, int to, spx_index_t *row, spx_index_t *col,
                   spx_index_t nr_rows, spx_index_t nr_cols);

/* Restores every option to its default (the reference keeps options in a
 * process-wide singleton with no reset; tests need one). */
void spx_hip_options_reset(void);

#ifdef __cplusplus
}
#endif

#endif /* SPARSEX_HIP_H */
