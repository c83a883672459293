// device.hpp -- HBM-resident form of a tuned matrix and the launch entry
// points of the HIP interpreter (implemented in device_runtime.cpp, which launches
// the kernels of spmv_kernels.hip, spmv_xw_kernels.hip and spmv_sx_kernels.hip).
//
// Replaces the reference's JIT'd per-partition spmv_fn + thread-pool dispatch
// (src/internals/CsxKernels.cpp:35-129, src/internals/CsxSpmv.cpp:28-86).
#pragma once

#include "gpu_emit.hpp"

#include <functional>
#include <string>
#include <vector>

namespace spx {

struct DeviceMatrix;   // opaque; owns device allocations

// Throws FatalError (message includes the HIP error string) on any failure.
int device_count();                       // 0 when no usable HIP device
DeviceMatrix *device_upload(const GpuStream &s, size_t nrows, size_t ncols,
                            bool symmetric, idx_t own_row_lo, idx_t own_row_hi,
                            int device);
void device_free(DeviceMatrix *m);

// y <- alpha*A*x + beta*y on device pointers, asynchronous on `stream`
// (a hipStream_t passed as void*; NULL = default stream).
void device_spmv(DeviceMatrix *m, double alpha, const double *d_x, double beta,
                 double *d_y, void *stream);

// The float twin of the stream's values (spx.gpu.values_f32: general streams, and symmetric ones where the caller
// read "all" -- the twin of `values` only, the diagonal and the thin mirror list are rounded by the float product
// in registers): device_build_values_f32
// allocates it (an allocation of its own, also with spx.gpu.arena) and fills it from the doubles in HBM with
// csx_narrow_values_kernel -- synchronous, once per tune or restore, after the launch tuner has settled;
// FatalError naming the size where HBM has no room.  device_values_f32_bytes: 4 bytes per stream value, 0 without
// a twin.  device_spmv_f32: device_spmv with fl32(A) -- the handle's family and wavefronts, the kernels that
// load floats; FatalError where there is no twin.  device_set_values and device_poke keep the twin true.
void device_build_values_f32(DeviceMatrix *m);
int64_t device_values_f32_bytes(const DeviceMatrix *m);
double device_time_narrow_values(DeviceMatrix *m);     // seconds of one run of the narrowing kernel (tools)
void device_spmv_f32(DeviceMatrix *m, double alpha, const double *d_x, double beta,
                     double *d_y, void *stream);

// y <- alpha*A^T*x + beta*y on device pointers (d_x: nrows doubles, global rows for a row slice; d_y: ncols),
// asynchronous on `stream`, no allocation.  Symmetric matrices run device_spmv.  General ones: csx_spmv_t_kernel
// (spmv_t_kernels.hip) over the same stream, results through atomics; a row slice yields this process' partial
// vector over all columns.  The caller keeps attached general matrices away.
void device_spmv_trans(DeviceMatrix *m, double alpha, const double *d_x, double beta,
                       double *d_y, void *stream);
// spx.gpu.trans_windows as read where the device copy is built (0 false, 1 true, -1 auto) / what it came to:
// 0 symmetric, 1 one atomic per nonzero, 2 unit windows accumulate in LDS
void device_set_trans_windows(DeviceMatrix *m, int mode);
int device_trans_mode(const DeviceMatrix *m);

// Y <- alpha*A*X + beta*Y for nvec vectors at once (column-major: vector j of X at d_X + j * ldx, of Y at
// d_Y + j * ldy); column j is what device_spmv writes for it.  Groups of device_mv_group(m) vectors share one
// pass over the stream (spmv_mv_kernels.hip); asynchronous on `stream`, no allocation.
void device_spmm(DeviceMatrix *m, double alpha, const double *d_X, size_t ldx, size_t nvec, double beta,
                 double *d_Y, size_t ldy, void *stream);
// vectors per pass over the stream: 2, 4 or 8, or 1 (streams with symmetric tiles or read-once segments: one
// single-vector product per column)
int device_mv_group(const DeviceMatrix *m);
// ... for nvec vectors of ROW-MAJOR blocks (entry (i, j) of X at d_X + i * ldx + j, of Y at d_Y + i * ldy + j);
// column j is what device_spmv writes for column j of X.  General streams only (FatalError otherwise: the
// single-vector kernels cannot read a strided x); groups of device_mv_group_rm(m) vectors, then 4 / 2 / 1, share
// one pass over the stream (spmv_mvr_kernels.hip); asynchronous on `stream`, no allocation.
void device_spmm_rm(DeviceMatrix *m, double alpha, const double *d_X, size_t ldx, size_t nvec, double beta,
                    double *d_Y, size_t ldy, void *stream);
// vectors per pass of that product: 8, 4, 2 or 1; 0: a stream it does not serve (symmetric)
int device_mv_group_rm(const DeviceMatrix *m);
// The two multi-vector products with fl32(A), through the kernels that read the float twin of the values
// (spmv_mv_f32_kernels.hip, spmv_mvr_f32_kernels.hip): column j is what device_spmv_f32 writes for column j of X.
// The groups, families, wavefronts, LDS and staging of device_spmm / device_spmm_rm; FatalError where there is no
// twin (and every FatalError of the fp64 product of the same layout).  device_mv_group_f32: device_mv_group where
// the plain K-vector kernels run; 1 on streams with symmetric tiles or read-once segments, spx.gpu.sym_matmat or
// not (one device_spmv_f32 per column: never the fp64 group kernel); 0 without a twin.  The row-major group is
// device_mv_group_rm.
void device_spmm_f32(DeviceMatrix *m, double alpha, const double *d_X, size_t ldx, size_t nvec, double beta,
                     double *d_Y, size_t ldy, void *stream);
int device_mv_group_f32(const DeviceMatrix *m);
void device_spmm_rm_f32(DeviceMatrix *m, double alpha, const double *d_X, size_t ldx, size_t nvec, double beta,
                        double *d_Y, size_t ldy, void *stream);

// The product in K launches over consecutive parts of the row-blocks (equal work each), so that
// the exchange of a row-partitioned matrix can start on the rows of part k while part k + 1 is
// computed (dist.cpp).  Plain general streams only: device_plan_chunks returns 0 for the others;
// `row_bounds` receives the first row of every part and the end of the own rows.
// `slot`: 0 = the cut of an attached exchange plan, 1 = a caller's own (spx_hip_matvec_parts): independent of each other
size_t device_plan_chunks(DeviceMatrix *m, size_t K, std::vector<size_t> &row_bounds, int slot = 0);
// `position` (symmetric streams, whose parts may run in any order): bit 0 = this part is launched first, bit 1 = last;
// -1 = by its number
void device_spmv_chunk(DeviceMatrix *m, size_t k, double alpha, const double *d_x, double beta,
                       double *d_y, void *stream, int slot = 0, int position = -1);

// host-vector convenience path used by spx_matvec_*: H2D x (and y when
// beta != 0), kernel, D2H y; synchronous.  Vectors the library allocated itself
// are pinned (device_host_alloc) and are copied from / to directly; user
// buffers go through pinned staging copies.
// `after(d_y, stream)`, if given, runs between the kernel and the copy back (the
// exchange of a row-partitioned matrix).
// `x_version` != 0 names the contents of h_x (spx.vec.device: library-created
// vectors carry a version that every spx_vec_* mutator advances): the copy of x in
// HBM is reused while the version stays the same.
void device_spmv_host(DeviceMatrix *m, double alpha, const double *h_x, bool x_pinned,
                      double beta, double *h_y, bool y_pinned,
                      const std::function<void(double *, void *)> &after = nullptr,
                      uint64_t x_version = 0);

// true while `stream` (a hipStream_t) is being captured into a hipGraph
bool device_stream_is_capturing(void *stream);

// page-locked host memory for the library's own vectors; nullptr when there is
// no HIP device (the caller falls back to malloc)
void *device_host_alloc(size_t bytes);
void device_host_free(void *p);
// a client's buffer page-locked where it lies (1: done, 2: it already was, 0: not possible) / released again
size_t device_host_parts_min_bytes();    // vectors of this size and more: y back in parts (32 MB; tests lower it)
int device_host_register(void *p, size_t bytes);
void device_host_unregister(void *p);

// symmetric slice: the first kernel clears y on rows [first_row, own rows) only
// (default 0: the whole partial vector is defined, for a caller-side all-reduce)
void device_set_init_rows(DeviceMatrix *m, size_t first_row);

// symmetric tiles: hand the transposed sums over with global atomics (true) or
// through the spill array and a second kernel (false)
void device_set_sym_atomic(DeviceMatrix *m, bool on);
bool device_get_sym_atomic(const DeviceMatrix *m);
bool device_has_spill(const DeviceMatrix *m);

// spx.gpu.deterministic: every wavefront of a workgroup adds into a y tile of its own, the
// copies are summed in wavefront order -- repeated products are bit-identical
void device_set_deterministic(DeviceMatrix *m, bool on);
bool device_get_deterministic(const DeviceMatrix *m);
// the per-wavefront tiles alone (also a speed option: no two wavefronts add to the same LDS
// address; spx_mat_tune measures it on matrices without symmetric tiles)
void device_set_wave_tiles(DeviceMatrix *m, bool on);
bool device_get_wave_tiles(const DeviceMatrix *m);
bool device_has_tiles(const DeviceMatrix *m);

// wavefronts per workgroup of the SpMV kernel: 2, 4 or 8
void device_set_waves(DeviceMatrix *m, int waves);
int device_get_waves(const DeviceMatrix *m);

// unit windows of x in LDS + pipelined unit passes (csx_spmv_xw_kernel; xwindows.hpp): available where
// the stream was uploaded with a window budget and some row-block's columns fit it
bool device_has_xw(const DeviceMatrix *m);
int device_host_order(const DeviceMatrix *m, int32_t *order, int cap);   // the order of those parts when x went up piece by piece as they needed it (returns their number; 0: x went up whole or not at all)
void device_set_host_parts(DeviceMatrix *m, size_t parts);   // spx.rt.host_parts: 0 = the built-in choice, else at most 64
int device_host_parts(const DeviceMatrix *m);   // parts of the last product on host vectors whose y went back part by part (0: whole)
void device_set_xw(DeviceMatrix *m, bool on);
bool device_get_xw(const DeviceMatrix *m);
void device_xw_info(const DeviceMatrix *m, uint64_t &elems_lds, uint64_t &unit_elems, uint64_t &staged_doubles,
                    uint32_t &lds_bytes);

// the read-once passes of a symmetric stream pipelined (csx_spmv_sx_kernel; sxplan.hpp): available where the
// stream holds read-once row segments, no tiles, and was uploaded with GpuStream::sx_plan
bool device_has_sx(const DeviceMatrix *m);
void device_set_sx(DeviceMatrix *m, bool on);
bool device_get_sx(const DeviceMatrix *m);
void device_sx_info(const DeviceMatrix *m, uint64_t &elems_sx, uint64_t &elems_sym, size_t &rowblocks);

// seconds per SpMV (alpha = 1, beta = 0) over `launches` back-to-back launches
// on a private stream with scratch vectors -- what spx_mat_tune() measures to
// choose launch parameters
double device_time_spmv(DeviceMatrix *m, int warmup, int launches);

// copies the descriptor stream back from HBM (for spx_mat_save)
void device_download(const DeviceMatrix *m, GpuStream &s);

// one stored value (diagonal: of the symmetric path's diagonal array) read from /
// written to HBM where it lies (spx_mat_get_entry / spx_mat_set_entry);
// synchronous
double device_peek(const DeviceMatrix *m, bool diagonal, size_t index);
void device_poke(DeviceMatrix *m, bool diagonal, size_t index, double value);
void device_poke_mirror(DeviceMatrix *m, size_t index, double value);   // GpuStream::mirror_val

// New values, same pattern (values_plan.hpp).  device_values_plan_set uploads the three source arrays of a plan
// (replacing an earlier one) and returns the HBM they take; device_set_values gathers the caller's CSR value
// array (in HBM, `csr_nnz` doubles) into the stream's values, mirror list and diagonal: it only enqueues on
// `stream` -- no allocation, no wait, legal during stream capture -- and counts as a product for device_poke's
// wait-once rule.  device_set_values_host takes the array from host memory: a temporary HBM buffer filled in
// pieces through page-locked staging, the same kernels, a wait, the buffer freed.  Both setters refuse a calling
// thread whose current device is not the matrix' one; device_values_plan_set works on the matrix' device and
// leaves the current device as it found it.
struct ValuesPlan;
size_t device_values_plan_set(DeviceMatrix *m, const ValuesPlan &plan);
void device_values_plan_drop(DeviceMatrix *m);
void device_set_values(DeviceMatrix *m, const double *d_csr_values, void *stream);
void device_set_values_host(DeviceMatrix *m, const double *h_csr_values, size_t csr_nnz);
// The diagonal (diag_plan.hpp).  device_diag_plan_set uploads the positions of a general stream's diagonal entries
// (replacing an earlier plan; a symmetric stream has nothing to upload) and returns the HBM they take, on the
// matrix' device, the current device left as it was.  device_get_diag enqueues ONE gather kernel on `stream` that
// writes d_diag[own_lo, own_hi) -- no allocation, no wait, legal during stream capture; it counts as a product
// for device_poke's wait-once rule.  device_get_diag_host: the same through a temporary HBM buffer, synchronous,
// into host memory.  Both readers refuse a calling thread whose current device is not the matrix' one, and a
// general stream without a plan.
struct DiagPlan;
size_t device_diag_plan_set(DeviceMatrix *m, const DiagPlan &plan);
void device_diag_plan_drop(DeviceMatrix *m);
void device_get_diag(DeviceMatrix *m, double *d_diag, void *stream);
void device_get_diag_host(DeviceMatrix *m, double *h_diag);
// Row and column norms and diagonal scaling of a GENERAL stream where it lies (scale_kernels.hip; the caller keeps
// symmetric and attached matrices away).  `kind`: NORM_SUM_ABS / NORM_SUM_SQ / NORM_MAX_ABS (spmv_launch.hpp).
// device_mat_norms zero-fills d_rows[own_lo, own_hi) and all ncols of d_cols, then one csx_norms_kernel launch per
// launch of the forward product adds to them; either pointer may be null.  device_mat_scale rewrites the doubles
// in HBM, a(r,c) <- fl(fl(dr[r] * a) * dc[c]) (either vector may be null: that product is not formed), and the float
// twin in the same launches.  Both only enqueue on `stream` -- no allocation, no wait, legal during stream capture
// -- refuse a calling thread whose current device is not the matrix' one, and count as a product for
// device_poke's wait-once rule.  The _host forms: the same through temporary HBM buffers, synchronous (a row slice
// reads and writes [own_lo, own_hi) of h_rows / h_dr).
void device_mat_norms(DeviceMatrix *m, int kind, double *d_rows, double *d_cols, void *stream);
void device_mat_scale(DeviceMatrix *m, const double *d_dr, const double *d_dc, void *stream);
void device_mat_norms_host(DeviceMatrix *m, int kind, double *h_rows, double *h_cols);
void device_mat_scale_host(DeviceMatrix *m, const double *h_dr, const double *h_dc);
// The same for a SYMMETRIC stream (sym_scale_kernels.hip; the caller keeps general and attached matrices away): one
// vector of nrows doubles.  device_mat_sym_norms writes ALL nrows elements of d_out -- the diagonal's term on the
// own rows, zero elsewhere -- then joins in the thin mirror list and one csx_sym_norms_kernel launch per launch of
// the forward product: a value stored once counts for its row and its column, a value stored twice for the row of
// each copy.  device_mat_sym_scale rewrites a(r,c) <- fl(fl(d[max(r,c)] * a) * d[min(r,c)]) in the stream, its float
// twin, the diagonal array and the mirror list; it reads d wherever the entries reach, [0, own_hi).  Calling rules
// as above.  device_sym_scale_lds: the dynamic LDS of a norms launch, in bytes (0: not a symmetric stream).
void device_mat_sym_norms(DeviceMatrix *m, int kind, double *d_out, void *stream);
void device_mat_sym_scale(DeviceMatrix *m, const double *d_d, void *stream);
void device_mat_sym_norms_host(DeviceMatrix *m, int kind, double *h_out);
void device_mat_sym_scale_host(DeviceMatrix *m, const double *h_d);
size_t device_sym_scale_lds(const DeviceMatrix *m);
size_t device_n_values(const DeviceMatrix *m);     // doubles in the stream's value array

struct DeviceMatrixInfo {
    size_t n_rowblocks, n_shared_rows;
    size_t value_bytes, index_bytes;
    int device;
};
void device_info(const DeviceMatrix *m, DeviceMatrixInfo &info);

}  // namespace spx
