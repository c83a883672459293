// dist_kernels.hip -- device side of the exchange plan of a row-partitioned
// matrix (dist.hpp): its device arrays and the pack / unpack / scatter kernels.
// The built-in transport, RCCL point-to-point over xGMI, is dist_rccl.cpp.
//
// A symmetric process adds into rows in front of its own (the reference's local
// buffers, src/api/matvec.c:302-318); only those entries travel, packed, to
// their owners, which add them in a fixed order (the reference's map reduction,
// src/internals/Vector.cpp:291-299).
#include "dist.hpp"
#include "hip_check.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace spx {

struct DistDevice {
    int device = 0;
    size_t n_send = 0, n_recv = 0, n_fix = 0;
    idx_t *send_rows = nullptr;
    double *sendbuf = nullptr, *recvbuf = nullptr;
    idx_t *fix_rows = nullptr;
    uint32_t *fix_ptr = nullptr, *fix_pos = nullptr;
    // halo of x
    size_t n_halo_send = 0, n_halo_recv = 0;
    idx_t *halo_send_rows = nullptr, *halo_cols = nullptr;
    double *halo_sendbuf = nullptr, *halo_recvbuf = nullptr;
    // overlapped step
    uint32_t *rd_pack_pos = nullptr, *rd_scat_pos = nullptr;
    std::vector<size_t> rd_pack_ptr, rd_scat_ptr;
    hipStream_t comm = nullptr;
    std::vector<hipEvent_t> ev_part;      // one per part of the product
    hipEvent_t ev_done = nullptr;
};

// sendbuf[k] = y[send_rows[k]]: the sums this process formed for rows of others
__global__ void dist_pack_kernel(const idx_t *rows, const double *y, double *buf, size_t n)
{
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) buf[k] = y[rows[k]];
}

// y[row] += what the other processes sent for it, in the order of the senders
__global__ void dist_unpack_kernel(const idx_t *rows, const uint32_t *ptr, const uint32_t *pos,
                                   const double *buf, double *y, size_t n)
{
    const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    double s = 0.0;
    for (uint32_t k = ptr[t]; k < ptr[t + 1]; ++k) s += buf[pos[k]];
    y[rows[t]] += s;
}

// y[cols[k]] = what the owner of entry cols[k] sent for it (distinct entries, plain stores)
__global__ void dist_scatter_kernel(const idx_t *cols, const double *buf, double *y, size_t n)
{
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) y[cols[k]] = buf[k];
}

// the same through position lists (one round of the overlapped step)
__global__ void dist_pack_pos_kernel(const uint32_t *pos, const idx_t *rows, const double *y, double *buf, size_t n)
{
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) buf[pos[k]] = y[rows[pos[k]]];
}
__global__ void dist_scatter_pos_kernel(const uint32_t *pos, const idx_t *cols, const double *buf, double *y, size_t n)
{
    const size_t k = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) y[cols[pos[k]]] = buf[pos[k]];
}

template <typename T>
static T *to_device(const std::vector<T> &v, size_t min_elems = 1)
{
    T *d = nullptr;
    const size_t n = std::max(v.size(), min_elems);
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d), n * sizeof(T)));
    if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

DistDevice *dist_device_create(const DistPlan &p)
{
    DistDevice *d = new DistDevice;
    HIP_CHECK(hipGetDevice(&d->device));
    d->n_send = p.send_rows.size();
    d->n_recv = p.n_recv;
    d->n_fix = p.fix_rows.size();
    d->send_rows = to_device(p.send_rows);
    d->fix_rows = to_device(p.fix_rows);
    d->fix_ptr = to_device(p.fix_ptr, 2);
    d->fix_pos = to_device(p.fix_pos);
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d->sendbuf), std::max<size_t>(d->n_send, 1) * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d->recvbuf), std::max<size_t>(d->n_recv, 1) * sizeof(double)));
    d->n_halo_send = p.halo_send_rows.size();
    d->n_halo_recv = p.halo_cols.size();
    d->halo_send_rows = to_device(p.halo_send_rows);
    d->halo_cols = to_device(p.halo_cols);
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d->halo_sendbuf), std::max<size_t>(d->n_halo_send, 1) * sizeof(double)));
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d->halo_recvbuf), std::max<size_t>(d->n_halo_recv, 1) * sizeof(double)));
    return d;
}

void dist_device_free(DistDevice *d)
{
    if (!d) return;
    (void) hipFree(d->send_rows); (void) hipFree(d->fix_rows); (void) hipFree(d->fix_ptr);
    (void) hipFree(d->fix_pos); (void) hipFree(d->sendbuf); (void) hipFree(d->recvbuf);
    (void) hipFree(d->halo_send_rows); (void) hipFree(d->halo_cols);
    (void) hipFree(d->halo_sendbuf); (void) hipFree(d->halo_recvbuf);
    (void) hipFree(d->rd_pack_pos); (void) hipFree(d->rd_scat_pos);
    for (hipEvent_t e : d->ev_part) (void) hipEventDestroy(e);
    if (d->ev_done) (void) hipEventDestroy(d->ev_done);
    if (d->comm) (void) hipStreamDestroy(d->comm);
    delete d;
}

const double *dist_device_pack(DistDevice *d, const double *d_y, void *stream)
{
    if (d->n_send)
        hipLaunchKernelGGL(dist_pack_kernel, dim3((unsigned) ((d->n_send + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), d->send_rows, d_y, d->sendbuf, d->n_send);
    return d->sendbuf;
}

double *dist_device_recvbuf(DistDevice *d) { return d->recvbuf; }

void dist_device_unpack(DistDevice *d, double *d_y, void *stream)
{
    if (d->n_fix)
        hipLaunchKernelGGL(dist_unpack_kernel, dim3((unsigned) ((d->n_fix + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), d->fix_rows, d->fix_ptr, d->fix_pos,
                           d->recvbuf, d_y, d->n_fix);
}

const double *dist_device_halo_pack(DistDevice *d, const double *d_y, void *stream)
{
    if (d->n_halo_send)
        hipLaunchKernelGGL(dist_pack_kernel, dim3((unsigned) ((d->n_halo_send + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), d->halo_send_rows, d_y, d->halo_sendbuf, d->n_halo_send);
    return d->halo_sendbuf;
}

double *dist_device_halo_recvbuf(DistDevice *d) { return d->halo_recvbuf; }

void dist_device_halo_scatter(DistDevice *d, double *d_y, void *stream)
{
    if (d->n_halo_recv)
        hipLaunchKernelGGL(dist_scatter_kernel, dim3((unsigned) ((d->n_halo_recv + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), d->halo_cols, d->halo_recvbuf, d_y, d->n_halo_recv);
}

void dist_device_set_rounds(DistDevice *d, const DistPlan &p)
{
    (void) hipFree(d->rd_pack_pos); (void) hipFree(d->rd_scat_pos);
    d->rd_pack_pos = to_device(p.rd_pack_pos);
    d->rd_scat_pos = to_device(p.rd_scat_pos);
    d->rd_pack_ptr = p.rd_pack_ptr;
    d->rd_scat_ptr = p.rd_scat_ptr;
    if (!d->comm) {
        // (highest priority: its pack / copy / scatter kernels are tiny and must not queue behind the
        // thousands of workgroups of the product part that runs next to them)
        int pri_lo = 0, pri_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&pri_lo, &pri_hi) != hipSuccess) {
            (void) hipGetLastError();
            pri_hi = 0;
        }
        if (hipStreamCreateWithPriority(&d->comm, hipStreamNonBlocking, pri_hi) != hipSuccess) {
            (void) hipGetLastError();
            HIP_CHECK(hipStreamCreateWithFlags(&d->comm, hipStreamNonBlocking));
        }
        HIP_CHECK(hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming));
    }
    while (d->ev_part.size() < p.rounds) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        d->ev_part.push_back(e);
    }
}

void *dist_device_comm_stream(DistDevice *d) { return d->comm; }
double *dist_device_halo_sendbuf(DistDevice *d) { return d->halo_sendbuf; }

void dist_device_part_done(DistDevice *d, size_t part, void *main_stream)
{
    HIP_CHECK(hipEventRecord(d->ev_part.at(part), static_cast<hipStream_t>(main_stream)));
}

void dist_device_round_begin(DistDevice *d, size_t round)
{
    HIP_CHECK(hipStreamWaitEvent(d->comm, d->ev_part.at(round), 0));
}

void dist_device_round_pack(DistDevice *d, size_t r, const double *d_y)
{
    const size_t lo = d->rd_pack_ptr[r], n = d->rd_pack_ptr[r + 1] - lo;
    if (n)
        hipLaunchKernelGGL(dist_pack_pos_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, d->comm,
                           d->rd_pack_pos + lo, d->halo_send_rows, d_y, d->halo_sendbuf, n);
}

void dist_device_round_scatter(DistDevice *d, size_t r, double *d_y)
{
    const size_t lo = d->rd_scat_ptr[r], n = d->rd_scat_ptr[r + 1] - lo;
    if (n)
        hipLaunchKernelGGL(dist_scatter_pos_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, d->comm,
                           d->rd_scat_pos + lo, d->halo_cols, d->halo_recvbuf, d_y, n);
}

void dist_device_rounds_end(DistDevice *d, void *main_stream)
{
    HIP_CHECK(hipEventRecord(d->ev_done, d->comm));
    HIP_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(main_stream), d->ev_done, 0));
}

}  // namespace spx
