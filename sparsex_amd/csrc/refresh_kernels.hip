// refresh_kernels.hip -- new values for a tuned matrix whose pattern stays (values_plan.hpp):
// dst[i] = src[map[i]] for every position i of the stream's values with a source, on the caller's stream.
//
// Bandwidth-bound: per stored value 4 B of plan, an 8 B gather from the caller's CSR value array and an 8 B
// store.  A lane takes four consecutive positions: one 16-byte load of the plan, four 8-byte gathers (the
// caller's order is the matrix' row order, so neighbouring positions mostly gather from neighbouring
// addresses) and two 16-byte stores -- the stream's value arrays come from hipMalloc and are 16-byte aligned.
// A group of four that holds a position WITHOUT a source (pass padding, a lane beyond its segment's length,
// an absent cell of a tile) stores its other values one by one and leaves that position alone: it keeps the
// bits the tune put there.  The plan is padded to a multiple of four entries (no source), so that the last
// group needs no bounds of its own.
//
// A stream with a float twin of its values (spx.gpu.values_f32) gets both arrays written in the same pass: a
// full group stores one float4 more, the others store the float next to every double they store and leave the
// float bits of a position without a source alone as well.  The twin itself is built once per tune or restore
// by csx_narrow_values_kernel from the doubles already in HBM: per lane four consecutive values, two 16-byte
// loads, one 16-byte store; 12 B per value, no host pass.
#include "spmv_launch.hpp"

#include "hip_check.hpp"

#include <hip/hip_runtime.h>

namespace spx {

namespace {

constexpr uint32_t REFRESH_NONE = 0xffffffffu;
constexpr unsigned REFRESH_BLOCK = 256;

// n_quads groups of four positions; `dst` 16-byte aligned when ALIGNED (the diagonal array of a slice that
// starts on an odd row is not: its groups store value by value)
// F32: dst32 is the float twin of dst (16-byte aligned like it), written next to it
template <bool ALIGNED, bool F32 = false>
__global__ void __launch_bounds__(REFRESH_BLOCK)
csx_refresh_values_kernel(double *__restrict__ dst, const uint4 *__restrict__ map, const double *__restrict__ src,
                          size_t n, size_t n_quads, float *__restrict__ dst32 = nullptr)
{
    const size_t q = (size_t) blockIdx.x * REFRESH_BLOCK + threadIdx.x;
    if (q >= n_quads) return;
    const uint4 m = map[q];
    const size_t i = q * 4;
    const bool full = m.x != REFRESH_NONE && m.y != REFRESH_NONE && m.z != REFRESH_NONE && m.w != REFRESH_NONE;
    if (ALIGNED && full) {
        // (a full group lies inside the array: only padding entries reach beyond n, and they have no source)
        const double a = src[m.x], b = src[m.y], c = src[m.z], d = src[m.w];
        double2 *out = reinterpret_cast<double2 *>(dst + i);
        out[0] = make_double2(a, b);
        out[1] = make_double2(c, d);
        if (F32)
            *reinterpret_cast<float4 *>(dst32 + i) =
                make_float4(__double2float_rn(a), __double2float_rn(b), __double2float_rn(c), __double2float_rn(d));
        return;
    }
#define SPX_REFRESH_ONE(mk, k)                                                                   \
    if (mk != REFRESH_NONE && i + k < n) {                                                       \
        const double v = src[mk];                                                                \
        dst[i + k] = v;                                                                          \
        if (F32) dst32[i + k] = __double2float_rn(v);                                            \
    }
    SPX_REFRESH_ONE(m.x, 0)
    SPX_REFRESH_ONE(m.y, 1)
    SPX_REFRESH_ONE(m.z, 2)
    SPX_REFRESH_ONE(m.w, 3)
#undef SPX_REFRESH_ONE
}

// the float twin of a value array: n_quads groups of four, dst[i] = (float) src[i], round to nearest even
__global__ void __launch_bounds__(REFRESH_BLOCK)
csx_narrow_values_kernel(float4 *__restrict__ dst, const double2 *__restrict__ src, size_t n_quads)
{
    const size_t q = (size_t) blockIdx.x * REFRESH_BLOCK + threadIdx.x;
    if (q >= n_quads) return;
    const double2 a = src[2 * q], b = src[2 * q + 1];
    dst[q] = make_float4(__double2float_rn(a.x), __double2float_rn(a.y), __double2float_rn(b.x), __double2float_rn(b.y));
}

// The way back for the diagonal (diag_plan.hpp): dst[i] = pos[i] != none ? values[pos[i]] : +0.0 for the n own
// rows of a general stream; PLAN false: dst[i] = values[i], the diagonal array of a symmetric one.  The sibling of
// csx_refresh_values_kernel: a lane takes four consecutive rows, one 16-byte load of the plan (it comes from
// hipMalloc; NOT padded: the last group loads its entries one by one), four 8-byte gathers -- the diagonal
// entries of neighbouring rows mostly lie in the same row-block -- and two 16-byte stores.  `dst` is a caller's
// pointer plus the slice's first row and may be only 8-byte aligned: its groups store value by value (!ALIGNED),
// as does the last group of an n that is no multiple of four.  Nothing outside [dst, dst + n) is written.
template <bool ALIGNED, bool PLAN>
__global__ void __launch_bounds__(REFRESH_BLOCK)
csx_gather_diag_kernel(double *__restrict__ dst, const uint32_t *__restrict__ pos, const double *__restrict__ values,
                       size_t n)
{
    const size_t q = (size_t) blockIdx.x * REFRESH_BLOCK + threadIdx.x;
    const size_t i = q * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        double v[4];
        if (PLAN) {
            const uint4 m = *reinterpret_cast<const uint4 *>(pos + i);
            v[0] = m.x != REFRESH_NONE ? values[m.x] : 0.0;
            v[1] = m.y != REFRESH_NONE ? values[m.y] : 0.0;
            v[2] = m.z != REFRESH_NONE ? values[m.z] : 0.0;
            v[3] = m.w != REFRESH_NONE ? values[m.w] : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = values[i + k];
        }
        if (ALIGNED) {
            double2 *out = reinterpret_cast<double2 *>(dst + i);
            out[0] = make_double2(v[0], v[1]);
            out[1] = make_double2(v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[i + k] = v[k];
        }
        return;
    }
    for (size_t k = i; k < n; ++k) {
        if (PLAN) {
            const uint32_t m = pos[k];
            dst[k] = m != REFRESH_NONE ? values[m] : 0.0;
        } else {
            dst[k] = values[k];
        }
    }
}

}  // namespace

void launch_gather_diag(void *stream, double *dst, const uint32_t *pos, const double *values, size_t n)
{
    if (!n) return;
    const size_t n_quads = (n + 3) / 4;
    const size_t blocks = (n_quads + REFRESH_BLOCK - 1) / REFRESH_BLOCK;
    if (blocks > 0x7fffffffull) throw FatalError("diagonal: array too long for one launch");
    if (pos && (reinterpret_cast<uintptr_t>(pos) & 15u) != 0) throw FatalError("diagonal: the plan must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
    const dim3 grid((unsigned) blocks), block(REFRESH_BLOCK);
    if (pos) {
        if (aligned) hipLaunchKernelGGL((csx_gather_diag_kernel<true, true>), grid, block, 0, st, dst, pos, values, n);
        else hipLaunchKernelGGL((csx_gather_diag_kernel<false, true>), grid, block, 0, st, dst, pos, values, n);
    } else {
        if (aligned) hipLaunchKernelGGL((csx_gather_diag_kernel<true, false>), grid, block, 0, st, dst, pos, values, n);
        else hipLaunchKernelGGL((csx_gather_diag_kernel<false, false>), grid, block, 0, st, dst, pos, values, n);
    }
    HIP_CHECK(hipGetLastError());
}

void launch_refresh_values(void *stream, double *dst, const uint32_t *map, const double *src, size_t n, float *dst_f32)
{
    if (!n) return;
    const size_t n_quads = (n + 3) / 4;
    const size_t blocks = (n_quads + REFRESH_BLOCK - 1) / REFRESH_BLOCK;
    if (blocks > 0x7fffffffull) throw FatalError("value refresh: array too long for one launch");
    const uint4 *map4 = reinterpret_cast<const uint4 *>(map);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dst_f32) {
        if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(dst_f32)) & 15u) != 0)
            throw FatalError("value refresh: a value array with a float twin must be 16-byte aligned");
        hipLaunchKernelGGL((csx_refresh_values_kernel<true, true>), dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, st, dst, map4, src, n,
                           n_quads, dst_f32);
    } else if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0)
        hipLaunchKernelGGL(csx_refresh_values_kernel<true>, dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, st, dst, map4, src, n, n_quads,
                           static_cast<float *>(nullptr));
    else
        hipLaunchKernelGGL(csx_refresh_values_kernel<false>, dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, st, dst, map4, src, n, n_quads,
                           static_cast<float *>(nullptr));
    HIP_CHECK(hipGetLastError());
}

void launch_narrow_values(void *stream, float *dst, const double *src, size_t n)
{
    if (!n) return;
    if ((n & 3u) || ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u))
        throw FatalError("float twin of the values: arrays of a multiple of four elements, 16-byte aligned");
    const size_t n_quads = n / 4;
    const size_t blocks = (n_quads + REFRESH_BLOCK - 1) / REFRESH_BLOCK;
    if (blocks > 0x7fffffffull) throw FatalError("float twin of the values: array too long for one launch");
    hipLaunchKernelGGL(csx_narrow_values_kernel, dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<float4 *>(dst), reinterpret_cast<const double2 *>(src), n_quads);
    HIP_CHECK(hipGetLastError());
}

}  // namespace spx
