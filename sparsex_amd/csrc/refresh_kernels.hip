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
#include "spmv_launch.hpp"

#include "hip_check.hpp"

#include <hip/hip_runtime.h>

namespace spx {

namespace {

constexpr uint32_t REFRESH_NONE = 0xffffffffu;
constexpr unsigned REFRESH_BLOCK = 256;

// n_quads groups of four positions; `dst` 16-byte aligned when ALIGNED (the diagonal array of a slice that
// starts on an odd row is not: its groups store value by value)
template <bool ALIGNED>
__global__ void __launch_bounds__(REFRESH_BLOCK)
csx_refresh_values_kernel(double *__restrict__ dst, const uint4 *__restrict__ map, const double *__restrict__ src,
                          size_t n, size_t n_quads)
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
        return;
    }
    if (m.x != REFRESH_NONE && i < n) dst[i] = src[m.x];
    if (m.y != REFRESH_NONE && i + 1 < n) dst[i + 1] = src[m.y];
    if (m.z != REFRESH_NONE && i + 2 < n) dst[i + 2] = src[m.z];
    if (m.w != REFRESH_NONE && i + 3 < n) dst[i + 3] = src[m.w];
}

}  // namespace

void launch_refresh_values(void *stream, double *dst, const uint32_t *map, const double *src, size_t n)
{
    if (!n) return;
    const size_t n_quads = (n + 3) / 4;
    const size_t blocks = (n_quads + REFRESH_BLOCK - 1) / REFRESH_BLOCK;
    if (blocks > 0x7fffffffull) throw FatalError("value refresh: array too long for one launch");
    const uint4 *map4 = reinterpret_cast<const uint4 *>(map);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0)
        hipLaunchKernelGGL(csx_refresh_values_kernel<true>, dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, st, dst, map4, src, n, n_quads);
    else
        hipLaunchKernelGGL(csx_refresh_values_kernel<false>, dim3((unsigned) blocks), dim3(REFRESH_BLOCK), 0, st, dst, map4, src, n, n_quads);
    HIP_CHECK(hipGetLastError());
}

}  // namespace spx
