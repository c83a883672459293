// spmv_mv_instances.hpp -- the instances of the multi-vector row-block kernel that one translation unit holds:
// the kernel template over mv_body (spmv_mv_device.hpp), the (family, K, waves) -> kernel lookup, the launch
// and the dynamic-LDS allowance, given the argument struct (the layout: MvArgs or MvrArgs), the type of the
// stream's values and the set of K.  For the .hip units only (HIP header); what host code sees of them are the
// launchers of spmv_launch.hpp, which each unit defines by naming its table.
#pragma once

#include "spmv_mv_device.hpp"

#include <hip/hip_runtime.h>

namespace spx {

// LDS: K y tiles (F == det: per wavefront), then the x window(s) where they are staged
template <class Args, class V, MvFamily F, int K, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void csx_spmv_mv_kernel(Args a, XcdSplit xs)
{
    extern __shared__ double lds_dyn[];
    mv_body<K, WAVES, F == MvFamily::accum, F == MvFamily::det, V>(a, xs, lds_dyn);
}

// Ks: the group widths the unit serves, narrowest first
template <class Args, class V, int... Ks>
struct MvInstances {
    typedef void (*Kernel)(Args, XcdSplit);

    template <int K, int WAVES>
    static Kernel of_family(MvFamily family)
    {
        switch (family) {
        case MvFamily::accum: return csx_spmv_mv_kernel<Args, V, MvFamily::accum, K, WAVES>;
        case MvFamily::det: return csx_spmv_mv_kernel<Args, V, MvFamily::det, K, WAVES>;
        case MvFamily::plain: break;
        }
        return csx_spmv_mv_kernel<Args, V, MvFamily::plain, K, WAVES>;
    }

    template <int K>
    static Kernel of_waves(MvFamily family, int waves)
    {
        return waves == 2 ? of_family<K, 2>(family) : waves == 8 ? of_family<K, 8>(family) : of_family<K, 4>(family);
    }

    // (a K outside the set runs as the narrowest, as a number of wavefronts outside 2, 4, 8 runs as 4)
    static Kernel kernel(MvFamily family, int K, int waves)
    {
        Kernel k = nullptr;
        ((k = (!k || K == Ks) ? of_waves<Ks>(family, waves) : k), ...);
        return k;
    }

    static void launch(MvFamily family, int K, int waves, unsigned blocks, size_t lds_bytes, void *stream, const Args &a,
                       const XcdSplit &xs)
    {
        const int w = (waves == 2 || waves == 8) ? waves : 4;
        hipLaunchKernelGGL(kernel(family, K, w), dim3(blocks), dim3(64 * w), lds_bytes, static_cast<hipStream_t>(stream), a,
                           xs);
    }

    // dynamic LDS beyond the default 64 KB, for every instance
    static void allow_lds(size_t bytes)
    {
        const int b = (int) bytes;
        for (MvFamily f : {MvFamily::plain, MvFamily::accum, MvFamily::det})
            for (int K : {Ks...})
                for (int w : {2, 4, 8})
                    (void) hipFuncSetAttribute(reinterpret_cast<const void *>(kernel(f, K, w)),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, b);
    }
};

}  // namespace spx
