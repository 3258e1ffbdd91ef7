// fused_macenko_wide.hip -- the Macenko, 1024-thread (one workgroup per CU) instantiations of the persistent fused kernel (stats_fused.hpp), in a translation unit of their own so
// that the three families compile side by side (each takes about a minute).
#include "stats_kernels.hpp"
#include "sl_host.hpp"

namespace sl {

void launch_fused_macenko_wide(const FusedArgs& a, bool transform, bool aligned, unsigned grid, hipStream_t s) {
    constexpr int METHOD = kMethodMacenko, NT = 2 * kFusedThreads;
    const dim3 g(grid), b(NT);
    if (transform) launch_aligned(aligned, k_fused<METHOD, true, true, NT>, k_fused<METHOD, true, false, NT>, g, b, 0, s, a);
    else launch_aligned(aligned, k_fused<METHOD, false, true, NT>, k_fused<METHOD, false, false, NT>, g, b, 0, s, a);
}

}  // namespace sl
