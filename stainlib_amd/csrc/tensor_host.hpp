// tensor_host.hpp -- host-side helpers of the translation units that write the model-ready tensor (tensor_out.hip, jitter.hip).
#pragma once
#include <cmath>
#include <type_traits>

#include "tensor_kernels.hpp"
#include "sl_host.hpp"

namespace sl {

inline bool format_ok(const SlTensorFormat* f) {
    if (!f || f->struct_size != (uint32_t)sizeof(SlTensorFormat)) return false;
    if (f->dtype < SL_DTYPE_F32 || f->dtype > SL_DTYPE_BF16) return false;
    if (f->layout != SL_LAYOUT_NCHW && f->layout != SL_LAYOUT_NHWC) return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(f->mean[c]) || !std::isfinite(f->std[c]) || !(f->std[c] > 0.0)) return false;
    return true;
}

// scale32 / shift32 of the definition: binary64 on the host, rounded to binary32 once
inline TensorK tensor_k(const SlTensorFormat& f) {
    TensorK k;
    for (int c = 0; c < 3; ++c) {
        k.sc[c] = (float)(1.0 / (255.0 * f.std[c]));
        k.sh[c] = (float)(-f.mean[c] / f.std[c]);
    }
    return k;
}

// f(dtype tag, layout tag, aligned tag, wide tag) for the runtime format
template <class F>
inline void with_format(int dtype, int layout, bool aligned, bool wide, F&& f) {
    auto l4 = [&](auto dt, auto lay, auto al) { if (wide) f(dt, lay, al, std::true_type{}); else f(dt, lay, al, std::false_type{}); };
    auto l3 = [&](auto dt, auto lay) { if (aligned) l4(dt, lay, std::true_type{}); else l4(dt, lay, std::false_type{}); };
    auto l2 = [&](auto dt) {
        if (layout == SL_LAYOUT_NCHW) l3(dt, std::integral_constant<int, kLayNCHW>{}); else l3(dt, std::integral_constant<int, kLayNHWC>{});
    };
    if (dtype == SL_DTYPE_F32) l2(std::integral_constant<int, kDtF32>{});
    else if (dtype == SL_DTYPE_F16) l2(std::integral_constant<int, kDtF16>{});
    else l2(std::integral_constant<int, kDtBF16>{});
}

}  // namespace sl
