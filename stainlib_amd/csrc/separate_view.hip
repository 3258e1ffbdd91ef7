// separate_view.hip -- C-ABI launcher of the stain separation in the view pass (kernel: separate_view_kernels.hpp).
#include "separate_view_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

namespace {

// f(conc dtype tag) for the planes of one call (kDtNone: none wanted)
template <class F>
void with_planes(int cdt, F&& f) {
    if (cdt == SL_DTYPE_F32) f(std::integral_constant<int, kDtF32>{});
    else if (cdt == SL_DTYPE_F16) f(std::integral_constant<int, kDtF16>{});
    else if (cdt == SL_DTYPE_BF16) f(std::integral_constant<int, kDtBF16>{});
    else f(std::integral_constant<int, kDtNone>{});
}

}  // namespace

extern "C" int sl_stain_separate_view(const uint8_t* rgb, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink,
                                      const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                      double lasso_lambda, const SlSeparateOut* outs, const SlTensorFormat* fmt, void* stream) {
    // what sl_stain_separate refuses
    if (const int rc = check_shape(rgb, n, h, w)) return rc;
    if (!outs || !M_src || !maxC_src || !lambda_ok(lasso_lambda)) return SL_ERR_BADARG;
    if ((M_tgt == nullptr) != (maxC_tgt == nullptr)) return SL_ERR_BADARG;       // both: a target; neither: every tile's own matrix
    if (outs->struct_size != (uint32_t)sizeof(SlSeparateOut)) return SL_ERR_BADARG;       // (before any other field is read)
    const SlSeparateOut o = *outs;
    if (o.conc_dtype < SL_DTYPE_F32 || o.conc_dtype > SL_DTYPE_BF16) return SL_ERR_BADARG;
    // what the views refuse
    long npx = 0, npatch = 0;
    if (const int rc = view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch)) return rc;
    if (shrink != 1 && o.conc) return SL_ERR_BADARG;                             // a mean of floats is another definition
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const void* const ptrs[5] = {o.norm, o.stain[0], o.stain[1], o.conc, rgb};
    bool any = false;
    for (int i = 0; i < 4; ++i) {
        if (!ptrs[i]) continue;
        any = true;
        for (int j = i + 1; j < 5; ++j)
            if (ptrs[j] == ptrs[i]) return SL_ERR_BADARG;
    }
    if (!any) return SL_ERR_BADARG;
    const size_t img_elem = fmt ? elem_bytes(fmt->dtype) : 1;
    for (int i = 0; i < 3; ++i)
        if (ptrs[i] && ((uintptr_t)ptrs[i] % img_elem) != 0) return SL_ERR_BADARG;
    if (o.conc && ((uintptr_t)o.conc % elem_bytes(o.conc_dtype)) != 0) return SL_ERR_BADARG;

    const SeparateViewOut d{{o.norm, o.stain[0], o.stain[1]}, o.conc};
    with_format_or_u8(fmt, false, false, [&](auto dt, auto lay, auto, auto) {     // (no ALIGNED / WIDE variants: see view_kernels.hpp)
        with_planes(o.conc ? o.conc_dtype : kDtNone, [&](auto cdt) {
            hipLaunchKernelGGL((k_separate_view<decltype(dt)::value, decltype(lay)::value, decltype(cdt)::value>),
                               dim3((unsigned)(n * npatch)), dim3(kWG), 0, (hipStream_t)stream, rgb, d, h, w, oh, ow, (int)npx, (int)npatch,
                               windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda, fmt ? tensor_k(*fmt) : TensorK{});
        });
    });
    return launch_status();
}
