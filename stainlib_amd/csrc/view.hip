// view.hip -- C-ABI launcher of the fused crop / flip / rot90 view of the apply pass (kernel: view_kernels.hpp).
#include "view_kernels.hpp"
#include "tensor_host.hpp"

using namespace sl;

extern "C" int sl_normalize_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                 const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                 const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt,
                                 void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!windows || oh < 1 || ow < 1 || oh > h || ow > w) return SL_ERR_BADARG;
    if (d_mask < 0 || d_mask > 7) return SL_ERR_BADARG;
    if ((d_mask & 1) && (ow > h || oh > w)) return SL_ERR_BADARG;               // the transposed window must fit too
    if ((M_tgt == nullptr) != (maxC_tgt == nullptr)) return SL_ERR_BADARG;
    if (!M_src) {                                                                // the source bytes themselves: nothing else applies
        if (M_tgt || maxC_src || alpha_beta) return SL_ERR_BADARG;
    } else {
        if (!maxC_src) return SL_ERR_BADARG;
        if (!alpha_beta && !M_tgt) return SL_ERR_BADARG;                         // sl_normalize_apply has no "no target"
    }
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const long npx = (ow + kViewB - 1) / kViewB, npatch = npx * ((oh + kViewB - 1) / kViewB);
    if ((long)n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                    // one workgroup per (tile, patch)
    const SlParams p = params_or_defaults(params);
    const float ylimf = tissue_ylimf(p);
    const int mode = !M_src ? kViewRaw : (!alpha_beta ? kViewApply : (augment_background ? kViewJitAll : kViewJitTissue));
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto dt, auto lay, auto, auto) {
        auto go = [&](auto m) {
            hipLaunchKernelGGL((k_view<decltype(dt)::value, decltype(lay)::value, decltype(m)::value>), dim3((unsigned)(n * npatch)), dim3(kWG),
                               0, s, rgb, out, h, w, oh, ow, (int)npx, (int)npatch, windows, d_mask, M_src, maxC_src, M_tgt, maxC_tgt,
                               alpha_beta, p.lasso_lambda, ylimf, fmt ? tensor_k(*fmt) : TensorK{});
        };
        if (mode == kViewRaw) go(std::integral_constant<int, kViewRaw>{});
        else if (mode == kViewApply) go(std::integral_constant<int, kViewApply>{});
        else if (mode == kViewJitTissue) go(std::integral_constant<int, kViewJitTissue>{});
        else go(std::integral_constant<int, kViewJitAll>{});
    };
    if (fmt) with_format(fmt->dtype, fmt->layout, false, false, launch);         // (no ALIGNED / WIDE variants: see view_kernels.hpp)
    else launch(std::integral_constant<int, kDtU8>{}, std::integral_constant<int, kLayNHWC>{}, std::false_type{}, std::false_type{});
    return launch_status();
}
