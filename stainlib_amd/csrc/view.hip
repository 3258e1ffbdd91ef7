// view.hip -- C-ABI launchers of the fused crop / flip / rot90 view of the apply pass, with its 2x / 4x box shrink (kernel: view_kernels.hpp),
// and of the resizing view with its per-tile window sides (kernel: view_resize_kernels.hpp).
#include "view_resize_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

extern "C" int sl_normalize_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                        int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt,
                                        const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                        const SlTensorFormat* fmt, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    long npx = 0, npatch = 0;
    if (const int rc = view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch)) return rc;
    int mode = 0;
    if (const int rc = route_of(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, mode)) return rc;
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    const float ylimf = tissue_ylimf(p);
    hipStream_t s = (hipStream_t)stream;
    with_format_or_u8(fmt, false, false, [&](auto dt, auto lay, auto, auto) {     // (no ALIGNED / WIDE variants: see view_kernels.hpp)
        with_mode(mode, [&](auto m) {
            hipLaunchKernelGGL((k_view<decltype(dt)::value, decltype(lay)::value, decltype(m)::value>), dim3((unsigned)(n * npatch)), dim3(kWG),
                               0, s, rgb, out, h, w, oh, ow, (int)npx, (int)npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt,
                               alpha_beta, p.lasso_lambda, ylimf, fmt ? tensor_k(*fmt) : TensorK{});
        });
    });
    return launch_status();
}

extern "C" int sl_normalize_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                 const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                 const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt,
                                 void* stream) {
    return sl_normalize_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, 1, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                                    augment_background, params, fmt, stream);
}

extern "C" int sl_normalize_view_resize(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                        int d_mask, int max_wh, int max_ww, const double* M_src, const double* maxC_src,
                                        const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background,
                                        const SlParams* params, const SlTensorFormat* fmt, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    long npatch = 0;
    if (const int rc = view_resize_geometry(n, h, w, oh, ow, windows, d_mask, max_wh, max_ww, npatch)) return rc;
    int mode = 0;
    if (const int rc = route_of(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, mode)) return rc;
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    const float ylimf = tissue_ylimf(p);
    hipStream_t s = (hipStream_t)stream;
    with_format_or_u8(fmt, false, false, [&](auto dt, auto lay, auto, auto) {
        with_mode(mode, [&](auto m) {
            hipLaunchKernelGGL((k_view_resize<decltype(dt)::value, decltype(lay)::value, decltype(m)::value>), dim3((unsigned)(n * npatch)),
                               dim3(kWG), 0, s, rgb, out, h, w, oh, ow, (int)npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt,
                               maxC_tgt, alpha_beta, p.lasso_lambda, ylimf, fmt ? tensor_k(*fmt) : TensorK{});
        });
    });
    return launch_status();
}
