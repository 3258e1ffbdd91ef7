// view.hip -- C-ABI launchers of the fused crop / flip / rot90 view of the apply pass, with its 2x / 4x box shrink (kernel: view_kernels.hpp),
// and of the resizing view with its per-tile window sides (kernel: view_resize_kernels.hpp).  Checks and dispatch: route_host.hpp.
#include "view_resize_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

extern "C" int sl_normalize_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                        int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt,
                                        const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                        const SlTensorFormat* fmt, void* stream) {
    long npx = 0, npatch = 0;
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, n, h, w, [&] { return view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch); },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    return launch_route_view(SL_VIEW_FAMILY(k_view), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npx, (int)npatch, windows,
                             d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{});
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
    long npatch = 0;
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, n, h, w,
                                         [&] { return view_resize_geometry(n, h, w, oh, ow, windows, d_mask, max_wh, max_ww, npatch); }, M_src,
                                         maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    return launch_route_view(SL_VIEW_FAMILY(k_view_resize), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npatch, windows,
                             d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{});
}
