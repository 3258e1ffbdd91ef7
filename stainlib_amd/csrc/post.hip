// post.hip -- C-ABI launchers of the post stage, the tone curve and the additive noise on the bytes a call writes (kernels:
// post_kernels.hpp): the full-tile sweep, and the view pass with the stage on its write side on the four routes, fixed-size (with the box
// shrink) or resizing.  A translation unit of its own, so that no other one instantiates a write side with PostStage.
#include "post_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

// tables and codes of a call: each may be null, not both; the codes are read as int32
static bool post_args_ok(const uint8_t* tables, const int32_t* codes) {
    if (!tables && !codes) return false;
    return !((uintptr_t)codes & 3u);
}

extern "C" int sl_post_augment(const uint8_t* rgb, void* out, int n, int h, int w, const uint8_t* tables, const int32_t* codes,
                               const SlTensorFormat* fmt, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!post_args_ok(tables, codes)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    const long P = L.P;
    PostViewArgs pv;
    pv.tables = tables;
    pv.codes = codes;
    // a format: the ALIGNED / WIDE decisions of sl_normalize_apply_tensor; the uint8 image: ALIGNED as in sl_normalize_apply
    with_format_or_u8(fmt, aligned4(rgb, P) && (fmt || aligned4(out, P)), fmt && wide_ok(out, P, fmt->dtype), [&](auto dt, auto lay, auto al, auto wide) {
        hipLaunchKernelGGL((k_post<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value>), L.grid, L.block, 0,
                           (hipStream_t)stream, rgb, out, (int)P, L.parts, pv, fmt ? tensor_k(*fmt) : TensorK{});
    });
    return launch_status();
}

extern "C" int sl_normalize_post_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                      int shrink, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt,
                                      const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                      const SlTensorFormat* fmt, const uint8_t* tables, const int32_t* codes, void* stream) {
    const bool resizing = max_wh != 0;
    long npx = 0, npatch = 0;
    RouteView v;
    const auto geometry = [&] {
        if (!resizing) return max_ww == 0 ? view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch) : (int)SL_ERR_BADARG;
        if (shrink != 1) return (int)SL_ERR_BADARG;                              // windows of their own sizes have no box shrink
        return view_resize_geometry(n, h, w, oh, ow, windows, d_mask, max_wh, max_ww, npatch);
    };
    if (const int rc = route_view_checks(rgb, out, n, h, w, geometry, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params,
                                         fmt, v))
        return rc;
    if (!post_args_ok(tables, codes)) return SL_ERR_BADARG;
    PostViewArgs pv;
    pv.tables = tables;
    pv.codes = codes;
    if (resizing)
        return launch_route_view(SL_VIEW_FAMILY(k_post_view_resize), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npatch, windows,
                                 d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                                 fmt ? tensor_k(*fmt) : TensorK{}, pv);
    return launch_route_view(SL_VIEW_FAMILY(k_post_view), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npx, (int)npatch, windows,
                             d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{}, pv);
}
