// view_blur.hip -- C-ABI launcher of the blurred view: a per-tile integer separable Gaussian of radius <= 8 inside the view pass (kernel:
// view_blur_kernels.hpp).  The route checks and the dispatch are the views' own (route_host.hpp); the geometry check is here.
#include "view_blur_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

// The geometry of a blurred view of n tiles under the shrink s and the radius bound max_r: what view_geometry refuses, the bound's range,
// and the patches -- blur_patch_edge outputs square -- per output row and per tile.  The codes themselves may live on the device.
static int view_blur_geometry(int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int s, int max_r, const int32_t* codes,
                              long& npx, long& npatch) {
    if (const int rc = view_geometry(n, h, w, oh, ow, windows, d_mask, s, npx, npatch)) return rc;
    if (!codes || ((uintptr_t)codes & 3) || max_r < 0 || max_r > kBlurMaxR) return SL_ERR_BADARG;
    const int B = blur_patch_edge(max_r, s);
    npx = (ow + B - 1) / B;
    npatch = npx * ((oh + B - 1) / B);
    if ((long)n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                    // one workgroup per (tile, patch)
    return SL_OK;
}

extern "C" int sl_normalize_blur_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                      int shrink, int max_r, const double* M_src, const double* maxC_src, const double* M_tgt,
                                      const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                      const SlTensorFormat* fmt, const int32_t* codes, void* stream) {
    long npx = 0, npatch = 0;
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, n, h, w,
                                         [&] { return view_blur_geometry(n, h, w, oh, ow, windows, d_mask, shrink, max_r, codes, npx, npatch); },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    return launch_route_view(SL_VIEW_FAMILY(k_view_blur), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npx, (int)npatch,
                             windows, d_mask, shrink, max_r, codes, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{});
}
