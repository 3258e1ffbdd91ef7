// hed_view.hip -- C-ABI launchers of HED augmentation behind the apply pass: the byte sums of the image a route would write, and the
// view pass with the HED stage and the view's box shrink (kernels: hed_view_kernels.hpp), and the resizing view with the HED stage
// (kernel: view_resize_kernels.hpp).  A translation unit of its own, so that view.hip does not instantiate HedStage<1>.
#include "hed_view_kernels.hpp"
#include "view_resize_kernels.hpp"  // (behind HedStage<1>)
#include "route_host.hpp"

using namespace sl;

extern "C" int sl_normalize_sums(const uint8_t* rgb, int n, int h, int w, const double* M_src, const double* maxC_src, const double* M_tgt,
                                 const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                 double cutoff_lo, double cutoff_hi, uint64_t* sums, int32_t* applied, void* stream) {
    if (const int rc = check_shape(rgb, n, h, w)) return rc;
    if (!sums || ((uintptr_t)sums & 7u)) return SL_ERR_BADARG;
    int mode = 0;
    if (const int rc = route_of(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, mode)) return rc;
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (!(cutoff_lo <= cutoff_hi)) return SL_ERR_BADARG;                         // (a NaN bound too; infinities pass)
    const SlParams p = params_or_defaults(params);
    const TileLaunch L(n, h, w, kWG);
    const long P = L.P;
    const float ylimf = tissue_ylimf(p);
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(uint64_t) % 4 == 0, "zero_async clears whole words");
    if (const int rc = zero_async(sums, sizeof(uint64_t) * (size_t)n, s)) return rc;
    with_mode(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        launch_aligned(aligned4(rgb, P), k_sums<true, M>, k_sums<false, M>, L.grid, L.block, 0, s, rgb, (int)P, L.parts, M_src, maxC_src, M_tgt,
                       maxC_tgt, alpha_beta, p.lasso_lambda, ylimf, (unsigned long long*)sums);
    });
    if (applied)
        hipLaunchKernelGGL(k_sums_applied, dim3((unsigned)((n + kWG - 1) / kWG)), dim3(kWG), 0, s, (const unsigned long long*)sums, n, (int)P,
                           cutoff_lo, cutoff_hi, applied);
    return launch_status();
}

// SL_OK and the stage's arguments, or SL_ERR_BADARG: the three per-tile arrays, and the pinned semantics only -- any other skimage_mode,
// inside the SL_HED_* range or outside it, is refused (see the header)
static int hed_view_args(const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode, HedViewArgs& hv) {
    if (!hed_sigma || !hed_bias || !hed_applied) return SL_ERR_BADARG;
    if (skimage_mode != SL_HED_SKIMAGE_018) return SL_ERR_BADARG;
    hv.sigma = hed_sigma; hv.bias = hed_bias; hv.applied = hed_applied;
    hed_matrices(hv.R, hv.H);                                                    // sl_hed_augment's
    return SL_OK;
}

extern "C" int sl_normalize_hed_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                            int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt,
                                            const double* maxC_tgt, const double* alpha_beta, int augment_background,
                                            const SlParams* params, const SlTensorFormat* fmt, const double* hed_sigma,
                                            const double* hed_bias, const int32_t* hed_applied, int skimage_mode, void* stream) {
    long npx = 0, npatch = 0;
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, n, h, w, [&] { return view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch); },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    HedViewArgs hv;
    if (const int rc = hed_view_args(hed_sigma, hed_bias, hed_applied, skimage_mode, hv)) return rc;
    return launch_route_view(SL_VIEW_FAMILY(k_hed_view), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npx, (int)npatch,
                             windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{}, hv);
}

extern "C" int sl_normalize_hed_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                     const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                     const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt,
                                     const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode,
                                     void* stream) {
    return sl_normalize_hed_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, 1, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                                        augment_background, params, fmt, hed_sigma, hed_bias, hed_applied, skimage_mode, stream);
}

extern "C" int sl_normalize_hed_view_resize(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                            int d_mask, int max_wh, int max_ww, const double* M_src, const double* maxC_src,
                                            const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background,
                                            const SlParams* params, const SlTensorFormat* fmt, const double* hed_sigma,
                                            const double* hed_bias, const int32_t* hed_applied, int skimage_mode, void* stream) {
    long npatch = 0;
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, n, h, w,
                                         [&] { return view_resize_geometry(n, h, w, oh, ow, windows, d_mask, max_wh, max_ww, npatch); }, M_src,
                                         maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    HedViewArgs hv;
    if (const int rc = hed_view_args(hed_sigma, hed_bias, hed_applied, skimage_mode, hv)) return rc;
    return launch_route_view(SL_VIEW_FAMILY(k_hed_view_resize), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npatch, windows,
                             d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{}, hv);
}
