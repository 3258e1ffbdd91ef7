// hed_view.hip -- C-ABI launchers of HED augmentation behind the apply pass: the byte sums of the image a route would write, and the
// view pass with the HED stage (kernels: hed_view_kernels.hpp).  A translation unit of its own: view.hip compiles as before.
#include "hed_view_kernels.hpp"
#include "tensor_host.hpp"

using namespace sl;

namespace {
// the pointer pattern by which sl_normalize_view names `full`: SL_OK and the kView* mode, or SL_ERR_BADARG
int route_of(const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
             int augment_background, int& mode) {
    if ((M_tgt == nullptr) != (maxC_tgt == nullptr)) return SL_ERR_BADARG;
    if (!M_src) {                                                                // the source bytes themselves: nothing else applies
        if (M_tgt || maxC_src || alpha_beta) return SL_ERR_BADARG;
    } else {
        if (!maxC_src) return SL_ERR_BADARG;
        if (!alpha_beta && !M_tgt) return SL_ERR_BADARG;                         // sl_normalize_apply has no "no target"
    }
    mode = !M_src ? kViewRaw : (!alpha_beta ? kViewApply : (augment_background ? kViewJitAll : kViewJitTissue));
    return SL_OK;
}

// f(mode tag) for the runtime mode
template <class F>
void with_mode(int mode, F&& f) {
    if (mode == kViewRaw) f(std::integral_constant<int, kViewRaw>{});
    else if (mode == kViewApply) f(std::integral_constant<int, kViewApply>{});
    else if (mode == kViewJitTissue) f(std::integral_constant<int, kViewJitTissue>{});
    else f(std::integral_constant<int, kViewJitAll>{});
}

void inv3(const double* m, double* o) {                                          // (hed.hip's, for the same hed_from_rgb)
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    o[0] = (e * i - f * h) / det; o[1] = (c * h - b * i) / det; o[2] = (b * f - c * e) / det;
    o[3] = (f * g - d * i) / det; o[4] = (a * i - c * g) / det; o[5] = (c * d - a * f) / det;
    o[6] = (d * h - e * g) / det; o[7] = (b * g - a * h) / det; o[8] = (a * e - b * d) / det;
}
}  // namespace

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

extern "C" int sl_normalize_hed_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                     const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                     const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt,
                                     const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode,
                                     void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!windows || oh < 1 || ow < 1 || oh > h || ow > w) return SL_ERR_BADARG;
    if (d_mask < 0 || d_mask > 7) return SL_ERR_BADARG;
    if ((d_mask & 1) && (ow > h || oh > w)) return SL_ERR_BADARG;               // the transposed window must fit too
    int mode = 0;
    if (const int rc = route_of(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, mode)) return rc;
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    if (!hed_sigma || !hed_bias || !hed_applied) return SL_ERR_BADARG;
    if (skimage_mode < SL_HED_SKIMAGE_018 || skimage_mode > SL_HED_EXPERIMENTAL_LOG10) return SL_ERR_BADARG;
    if (skimage_mode != SL_HED_SKIMAGE_018) return SL_ERR_BADARG;               // the pinned semantics only (see the header)
    const long npx = (ow + kViewB - 1) / kViewB, npatch = npx * ((oh + kViewB - 1) / kViewB);
    if ((long)n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                    // one workgroup per (tile, patch)
    const SlParams p = params_or_defaults(params);
    const float ylimf = tissue_ylimf(p);
    HedViewArgs hv;
    hv.sigma = hed_sigma; hv.bias = hed_bias; hv.applied = hed_applied;
    // skimage.color.rgb_from_hed (colorconv.py:475-478), hed_from_rgb = inv(.): sl_hed_augment's
    const double R[9] = {0.65, 0.70, 0.29, 0.07, 0.99, 0.11, 0.27, 0.57, 0.78};
    for (int i = 0; i < 9; ++i) hv.R[i] = R[i];
    inv3(R, hv.H);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto dt, auto lay, auto, auto) {
        with_mode(mode, [&](auto m) {
            hipLaunchKernelGGL((k_hed_view<decltype(dt)::value, decltype(lay)::value, decltype(m)::value>), dim3((unsigned)(n * npatch)),
                               dim3(kWG), 0, s, rgb, out, h, w, oh, ow, (int)npx, (int)npatch, windows, d_mask, M_src, maxC_src, M_tgt, maxC_tgt,
                               alpha_beta, p.lasso_lambda, ylimf, fmt ? tensor_k(*fmt) : TensorK{}, hv);
        });
    };
    if (fmt) with_format(fmt->dtype, fmt->layout, false, false, launch);         // (no ALIGNED / WIDE variants: see view_kernels.hpp)
    else launch(std::integral_constant<int, kDtU8>{}, std::integral_constant<int, kLayNHWC>{}, std::false_type{}, std::false_type{});
    return launch_status();
}
