// jitter.hip -- C-ABI launcher of the stain jitter in the apply pass (kernel: jitter_kernels.hpp).
#include "jitter_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

extern "C" int sl_normalize_jitter(const uint8_t* rgb, void* out, int n, int h, int w, const double* M_src, const double* maxC_src,
                                   const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background,
                                   const SlParams* params, const SlTensorFormat* fmt, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!M_src || !maxC_src || !alpha_beta) return SL_ERR_BADARG;
    if ((M_tgt == nullptr) != (maxC_tgt == nullptr)) return SL_ERR_BADARG;       // both: a target; neither: every tile's own matrix
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    const TileLaunch L(n, h, w, kWG);
    const long P = L.P;
    const float ylimf = tissue_ylimf(p);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto dt, auto lay, auto al, auto wide) {
        auto go = [&](auto all) {
            hipLaunchKernelGGL((k_apply_jitter<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value, decltype(all)::value>),
                               L.grid, L.block, 0, s, rgb, out, (int)P, L.parts, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, p.lasso_lambda, ylimf,
                               fmt ? tensor_k(*fmt) : TensorK{});
        };
        if (augment_background) go(std::true_type{}); else go(std::false_type{});
    };
    // a format: the ALIGNED / WIDE decisions of sl_normalize_apply_tensor; the uint8 image: ALIGNED as in sl_normalize_apply
    with_format_or_u8(fmt, aligned4(rgb, P) && (fmt || aligned4(out, P)), fmt && wide_ok(out, P, fmt->dtype), launch);
    return launch_status();
}
