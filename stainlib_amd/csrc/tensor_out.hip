// tensor_out.hip -- C-ABI launchers of the model-ready tensor output (kernels: tensor_kernels.hpp).
#include "tensor_host.hpp"

using namespace sl;

extern "C" void sl_default_tensor_format(SlTensorFormat* f) {
    if (!f) return;
    f->struct_size = (uint32_t)sizeof(SlTensorFormat);
    f->dtype = SL_DTYPE_F32;
    f->layout = SL_LAYOUT_NCHW;
    f->reserved = 0;
    for (int c = 0; c < 3; ++c) { f->mean[c] = 0.0; f->std[c] = 1.0; }
}

extern "C" int sl_to_tensor(const uint8_t* rgb, void* out, int n, int h, int w, const SlTensorFormat* fmt, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!format_ok(fmt)) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    const TensorK k = tensor_k(*fmt);
    with_format(fmt->dtype, fmt->layout, aligned4(rgb, L.P), wide_ok(out, L.P, fmt->dtype), [&](auto dt, auto lay, auto al, auto wide) {
        hipLaunchKernelGGL((k_to_tensor<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value>), L.grid, L.block, 0,
                           (hipStream_t)stream, rgb, out, (int)L.P, L.parts, k);
    });
    return launch_status();
}

extern "C" int sl_normalize_apply_tensor(const uint8_t* rgb, void* out, int n, int h, int w, const double* M_src, const double* maxC_src,
                                         const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlTensorFormat* fmt,
                                         void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!M_src || !maxC_src || !M_tgt || !maxC_tgt || !lambda_ok(lasso_lambda)) return SL_ERR_BADARG;
    if (!format_ok(fmt)) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    const TensorK k = tensor_k(*fmt);
    with_format(fmt->dtype, fmt->layout, aligned4(rgb, L.P), wide_ok(out, L.P, fmt->dtype), [&](auto dt, auto lay, auto al, auto wide) {
        hipLaunchKernelGGL((k_apply_tensor<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value>), L.grid, L.block, 0,
                           (hipStream_t)stream, rgb, out, (int)L.P, L.parts, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda, k);
    });
    return launch_status();
}
