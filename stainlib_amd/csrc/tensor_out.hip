// tensor_out.hip -- C-ABI launchers of the model-ready tensor output (kernels: tensor_kernels.hpp).
#include <cmath>
#include <type_traits>

#include "tensor_kernels.hpp"
#include "sl_host.hpp"

using namespace sl;

namespace {

bool format_ok(const SlTensorFormat* f) {
    if (!f || f->struct_size != (uint32_t)sizeof(SlTensorFormat)) return false;
    if (f->dtype < SL_DTYPE_F32 || f->dtype > SL_DTYPE_BF16) return false;
    if (f->layout != SL_LAYOUT_NCHW && f->layout != SL_LAYOUT_NHWC) return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(f->mean[c]) || !std::isfinite(f->std[c]) || !(f->std[c] > 0.0)) return false;
    return true;
}

// scale32 / shift32 of the definition: binary64 on the host, rounded to binary32 once
TensorK tensor_k(const SlTensorFormat& f) {
    TensorK k;
    for (int c = 0; c < 3; ++c) {
        k.sc[c] = (float)(1.0 / (255.0 * f.std[c]));
        k.sh[c] = (float)(-f.mean[c] / f.std[c]);
    }
    return k;
}

// f(dtype tag, layout tag, aligned tag, wide tag) for the runtime format
template <class F>
void with_format(int dtype, int layout, bool aligned, bool wide, F&& f) {
    auto l4 = [&](auto dt, auto lay, auto al) { if (wide) f(dt, lay, al, std::true_type{}); else f(dt, lay, al, std::false_type{}); };
    auto l3 = [&](auto dt, auto lay) { if (aligned) l4(dt, lay, std::true_type{}); else l4(dt, lay, std::false_type{}); };
    auto l2 = [&](auto dt) {
        if (layout == SL_LAYOUT_NCHW) l3(dt, std::integral_constant<int, kLayNCHW>{}); else l3(dt, std::integral_constant<int, kLayNHWC>{});
    };
    if (dtype == SL_DTYPE_F32) l2(std::integral_constant<int, kDtF32>{});
    else if (dtype == SL_DTYPE_F16) l2(std::integral_constant<int, kDtF16>{});
    else l2(std::integral_constant<int, kDtBF16>{});
}

int check_shape(const void* rgb, const void* out, int n, int h, int w) {
    if (!rgb || !out || n <= 0 || h <= 0 || w <= 0) return SL_ERR_BADARG;
    if ((long)h * w > (1L << 30)) return SL_ERR_BADARG;
    return SL_OK;
}

}  // namespace

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
    const long P = (long)h * w;
    const int parts = parts_for(P);
    const dim3 grid((unsigned)((long)n * parts)), block(kWG);
    const TensorK k = tensor_k(*fmt);
    with_format(fmt->dtype, fmt->layout, aligned4(rgb, P), wide_ok(out, P, fmt->dtype), [&](auto dt, auto lay, auto al, auto wide) {
        hipLaunchKernelGGL((k_to_tensor<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value>), grid, block, 0,
                           (hipStream_t)stream, rgb, out, (int)P, parts, k);
    });
    return launch_status();
}

extern "C" int sl_normalize_apply_tensor(const uint8_t* rgb, void* out, int n, int h, int w, const double* M_src, const double* maxC_src,
                                         const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlTensorFormat* fmt,
                                         void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!M_src || !maxC_src || !M_tgt || !maxC_tgt) return SL_ERR_BADARG;
    if (!format_ok(fmt)) return SL_ERR_BADARG;
    const long P = (long)h * w;
    const int parts = parts_for(P);
    const dim3 grid((unsigned)((long)n * parts)), block(kWG);
    const TensorK k = tensor_k(*fmt);
    with_format(fmt->dtype, fmt->layout, aligned4(rgb, P), wide_ok(out, P, fmt->dtype), [&](auto dt, auto lay, auto al, auto wide) {
        hipLaunchKernelGGL((k_apply_tensor<decltype(dt)::value, decltype(lay)::value, decltype(al)::value, decltype(wide)::value>), grid, block, 0,
                           (hipStream_t)stream, rgb, out, (int)P, parts, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda, k);
    });
    return launch_status();
}
