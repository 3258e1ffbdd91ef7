// separate.hip -- C-ABI launcher of the stain separation (kernel: separate_kernels.hpp).
#include <type_traits>

#include "separate_kernels.hpp"
#include "sl_host.hpp"

using namespace sl;

namespace {

// f(norm tag, stains tag, conc dtype tag, aligned tag) for the outputs of one call (at least one of them wanted)
template <class F>
void with_outputs(bool norm, bool stains, int cdt, bool aligned, F&& f) {
    auto l4 = [&](auto nt, auto st, auto dt) { if (aligned) f(nt, st, dt, std::true_type{}); else f(nt, st, dt, std::false_type{}); };
    auto l3 = [&](auto nt, auto st) {
        if (cdt == SL_DTYPE_F32) l4(nt, st, std::integral_constant<int, kDtF32>{});
        else if (cdt == SL_DTYPE_F16) l4(nt, st, std::integral_constant<int, kDtF16>{});
        else if (cdt == SL_DTYPE_BF16) l4(nt, st, std::integral_constant<int, kDtBF16>{});
        else if constexpr (decltype(nt)::value || decltype(st)::value) l4(nt, st, std::integral_constant<int, kDtNone>{});
    };
    auto l2 = [&](auto nt) { if (stains) l3(nt, std::true_type{}); else l3(nt, std::false_type{}); };
    if (norm) l2(std::true_type{}); else l2(std::false_type{});
}

}  // namespace

extern "C" void sl_default_separate_out(SlSeparateOut* o) {
    if (!o) return;
    o->struct_size = (uint32_t)sizeof(SlSeparateOut);
    o->conc_dtype = SL_DTYPE_F32;
    o->norm = nullptr;
    o->stain[0] = o->stain[1] = nullptr;
    o->conc = nullptr;
}

extern "C" int sl_stain_separate(const uint8_t* rgb, int n, int h, int w, const double* M_src, const double* maxC_src,
                                 const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlSeparateOut* outs,
                                 void* stream) {
    if (const int rc = check_shape(rgb, n, h, w)) return rc;
    if (!outs || !M_src || !maxC_src || !lambda_ok(lasso_lambda)) return SL_ERR_BADARG;
    if ((M_tgt == nullptr) != (maxC_tgt == nullptr)) return SL_ERR_BADARG;       // both: a target; neither: every tile's own matrix
    const TileLaunch L(n, h, w, kWG);
    const long P = L.P;
    if (outs->struct_size != (uint32_t)sizeof(SlSeparateOut)) return SL_ERR_BADARG;       // (before any other field is read)
    const SlSeparateOut o = *outs;
    if (o.conc_dtype < SL_DTYPE_F32 || o.conc_dtype > SL_DTYPE_BF16) return SL_ERR_BADARG;
    const void* const ptrs[5] = {o.norm, o.stain[0], o.stain[1], o.conc, rgb};
    bool any = false;
    for (int i = 0; i < 4; ++i) {
        if (!ptrs[i]) continue;
        any = true;
        for (int j = i + 1; j < 5; ++j)
            if (ptrs[j] == ptrs[i]) return SL_ERR_BADARG;
    }
    if (!any) return SL_ERR_BADARG;
    if (o.conc && ((uintptr_t)o.conc % elem_bytes(o.conc_dtype)) != 0) return SL_ERR_BADARG;

    bool aligned = aligned4(rgb, P);
    for (int i = 0; i < 3; ++i) aligned = aligned && (!ptrs[i] || aligned4(ptrs[i], P));
    if (o.conc) aligned = aligned && wide_ok(o.conc, P, o.conc_dtype);
    const SeparateOut d{o.norm, {o.stain[0], o.stain[1]}, o.conc};
    with_outputs(o.norm != nullptr, o.stain[0] || o.stain[1], o.conc ? o.conc_dtype : kDtNone, aligned, [&](auto nt, auto st, auto dt, auto al) {
        hipLaunchKernelGGL((k_separate<decltype(nt)::value, decltype(st)::value, decltype(dt)::value, decltype(al)::value>), L.grid, L.block, 0,
                           (hipStream_t)stream, rgb, d, (int)P, L.parts, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda);
    });
    return launch_status();
}
