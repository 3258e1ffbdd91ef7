// route_host.hpp -- host-side helpers of the entry points on the apply-pass frame (jitter.hip, view.hip, hed_view.hip).
// The *route* is the pointer pattern (M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background) by which a call names the
// image it would write: the tiles' own bytes, sl_normalize_apply's, the jitter under a target or the jitter under the tile's own matrix.
#pragma once
#include "view_resize_kernels.hpp" // kView*, kViewB (view_kernels.hpp through it), resize_patch_edge
#include "tensor_host.hpp"

namespace sl {

// SL_OK and the kView* mode of a route, or SL_ERR_BADARG.  (sl_normalize_apply, sl_normalize_apply_tensor, sl_normalize_jitter and
// sl_stain_separate each accept one fixed part of this pattern and keep their own, narrower rule.)
inline int route_of(const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
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
inline void with_mode(int mode, F&& f) {
    if (mode == kViewRaw) f(std::integral_constant<int, kViewRaw>{});
    else if (mode == kViewApply) f(std::integral_constant<int, kViewApply>{});
    else if (mode == kViewJitTissue) f(std::integral_constant<int, kViewJitTissue>{});
    else f(std::integral_constant<int, kViewJitAll>{});
}

// The geometry of a view of n tiles of h x w (check_shape has accepted them) under the shrink s: SL_OK and the patches (kViewB / s output
// pixels square) per output row and per tile, or SL_ERR_BADARG.  The window is s times the output.
inline int view_geometry(int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int s, long& npx, long& npatch) {
    if (s != 1 && s != 2 && s != 4) return SL_ERR_BADARG;
    if (!windows || oh < 1 || ow < 1 || (long)s * oh > h || (long)s * ow > w) return SL_ERR_BADARG;
    if (d_mask < 0 || d_mask > 7) return SL_ERR_BADARG;
    if ((d_mask & 1) && ((long)s * ow > h || (long)s * oh > w)) return SL_ERR_BADARG;   // the transposed window must fit too
    const int B = kViewB / s;
    npx = (ow + B - 1) / B;
    npatch = npx * ((oh + B - 1) / B);
    if ((long)n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                    // one workgroup per (tile, patch)
    return SL_OK;
}

// The geometry of a resizing view (view_resize_kernels.hpp) of n tiles of h x w whose windows are at most max_wh x max_ww: SL_OK and the
// upper bound of the patches of a tile -- those of the largest window the kernel lets through, in either orientation d_mask allows --
// or SL_ERR_BADARG.  The window sides themselves may live on the device and are clamped there.
inline int view_resize_geometry(int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int max_wh, int max_ww, long& npatch) {
    if (!windows || oh < 1 || ow < 1) return SL_ERR_BADARG;
    if (d_mask < 0 || d_mask > 7) return SL_ERR_BADARG;
    if (max_wh < 1 || max_wh > h || max_ww < 1 || max_ww > w) return SL_ERR_BADARG;
    if ((long)max_wh * max_ww > kResizeMaxArea) return SL_ERR_BADARG;
    if ((long)(oh > ow ? oh : ow) * (max_wh > max_ww ? max_wh : max_ww) > kResizeMaxProduct) return SL_ERR_BADARG;
    auto patches = [&](int nu, int nv) {
        const int bu = resize_patch_edge(nu, resize_side_max(nu, max_wh)), bv = resize_patch_edge(nv, resize_side_max(nv, max_ww));
        return (long)((nu + bu - 1) / bu) * ((nv + bv - 1) / bv);
    };
    npatch = patches(oh, ow);
    if (d_mask & 1) npatch = std::max(npatch, patches(ow, oh));
    if ((long)n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                    // one workgroup per (tile, patch)
    return SL_OK;
}

// f(dtype tag, layout tag, aligned tag, wide tag) for a format format_ok has accepted (with_format), or for the uint8 image when there
// is none: kDtU8 / kLayNHWC -- its layout and the wide stores do not apply.
template <class F>
inline void with_format_or_u8(const SlTensorFormat* fmt, bool aligned, bool wide, F&& f) {
    if (fmt) return with_format(fmt->dtype, fmt->layout, aligned, wide, f);
    const std::integral_constant<int, kDtU8> u8{};
    const std::integral_constant<int, kLayNHWC> lay{};
    if (aligned) f(u8, lay, std::true_type{}, std::false_type{});
    else f(u8, lay, std::false_type{}, std::false_type{});
}

// ---- the four route views (sl_normalize_view_shrink / _view_resize, sl_normalize_hed_view_shrink / _hed_view_resize) -------------------
struct RouteView { int mode; SlParams p; float ylimf; };      // what the common checks hand on: kView*, the parameters, tissue_ylimf

// The common checks, in the order the entry points have always made them -- a call that is wrong in two ways keeps its return code --:
// check_shape, the geometry (a callable returning view_geometry's or view_resize_geometry's code), route_of, params_ok, format_ok.
template <class Geometry>
inline int route_view_checks(const uint8_t* rgb, const void* out, int n, int h, int w, Geometry&& geometry, const double* M_src,
                             const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
                             int augment_background, const SlParams* params, const SlTensorFormat* fmt, RouteView& v) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (const int rc = geometry()) return rc;
    if (const int rc = route_of(M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, v.mode)) return rc;
    if (!params_ok(params)) return SL_ERR_BADARG;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    v.p = params_or_defaults(params);
    v.ylimf = tissue_ylimf(v.p);
    return SL_OK;
}

// A kernel family k<DT, LAYOUT, MODE> as a value (a function template cannot be a template argument, a generic lambda can be passed),
// and its launch on nblocks workgroups of kWG threads with args (no ALIGNED / WIDE variants: view_kernels.hpp)
#define SL_VIEW_FAMILY(k) [](auto dt, auto lay, auto m) { return k<decltype(dt)::value, decltype(lay)::value, decltype(m)::value>; }
template <class Family, class... Args>
inline int launch_route_view(Family family, const SlTensorFormat* fmt, int mode, long nblocks, void* stream, Args... args) {
    with_format_or_u8(fmt, false, false, [&](auto dt, auto lay, auto, auto) {
        with_mode(mode, [&](auto m) {
            hipLaunchKernelGGL(family(dt, lay, m), dim3((unsigned)nblocks), dim3(kWG), 0, (hipStream_t)stream, args...);
        });
    });
    return launch_status();
}

}  // namespace sl
