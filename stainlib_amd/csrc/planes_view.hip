// planes_view.hip -- C-ABI launcher of the companion planes of a view pass (kernel: planes_view_kernels.hpp).  The geometry checks are
// the image views' own (route_host.hpp: view_geometry, view_resize_geometry) on n c planes in the place of n tiles.
#include "planes_view_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

extern "C" int sl_view_planes(const void* planes, void* out, int n, int c, int h, int w, int elem_bytes, int oh, int ow,
                              const int32_t* windows, int d_mask, int shrink, int max_wh, int max_ww, int mode, void* stream) {
    if (!planes || !out || !windows) return SL_ERR_BADARG;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return SL_ERR_BADARG;
    if ((long)h * w > (1L << 30)) return SL_ERR_BADARG;
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return SL_ERR_BADARG;
    if ((((uintptr_t)planes | (uintptr_t)out) & (uintptr_t)(elem_bytes - 1)) != 0) return SL_ERR_BADARG;
    if (mode != SL_PLANES_NEAREST && mode != SL_PLANES_AREA) return SL_ERR_BADARG;
    if (mode == SL_PLANES_AREA && elem_bytes != 1) return SL_ERR_BADARG;
    if (max_wh < 0 || max_ww < 0 || (max_wh == 0) != (max_ww == 0)) return SL_ERR_BADARG;
    const bool resizing = max_wh > 0;
    if (resizing && shrink != 1) return SL_ERR_BADARG;
    const long nplanes = (long)n * c;
    if (nplanes > 0x7fffffffL) return SL_ERR_BADARG;
    long npx = 1, npatch = 0;                                                    // one workgroup per (plane, patch): the geometry checks the grid
    if (const int rc = resizing ? view_resize_geometry((int)nplanes, h, w, oh, ow, windows, d_mask, max_wh, max_ww, npatch)
                                : view_geometry((int)nplanes, h, w, oh, ow, windows, d_mask, shrink, npx, npatch))
        return rc;
    auto launch = [&](auto es, auto m) {
        hipLaunchKernelGGL((k_view_planes<decltype(es)::value, decltype(m)::value>), dim3((unsigned)(nplanes * npatch)), dim3(kWG), 0,
                           (hipStream_t)stream, (const uint8_t*)planes, (uint8_t*)out, c, h, w, oh, ow, (int)npx, (int)npatch, windows, d_mask,
                           shrink, max_wh, max_ww);
    };
    const std::integral_constant<int, kPlanesNearest> nearest{};
    // (without a shrink or a resize both modes are the same permutation: the nearest kernel)
    if (mode == SL_PLANES_AREA && (resizing || shrink != 1)) launch(std::integral_constant<int, 1>{}, std::integral_constant<int, kPlanesArea>{});
    else if (elem_bytes == 1) launch(std::integral_constant<int, 1>{}, nearest);
    else if (elem_bytes == 2) launch(std::integral_constant<int, 2>{}, nearest);
    else if (elem_bytes == 4) launch(std::integral_constant<int, 4>{}, nearest);
    else launch(std::integral_constant<int, 8>{}, nearest);
    return launch_status();
}
