// view_elastic.hip -- C-ABI launchers of the elastic views: the affine view plus a smooth displacement field in the view pass, bilinear for
// the images (kernel: view_elastic_kernels.hpp) and nearest for their companion planes (kernel: planes_elastic_kernels.hpp).  The route
// checks and the dispatch are the views' own (route_host.hpp); the geometry check is here.
#include "view_elastic_kernels.hpp"
#include "planes_elastic_kernels.hpp"
#include "route_host.hpp"

using namespace sl;

// The geometry of an elastic view of n tiles (or planes): SL_OK and the upper bound of the patches of a tile -- those of the smallest
// patch edge the bounds max_r and max_d let through --, or SL_ERR_BADARG.  The windows and the field themselves may live on the device
// and are clamped there.
static int view_elastic_geometry(long n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, const int32_t* field, int cell_log2,
                                 int max_d, long& npatch) {
    if (!windows || oh < 1 || ow < 1) return SL_ERR_BADARG;
    if (h > kAffineMaxSide || w > kAffineMaxSide || oh > kAffineMaxSide || ow > kAffineMaxSide) return SL_ERR_BADARG;
    if (max_r < 1 || max_r > kAffineMaxR) return SL_ERR_BADARG;
    if (!field || ((uintptr_t)field & 3u) != 0) return SL_ERR_BADARG;
    if (cell_log2 < kElasticMinCellLog2 || cell_log2 > kElasticMaxCellLog2) return SL_ERR_BADARG;
    if (max_d < 0 || max_d > kElasticMaxD) return SL_ERR_BADARG;
    npatch = elastic_grid_patches(oh, ow, max_r, max_d);
    if (n * npatch > 0x7fffffffL) return SL_ERR_BADARG;                          // one workgroup per (tile, patch)
    return SL_OK;
}

extern "C" int sl_normalize_view_elastic(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                         int max_r, const int32_t* field, int cell_log2, int max_d, uint32_t fill_rgb, const double* M_src,
                                         const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
                                         int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream) {
    long npatch = 0;
    RouteView v;
    const int nn = n == 0 ? 1 : n;                                               // an empty batch: every check of one tile, no launch
    if (const int rc = route_view_checks(rgb, out, nn, h, w,
                                         [&] {
                                             if (fill_rgb >= (1u << 24)) return SL_ERR_BADARG;
                                             return view_elastic_geometry(nn, h, w, oh, ow, windows, max_r, field, cell_log2, max_d, npatch);
                                         },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    if (n == 0) return SL_OK;
    return launch_route_view(SL_VIEW_FAMILY(k_view_elastic), fmt, v.mode, n * npatch, stream, rgb, out, h, w, oh, ow, (int)npatch, windows,
                             max_r, field, cell_log2, max_d, fill_rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v.p.lasso_lambda, v.ylimf,
                             fmt ? tensor_k(*fmt) : TensorK{});
}

extern "C" int sl_view_planes_elastic(const void* planes, void* out, int n, int c, int h, int w, int elem_bytes, int oh, int ow,
                                      const int32_t* windows, int max_r, const int32_t* field, int cell_log2, int max_d, uint64_t fill_bits,
                                      void* stream) {
    if (!planes || !out || !windows) return SL_ERR_BADARG;
    if (n < 0 || c <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return SL_ERR_BADARG;
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return SL_ERR_BADARG;
    if ((((uintptr_t)planes | (uintptr_t)out) & (uintptr_t)(elem_bytes - 1)) != 0) return SL_ERR_BADARG;
    const long nplanes = (long)n * c;
    if (nplanes > 0x7fffffffL) return SL_ERR_BADARG;
    long npatch = 0;                                                             // one workgroup per (plane, patch)
    if (const int rc = view_elastic_geometry(nplanes, h, w, oh, ow, windows, max_r, field, cell_log2, max_d, npatch)) return rc;
    if (n == 0) return SL_OK;                                                    // an empty batch: nothing is launched
    // the fill element: the low elem_bytes bytes of fill_bits, the rest is not looked at
    const uint32_t lo = (uint32_t)fill_bits & (elem_bytes == 1 ? 0xffu : elem_bytes == 2 ? 0xffffu : 0xffffffffu), hi = (uint32_t)(fill_bits >> 32);
    auto launch = [&](auto es) {
        hipLaunchKernelGGL((k_view_planes_elastic<decltype(es)::value>), dim3((unsigned)(nplanes * npatch)), dim3(kWG), 0, (hipStream_t)stream,
                           (const uint8_t*)planes, (uint8_t*)out, c, h, w, oh, ow, (int)npatch, windows, max_r, field, cell_log2, max_d, lo, hi);
    };
    if (elem_bytes == 1) launch(std::integral_constant<int, 1>{});
    else if (elem_bytes == 2) launch(std::integral_constant<int, 2>{});
    else if (elem_bytes == 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 8>{});
    return launch_status();
}
