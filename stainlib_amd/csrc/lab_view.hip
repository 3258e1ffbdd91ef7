// lab_view.hip -- C-ABI launchers of the Lab family in the one-pass loader: the Reinhard / luminosity map, per tile or under a slide's
// pooled tables, with the view (crop, flip, quarter turn) and the tensor conversion in the same sweep (kernel: lab_view_kernels.hpp).
// The statistics and the tables in front of it are lab.hip's and slide_lab.hip's, unchanged.
#include "lab_view_kernels.hpp"
#include "lab_host.hpp"
#include "route_host.hpp"

using namespace sl;

namespace {

// what the three entry points check of the output side, behind their shape check
int lab_view_check(const void* rgb, const void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink,
                   const SlTensorFormat* fmt, long& npx, long& npatch) {
    if (const int rc = view_geometry(n, h, w, oh, ow, windows, d_mask, shrink, npx, npatch)) return rc;
    if (fmt && !format_ok(fmt)) return SL_ERR_BADARG;
    if (out && out == (const void*)rgb) return SL_ERR_BADARG;                    // no in-place view
    return SL_OK;
}

// k_lab_view over n tiles: one workgroup per (tile, run of kLabViewRun patches)
template <bool AB_TABLES>
int lab_view_launch(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, long npx, long npatch, const int32_t* windows,
                    int d_mask, int shrink, const LabMapTabs* tabs, size_t stride_bytes, const double* status, int mask_background, double thr,
                    double* p_out, const SlTensorFormat* fmt, hipStream_t s) {
    const long nrun = (npatch + kLabViewRun - 1) / kLabViewRun;
    with_format_or_u8(fmt, false, false, [&](auto dt, auto lay, auto, auto) {     // (no ALIGNED / WIDE variants: see view_kernels.hpp)
        hipLaunchKernelGGL((k_lab_view<decltype(dt)::value, decltype(lay)::value, AB_TABLES>), dim3((unsigned)(n * nrun)), dim3(kWG), 0, s,
                           rgb, out, h, w, oh, ow, (int)npx, (int)npatch, (int)nrun, windows, d_mask, shrink, tabs, stride_bytes, status,
                           mask_background, thr, p_out, fmt ? tensor_k(*fmt) : TensorK{});
    });
    return launch_status();
}

}  // namespace

extern "C" int sl_reinhard_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                       int shrink, const double* target_means, const double* target_stds, int mask_background,
                                       double luminosity_threshold, double* stats_out, void* workspace, size_t workspace_bytes,
                                       const SlTensorFormat* fmt, void* stream) {
    if (const int rc = lab_check(rgb, out, n, h, w, workspace, workspace_bytes)) return rc;
    long npx = 0, npatch = 0;
    if (const int rc = lab_view_check(rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, fmt, npx, npatch)) return rc;
    if (!target_means || !target_stds) return SL_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = lab_reinhard_tables(rgb, n, (long)h * w, target_means, target_stds, luminosity_threshold, stats_out, workspace, s))
        return rc;
    return lab_view_launch<true>(rgb, out, n, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, lab_tabs_of(workspace, n), sizeof(LabTileTabs),
                                 nullptr, mask_background ? 1 : 0, luminosity_threshold, nullptr, fmt, s);
}

extern "C" int sl_luminosity_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                         int d_mask, int shrink, double percentile, double* p_out, void* workspace, size_t workspace_bytes,
                                         const SlTensorFormat* fmt, void* stream) {
    if (const int rc = lab_check(rgb, out, n, h, w, workspace, workspace_bytes)) return rc;
    long npx = 0, npatch = 0;
    if (const int rc = lab_view_check(rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, fmt, npx, npatch)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = lab_luminosity_tables(rgb, n, (long)h * w, percentile, workspace, s)) return rc;
    // (k_lab_map<1>'s arguments: no background mask, every L8 below the limit)
    return lab_view_launch<false>(rgb, out, n, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, lab_tabs_of(workspace, n), sizeof(LabTileTabs),
                                  nullptr, 0, 2.0, p_out, fmt, s);
}

extern "C" int sl_slab_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                   int shrink, const double* state, int mode, int mask_background, double luminosity_threshold,
                                   const SlTensorFormat* fmt, void* stream) {
    if (!slab_shape_ok(n, h, w) || !state || (mode != 0 && mode != 1)) return SL_ERR_BADARG;
    if (n > 0 && (!rgb || !out)) return SL_ERR_BADARG;
    long npx = 0, npatch = 0;
    const int32_t none[3] = {0, 0, 0};                                   // (an empty shard needs no windows)
    if (const int rc = lab_view_check(rgb, out, n, h, w, oh, ow, n > 0 ? windows : none, d_mask, shrink, fmt, npx, npatch)) return rc;
    if (n == 0) return SL_OK;                                            // an empty shard: nothing to launch
    // (k_slab_map's arguments: its one instantiation maps a and b through the tables in both modes -- mode 1's hold lab_adiv / lab_bdiv)
    return lab_view_launch<true>(rgb, out, n, h, w, oh, ow, npx, npatch, windows, d_mask, shrink,
                                 reinterpret_cast<const LabMapTabs*>(state + SL_SLAB_TABLES), 0, state + SL_SLAB_STATUS,
                                 (mode == 0 && mask_background) ? 1 : 0, luminosity_threshold, nullptr, fmt, (hipStream_t)stream);
}

// ---- the entry points without a shrink: shrink = 1 ----------------------------------------------------------------------------------
extern "C" int sl_reinhard_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                const double* target_means, const double* target_stds, int mask_background, double luminosity_threshold,
                                double* stats_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt, void* stream) {
    return sl_reinhard_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, 1, target_means, target_stds, mask_background,
                                   luminosity_threshold, stats_out, workspace, workspace_bytes, fmt, stream);
}

extern "C" int sl_luminosity_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                  double percentile, double* p_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt,
                                  void* stream) {
    return sl_luminosity_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, 1, percentile, p_out, workspace, workspace_bytes, fmt, stream);
}

extern "C" int sl_slab_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                            const double* state, int mode, int mask_background, double luminosity_threshold, const SlTensorFormat* fmt,
                            void* stream) {
    return sl_slab_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, 1, state, mode, mask_background, luminosity_threshold, fmt, stream);
}
