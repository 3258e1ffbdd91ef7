// sl_host.hpp -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stainlib_hip.h"

namespace sl {

inline int hip_err(hipError_t e) { return e == hipSuccess ? SL_OK : SL_ERR_HIP_BASE - (int)e; }

#define SL_HIP_TRY(expr)                                   \
    do {                                                   \
        hipError_t e__ = (expr);                           \
        if (e__ != hipSuccess) return ::sl::hip_err(e__);  \
    } while (0)

inline int launch_status() { return hip_err(hipGetLastError()); }

// An SlParams handed over by the caller: NULL (defaults) or a struct of THIS header's size (SlParams.struct_size, set by sl_default_params).
// (and with its enumerated fields inside their ranges: an unknown two_sweep used to run as "automatic" without a word)
// (... and its numbers inside the ranges numpy and the lasso accept: np.percentile raises outside [0, 100], a negative penalty has no
//  minimiser; NaN fails every comparison.  luminosity_threshold is unrestricted: every value, NaN included, has a meaning in the reference)
inline bool lambda_ok(double lasso_lambda) { return lasso_lambda >= 0.0; }
inline bool percentile_ok(double pct) { return pct >= 0.0 && pct <= 100.0; }
inline bool params_ok(const SlParams* p) {
    return !p || (p->struct_size == (uint32_t)sizeof(SlParams) && p->two_sweep >= 0 && p->two_sweep <= 4 && percentile_ok(p->angular_percentile) &&
                  lambda_ok(p->lasso_lambda));
}

// The angular percentile the selection kernels run with.  The reference takes the pair (100 - pct, pct) and orders the two stain vectors
// afterwards (macenko_stain_extractor.py:33-43), so pct and 100 - pct give the same matrix; the kernels are built for the upper one --
// bracket 0 below bracket 1, the plain pixels between them.
inline double folded_percentile(double pct) { return pct < 100.0 - pct ? 100.0 - pct : pct; }

// The SlParams a call runs with, once params_ok has accepted them: the caller's, or the defaults for NULL.
inline SlParams params_or_defaults(const SlParams* params) {
    SlParams p;
    sl_default_params(&p);
    if (params) p = *params;
    return p;
}

// Largest index into OpenCV's LabCbrtTab_b whose 8-bit L satisfies L/255.0 < threshold, +1,
// shifted to the fixed-point scale the kernels compare against (see is_tissue()).
// 0 means "no pixel is tissue".
uint32_t y_limit_for_threshold(double luminosity_threshold);

// The tissue limit as the sweep kernels take it: y_limit_for_threshold - 2048 as a float (exact: y_lim < 2^24).
inline float tissue_ylimf(const SlParams& p) { return (float)y_limit_for_threshold(p.luminosity_threshold) - 2048.0f; }

// resident persistent-sweep workgroups of the current device (2 per CU; see common.hip)
int max_resident_grid();

// zeroes `bytes` at p with a kernel on s and returns the launch status: see common.hip (hipMemsetAsync is not capture-safe here).
// p must be 4-byte aligned and bytes a multiple of 4 (callers static_assert it where the size is a sizeof); nothing checks it here.
int zero_async(void* p, size_t bytes, hipStream_t s);

// workspace of the Lab family (lab.hip)
size_t lab_workspace_bytes(int n_tiles);

// The launchers that give every (tile, part) a workgroup of its own hand n * parts to dim3 as an unsigned: a batch whose product
// does not fit a signed 32-bit grid is refused where the shape is checked (the view routes check n * npatch the same way:
// view_geometry of route_host.hpp), never truncated.
inline bool grid_fits(int n, long parts) { return (long)n * parts <= 0x7fffffffL; }

// Workgroups a tile of P pixels is split into for the streaming sweeps: ~32 Ki pixels each,
// at least 1, so that a batch of >=32 tiles launches >>256 workgroups.
inline int parts_for(long P) {
    long p = (P + 32767) / 32768;
    return (int)(p < 1 ? 1 : p);
}

// The shape checks every per-tile entry point starts with: the input, a positive batch and tile, at most 2^30 pixels per tile, and
// a (tile, part) grid that fits (grid_fits).
inline int check_shape(const void* rgb, int n, int h, int w) {
    if (!rgb || n <= 0 || h <= 0 || w <= 0) return SL_ERR_BADARG;
    if ((long)h * w > (1L << 30)) return SL_ERR_BADARG;
    if (!grid_fits(n, parts_for((long)h * w))) return SL_ERR_BADARG;
    return SL_OK;
}
inline int check_shape(const void* rgb, const void* out, int n, int h, int w) { return out ? check_shape(rgb, n, h, w) : SL_ERR_BADARG; }

inline bool aligned4(const void* p, long pixels_per_tile) {
    return ((uintptr_t)p & 3u) == 0 && (pixels_per_tile & 3) == 0;
}

inline size_t elem_bytes(int dtype) { return dtype == SL_DTYPE_F32 ? 4 : 2; }      // of an SL_DTYPE_*

// The wide store path of the float outputs (tensor_out.hip, separate.hip) needs every tile's (NHWC) or every plane's (planar) first
// element on a 16-byte boundary: the pointer itself and P elements (3 P for NHWC) a multiple of 16 bytes -- either way P a multiple
// of the 4 (float32) or 8 (half types) pixels of a group.
inline bool wide_ok(const void* out, long P, int dtype) {
    const long px = 16 / (long)elem_bytes(dtype);
    return ((uintptr_t)out & 15u) == 0 && P % px == 0;
}

inline void inv3(const double* m, double* o) {
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    o[0] = (e * i - f * h) / det; o[1] = (c * h - b * i) / det; o[2] = (b * f - c * e) / det;
    o[3] = (f * g - d * i) / det; o[4] = (a * i - c * g) / det; o[5] = (c * d - a * f) / det;
    o[6] = (d * h - e * g) / det; o[7] = (b * g - a * h) / det; o[8] = (a * e - b * d) / det;
}

// The constants of every HED kernel (hed.hip, hed_view.hip), row-major: R = skimage.color.rgb_from_hed (colorconv.py:475-478),
// H = hed_from_rgb = inv(R).
inline void hed_matrices(double* R, double* H) {
    const double m[9] = {0.65, 0.70, 0.29, 0.07, 0.99, 0.11, 0.27, 0.57, 0.78};
    for (int k = 0; k < 9; ++k) R[k] = m[k];
    inv3(m, H);
}

// Launches k_aligned when `aligned`(aligned4 of every tile pointer the kernel reads or writes), else k_unaligned: the two
// instantiations of one sweep kernel, with the same geometry and arguments.
template <class K, class... Args>
inline void launch_aligned(bool aligned, K k_aligned, K k_unaligned, dim3 grid, dim3 block, unsigned lds, hipStream_t s, Args... args) {
    if (aligned) hipLaunchKernelGGL(k_aligned, grid, block, lds, s, args...);
    else hipLaunchKernelGGL(k_unaligned, grid, block, lds, s, args...);
}

// The geometry of the launchers that give every (tile, part) a workgroup of its own.  `threads` is always kWG: a parameter only
// because kWG lives in sl_device.hpp, which this host-side header does not include (common.hip builds without it).
struct TileLaunch {
    long P;
    int parts;
    dim3 grid, block;
    TileLaunch(int n, int h, int w, int threads) : P((long)h * w), parts(parts_for(P)), grid((unsigned)((long)n * parts)), block(threads) {}
};

// parts_for(P) for n tiles walked by max_grid persistent workgroups: no more parts than it takes to give every workgroup ~4 items.
// (n <= 0 is taken as one tile: workspace sizing asks before the tile count is checked.)
inline int sweep_parts(long P, int n, int max_grid) {
    const int parts = parts_for(P);
    const long want = (4L * max_grid + n - 1) / (n > 0 ? n : 1);
    return parts > want ? (int)(want < 1 ? 1 : want) : parts;
}

// Brackets one launch with two caller-provided events when the class is selected (see SlProfile).
struct ProfScope {
    SlProfile* p;
    hipStream_t s;
    bool on;
    ProfScope(SlProfile* prof, int cls, int tiles, hipStream_t stream) : p(prof), s(stream), on(false) {
        if (p && (p->mask & cls) && p->events && p->used + 2 <= p->capacity) {
            on = true;
            if (p->tags) p->tags[p->used / 2] = cls;
            if (p->tiles) p->tiles[p->used / 2] = tiles;
            (void)hipEventRecord((hipEvent_t)p->events[p->used], s);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord((hipEvent_t)p->events[p->used + 1], s);
            p->used += 2;
        }
    }
};

}  // namespace sl
