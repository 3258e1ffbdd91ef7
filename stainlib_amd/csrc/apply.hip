// apply.hip -- C-ABI launchers of the per-pixel sweeps in apply_kernels.hpp and of k_apply (apply_pass.hpp).
#include "apply_pass.hpp"
#include "sl_host.hpp"

using namespace sl;

extern "C" int sl_normalize_apply(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* M_src,
                                  const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                  double lasso_lambda, float* prequant, void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!M_src || !maxC_src || !M_tgt || !maxC_tgt || !lambda_ok(lasso_lambda)) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    const bool al = aligned4(rgb, L.P) && aligned4(out, L.P);
    launch_aligned(al, prequant ? k_apply<true, true> : k_apply<true, false>, prequant ? k_apply<false, true> : k_apply<false, false>, L.grid,
                   L.block, 0, (hipStream_t)stream, rgb, out, (int)L.P, L.parts, M_src, maxC_src, M_tgt, maxC_tgt, lasso_lambda, prequant);
    return launch_status();
}

extern "C" int sl_stain_augment(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* M,
                                const double* alpha_beta, int augment_background, const SlParams* params,
                                void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!M || !alpha_beta || !params_ok(params)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    const long P = (long)h * w;
    const int max_grid = max_resident_grid();
    const int parts = sweep_parts(P, n, max_grid);
    const long items = (long)n * parts;
    const dim3 grid((unsigned)(items < max_grid ? items : max_grid)), block(kAugThreads);
    const uint32_t y_lim = y_limit_for_threshold(p.luminosity_threshold);
    hipStream_t s = (hipStream_t)stream;
    launch_aligned(aligned4(rgb, P) && aligned4(out, P), k_stain_augment<true>, k_stain_augment<false>, grid, block, 0, s, rgb, out, (int)P,
                   parts, (int)items, M, alpha_beta, augment_background, y_lim, p.lasso_lambda);
    return launch_status();
}

extern "C" int sl_grayscale_augment(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* alpha_beta,
                                   void* stream) {
    if (const int rc = check_shape(rgb, out, n, h, w)) return rc;
    if (!alpha_beta) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    launch_aligned(aligned4(rgb, L.P) && aligned4(out, L.P), k_grayscale<true>, k_grayscale<false>, L.grid, L.block, 0, (hipStream_t)stream, rgb,
                   out, (int)L.P, L.parts, alpha_beta);
    return launch_status();
}

extern "C" int sl_concentrations(const uint8_t* rgb, int n, int h, int w, const double* M, double lasso_lambda,
                                 float* C_out, void* stream) {
    if (const int rc = check_shape(rgb, C_out, n, h, w)) return rc;
    if (!M || !lambda_ok(lasso_lambda)) return SL_ERR_BADARG;
    const TileLaunch L(n, h, w, kWG);
    hipLaunchKernelGGL(k_concentrations, L.grid, L.block, 0, (hipStream_t)stream, rgb, (int)L.P, L.parts, M, lasso_lambda, C_out);
    return launch_status();
}

extern "C" int sl_tissue_mask(const uint8_t* rgb, int n, int h, int w, double luminosity_threshold,
                              uint8_t* mask_out, int64_t* counts, void* stream) {
    if (const int rc = check_shape(rgb, n, h, w)) return rc;
    const TileLaunch L(n, h, w, kWG);
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(int64_t) % 4 == 0, "zero_async clears whole words");
    if (counts) {
        if (const int rc = zero_async(counts, sizeof(int64_t) * (size_t)n, s)) return rc;
    }
    hipLaunchKernelGGL(k_tissue_mask, L.grid, L.block, 0, s, rgb, (int)L.P, L.parts,
                       y_limit_for_threshold(luminosity_threshold), mask_out, (unsigned long long*)counts);
    return launch_status();
}
