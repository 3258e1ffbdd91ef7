// recipe.hip -- C-ABI entry points of the one-pass recipe: a colour stage on source pixels (HED or HSB), a view of any kind and the post
// stage on written pixels in ONE launch (include/stainlib_hip.h: SlViewStages).  Here: the checks -- the parent entry
// point's, in its order, then the stages' --, the forwarding of the calls an existing entry point covers, and the dispatch on (colour,
// post).  No kernel is instantiated in this translation unit: the families live in recipe_*.hip (recipe_host.hpp says why).
#include "recipe_host.hpp"
#include "route_host.hpp"
#include "view_elastic_kernels.hpp"  // the affine and elastic geometry: kAffineMaxSide, affine_grid_patches, elastic_grid_patches

using namespace sl;

namespace {

struct Stages { int hed; bool post; };   // which colour stage (0, 1: HED, 2: HSB) and whether the post stage is there

// SL_OK, which stages a call has and their arguments in c; or SL_ERR_BADARG
int stages_of(const SlViewStages* s, RecipeCall& c, Stages& st) {
    if (!s || s->struct_size != sizeof(SlViewStages)) return SL_ERR_BADARG;
    const bool any_hed = s->hed_sigma || s->hed_bias || s->hed_applied;
    const bool all_hed = s->hed_sigma && s->hed_bias && s->hed_applied;
    if (any_hed != all_hed) return SL_ERR_BADARG;                                // an incomplete triple
    if (all_hed && s->hsb_codes) return SL_ERR_BADARG;                           // one colour stage
    if (s->skimage_mode != SL_HED_SKIMAGE_018) return SL_ERR_BADARG;
    if (((uintptr_t)s->hsb_codes | (uintptr_t)s->noise_codes) & 3u) return SL_ERR_BADARG;
    st.hed = all_hed ? 1 : (s->hsb_codes ? 2 : 0);
    st.post = s->tone_tables || s->noise_codes;
    if (st.hed == 0 && !st.post) return SL_ERR_BADARG;                           // no stage at all
    c.hed = HedViewArgs{};
    if (st.hed == 1) {
        c.hed.sigma = s->hed_sigma; c.hed.bias = s->hed_bias; c.hed.applied = s->hed_applied;
        hed_matrices(c.hed.R, c.hed.H);                                          // sl_hed_augment's
    }
    c.hsb.codes = s->hsb_codes;
    c.post.tables = s->tone_tables;
    c.post.codes = s->noise_codes;
    return SL_OK;
}

// the common part of a call that has passed route_view_checks
void route_into(RecipeCall& c, const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, const double* M_src,
                const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, const RouteView& v,
                const SlTensorFormat* fmt, void* stream) {
    c.rgb = rgb; c.out = out; c.n = n; c.h = h; c.w = w; c.oh = oh; c.ow = ow; c.windows = windows;
    c.M_src = M_src; c.maxC_src = maxC_src; c.M_tgt = M_tgt; c.maxC_tgt = maxC_tgt; c.alpha_beta = alpha_beta;
    c.mode = v.mode; c.lam = v.p.lasso_lambda; c.ylimf = v.ylimf; c.fmt = fmt; c.stream = stream;
}

// the affine view's geometry check (view_affine.hip holds the same lines for its own entry points)
int affine_geometry(long n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, long& npatch) {
    if (!windows || oh < 1 || ow < 1) return SL_ERR_BADARG;
    if (h > kAffineMaxSide || w > kAffineMaxSide || oh > kAffineMaxSide || ow > kAffineMaxSide) return SL_ERR_BADARG;
    if (max_r < 1 || max_r > kAffineMaxR) return SL_ERR_BADARG;
    npatch = affine_grid_patches(oh, ow, max_r);
    if (n * npatch > 0x7fffffffL) return SL_ERR_BADARG;
    return SL_OK;
}

// the elastic view's (view_elastic.hip)
int elastic_geometry(long n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, const int32_t* field, int cell_log2, int max_d,
                     long& npatch) {
    if (!windows || oh < 1 || ow < 1) return SL_ERR_BADARG;
    if (h > kAffineMaxSide || w > kAffineMaxSide || oh > kAffineMaxSide || ow > kAffineMaxSide) return SL_ERR_BADARG;
    if (max_r < 1 || max_r > kAffineMaxR) return SL_ERR_BADARG;
    if (!field || ((uintptr_t)field & 3u) != 0) return SL_ERR_BADARG;
    if (cell_log2 < kElasticMinCellLog2 || cell_log2 > kElasticMaxCellLog2) return SL_ERR_BADARG;
    if (max_d < 0 || max_d > kElasticMaxD) return SL_ERR_BADARG;
    npatch = elastic_grid_patches(oh, ow, max_r, max_d);
    if (n * npatch > 0x7fffffffL) return SL_ERR_BADARG;
    return SL_OK;
}

// f(HED tag, POST tag) for the stages of an affine / elastic call
template <class F>
int with_stages(const Stages& st, F&& f) {
    const std::integral_constant<int, 0> h0{};
    const std::integral_constant<int, 1> h1{};
    const std::integral_constant<int, 2> h2{};
    if (st.hed == 0) return f(h0, std::true_type{});                             // (no stage at all was refused)
    if (st.hed == 1) return st.post ? f(h1, std::true_type{}) : f(h1, std::false_type{});
    return st.post ? f(h2, std::true_type{}) : f(h2, std::false_type{});
}

}  // namespace

extern "C" int sl_normalize_stages_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask,
                                        int shrink, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt,
                                        const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params,
                                        const SlTensorFormat* fmt, const SlViewStages* stages, void* stream) {
    const bool resizing = max_wh != 0;
    const int nn = n == 0 ? 1 : n;                                               // an empty batch: every check of one tile, no launch
    RecipeCall c{};
    RouteView v;
    const auto geometry = [&] {
        if (!resizing) return max_ww == 0 ? view_geometry(nn, h, w, oh, ow, windows, d_mask, shrink, c.npx, c.npatch) : (int)SL_ERR_BADARG;
        if (shrink != 1) return (int)SL_ERR_BADARG;                              // windows of their own sizes have no box shrink
        return view_resize_geometry(nn, h, w, oh, ow, windows, d_mask, max_wh, max_ww, c.npatch);
    };
    if (const int rc = route_view_checks(rgb, out, nn, h, w, geometry, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params,
                                         fmt, v))
        return rc;
    Stages st;
    if (const int rc = stages_of(stages, c, st)) return rc;
    if (n == 0) return SL_OK;
    // the calls an existing entry point covers: its family is not built a second time
    if (!st.post) {
        if (st.hed == 2)
            return sl_normalize_hsb_view(rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                         alpha_beta, augment_background, params, fmt, stages->hsb_codes, stream);
        if (resizing)
            return sl_normalize_hed_view_resize(rgb, out, n, h, w, oh, ow, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                                alpha_beta, augment_background, params, fmt, stages->hed_sigma, stages->hed_bias,
                                                stages->hed_applied, stages->skimage_mode, stream);
        return sl_normalize_hed_view_shrink(rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                                            augment_background, params, fmt, stages->hed_sigma, stages->hed_bias, stages->hed_applied,
                                            stages->skimage_mode, stream);
    }
    if (st.hed == 0)
        return sl_normalize_post_view(rgb, out, n, h, w, oh, ow, windows, d_mask, shrink, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                      alpha_beta, augment_background, params, fmt, stages->tone_tables, stages->noise_codes, stream);
    route_into(c, rgb, out, n, h, w, oh, ow, windows, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v, fmt, stream);
    c.d_mask = d_mask; c.shrink = shrink; c.max_wh = max_wh; c.max_ww = max_ww;
    if (resizing) return st.hed == 1 ? recipe_launch_resize<1>(c) : recipe_launch_resize<2>(c);
    return st.hed == 1 ? recipe_launch_view<1>(c) : recipe_launch_view<2>(c);
}

extern "C" int sl_normalize_stages_view_affine(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                               int max_r, uint32_t fill_rgb, const double* M_src, const double* maxC_src, const double* M_tgt,
                                               const double* maxC_tgt, const double* alpha_beta, int augment_background,
                                               const SlParams* params, const SlTensorFormat* fmt, const SlViewStages* stages, void* stream) {
    const int nn = n == 0 ? 1 : n;
    RecipeCall c{};
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, nn, h, w,
                                         [&] {
                                             if (fill_rgb >= (1u << 24)) return (int)SL_ERR_BADARG;
                                             return affine_geometry(nn, h, w, oh, ow, windows, max_r, c.npatch);
                                         },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    Stages st;
    if (const int rc = stages_of(stages, c, st)) return rc;
    if (n == 0) return SL_OK;
    route_into(c, rgb, out, n, h, w, oh, ow, windows, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v, fmt, stream);
    c.max_r = max_r; c.fill = fill_rgb;
    return with_stages(st, [&](auto hed, auto post) { return recipe_launch_affine<decltype(hed)::value, decltype(post)::value>(c); });
}

extern "C" int sl_normalize_stages_view_elastic(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows,
                                                int max_r, const int32_t* field, int cell_log2, int max_d, uint32_t fill_rgb,
                                                const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                const double* alpha_beta, int augment_background, const SlParams* params,
                                                const SlTensorFormat* fmt, const SlViewStages* stages, void* stream) {
    const int nn = n == 0 ? 1 : n;
    RecipeCall c{};
    RouteView v;
    if (const int rc = route_view_checks(rgb, out, nn, h, w,
                                         [&] {
                                             if (fill_rgb >= (1u << 24)) return (int)SL_ERR_BADARG;
                                             return elastic_geometry(nn, h, w, oh, ow, windows, max_r, field, cell_log2, max_d, c.npatch);
                                         },
                                         M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, augment_background, params, fmt, v))
        return rc;
    Stages st;
    if (const int rc = stages_of(stages, c, st)) return rc;
    if (n == 0) return SL_OK;
    route_into(c, rgb, out, n, h, w, oh, ow, windows, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, v, fmt, stream);
    c.max_r = max_r; c.field = field; c.cell_log2 = cell_log2; c.max_d = max_d; c.fill = fill_rgb;
    return with_stages(st, [&](auto hed, auto post) { return recipe_launch_elastic<decltype(hed)::value, decltype(post)::value>(c); });
}
