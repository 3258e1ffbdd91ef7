// recipe_launch.hpp -- the launchers of the recipe's kernel families (recipe_kernels.hpp), defined here and explicitly instantiated by the
// recipe_*.hip translation units; recipe.hip sees their declarations only (recipe_host.hpp).
#pragma once
#include "recipe_kernels.hpp"
#include "recipe_host.hpp"
#include "route_host.hpp"

namespace sl {

// SL_VIEW_FAMILY with the recipe's further template arguments
#define SL_RECIPE_FAMILY(k, ...) \
    [](auto dt, auto lay, auto m) { return k<decltype(dt)::value, decltype(lay)::value, decltype(m)::value, __VA_ARGS__>; }

template <int HED, bool POST>
int recipe_launch_affine(const RecipeCall& c) {
    return launch_route_view(SL_RECIPE_FAMILY(k_recipe_affine, HED, POST), c.fmt, c.mode, c.n * c.npatch, c.stream, c.rgb, c.out, c.h, c.w, c.oh,
                             c.ow, (int)c.npatch, c.windows, c.max_r, c.fill, c.M_src, c.maxC_src, c.M_tgt, c.maxC_tgt, c.alpha_beta, c.lam,
                             c.ylimf, c.fmt ? tensor_k(*c.fmt) : TensorK{}, recipe_stage_args<HED>(c), c.post);
}

template <int HED, bool POST>
int recipe_launch_elastic(const RecipeCall& c) {
    return launch_route_view(SL_RECIPE_FAMILY(k_recipe_elastic, HED, POST), c.fmt, c.mode, c.n * c.npatch, c.stream, c.rgb, c.out, c.h, c.w, c.oh,
                             c.ow, (int)c.npatch, c.windows, c.max_r, c.field, c.cell_log2, c.max_d, c.fill, c.M_src, c.maxC_src, c.M_tgt,
                             c.maxC_tgt, c.alpha_beta, c.lam, c.ylimf, c.fmt ? tensor_k(*c.fmt) : TensorK{}, recipe_stage_args<HED>(c), c.post);
}

template <int HED>
int recipe_launch_view(const RecipeCall& c) {
    return launch_route_view(SL_RECIPE_FAMILY(k_recipe_view, HED), c.fmt, c.mode, c.n * c.npatch, c.stream, c.rgb, c.out, c.h, c.w, c.oh, c.ow,
                             (int)c.npx, (int)c.npatch, c.windows, c.d_mask, c.shrink, c.M_src, c.maxC_src, c.M_tgt, c.maxC_tgt, c.alpha_beta,
                             c.lam, c.ylimf, c.fmt ? tensor_k(*c.fmt) : TensorK{}, recipe_stage_args<HED>(c), c.post);
}

template <int HED>
int recipe_launch_resize(const RecipeCall& c) {
    return launch_route_view(SL_RECIPE_FAMILY(k_recipe_resize, HED), c.fmt, c.mode, c.n * c.npatch, c.stream, c.rgb, c.out, c.h, c.w, c.oh, c.ow,
                             (int)c.npatch, c.windows, c.d_mask, c.max_wh, c.max_ww, c.M_src, c.maxC_src, c.M_tgt, c.maxC_tgt, c.alpha_beta,
                             c.lam, c.ylimf, c.fmt ? tensor_k(*c.fmt) : TensorK{}, recipe_stage_args<HED>(c), c.post);
}

}  // namespace sl
