// recipe_host.hpp -- what recipe.hip (the C entry points of the one-pass recipe: checks, forwarding, dispatch) shares with the translation
// units that hold the kernel families (recipe_*.hip): one checked call as a plain struct, and the launchers as function templates that
// are DECLARED here, DEFINED in recipe_launch.hpp and explicitly instantiated one or two per translation unit, so that make -j spreads the
// ~390 kernels over a dozen compiler processes (post.hip's header comment: a stage instantiates a whole family wherever it is named).
#pragma once
#include "hsb_kernels.hpp"           // HsbViewArgs; view_kernels.hpp (HedViewArgs) through it
#include "post_kernels.hpp"          // PostViewArgs
#include "tensor_host.hpp"

namespace sl {

struct RecipeCall {
    const uint8_t* rgb;
    void* out;
    int n, h, w, oh, ow;
    const int32_t* windows;
    long npx, npatch;                // the geometry check's
    int d_mask, shrink, max_wh, max_ww;                        // the fixed-size / resizing views
    int max_r;                                                 // the affine and elastic views
    const int32_t* field;
    int cell_log2, max_d;
    uint32_t fill;
    const double *M_src, *maxC_src, *M_tgt, *maxC_tgt, *alpha_beta;
    int mode;                        // kView*
    double lam;
    float ylimf;
    const SlTensorFormat* fmt;
    HedViewArgs hed;                 // HED == 1
    HsbViewArgs hsb;                 // HED == 2
    PostViewArgs post;               // POST
    void* stream;
};

// the colour stage's arguments of a call, by the stage
template <int HED> inline const typename StageArgs<HED>::type& recipe_stage_args(const RecipeCall& c) { return c.hed; }
template <> inline const HsbViewArgs& recipe_stage_args<2>(const RecipeCall& c) { return c.hsb; }

// launch_status() of the one launch each makes
template <int HED, bool POST> int recipe_launch_affine(const RecipeCall& c);
template <int HED, bool POST> int recipe_launch_elastic(const RecipeCall& c);
template <int HED> int recipe_launch_view(const RecipeCall& c);       // fixed-size / box shrink, colour and post
template <int HED> int recipe_launch_resize(const RecipeCall& c);     // resizing, colour and post

}  // namespace sl
