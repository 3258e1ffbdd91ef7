// recipe_kernels.hpp -- the one-pass augmentation recipe: at most one colour stage on SOURCE pixels (HED or HSB), one view, and the post
// stage on WRITTEN pixels (tone table, then noise), composed from the hooks the view kernels already carry:
//
//     out[t] = convert( post( view( colour(full[t]) ) ) )
//
//   k_recipe_affine    affine_body (view_affine_kernels.hpp) with HedStage<HED> behind the route arithmetic and Post on the write side
//   k_recipe_elastic   elastic_body (view_elastic_kernels.hpp) likewise
//   k_recipe_view      view_body (view_kernels.hpp) with a colour stage AND the post stage: the fixed-size views and the box shrink
//   k_recipe_resize    view_resize_body (view_resize_kernels.hpp) with both
//
// HED: 1 the HED augmentation (HedStage<1>, hed_view_kernels.hpp), 2 the HSB map (HedStage<2>, hsb_kernels.hpp), 0 none.  POST: the post
// stage (PostStage, post_kernels.hpp) or none.  Nothing here is new arithmetic: each stage is the statement-for-statement stage of its
// own entry point, so a recipe is bit for bit the chain of those calls.  The fill of an affine / elastic view is in output space: it does
// not pass the colour stage and does pass the post stage, and so does a patch that misses its tile or a tile past max_r.
// Families an existing entry point has (a colour stage alone or the post stage alone on a fixed-size / resizing view) are NOT
// instantiated here: sl_normalize_stages_view forwards those calls.
// LDS per workgroup: the view's own (2 KB table, 16.25 KB block, the elastic nodes) + 1 KB (HED's ln table) + 256 B (the tone table).
#pragma once
#include <type_traits>
#include "hed_view_kernels.hpp"      // HedStage<1>
#include "hsb_kernels.hpp"           // HedStage<2>
#include "post_kernels.hpp"          // PostStage
#include "view_elastic_kernels.hpp"  // view_affine_kernels.hpp through it

namespace sl {

// the write-side stage of a kernel and its set-up: PostStage fills its table here, in front of the body's barriers
template <bool POST>
struct RecipePost {
    typedef PostStage type;
    static __device__ __forceinline__ void init(PostStage& post, int tile, const PostViewArgs& pv, uint8_t* s_tone) {
        post.init(threadIdx.x, tile, pv, s_tone);
    }
};
template <>
struct RecipePost<false> {
    typedef ViewNoPost type;
    static __device__ __forceinline__ void init(ViewNoPost&, int, const PostViewArgs&, uint8_t*) {}
};

template <int DT, int LAYOUT, int MODE, int HED, bool POST>
static __global__ __launch_bounds__(kWG) void k_recipe_affine(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                              int ow, int npatch, const int32_t* __restrict__ windows, int max_r,
                                                              uint32_t fill, const double* __restrict__ M_src,
                                                              const double* __restrict__ maxC_src, const double* M_tgt,
                                                              const double* maxC_tgt, const double* __restrict__ alpha_beta, double lam,
                                                              float ylimf, TensorK fmt, typename StageArgs<HED>::type hv, PostViewArgs pv) {
    __shared__ uint8_t s_tone[POST ? 256 : 1];
    typename RecipePost<POST>::type post;
    RecipePost<POST>::init(post, blockIdx.x / npatch, pv, s_tone);
    affine_body<DT, LAYOUT, MODE, HED>(rgb, out, h, w, oh, ow, npatch, windows, max_r, fill, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam,
                                       ylimf, fmt, &hv, post);
}

template <int DT, int LAYOUT, int MODE, int HED, bool POST>
static __global__ __launch_bounds__(kWG) void k_recipe_elastic(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                               int ow, int npatch, const int32_t* __restrict__ windows, int max_r,
                                                               const int32_t* __restrict__ field, int cell_log2, int max_d, uint32_t fill,
                                                               const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                               const double* M_tgt, const double* maxC_tgt,
                                                               const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt,
                                                               typename StageArgs<HED>::type hv, PostViewArgs pv) {
    __shared__ uint8_t s_tone[POST ? 256 : 1];
    typename RecipePost<POST>::type post;
    RecipePost<POST>::init(post, blockIdx.x / npatch, pv, s_tone);
    elastic_body<DT, LAYOUT, MODE, HED>(rgb, out, h, w, oh, ow, npatch, windows, max_r, field, cell_log2, max_d, fill, M_src, maxC_src, M_tgt,
                                        maxC_tgt, alpha_beta, lam, ylimf, fmt, &hv, post);
}

// (k_post_view with a colour stage; HED = 1, 2)
template <int DT, int LAYOUT, int MODE, int HED>
static __global__ __launch_bounds__(kWG) void k_recipe_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                            int ow, int npx, int npatch, const int32_t* __restrict__ windows, int d_mask,
                                                            int shrink, const double* __restrict__ M_src,
                                                            const double* __restrict__ maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                            const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt,
                                                            typename StageArgs<HED>::type hv, PostViewArgs pv) {
    __shared__ uint8_t s_tone[256];
    PostStage post;
    post.init(threadIdx.x, blockIdx.x / npatch, pv, s_tone);
    view_body<DT, LAYOUT, MODE, HED>(rgb, out, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta,
                                     lam, ylimf, fmt, &hv, post);
}

// (k_post_view_resize with a colour stage; HED = 1, 2)
template <int DT, int LAYOUT, int MODE, int HED>
static __global__ __launch_bounds__(kWG) void k_recipe_resize(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                              int ow, int npatch, const int32_t* __restrict__ windows, int d_mask,
                                                              int max_wh, int max_ww, const double* __restrict__ M_src,
                                                              const double* __restrict__ maxC_src, const double* M_tgt,
                                                              const double* maxC_tgt, const double* __restrict__ alpha_beta, double lam,
                                                              float ylimf, TensorK fmt, typename StageArgs<HED>::type hv, PostViewArgs pv) {
    __shared__ uint8_t s_tone[256];
    PostStage post;
    post.init(threadIdx.x, blockIdx.x / npatch, pv, s_tone);
    view_resize_body<DT, LAYOUT, MODE, HED>(rgb, out, h, w, oh, ow, npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                            alpha_beta, lam, ylimf, fmt, &hv, post);
}

}  // namespace sl
