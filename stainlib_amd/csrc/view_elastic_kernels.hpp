// view_elastic_kernels.hpp -- elastic deformation of a training loader inside the view pass: the affine view's map from the output to the
// source plus a smooth per-pixel displacement, a quadratic B-spline of a coarse control lattice, all in integers.
//
//   k_view_elastic   k_view_affine (view_affine_kernels.hpp) with a source block grown by the call's displacement bound, the patch's
//                    lattice nodes staged beside it, and elastic_at in place of affine_at on the write side
//
// Definition (include/stainlib_hip.h, sl_normalize_view_elastic; view_elastic_geometry.hpp): (Y, X) of output pixel (i, j) is the affine
// view's plus (d[0] << 8, d[1] << 8), d the spline of field[t] at (i, j) in 1/256 source pixel; from (Y, X) on everything is the affine
// view's: affine_taps, the four taps with the fill outside the tile, affine_blend.
//
// What is shared with k_view_affine: everything but the geometry -- view_read / view_stage / view_route on the block, ONE
// barrier, the slots, selects and blend of the write side, view_store_px4.  What is new: ElasticTile's patch edge min(64, 1 + (62 - 2
// max_d) Q / R), elastic_patch's block -- the box of the four affine corners grown by max_d pixels, cut to the tile -- and the field.
//
// The field: a patch of at most 64 outputs a side touches at most 7 x 7 lattice nodes (cells are at least 16 outputs).  They are STAGED
// IN LDS behind the stage's barrier -- 98 dwords, one global load per lane of the first two waves, clamped to +-256 max_d once per node
// -- and not read through the scalar / vector cache per output: the 3 x 3 nodes of an output are chosen per lane (a lane's row and column
// decide them), so a scalar load cannot serve them, and 18 cached global loads per output pixel would put some 280 vector-memory
// instructions per lane and patch into a write side that has none.  From LDS they are 9 ds_read_b64 per output pixel (dy and dx of a node
// are adjacent dwords), addresses uniform over the 16 .. 64 outputs of a cell row, i.e. broadcasts with at most a few distinct
// addresses per wave and no bank conflict worth counting.  A lane's four adjacent outputs share the row weights and the node row.
#pragma once
#include "view_affine_kernels.hpp"
#include "view_elastic_geometry.hpp"

namespace sl {

// the patch's lattice nodes into LDS, clamped (before the block's barrier; kElasticLds <= kWG: one slot per lane)
__device__ __forceinline__ void elastic_stage(const ElasticTile& t, const ElasticNodes& e, const int32_t* __restrict__ field, int tile,
                                              int oh, int ow, int32_t* s_nodes, int tid) {
    static_assert(kElasticLds <= kWG, "one slot per lane");
    const int gh = elastic_grid_side(oh, t.k), gw = elastic_grid_side(ow, t.k);
    int v;
    if (tid < kElasticLds && elastic_stage_node(field + (size_t)tile * ((size_t)gh * gw * 2), gw, e, t.lim, tid, v)) s_nodes[tid] = v;
}

// ---- write side: affine_write with elastic_at in place of affine_at; the spline's row weights once per output row of a lane
// ---- (Post: affine_write's)
template <int DT, int LAYOUT, class Post = ViewNoPost>
__device__ __forceinline__ void elastic_write(const ElasticTile& t, const ViewPatch& g, const ElasticNodes& e, bool none, const uint32_t* s_px,
                                              const int32_t* s_nodes, void* out, int tile, int h, int w, int oh, int ow, uint32_t fill,
                                              TensorK fmt, int tid, const Post& post = Post()) {
    const int i0 = g.i0, j0 = g.j0, bh = g.bh, bw = g.bw;
    const TensorK F = tensor_consts(fmt);
    const size_t PO = (size_t)oh * ow;
    const PatchLanes ln = patch_lanes(bw, tid, kWG);         // 1 .. 16 lanes per row, 256 .. 16 rows per pass
    const int jl = ln.jl;
    if (jl >= bw) return;                                    // (nothing below has a barrier)
    for (int il = ln.il0; il < bh; il += ln.rows) {
        uint32_t px[4];
        const ElasticW wy = elastic_weights(i0 + il, t.k);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (none) { px[p] = fill; continue; }            // (block-uniform)
            const AffineTaps a = affine_taps(elastic_at(t, e, s_nodes, wy, i0 + il, j0 + min(jl + p, bw - 1), oh, ow));
            const int r0 = affine_lds_row(g, a.ky), r1 = affine_lds_row(g, a.ky + 1);
            const int c0 = affine_lds_col(g, a.kx), c1 = affine_lds_col(g, a.kx + 1);
            const bool y0in = affine_inside(a.ky, h), y1in = affine_inside(a.ky + 1, h);
            const bool x0in = affine_inside(a.kx, w), x1in = affine_inside(a.kx + 1, w);
            const uint32_t p00 = y0in && x0in ? s_px[r0 + c0] : fill, p01 = y0in && x1in ? s_px[r0 + c1] : fill;
            const uint32_t p10 = y1in && x0in ? s_px[r1 + c0] : fill, p11 = y1in && x1in ? s_px[r1 + c1] : fill;
            px[p] = affine_blend(p00, p01, p10, p11, a.fy, a.fx);
        }
        if constexpr (Post::kOn) post.apply(px, g, il, jl, ow);
        const int nvalid = min(4, bw - jl);
        const size_t pix = (size_t)(i0 + il) * ow + (j0 + jl);
        view_store_px4<DT, LAYOUT>(px, out, tile, PO, pix, nvalid, F);
    }
}

// affine_body with the geometry and the write side above (HED, Post: as there).  npatch: the host's upper bound of the patches of a tile.
// The recipes (recipe_kernels.hpp) instantiate it; k_view_elastic below holds the same text written out with no stage, its TWIN, for
// affine_body's reason.
template <int DT, int LAYOUT, int MODE, int HED = 0, class Post = ViewNoPost>
__device__ __forceinline__ void elastic_body(const uint8_t* rgb, void* out, int h, int w, int oh, int ow, int npatch, const int32_t* windows,
                                             int max_r, const int32_t* field, int cell_log2, int max_d, uint32_t fill, const double* M_src,
                                             const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
                                             double lam, float ylimf, TensorK fmt, const typename StageArgs<HED>::type* hv = nullptr,
                                             const Post& post = Post()) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    __shared__ __attribute__((aligned(8))) int32_t s_nodes[kElasticLds];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block and the nodes of this patch -- or no patch: the grid is sized for the
    // call's bounds --, or no block: the fill alone
    const ElasticTile vt(windows, tile, h, w, max_r, cell_log2, max_d);
    ViewPatch g;
    ElasticNodes e;
    bool none;
    if (!elastic_patch(vt, patch, h, w, oh, ow, g, e, none)) return;
    if (none) {
        if constexpr (Post::kOn) __syncthreads();                // the post stage's table
        elastic_write<DT, LAYOUT>(vt, g, e, true, s_px, s_nodes, out, tile, h, w, oh, ow, fill, fmt, tid, post);
        return;
    }
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    HedStage<HED> hed;
    hed.init(tid, tile, hv);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    elastic_stage(vt, e, field, tile, oh, ow, s_nodes, tid);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) {
            compute(c, px);
            hed.apply(px);
        });
    };
    view_route<MODE, HED>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();

    elastic_write<DT, LAYOUT>(vt, g, e, false, s_px, s_nodes, out, tile, h, w, oh, ow, fill, fmt, tid, post);
}

// elastic_body<DT, LAYOUT, MODE, 0, ViewNoPost> written out (see there)
template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_view_elastic(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                             int ow, int npatch, const int32_t* __restrict__ windows, int max_r,
                                                             const int32_t* __restrict__ field, int cell_log2, int max_d, uint32_t fill,
                                                             const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                             const double* M_tgt, const double* maxC_tgt,
                                                             const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    __shared__ __attribute__((aligned(8))) int32_t s_nodes[kElasticLds];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block and the nodes of this patch -- or no patch: the grid is sized for the
    // call's bounds --, or no block: the fill alone
    const ElasticTile vt(windows, tile, h, w, max_r, cell_log2, max_d);
    ViewPatch g;
    ElasticNodes e;
    bool none;
    if (!elastic_patch(vt, patch, h, w, oh, ow, g, e, none)) return;
    if (none) {
        elastic_write<DT, LAYOUT>(vt, g, e, true, s_px, s_nodes, out, tile, h, w, oh, ow, fill, fmt, tid);
        return;
    }
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    elastic_stage(vt, e, field, tile, oh, ow, s_nodes, tid);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) { compute(c, px); });
    };
    view_route<MODE, 0>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();

    elastic_write<DT, LAYOUT>(vt, g, e, false, s_px, s_nodes, out, tile, h, w, oh, ow, fill, fmt, tid);
}

}  // namespace sl
