// view_affine_kernels.hpp -- rotation by any angle, zoom, shear and translation of a training loader inside the view pass: per tile an
// affine map from the output to the source, sampled bilinearly with 8-bit weights in integers.
//
//   k_view_affine   k_view_resize (view_resize_kernels.hpp) with a six-column window, a source block that is the bounding box of a
//                   rotated patch, and the bilinear write side
//
// Definition (include/stainlib_hip.h, sl_normalize_view_affine): windows[t] = (cy, cx, a00, a01, a10, a11) in 2^-16 source pixels; output
// pixel (i, j) is sampled at Y = cy + ((a00 u + a01 v) >> 1), X = cx + ((a10 u + a11 v) >> 1), u = 2 i + 1 - oh, v = 2 j + 1 - ow; with
// ty = Y - Q/2: ky = ty >> 16, fy = (ty >> 8) & 255 (x likewise), the four taps p00 .. p11 of `full` at (ky, kx) .. (ky + 1, kx + 1) -- a
// tap outside the tile is the call's fill byte -- and per channel
//     b = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16.
//
// What is shared with k_view / k_view_resize: load12 / view_read (the read side), view_stage / view_unpack (the LDS stage, one packed dword
// per SOURCE pixel, pitch 65), the apply / jitter arithmetic per source pixel (view_route, view_kernels.hpp: the one copy this kernel
// and view_resize_body run), the store tail from four packed pixels on (view_store_px4) and the lanes of a patch (patch_lanes,
// view_geometry.hpp).  What is new: the geometry (view_affine_geometry.hpp: AffineTile, affine_patch, affine_at, affine_taps,
// affine_blend) and the sampling of the write side (affine_write).
//
// Shape: ONE workgroup = one tile and one patch of b x b OUTPUT pixels, b = affine_patch_edge(max(Ry, Rx)) = min(64, 1 + 62 Q / R) per
// tile and block-uniform, so that the taps of the patch fit the 64 x 64 LDS block along both axes.  The source block is the bounding
// box of the patch's taps INTERSECTED with the tile (its extremes are at the patch's corners); it is read along source rows, computed
// per source pixel and staged once.  At 45 degrees the box is twice the area the patch's outputs cover: those pixels are computed and
// not used (DESIGN 4.21 for what that costs).  The windows may live on the device, so the grid is sized on the host from the call's
// bound max_r of the row sums (affine_grid_patches); a workgroup past its tile's own patch count returns before it loads a pixel, a
// patch whose box misses the tile -- and every patch of a tile whose row sums pass max_r -- reads nothing and writes the fill.
//   write side  output rows, 4 adjacent output pixels per lane; 16, 8, 4, 2 or 1 lanes per row -- the power of two that covers the
//               patch's width -- and 256 / that many rows per pass (patch_lanes, as in resize_write).  Per output pixel Y, X from the block's
//               scalars (two v_mad each), the four LDS slots (clamped into the block; inside a tile a tap IS in the block), four selects
//               against the fill decided from the ABSOLUTE coordinates (unsigned compares with h, w), the blend (affine_blend: r and b as
//               two 16-bit lanes of one dword in the row step), then view_store_px4.
// LDS banking of the tap reads (pitch 65: bank (r + x) % 32 within each 32-lane half; the two taps of a row are adjacent dwords): lanes of
// one output row are 4 outputs apart, i.e. 4 a01 / Q rows and 4 a11 / Q columns of LDS, so their bank stride is 4 (a01 + a11) / Q; the
// next output row is (a00 + a10) / Q banks on.
//   0 degrees    a01 = 0, a11 = Q: stride 4, rows 1 apart -- k_view's row-wise picture: lanes c and c + 8 share a bank, 2-way.
//   90 degrees   a01 = -+Q, a11 = 0: stride 4 pitches = 4 banks, rows 1 apart -- k_view's column-wise picture: 2-way.
//   45 degrees   A = [[c, -s], [s, c]] (the drawn orientation, e = 1): a01 + a11 = 0 -- the lanes of an output row walk an anti-diagonal
//                of LDS, which an odd pitch maps to ONE bank (two, with the floors): up to 16-way within a row, the half's second row
//                1.41 banks on.  The mirrored matrix (e = -1) and -45 degrees have stride 5.7: the floors spread the 16 lanes over
//                ~all banks, at most 2-way.  Any pitch has such an angle (pitch p: a01 p + a11 = 0 mod 32); 65 keeps the worst case
//                away from the axis-aligned views.  The pass issues ~45 VALU instructions per output pixel around its 4 reads and
//                ~60 per source pixel in front of LDS, twice as many source pixels as outputs at that angle: the conflict costs
//                what tools/view_affine_time.py measures at 45 degrees, and is left as it is.
// Lanes: a patch of b x b outputs has b ceil(b / 4) lane-passes of work: four passes of 252 lanes at 0 degrees (b = 63), two of 242 and
// one of 132 at 45 degrees (b = 44, 11 chunks -> 16 lanes per row, 11 busy), one pass of 256 at the limit (b = 32).
#pragma once
#include "view_resize_kernels.hpp"   // view_kernels.hpp through it: view_read, view_stage, store_view4, the modes
#include "view_affine_geometry.hpp"

namespace sl {

// ---- write side: output rows, 4 adjacent pixels per lane (behind a barrier after the stage, or with none: nothing staged).  fill: the
// ---- packed fill pixel r | g << 8 | b << 16.
// ---- Post: the stage on the written pixels (ViewNoPost: none), fill pixels included; its table is in LDS behind a barrier.
template <int DT, int LAYOUT, class Post = ViewNoPost>
__device__ __forceinline__ void affine_write(const AffineTile& t, const ViewPatch& g, bool none, const uint32_t* s_px, void* out, int tile,
                                             int h, int w, int oh, int ow, uint32_t fill, TensorK fmt, int tid, const Post& post = Post()) {
    const int i0 = g.i0, j0 = g.j0, bh = g.bh, bw = g.bw;
    const TensorK F = tensor_consts(fmt);
    const size_t PO = (size_t)oh * ow;
    const PatchLanes ln = patch_lanes(bw, tid, kWG);         // 1 .. 16 lanes per row, 256 .. 16 rows per pass
    const int jl = ln.jl;
    if (jl >= bw) return;                                    // (nothing below has a barrier)
    for (int il = ln.il0; il < bh; il += ln.rows) {
        uint32_t px[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (none) { px[p] = fill; continue; }            // (block-uniform)
            const AffineTaps a = affine_taps(affine_at(t, i0 + il, j0 + min(jl + p, bw - 1), oh, ow));
            const int r0 = affine_lds_row(g, a.ky), r1 = affine_lds_row(g, a.ky + 1);
            const int c0 = affine_lds_col(g, a.kx), c1 = affine_lds_col(g, a.kx + 1);
            const bool y0in = affine_inside(a.ky, h), y1in = affine_inside(a.ky + 1, h);
            const bool x0in = affine_inside(a.kx, w), x1in = affine_inside(a.kx + 1, w);
            const uint32_t p00 = y0in && x0in ? s_px[r0 + c0] : fill, p01 = y0in && x1in ? s_px[r0 + c1] : fill;
            const uint32_t p10 = y1in && x0in ? s_px[r1 + c0] : fill, p11 = y1in && x1in ? s_px[r1 + c1] : fill;
            px[p] = affine_blend(p00, p01, p10, p11, a.fy, a.fx);
        }
        if constexpr (Post::kOn) post.apply(px, g, il, jl, ow);  // (post_lane: the duplicates of a ragged last lane stay as they are)
        const int nvalid = min(4, bw - jl);
        const size_t pix = (size_t)(i0 + il) * ow + (j0 + jl);
        view_store_px4<DT, LAYOUT>(px, out, tile, PO, pix, nvalid, F);
    }
}

// view_resize_body with the geometry and the write side above; the arithmetic between view_read and the barrier is view_route
// (view_kernels.hpp).  npatch: the host's upper bound of the patches of a tile.  HED: the stage on SOURCE pixels (0: none) -- the fill is
// in output space and does not take it --; Post: the stage on written pixels, the fill included (ViewNoPost: none).  A PostStage has
// filled its table before the call; the barrier in front of the write side stands between that fill and its first use, and the `none`
// path, which has no barrier of its own, gets one (block-uniform).  The recipes (recipe_kernels.hpp) instantiate it with stages.
// k_view_affine below holds the same text written out with no stage -- its TWIN: a change to one is a change to the other.  Calling the
// body from it leaves registers, LDS and occupancy alone but re-orders the code of 28 of its 34 instantiations (tools/isa_diff.py; +-
// some tens of bytes each), and the existing kernels stay function for function what they were (as 4.19.1 for view_body).
template <int DT, int LAYOUT, int MODE, int HED = 0, class Post = ViewNoPost>
__device__ __forceinline__ void affine_body(const uint8_t* rgb, void* out, int h, int w, int oh, int ow, int npatch, const int32_t* windows,
                                            int max_r, uint32_t fill, const double* M_src, const double* maxC_src, const double* M_tgt,
                                            const double* maxC_tgt, const double* alpha_beta, double lam, float ylimf, TensorK fmt,
                                            const typename StageArgs<HED>::type* hv = nullptr, const Post& post = Post()) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block of this patch -- or no patch: the grid is sized for the call's bound --,
    // or no block: the fill alone
    const AffineTile vt(windows, tile, h, w, max_r);
    ViewPatch g;
    bool none;
    if (!affine_patch(vt, patch, h, w, oh, ow, g, none)) return;
    if (none) {
        if constexpr (Post::kOn) __syncthreads();                // the post stage's table
        affine_write<DT, LAYOUT>(vt, g, true, s_px, out, tile, h, w, oh, ow, fill, fmt, tid, post);
        return;
    }
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    HedStage<HED> hed;
    hed.init(tid, tile, hv);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) {
            compute(c, px);
            hed.apply(px);
        });
    };
    view_route<MODE, HED>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();

    affine_write<DT, LAYOUT>(vt, g, false, s_px, out, tile, h, w, oh, ow, fill, fmt, tid, post);
}

// affine_body<DT, LAYOUT, MODE, 0, ViewNoPost> written out (see there)
template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_view_affine(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                            int ow, int npatch, const int32_t* __restrict__ windows, int max_r,
                                                            uint32_t fill, const double* __restrict__ M_src,
                                                            const double* __restrict__ maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                            const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block of this patch -- or no patch: the grid is sized for the call's bound --,
    // or no block: the fill alone
    const AffineTile vt(windows, tile, h, w, max_r);
    ViewPatch g;
    bool none;
    if (!affine_patch(vt, patch, h, w, oh, ow, g, none)) return;
    if (none) {
        affine_write<DT, LAYOUT>(vt, g, true, s_px, out, tile, h, w, oh, ow, fill, fmt, tid);
        return;
    }
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) { compute(c, px); });
    };
    view_route<MODE, 0>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();

    affine_write<DT, LAYOUT>(vt, g, false, s_px, out, tile, h, w, oh, ow, fill, fmt, tid);
}

}  // namespace sl
