// view_resize_kernels.hpp -- the random-resized crop of a training loader inside the view pass: per tile a window of ANY size, resampled
// to the call's one output size by exact pixel-area averaging, then flipped and turned.
//
//   k_view_resize      k_view (view_kernels.hpp) with a per-tile window side and the area-resampling write side
//   k_hed_view_resize  the same with the HED stage (HedStage<1>, hed_view_kernels.hpp) in front of LDS
//
// Definition (include/stainlib_hip.h, sl_normalize_view_resize): windows[t] = (y0, x0, d, wh, ww); with (nu, nv) = (oh, ow) for an even
// number of quarter turns and (ow, oh) for an odd one, along an axis of nw window pixels and no outputs the coordinates are scaled by no:
// source pixel k covers [k no, (k + 1) no), output i covers [i nw, (i + 1) nw), c(i, k) = the length of their overlap (an integer; a row
// of c sums to nw, a column to no).  Per channel S[i, j] = sum_k sum_l cy(i, k) cx(j, l) window[k, l], b = (2 S + D) / (2 D) with
// D = wh ww (round half up), result = rot90(flip(b) if d & 4 else b, d & 3).  The resample commutes with the flip and the turn, so the
// kernel resamples in OUTPUT orientation: each output axis is one window axis, forwards or backwards.
//
// What is shared with k_view: load12 / view_read (the read side), view_stage / view_unpack (the LDS stage, one packed dword per SOURCE
// pixel, pitch 65), the apply / jitter / HED arithmetic per source pixel (view_route: the one copy this body and k_view_affine run;
// view_body holds its twin), cvt_chunk and store_view4.  What is new: the geometry (ResizeTile, resize_patch) and the write side
// (resize_write).  Its lanes-per-row assignment is patch_lanes' (view_geometry.hpp) and its store tail view_store_px4's, both WRITTEN
// OUT here: on the shared functions the uint8 views of 224^2 windows measured 0.2 - 0.4 % slower than the parent.
//
// Shape: ONE workgroup = one tile and one patch of at most 64 x 64 OUTPUT pixels whose source pixels fit the 64 x 64 LDS block.  Along an
// axis the patch edge is resize_patch_edge(no, nw) = min(64, 63 no / nw) outputs: b outputs starting anywhere touch at most
// ceil(b nw / no) + 1 <= 64 source pixels.  The edge is per tile and block-uniform.  The windows may live on the device, so the grid is
// sized on the host from the upper bound (max_wh, max_ww) of the window sides (view_resize_geometry, route_host.hpp): the edge does not
// grow with nw, so a tile has at most the bound's patches, and a workgroup past its tile's own count returns before it loads a pixel.
//   taps        threads 0..127 divide once each: for the patch's <= 64 output rows and <= 64 output columns the first source pixel an
//               output overlaps (relative to the LDS block) and how many (1..17), packed into s_tap.  No lane divides by nu or nv again.
//   write side  output rows, 4 adjacent output pixels per lane; 16, 8, 4, 2 or 1 lanes per row -- the power of two that covers the patch's
//               width -- and 256 / that many rows per pass (16 and 16 as at S = 1 for a patch wider than 32).  Per output pixel two
//               nested loops over its taps; the weights come from the tap's scaled coordinate (min - max of four edges, no table), the
//               three channel sums are 32-bit (S <= 255 D < 2^30 for D <= 2^22; weight products < 2^24: v_mad_u32_u24).
//   division    by 2 D, block-uniform: q0 = trunc(float(2 S + D) * (1 / float(2 D))) is within one of the quotient (2 D <= 2^23 is exact
//               in binary32, three roundings of 2^-24 relative on a value below 256), and one remainder test each way makes it exact for
//               every residue.
// LDS banking of the tap reads (pitch 65: bank (r + x) % 32): at step (ta, tb) of pixel p a lane reads row k0(i) + ta, column
// l0(j) + tb, so lanes of one output row are ~4 ww / nv columns apart and rows ~wh / nu apart -- the picture of the shrink's strided
// reads at that ratio under the same lanes per row: 2-way at ratios 1 and 2, 4-way at ratio 4 (lane strides of 16 and 4 banks), in between the
// strides are not constant and the lanes spread further.  The loop issues ~12 VALU instructions per LDS read, so the read is not what it waits for.
// Lanes: a patch of b x b outputs has b ceil(b / 4) lane-passes of work -- four passes of all lanes at ratio <= 1, one pass of 248 lanes at
// ratio 2 (b = 31), 60 lanes of one pass at ratio 4 (b = 15); the per-source-pixel arithmetic in front of LDS stays on all 256 lanes
// (DESIGN 4.17 for what that costs).
#pragma once
#include "view_kernels.hpp"

namespace sl {

// (the geometry -- the limits, resize_patch_edge, resize_side_max, ResizeTile, ResizeAxis, resize_patch -- is in view_geometry.hpp)

// ---- taps: for output t of each patch axis the first LDS pixel it overlaps | the number it overlaps << 8 (threads 0 .. 2 kViewB - 1)
__device__ __forceinline__ void resize_taps(const ResizeAxis& ai, const ResizeAxis& aj, uint32_t* s_tap, int tid) {
    if (tid >= 2 * kViewB) return;
    const ResizeAxis& a = tid < kViewB ? ai : aj;
    const int t = tid & (kViewB - 1);
    if (t >= a.nb) return;
    const uint32_t o = (uint32_t)a.at(t), nw = (uint32_t)a.nw, no = (uint32_t)a.no;
    const uint32_t k0 = o * nw / no, k1 = ((o + 1u) * nw + no - 1u) / no;
    s_tap[tid] = (k0 - (uint32_t)a.lo) | ((k1 - k0) << 8);
}

// (2 S + D) / (2 D) for S <= 255 D, D <= 2^22: rden = 1 / float(2 D) (block-uniform)
__device__ __forceinline__ uint32_t resize_round(uint32_t S, uint32_t D, float rden) {
    const uint32_t num = 2u * S + D, den = 2u * D;
    uint32_t q = (uint32_t)((float)num * rden);
    const int r = (int)(num - q * den);
    q = r < 0 ? q - 1u : (r >= (int)den ? q + 1u : q);
    return q;
}

// ---- write side: output rows, 4 adjacent pixels per lane (behind a barrier after the stage and resize_taps).  Lanes per output row: the
// ---- power of two that covers the patch's width, 1 .. 16 (block-uniform), so that a narrow patch spreads its rows over all the lanes
// ---- (patch_lanes' assignment, view_geometry.hpp; from `Chunk o` on: view_store_px4's text.  TWINS, see the head of this file).
template <int DT, int LAYOUT, class Post = ViewNoPost>
__device__ __forceinline__ void resize_write(const ViewPatch& g, const ResizeAxis& ai, const ResizeAxis& aj, const uint32_t* s_px,
                                             const uint32_t* s_tap, void* out, int tile, int oh, int ow, TensorK fmt, int tid,
                                             const Post& post = Post()) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;
    typedef typename Elem<SDT>::type T;
    const int i0 = g.i0, j0 = g.j0, bh = g.bh, bw = g.bw;
    const TensorK F = tensor_consts(fmt);
    const size_t PO = (size_t)oh * ow;
    const uint32_t D = (uint32_t)ai.nw * (uint32_t)aj.nw;
    const float rden = 1.0f / (float)(2u * D);
    const int n4 = (bw + 3) >> 2;                            // chunks of 4 pixels per output row, 1 .. 16
    const int lg = n4 <= 1 ? 0 : 32 - __builtin_clz((unsigned)(n4 - 1));       // log2 of the lanes per row: 0 .. 4
    const int lr = tid >> lg, lc = tid & ((1 << lg) - 1), rows = kWG >> lg;     // rows per pass: 16 .. 256
    const int jl = 4 * lc;
    if (jl >= bw) return;                                    // (nothing below has a barrier)
    for (int il = lr; il < bh; il += rows) {
        // the row axis of this lane: its taps, the output's interval [elo, ehi) and the first tap's start, all scaled by no
        const uint32_t ta = s_tap[il];
        const int na = (int)(ta >> 8), ka = (int)(ta & 0xffu);
        const int elo_a = ai.at(il) * ai.nw, ehi_a = elo_a + ai.nw, c0_a = (ai.lo + ka) * ai.no;
        uint32_t px[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int jj = min(jl + p, bw - 1);
            const uint32_t tb = s_tap[kViewB + jj];
            const int nb = (int)(tb >> 8), kb = (int)(tb & 0xffu);
            const int elo_b = aj.at(jj) * aj.nw, ehi_b = elo_b + aj.nw, c0_b = (aj.lo + kb) * aj.no;
            uint32_t S0 = 0, S1 = 0, S2 = 0;
            int ca = c0_a, ra = ka * ai.stride;
            for (int a = 0; a < na; ++a, ca += ai.no, ra += ai.stride) {
                const uint32_t wa = (uint32_t)(min(ca + ai.no, ehi_a) - max(ca, elo_a));
                int cb = c0_b, rb = ra + kb * aj.stride;
                for (int b = 0; b < nb; ++b, cb += aj.no, rb += aj.stride) {
                    const uint32_t wb = (uint32_t)(min(cb + aj.no, ehi_b) - max(cb, elo_b));
                    const uint32_t wgt = __umul24(wa, wb);   // <= D <= 2^22
                    const uint32_t v = s_px[rb];
                    S0 += __umul24(wgt, v & 0xffu);
                    S1 += __umul24(wgt, (v >> 8) & 0xffu);
                    S2 += __umul24(wgt, v >> 16);
                }
            }
            px[p] = resize_round(S0, D, rden) | (resize_round(S1, D, rden) << 8) | (resize_round(S2, D, rden) << 16);
        }
        if constexpr (Post::kOn) post.apply(px, g, il, jl, ow);
        Chunk o;
        o.w0 = px[0] | (px[1] << 24);
        o.w1 = (px[1] >> 8) | (px[2] << 16);
        o.w2 = (px[2] >> 16) | (px[3] << 8);
        const int nvalid = min(4, bw - jl);
        const size_t pix = (size_t)(i0 + il) * ow + (j0 + jl);
        if (TENSOR) {
            float v[12];
            cvt_chunk(o, F, v);
            T* const base = (T*)out + (size_t)tile * 3 * PO;
            store_view4<SDT, LAYOUT>(base, PO, pix, nvalid, v);
        } else {
            uint8_t* const p = (uint8_t*)out + ((size_t)tile * PO + pix) * 3;
            if (nvalid == 4) {
                sl_u32x3u u; u.x = o.w0; u.y = o.w1; u.z = o.w2;
                *(SL_GLOBAL sl_u32x3u*)as_global(p) = u;
            } else {
                for (int i = 0; i < 3 * nvalid; ++i) as_global(p)[i] = (uint8_t)chunk_byte(o, i);
            }
        }
    }
}

// view_body with the geometry and the write side above; the arithmetic between view_read and the barrier is view_route
// (view_kernels.hpp).  npatch: the host's upper bound of the patches of a tile.
template <int DT, int LAYOUT, int MODE, int HED, class Post = ViewNoPost>
__device__ __forceinline__ void view_resize_body(const uint8_t* rgb, void* out, int h, int w, int oh, int ow, int npatch,
                                                 const int32_t* windows, int d_mask, int max_wh, int max_ww,
                                                 const double* M_src, const double* maxC_src,
                                                 const double* M_tgt, const double* maxC_tgt, const double* alpha_beta,
                                                 double lam, float ylimf, TensorK fmt, const typename StageArgs<HED>::type* hv,
                                                 const Post& post = Post()) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    __shared__ uint32_t s_tap[2 * B];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block of this patch -- or none: the grid is sized for the largest window
    const ResizeTile vt(windows, tile, d_mask, h, w, oh, ow, max_wh, max_ww);
    ViewPatch g;
    ResizeAxis ai, aj;
    if (!resize_patch(vt, patch, oh, ow, g, ai, aj)) return;
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    HedStage<HED> hed;
    hed.init(tid, tile, hv);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    resize_taps(ai, aj, s_tap, tid);
    auto stage = [&](auto compute) {
        view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) {
            compute(c, px);
            hed.apply(px);
        });
    };
    view_route<MODE, HED>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();

    resize_write<DT, LAYOUT>(g, ai, aj, s_px, s_tap, out, tile, oh, ow, fmt, tid, post);
}

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_view_resize(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh,
                                                            int ow, int npatch, const int32_t* __restrict__ windows, int d_mask, int max_wh,
                                                            int max_ww, const double* __restrict__ M_src,
                                                            const double* __restrict__ maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                            const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt) {
    view_resize_body<DT, LAYOUT, MODE, 0>(rgb, out, h, w, oh, ow, npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                          alpha_beta, lam, ylimf, fmt, nullptr);
}

// (instantiated where HedStage<1> is: hed_view_resize.hip includes hed_view_kernels.hpp first)
template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_hed_view_resize(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w,
                                                                int oh, int ow, int npatch, const int32_t* __restrict__ windows, int d_mask,
                                                                int max_wh, int max_ww, const double* __restrict__ M_src,
                                                                const double* __restrict__ maxC_src, const double* M_tgt,
                                                                const double* maxC_tgt, const double* __restrict__ alpha_beta, double lam,
                                                                float ylimf, TensorK fmt, HedViewArgs hv) {
    view_resize_body<DT, LAYOUT, MODE, 1>(rgb, out, h, w, oh, ow, npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                          alpha_beta, lam, ylimf, fmt, &hv);
}

}  // namespace sl
