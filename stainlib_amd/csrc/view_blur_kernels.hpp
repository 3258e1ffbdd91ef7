// view_blur_kernels.hpp -- Gaussian blur inside the view pass: per tile a separable integer filter of radius <= 8 on the image the call
// would write, then the crop / flip / quarter turn / box shrink of that blurred image.  The first neighbourhood operator of
// the library: a patch needs a halo.
//
//   k_view_blur   k_view (view_kernels.hpp) with a source block grown by the call's radius bound and two LDS passes between the stage
//                 and the write side
//
// Definition (include/stainlib_hip.h, sl_normalize_blur_view): codes[t] = (w_0 .. w_8), w_0 + 2 (w_1 + .. + w_8) == 256; per channel of `full`
//     Hs[y, x] = sum_k w_|k| full[y, clamp(x + k, 0, w - 1)]                         (<= 65280: 16 bits, exact)
//     B[y, x]  = (sum_k w_|k| Hs[clamp(y + k, 0, h - 1), x] + 32768) >> 16           (rounded once)
// and the output is the existing view of B.
//
// What is shared with k_view: ViewTile (the window's decode), load12 / view_read (the read side), view_stage / view_unpack (the LDS stage,
// one packed dword per SOURCE pixel, pitch 65), view_route<MODE, 0> (the route arithmetic per source pixel, called), and the whole write
// side view_write with its box shrink (view_box) and store tail.  What is new: the geometry (view_blur_geometry.hpp) and the two passes.
//
// Shape: ONE workgroup = one tile and one patch of b x b OUTPUT pixels, b = (64 - 2 max_r) / s for the call's block-uniform bound max_r
// (a kernel argument: the codes may live on the device, so the host sizes the grid from the bound) and shrink s.  The staged block is the
// patch's s b x s b source pixels grown by max_r on every side and cut to the tile: at most 64 x 64, k_view's s_px.  Halo pixels are
// computed again by the neighbouring patch: (64 / 48)^2 = 1.78 times the per-pixel arithmetic at max_r = 8.
//   stage       view_route puts the grown block into s_px (packed r | g << 8 | b << 16), barrier
//   horizontal  for every ROW of the grown block and every column of the inner block: the 2 r + 1 taps of s_px along the row, the tap's
//               column clamped in TILE space and then made block-relative (blur_tap: a replicated border costs an index clamp, no load);
//               r and b summed as two 16-bit lanes of one dword (px & 0xff00ff; a lane's sum is at most 255 x 256 = 65280: no carry), g in
//               another; the pair into s_h as ONE 8-byte slot, barrier
//   vertical    for every pixel of the inner block: the 2 r + 1 taps of s_h along the column (one ds_read_b64 each), three 32-bit sums
//               (<= 256 x 65280 < 2^24), rounded once, the byte triple packed into s_px AT THE INNER BLOCK'S OWN ORIGIN -- nobody reads the
//               staged pixels any more --, barrier
//   write side  view_write on the inner block, as in k_view: the dihedral map, the box shrink of the blurred bytes, cvt_chunk, the stores.
// Which pass lives in LDS: both, each once.  The alternative -- lanes that keep a column of row sums in registers and slide down it -- needs
// a register window of 17 dwords x 2 per lane and a lane assignment that depends on the radius; the two-buffer form keeps every pass a plain
// "each lane, its pixels" loop whose indices the CPU check can walk, at 33 KB more LDS (52 KB per workgroup: three per CU in 160 KiB).
// Lanes of both passes (blur_lane_row / blur_lane_col): 16 lanes along a row take ADJACENT columns lc + 16 p, so the taps of one
// instruction are adjacent dwords (s_px; pitch 65: the 4 rows of a wave land 1 bank apart -> at most 2-way) or adjacent 8-byte slots
// (s_h).  A tile's own radius r <= max_r (block-uniform) bounds the tap loops: a tile of the identity runs one tap per pass.
// A patch whose grown block the tile did not cut along an axis (blur_cut; most patches of a large tile) takes that axis' pass WITHOUT the
// clamp: a tap is then the pixel's own slot plus a constant, an immediate offset of the LDS read, and the max / min / subtract per tap go.
#pragma once
#include "view_kernels.hpp"          // view_read, view_stage, view_route, view_write, the modes
#include "view_blur_geometry.hpp"

namespace sl {

// ---- horizontal pass: s_px (the grown block) -> s_h (rows of the grown block, columns of the inner block)
template <bool CLAMP>
__device__ __forceinline__ void blur_rows(const BlurWeights& bw, const ViewPatch& in, const ViewPatch& gr, int w, const uint32_t* s_px,
                                          BlurSum* s_h, int tid) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = blur_lane_row(tid, q);
        if (row >= gr.nu) continue;                          // (nothing below has a barrier)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int c = blur_lane_col(tid, p);
            if (c >= in.nv) continue;
            s_h[row * kViewPitch + c] = blur_row_sum<CLAMP>(bw, s_px + row * kViewPitch, in.xs + c, w, gr.xs);
        }
    }
}

// ---- vertical pass: s_h -> s_px, the blurred bytes of the inner block at LDS pixel 0 (behind a barrier after blur_rows)
template <bool CLAMP>
__device__ __forceinline__ void blur_cols(const BlurWeights& bw, const ViewPatch& in, const ViewPatch& gr, int h, const BlurSum* s_h,
                                          uint32_t* s_px, int tid) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = blur_lane_row(tid, q);
        if (y >= in.nu) continue;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int c = blur_lane_col(tid, p);
            if (c >= in.nv) continue;
            s_px[y * kViewPitch + c] = blur_col_px<CLAMP>(bw, s_h + c, kViewPitch, in.ys + y, h, gr.ys);
        }
    }
}

// npx: patches per output row, npatch: per tile -- both from the bound max_r (view_blur.hip: view_blur_geometry).
template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_view_blur(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                          int npx, int npatch, const int32_t* __restrict__ windows, int d_mask, int shrink,
                                                          int max_r, const int32_t* __restrict__ codes, const double* __restrict__ M_src,
                                                          const double* __restrict__ maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                          const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float2 s_tab[256];
    __shared__ uint32_t s_px[B * PITCH];
    __shared__ BlurSum s_h[B * PITCH];
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view and the weights of this tile (block-uniform), the two source blocks of this patch and the four chunks of this lane
    const int s = __builtin_amdgcn_readfirstlane(shrink);
    const int R = __builtin_amdgcn_readfirstlane(max_r);
    const ViewTile vt(windows, tile, d_mask, h, w, oh, ow, s);
    const BlurWeights bw(codes, tile, R);
    ViewPatch in, gr;
    blur_patch(vt, patch, npx, h, w, oh, ow, s, R, in, gr);
    Chunk c4[4];
    view_read(gr, src, nbytes, w, lr, lc, c4);
    auto stage = [&](auto compute) {
        view_stage(gr, s_px, lr, lc, c4, [&](const Chunk& c, uint32_t (&px)[4]) { compute(c, px); });
    };
    view_route<MODE, 0>(s_tab, stage, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam, ylimf);
    __syncthreads();
    if (blur_cut(gr.nv, in.nv, R)) blur_rows<true>(bw, in, gr, w, s_px, s_h, tid);       // (block-uniform: one scalar branch per pass)
    else blur_rows<false>(bw, in, gr, w, s_px, s_h, tid);
    __syncthreads();
    if (blur_cut(gr.nu, in.nu, R)) blur_cols<true>(bw, in, gr, h, s_h, s_px, tid);
    else blur_cols<false>(bw, in, gr, h, s_h, s_px, tid);
    __syncthreads();

    view_write<DT, LAYOUT>(in, s_px, out, tile, oh, ow, fmt, lr, lc, s);
}

}  // namespace sl
