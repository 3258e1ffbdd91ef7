// view_blur_geometry.hpp -- the geometry of the blurred view (view_blur_kernels.hpp): the decode of a tile's nine weights, the
// patch edge under the call's radius bound, the patch with its two source blocks (the pixels its outputs come from, and those grown by the
// bound and cut to the tile) and the ONE clamp rule of a tap.  Integers only, nothing of HIP included: a host compiler can include this
// header alone (tests/view_blur_geometry.cpp walks it lane by lane).
#pragma once
#include "view_geometry.hpp"         // kViewB, kViewPitch, Dihedral, ViewTile, ViewPatch, geom_min / geom_max

namespace sl {

constexpr int kBlurMaxR = 8;                     // the largest radius
constexpr int kBlurTaps = kBlurMaxR + 1;         // the weights of a tile: w_0 .. w_8
constexpr int kBlurQ = 256;                      // the weight sum per axis

// outputs per patch edge under the bound max_r (0 .. 8) and the shrink s (1, 2, 4): the patch's s b source pixels and max_r more on
// either side fit the 64 x 64 LDS block.  48 at max_r = 8, s = 1; 12 at s = 4.
SL_GEOM_FN int blur_patch_edge(int max_r, int s) { return (kViewB - 2 * max_r) >> (s >> 1); }

// The weights of one tile (block-uniform) and its radius.  The rule: every w_k in 0 .. 256, w_0 + 2 (w_1 + .. + w_8) == 256, and no weight
// beyond max_r; a tile that fails it gets the identity (256, 0, ..).
struct BlurWeights {
    int w[kBlurTaps], r;
    SL_GEOM_FN BlurWeights(const int32_t* codes, int tile, int max_r) {
        bool ok = true;
        int sum = 0;
        r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < kBlurTaps; ++k) {
            const int v = SL_GEOM_UNIFORM(codes[kBlurTaps * (size_t)tile + k]);
            ok = ok && v >= 0 && v <= kBlurQ && (k <= max_r || v == 0);
            const int c = geom_max(0, geom_min(v, kBlurQ));                      // (the sum cannot overflow, whatever the codes)
            w[k] = c;
            sum += k ? 2 * c : c;
            if (c != 0) r = k;
        }
        if (!ok || sum != kBlurQ) {
            w[0] = kBlurQ;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 1; k < kBlurTaps; ++k) w[k] = 0;
            r = 0;
        }
    }
};

// Patch `patch` of the tile under the bound max_r.  in: ViewPatch's fields for a patch of blur_patch_edge outputs square -- i0, j0, bh, bw,
// the source pixels ys, xs, nu x nv its outputs come from, and the map a0, ai, aj from output to LDS pixel when THAT block sits at LDS
// pixel 0 (view_write reads it so).  gr: the block that is read and staged (view_read, view_stage take ys, xs, nu, nv): `in` grown by max_r
// on every side and cut to the h x w tile, at most 64 x 64.
SL_GEOM_FN void blur_patch(const ViewTile& t, int patch, int npx, int h, int w, int oh, int ow, int s, int max_r, ViewPatch& in, ViewPatch& gr) {
    constexpr int PITCH = kViewPitch;
    const int B = blur_patch_edge(max_r, s);
    const bool tr = t.tr, ry = t.ry, rx = t.rx;
    in.i0 = (patch / npx) * B; in.j0 = (patch % npx) * B;
    in.bh = geom_min(B, oh - in.i0); in.bw = geom_min(B, ow - in.j0);
    const int u0 = tr ? in.j0 : in.i0, nub = tr ? in.bw : in.bh;                 // rows and columns in the window, in boxes (ViewPatch's lines)
    const int v0 = tr ? in.i0 : in.j0, nvb = tr ? in.bh : in.bw;
    in.nu = s * nub; in.nv = s * nvb;
    in.ys = t.y0 + s * (ry ? t.wh - u0 - nub : u0); in.xs = t.x0 + s * (rx ? t.ww - v0 - nvb : v0);
    const int su = ry ? -s * PITCH : s * PITCH, sv = rx ? -s : s;
    in.a0 = (ry ? (in.nu - s) * PITCH : 0) + (rx ? in.nv - s : 0);
    in.ai = tr ? sv : su; in.aj = tr ? su : sv;
    gr = in;
    gr.ys = geom_max(0, in.ys - max_r); gr.xs = geom_max(0, in.xs - max_r);
    gr.nu = geom_min(h, in.ys + in.nu + max_r) - gr.ys; gr.nv = geom_min(w, in.xs + in.nv + max_r) - gr.xs;
}

// The tap k (-8 .. 8) of the pixel at tile coordinate `at` along an axis of `lim` pixels, relative to the staged block's first pixel
// `base`: clamped in TILE space -- the border replicates the tile's edge, not the block's -- and then made block-relative.  With
// |k| <= max_r the result lies in the staged block, because that block is the grown one cut to the tile.
SL_GEOM_FN int blur_tap(int at, int k, int lim, int base) { return geom_max(0, geom_min(at + k, lim - 1)) - base; }
// CLAMP = false: a patch whose grown block the tile did not cut along this axis (blur_cut: block-uniform) -- no tap of it leaves the
// tile, the clamp does nothing, and the tap is the pixel's own slot plus a CONSTANT: an immediate offset of the LDS read.
template <bool CLAMP>
SL_GEOM_FN int blur_tap_at(int at, int k, int lim, int base) { return CLAMP ? blur_tap(at, k, lim, base) : at + k - base; }
// whether the tile cut the grown block (n pixels) of an inner block of n_in pixels along an axis
SL_GEOM_FN bool blur_cut(int n, int n_in, int max_r) { return n != n_in + 2 * max_r; }

// ---- the arithmetic of the two passes per pixel (the kernel's own lines: blur_rows / blur_cols call them, the CPU check runs them)
// A row sum: r | b << 16 as two 16-bit lanes of one dword -- a lane's sum is at most 255 x 256 = 65280, every partial sum below it: no
// carry -- and g in another.  One 8-byte LDS slot.
struct alignas(8) BlurSum { uint32_t rb, g; };

// Hs of the pixel at tile column X of the staged row `line` (packed pixels r | g << 8 | b << 16; block column 0 = tile column `base`)
template <bool CLAMP>
SL_GEOM_FN BlurSum blur_row_sum(const BlurWeights& bw, const uint32_t* line, int X, int w, int base) {
    const uint32_t px = line[X - base];
    BlurSum o;
    o.rb = (px & 0x00ff00ffu) * (uint32_t)bw.w[0];
    o.g = ((px >> 8) & 0xffu) * (uint32_t)bw.w[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k <= kBlurMaxR; ++k) {
        if (k > bw.r) break;                                                     // (block-uniform)
        const uint32_t a = line[blur_tap_at<CLAMP>(X, -k, w, base)], b = line[blur_tap_at<CLAMP>(X, k, w, base)];
        o.rb += ((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) * (uint32_t)bw.w[k];
        o.g += (((a >> 8) & 0xffu) + ((b >> 8) & 0xffu)) * (uint32_t)bw.w[k];
    }
    return o;
}

// B of the pixel at tile row Y of the column `col` of row sums (`pitch` slots from row to row; block row 0 = tile row `base`): three
// 32-bit sums (at most 256 x 65280 < 2^24), rounded once, packed r | g << 8 | b << 16
template <bool CLAMP>
SL_GEOM_FN uint32_t blur_col_px(const BlurWeights& bw, const BlurSum* col, int pitch, int Y, int h, int base) {
    const BlurSum m = col[(Y - base) * pitch];
    uint32_t r = (m.rb & 0xffffu) * (uint32_t)bw.w[0], b = (m.rb >> 16) * (uint32_t)bw.w[0], g = m.g * (uint32_t)bw.w[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 1; k <= kBlurMaxR; ++k) {
        if (k > bw.r) break;                                                     // (block-uniform)
        const BlurSum u = col[blur_tap_at<CLAMP>(Y, -k, h, base) * pitch], v = col[blur_tap_at<CLAMP>(Y, k, h, base) * pitch];
        r += ((u.rb & 0xffffu) + (v.rb & 0xffffu)) * (uint32_t)bw.w[k];
        b += ((u.rb >> 16) + (v.rb >> 16)) * (uint32_t)bw.w[k];
        g += (u.g + v.g) * (uint32_t)bw.w[k];
    }
    return ((r + 32768u) >> 16) | (((g + 32768u) >> 16) << 8) | (((b + 32768u) >> 16) << 16);
}

// The lanes of the two LDS passes: lane tid of 256 takes the columns lc + 16 p (p = 0 .. 3; adjacent lanes, adjacent dwords) of the rows
// lr + 16 q (q = 0 .. 3).
SL_GEOM_FN int blur_lane_row(int tid, int q) { return (tid >> 4) + 16 * q; }
SL_GEOM_FN int blur_lane_col(int tid, int p) { return (tid & 15) + 16 * p; }

}  // namespace sl
