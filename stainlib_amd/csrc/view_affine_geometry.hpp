// view_affine_geometry.hpp -- the geometry of the affine views (view_affine_kernels.hpp, planes_affine_kernels.hpp): the decode and the
// clamp of a six-column window (AffineTile), the per-tile patch edge, the patches of a tile and the source block of one (affine_patch),
// the coordinates an output pixel is sampled at (affine_at) and the host's bound of the grid (affine_grid_patches), in the style of
// view_geometry.hpp: integers only, no builtin outside __HIP_DEVICE_COMPILE__, nothing of HIP included -- a host compiler includes this
// header alone, and tests/view_affine_geometry.cpp walks it for every lane of every workgroup.
//
// Definition (include/stainlib_hip.h, sl_normalize_view_affine): windows[t] = (cy, cx, a00, a01, a10, a11) in units of 2^-16 source
// pixel, Q = 65536; for output pixel (i, j) of the call's oh x ow output, u = 2 i + 1 - oh, v = 2 j + 1 - ow:
//     Y = cy + ((a00 u + a01 v) >> 1)        X = cx + ((a10 u + a11 v) >> 1)        (arithmetic shift)
// Every quantity is 32-bit under the limits: h, w, oh, ow <= 8192 (|u|, |v| < 2^13), row sums Ry = |a00| + |a01|, Rx = |a10| + |a11|
// <= 2 Q (|a u + a' v| <= 2^17 (2^13 - 1) < 2^30), centres in [-2^28, side Q + 2^28] (side Q <= 2^29): |Y| < 2^30 + 2^29 + 2^28.
// u and v step by 2, so a u + a' v has the parity of a oh' + a' ow' for every pixel of a tile and differences of Y are exact halves of
// even numbers: over b outputs of an axis Y spans at most (b - 1) R.
#pragma once
#include "view_geometry.hpp"

namespace sl {

constexpr int kAffineQ = 65536;                  // one source pixel
constexpr int kAffineHalf = kAffineQ / 2;
constexpr int kAffineMaxSide = 8192;             // h, w, oh, ow
constexpr int kAffineMaxR = 2 * kAffineQ;        // a row sum: at most 2 source pixels per output pixel
constexpr int kAffineCentreSlack = 1 << 28;      // a centre lies within this of the tile

// outputs per patch edge under the row sum r (Q16, >= 0): min(64, 1 + 62 Q / max(r, 1)).  The taps of b outputs of an axis -- two per
// output, floor((Y - Q/2) / Q) and the next -- span at most floor((b - 1) r / Q) + 2 <= 64 pixels: the LDS block.  63 at the identity,
// 44 at 45 degrees, 32 at the limit; does not grow with r.
SL_GEOM_FN int affine_patch_edge(int r) {
    const int q = (62 * kAffineQ) / geom_max(r, 1);
    return q >= 63 ? 64 : 1 + q;
}

// The view of one tile (block-uniform): the clamped centre, the matrix, its patch edge; `fill`: the row sums pass the call's bound and the
// tile is written as fill everywhere (there is no sensible clamp of a matrix) -- nothing else of it is then used but the edge.
struct AffineTile {
    int cy, cx, a00, a01, a10, a11, b;
    bool fill;
    SL_GEOM_FN AffineTile(const int32_t* windows, int tile, int h, int w, int max_r) {
        const int32_t* const wv = windows + 6 * (size_t)tile;
        cy = geom_max(-kAffineCentreSlack, geom_min(SL_GEOM_UNIFORM(wv[0]), h * kAffineQ + kAffineCentreSlack));
        cx = geom_max(-kAffineCentreSlack, geom_min(SL_GEOM_UNIFORM(wv[1]), w * kAffineQ + kAffineCentreSlack));
        a00 = SL_GEOM_UNIFORM(wv[2]); a01 = SL_GEOM_UNIFORM(wv[3]); a10 = SL_GEOM_UNIFORM(wv[4]); a11 = SL_GEOM_UNIFORM(wv[5]);
        // (64-bit: a device window may hold anything, INT32_MIN included)
        const int64_t ry = (a00 < 0 ? -(int64_t)a00 : (int64_t)a00) + (a01 < 0 ? -(int64_t)a01 : (int64_t)a01);
        const int64_t rx = (a10 < 0 ? -(int64_t)a10 : (int64_t)a10) + (a11 < 0 ? -(int64_t)a11 : (int64_t)a11);
        const int64_t r = ry > rx ? ry : rx;
        fill = r > (int64_t)max_r;
        b = affine_patch_edge(fill ? max_r : (int)r);
    }
};

// the host's upper bound of the patches of a tile: those of the smallest edge the bound max_r lets through
SL_GEOM_FN long affine_grid_patches(int oh, int ow, int max_r) {
    const int b = affine_patch_edge(max_r);
    return (long)((oh + b - 1) / b) * (long)((ow + b - 1) / b);
}

// the source position (Q16) of output pixel (i, j): the definition, term for term
struct AffineYX { int Y, X; };
SL_GEOM_FN AffineYX affine_at(const AffineTile& t, int i, int j, int oh, int ow) {
    const int u = 2 * i + 1 - oh, v = 2 * j + 1 - ow;
    AffineYX p;
    p.Y = t.cy + ((t.a00 * u + t.a01 * v) >> 1);
    p.X = t.cx + ((t.a10 * u + t.a11 * v) >> 1);
    return p;
}

// Patch `patch` of the tile: false when the tile has fewer patches (the grid is sized for the call's bound).  g: the patch i0, j0,
// bh x bw and the source block of its taps INTERSECTED WITH THE TILE, ys, xs, nu x nv (view_read's and view_stage's; at most 64 x 64);
// none: the block is empty -- the tile is all fill, or every tap of the patch lies outside the tile -- and nothing is read.
// Y and X are affine in (i, j) up to one shared floor, so their extremes over the patch are at its four corners.
SL_GEOM_FN bool affine_patch(const AffineTile& t, int patch, int h, int w, int oh, int ow, ViewPatch& g, bool& none) {
    const int b = t.b;
    const int npi = (oh + b - 1) / b, npj = (ow + b - 1) / b;
    if (patch >= npi * npj) return false;
    g.i0 = (patch / npj) * b; g.j0 = (patch % npj) * b;
    g.bh = geom_min(b, oh - g.i0); g.bw = geom_min(b, ow - g.j0);
    g.nu = g.nv = 0; g.ys = g.xs = 0; g.a0 = 0; g.ai = kViewPitch; g.aj = 1;
    none = true;
    if (t.fill) return true;
    const int i1 = g.i0 + g.bh - 1, j1 = g.j0 + g.bw - 1;
    const AffineYX c00 = affine_at(t, g.i0, g.j0, oh, ow), c01 = affine_at(t, g.i0, j1, oh, ow), c10 = affine_at(t, i1, g.j0, oh, ow),
                   c11 = affine_at(t, i1, j1, oh, ow);
    const int ylo = geom_min(geom_min(c00.Y, c01.Y), geom_min(c10.Y, c11.Y)), yhi = geom_max(geom_max(c00.Y, c01.Y), geom_max(c10.Y, c11.Y));
    const int xlo = geom_min(geom_min(c00.X, c01.X), geom_min(c10.X, c11.X)), xhi = geom_max(geom_max(c00.X, c01.X), geom_max(c10.X, c11.X));
    // the taps: rows floor((ylo - Q/2) / Q) .. floor((yhi - Q/2) / Q) + 1, likewise columns; then the part of them the tile holds
    const int y0 = geom_max((ylo - kAffineHalf) >> 16, 0), y1 = geom_min(((yhi - kAffineHalf) >> 16) + 1, h - 1);
    const int x0 = geom_max((xlo - kAffineHalf) >> 16, 0), x1 = geom_min(((xhi - kAffineHalf) >> 16) + 1, w - 1);
    if (y0 > y1 || x0 > x1) return true;
    g.ys = y0; g.xs = x0;
    g.nu = geom_min(y1 - y0 + 1, kViewB); g.nv = geom_min(x1 - x0 + 1, kViewB);     // (the min: the LDS block, whatever the arithmetic above)
    none = false;
    return true;
}

// ---- write side: the lanes of a patch are view_geometry.hpp's patch_lanes.
// The four taps and the two 8-bit weights of one output pixel of the images: rows ky, ky + 1, columns kx, kx + 1 of the tile (any of
// them may lie outside it), weights fy, fx of the second row / column out of 256.
struct AffineTaps { int ky, kx, fy, fx; };
SL_GEOM_FN AffineTaps affine_taps(const AffineYX& p) {
    const int ty = p.Y - kAffineHalf, tx = p.X - kAffineHalf;
    AffineTaps a;
    a.ky = ty >> 16; a.fy = (ty >> 8) & 255;
    a.kx = tx >> 16; a.fx = (tx >> 8) & 255;
    return a;
}

// the LDS slot of tap row r / column c of the tile in the block of g, clamped into the block: a tap inside the tile IS inside the block
// (affine_patch), a tap outside it reads some slot of the block and is replaced by the fill (the caller's select on `inside`).
SL_GEOM_FN int affine_lds_row(const ViewPatch& g, int r) { return geom_max(0, geom_min(r - g.ys, g.nu - 1)) * kViewPitch; }
SL_GEOM_FN int affine_lds_col(const ViewPatch& g, int c) { return geom_max(0, geom_min(c - g.xs, g.nv - 1)); }
SL_GEOM_FN bool affine_inside(int k, int side) { return (unsigned)k < (unsigned)side; }

// the 8-bit bilinear blend of four packed pixels r | g << 8 | b << 16: per channel
//     ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16
// The row step runs on r and b together (two 16-bit lanes of one dword: (256 - fx) p + fx p' <= 256 x 255 cannot carry), the column step
// per channel (<= 256 x 65280 + 32768 < 2^32).
SL_GEOM_FN uint32_t affine_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int fy, int fx) {
    const uint32_t wx1 = (uint32_t)fx, wx0 = 256u - wx1, wy1 = (uint32_t)fy, wy0 = 256u - wy1;
    const uint32_t trb = wx0 * (p00 & 0x00ff00ffu) + wx1 * (p01 & 0x00ff00ffu), tg = wx0 * ((p00 >> 8) & 0xffu) + wx1 * ((p01 >> 8) & 0xffu);
    const uint32_t brb = wx0 * (p10 & 0x00ff00ffu) + wx1 * (p11 & 0x00ff00ffu), bg = wx0 * ((p10 >> 8) & 0xffu) + wx1 * ((p11 >> 8) & 0xffu);
    const uint32_t r = (wy0 * (trb & 0xffffu) + wy1 * (brb & 0xffffu) + 32768u) >> 16;
    const uint32_t b = (wy0 * (trb >> 16) + wy1 * (brb >> 16) + 32768u) >> 16;
    const uint32_t gg = (wy0 * tg + wy1 * bg + 32768u) >> 16;
    return r | (gg << 8) | (b << 16);
}

}  // namespace sl
