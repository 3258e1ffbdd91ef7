// view_elastic_geometry.hpp -- the geometry of the elastic views (view_elastic_kernels.hpp, planes_elastic_kernels.hpp): the affine view's
// decode with a patch edge that leaves room for the displacement (ElasticTile), the decode and the clamp of the control lattice
// (elastic_stage_node), the quadratic B-spline weights (elastic_weights), the coordinates an output pixel is sampled at (elastic_at), the
// patches of a tile with their source block and their lattice nodes (elastic_patch) and the host's bound of the grid
// (elastic_grid_patches).  In the style of view_affine_geometry.hpp, which it includes and reuses: integers only, no builtin outside
// __HIP_DEVICE_COMPILE__, nothing of HIP included -- a host compiler includes this header alone, and tests/view_elastic_geometry.cpp
// walks it for every lane of every workgroup.
//
// Definition (include/stainlib_hip.h, sl_normalize_view_elastic): windows[t] as in the affine view; field[t] an int32 lattice of
// gh x gw x 2 control displacements (dy, dx) in units of 1/256 source pixel, gh = ((oh + 2^k - 1) >> k) + 2, gw likewise from ow, k =
// cell_log2 (4 .. 8) and |field| <= 256 max_d (max_d 0 .. 8; the kernels clamp).  For output pixel (i, j):
//     along i:  t = ((2 i + 1) << 8) >> (k + 1);  a = t >> 8;  f = t & 255;  wy = ((256 - f)^2, 131072 - (256 - f)^2 - f^2, f^2)
//     along j:  b, wx likewise
//     r[q] = (sum_p wx[p] field[a + q][b + p][m] + 65536) >> 17        d[m] = (sum_q wy[q] r[q] + 65536) >> 17        (arithmetic shifts)
//     Y = cy + ((a00 u + a01 v) >> 1) + (d[0] << 8)                     X = cx + ((a10 u + a11 v) >> 1) + (d[1] << 8)
// Every quantity is 32-bit: the weights are >= 0 and sum to 2^17 (w1 = 65536 + 2 f (256 - f) >= 65536), so every partial sum of a row is
// at most 2^17 x 2048 = 2^28 in size, |r| and |d| <= max |field| (a convex combination, rounded to nearest), |d << 8| <= max_d Q = 2^19
// on top of the affine view's |Y| < 2^30 + 2^29 + 2^28; (2 i + 1) << 8 < 2^22.
#pragma once
#include "view_affine_geometry.hpp"

namespace sl {

constexpr int kElasticMinCellLog2 = 4, kElasticMaxCellLog2 = 8;       // cells of 16 .. 256 output pixels
constexpr int kElasticMaxD = 8;                                       // the largest displacement, in source pixels
constexpr int kElasticUnit = 256;                                     // field units per source pixel
constexpr int kElasticNodes = (kViewB >> kElasticMinCellLog2) + 3;    // lattice nodes of a patch per axis, at most: 7
constexpr int kElasticLds = kElasticNodes * kElasticNodes * 2;        // the staged nodes of a patch, in dwords: 98

// nodes of the lattice along an axis of `no` outputs
SL_GEOM_FN int elastic_grid_side(int no, int k) { return ((no + (1 << k) - 1) >> k) + 2; }

// outputs per patch edge under the row sum r (Q16, >= 0) and the displacement bound max_d (pixels): min(64, 1 + (62 - 2 max_d) Q /
// max(r, 1)).  Over b outputs of an axis the affine part of Y spans at most (b - 1) r <= (62 - 2 max_d) Q and the displacement adds at
// most max_d Q at either end: the taps -- two per output -- span at most 62 Q, that is 64 pixels: the LDS block.  63 / 47 at the identity
// for max_d = 0 / 8, 24 at the row-sum limit with max_d = 8.
SL_GEOM_FN int elastic_patch_edge(int r, int max_d) {
    const int q = ((62 - 2 * max_d) * kAffineQ) / geom_max(r, 1);
    return q >= 63 ? 64 : 1 + q;
}

// The view of one tile (block-uniform): AffineTile -- the clamped centre, the matrix, the fill rule -- with the elastic patch edge, the
// call's cell and the clamp of the control values.
struct ElasticTile : AffineTile {
    int k, lim;
    SL_GEOM_FN ElasticTile(const int32_t* windows, int tile, int h, int w, int max_r, int cell_log2, int max_d)
        : AffineTile(windows, tile, h, w, max_r), k(cell_log2), lim(kElasticUnit * max_d) {
        // (64-bit, as in AffineTile: a device window may hold anything)
        const int64_t ry = (a00 < 0 ? -(int64_t)a00 : (int64_t)a00) + (a01 < 0 ? -(int64_t)a01 : (int64_t)a01);
        const int64_t rx = (a10 < 0 ? -(int64_t)a10 : (int64_t)a10) + (a11 < 0 ? -(int64_t)a11 : (int64_t)a11);
        const int64_t r = ry > rx ? ry : rx;
        b = elastic_patch_edge(fill ? max_r : (int)r, max_d);
    }
};

// the host's upper bound of the patches of a tile: those of the smallest edge the bounds max_r and max_d let through
SL_GEOM_FN long elastic_grid_patches(int oh, int ow, int max_r, int max_d) {
    const int b = elastic_patch_edge(max_r, max_d);
    return (long)((oh + b - 1) / b) * (long)((ow + b - 1) / b);
}

// The spline along one axis at output o: the first of its three nodes and their weights out of 2^17, exact integers with no table.
struct ElasticW { int a, w0, w1, w2; };
SL_GEOM_FN ElasticW elastic_weights(int o, int k) {
    const int t = ((2 * o + 1) << 8) >> (k + 1);
    const int f = t & 255, g = 256 - f;
    ElasticW e;
    e.a = t >> 8; e.w0 = g * g; e.w2 = f * f; e.w1 = 131072 - e.w0 - e.w2;
    return e;
}

// The lattice nodes of a patch: rows na0 .. na0 + nr - 1, columns nb0 .. nb0 + nc - 1 of the tile's lattice (nr, nc <= kElasticNodes),
// staged at dword ((row - na0) kElasticNodes + (column - nb0)) 2 + m of a block of kElasticLds dwords.
struct ElasticNodes { int na0, nb0, nr, nc; };

// One staged dword: slot idx (< kElasticLds) of the patch's node block, from the tile's lattice `field` (gw nodes per row), clamped to
// +-lim without a negation -- safe for any int32, INT32_MIN included.  false: the slot lies outside the patch's nodes and nothing is read.
SL_GEOM_FN bool elastic_stage_node(const int32_t* field, int gw, const ElasticNodes& e, int lim, int idx, int& value) {
    const int r = idx / (2 * kElasticNodes), rem = idx - r * (2 * kElasticNodes), c = rem >> 1, m = rem & 1;
    if (r >= e.nr || c >= e.nc) return false;
    const int v = field[((size_t)(e.na0 + r) * (size_t)gw + (size_t)(e.nb0 + c)) * 2 + (size_t)m];
    value = geom_max(-lim, geom_min(v, lim));
    return true;
}

// the offset in the node block of the first node of the spline at (wy.a, wx.a)
SL_GEOM_FN int elastic_node_at(const ElasticNodes& e, int a, int b) { return ((a - e.na0) * kElasticNodes + (b - e.nb0)) * 2; }

// the displacement (dy, dx) in 1/256 pixel from the 3 x 3 staged nodes at `n` (elastic_node_at): the definition, term for term
struct ElasticD { int dy, dx; };
SL_GEOM_FN ElasticD elastic_displacement(const int32_t* n, const ElasticW& wy, const ElasticW& wx) {
    int ry[3], rx[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < 3; ++q) {
        const int32_t* const row = n + q * 2 * kElasticNodes;
        ry[q] = (wx.w0 * row[0] + wx.w1 * row[2] + wx.w2 * row[4] + 65536) >> 17;
        rx[q] = (wx.w0 * row[1] + wx.w1 * row[3] + wx.w2 * row[5] + 65536) >> 17;
    }
    ElasticD d;
    d.dy = (wy.w0 * ry[0] + wy.w1 * ry[1] + wy.w2 * ry[2] + 65536) >> 17;
    d.dx = (wy.w0 * rx[0] + wy.w1 * rx[1] + wy.w2 * rx[2] + 65536) >> 17;
    return d;
}

// the source position (Q16) of output pixel (i, j): affine_at plus the displacement.  wy: elastic_weights(i, t.k) -- a lane's four
// adjacent outputs share it.  nodes: the patch's staged node block.
SL_GEOM_FN AffineYX elastic_at(const ElasticTile& t, const ElasticNodes& e, const int32_t* nodes, const ElasticW& wy, int i, int j, int oh,
                               int ow) {
    const ElasticW wx = elastic_weights(j, t.k);
    const ElasticD d = elastic_displacement(nodes + elastic_node_at(e, wy.a, wx.a), wy, wx);
    AffineYX p = affine_at(t, i, j, oh, ow);
    p.Y += d.dy * (kAffineQ / kElasticUnit);
    p.X += d.dx * (kAffineQ / kElasticUnit);
    return p;
}

// Patch `patch` of the tile: affine_patch with the elastic edge, the box of the four affine corners grown by max_d pixels (|d| <= lim: a
// tap inside the tile IS inside the block) and the patch's lattice nodes.  false when the tile has fewer patches; none: nothing is read
// and the patch is the fill -- the nodes are then not staged either.
SL_GEOM_FN bool elastic_patch(const ElasticTile& t, int patch, int h, int w, int oh, int ow, ViewPatch& g, ElasticNodes& e, bool& none) {
    const int b = t.b;
    const int npi = (oh + b - 1) / b, npj = (ow + b - 1) / b;
    if (patch >= npi * npj) return false;
    g.i0 = (patch / npj) * b; g.j0 = (patch % npj) * b;
    g.bh = geom_min(b, oh - g.i0); g.bw = geom_min(b, ow - g.j0);
    g.nu = g.nv = 0; g.ys = g.xs = 0; g.a0 = 0; g.ai = kViewPitch; g.aj = 1;
    const int i1 = g.i0 + g.bh - 1, j1 = g.j0 + g.bw - 1;
    e.na0 = elastic_weights(g.i0, t.k).a; e.nb0 = elastic_weights(g.j0, t.k).a;
    e.nr = geom_min(elastic_weights(i1, t.k).a - e.na0 + 3, kElasticNodes);      // (the min: the node block, whatever the arithmetic above)
    e.nc = geom_min(elastic_weights(j1, t.k).a - e.nb0 + 3, kElasticNodes);
    none = true;
    if (t.fill) return true;
    const AffineYX c00 = affine_at(t, g.i0, g.j0, oh, ow), c01 = affine_at(t, g.i0, j1, oh, ow), c10 = affine_at(t, i1, g.j0, oh, ow),
                   c11 = affine_at(t, i1, j1, oh, ow);
    const int grow = (t.lim / kElasticUnit) * kAffineQ;
    const int ylo = geom_min(geom_min(c00.Y, c01.Y), geom_min(c10.Y, c11.Y)) - grow, yhi = geom_max(geom_max(c00.Y, c01.Y), geom_max(c10.Y, c11.Y)) + grow;
    const int xlo = geom_min(geom_min(c00.X, c01.X), geom_min(c10.X, c11.X)) - grow, xhi = geom_max(geom_max(c00.X, c01.X), geom_max(c10.X, c11.X)) + grow;
    const int y0 = geom_max((ylo - kAffineHalf) >> 16, 0), y1 = geom_min(((yhi - kAffineHalf) >> 16) + 1, h - 1);
    const int x0 = geom_max((xlo - kAffineHalf) >> 16, 0), x1 = geom_min(((xhi - kAffineHalf) >> 16) + 1, w - 1);
    if (y0 > y1 || x0 > x1) return true;
    g.ys = y0; g.xs = x0;
    g.nu = geom_min(y1 - y0 + 1, kViewB); g.nv = geom_min(x1 - x0 + 1, kViewB);     // (the min: the LDS block, whatever the arithmetic above)
    none = false;
    return true;
}

}  // namespace sl
