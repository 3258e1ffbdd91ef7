// planes_view_geometry.hpp -- the lane-to-address arithmetic of k_view_planes (planes_view_kernels.hpp): which source elements a lane
// loads, which LDS slots it fills, which slot an output element is gathered from and where it is stored.  Plain integer functions on
// the patch geometry of view_geometry.hpp, no builtin and nothing of HIP: a host compiler includes this header alone, and
// tests/planes_view_geometry.cpp runs it for every lane of every workgroup on byte buffers of exactly the input's and the output's size.
//
// All counts are in ELEMENTS of the plane (1, 2, 4 or 8 bytes each); the kernel multiplies by the element size, in size_t.
#pragma once
#include "view_geometry.hpp"

namespace sl {

constexpr int kPlanesWG = 256;                   // lanes of a workgroup (= kWG)
constexpr int kPlanesIdx = 2 * kViewB;           // the index table: kViewB entries for the patch's rows, kViewB for its columns

// The centre sample along an axis of nw window pixels and no outputs: the pixel under the centre of output i, ((2 i + 1) nw) // (2 no).
// i < no and no nw <= 2^30 (the resizing view's limit), so the product stays below 2^31.
SL_GEOM_FN uint32_t planes_nearest_index(uint32_t i, uint32_t nw, uint32_t no) { return ((2u * i + 1u) * nw) / (2u * no); }

// ---- read side: pass q (0 .. 3) of lane tid walks SOURCE rows -- 16 lanes per row, 4 adjacent elements each, 16 rows per pass.
// e: the first of the 4 elements, counted from the plane's first element; `vec`: all 4 lie inside the plane of P elements and are loaded
// as one vector, else (the last elements of a plane) each element k is loaded alone from min(e + k, P - 1).  Rows and chunks past the
// block re-read its last row / chunk (no predicated load); the LDS write is masked instead: the first n of the 4 go to slots
// slot .. slot + n - 1 (n = 0: none).
struct PlanesLoad {
    size_t e;
    int slot, n;
    bool vec;
};
SL_GEOM_FN PlanesLoad planes_load(const ViewPatch& g, int w, size_t P, int tid, int q) {
    const int lr = tid >> 4, lc = tid & 15;
    const int r = 16 * q + lr;
    const int cc = geom_min(lc, (g.nv - 1) >> 2);
    PlanesLoad L;
    L.e = (size_t)(g.ys + geom_min(r, g.nu - 1)) * (size_t)w + (size_t)(g.xs + 4 * cc);
    L.vec = L.e + 4 <= P;
    L.slot = r * kViewPitch + 4 * lc;
    L.n = r < g.nu ? geom_max(0, geom_min(4, g.nv - 4 * lc)) : 0;
    return L;
}

// ---- the index table of the nearest mode: entry t < kViewB is the LDS offset of row t of the patch, entry kViewB + t that of its
// column t; an output element (il, jl) of the patch is gathered from slot idx[il] + idx[kViewB + jl].
// Crop / shrink: ViewPatch's affine map names the FIRST pixel of the s x s box in source orientation; the centre sample of the
// definition, s i + s / 2 in the window's own orientation, is s / 2 rows and columns further -- whichever way the output runs.
SL_GEOM_FN int planes_index_shrink(const ViewPatch& g, int s, int e) {
    return e < kViewB ? g.a0 + (s >> 1) * (kViewPitch + 1) + e * g.ai : (e - kViewB) * g.aj;
}
// Resizing: output t of the axis is output a.at(t) along the WINDOW axis (the mirror is taken on the index, not on the formula), its
// centre sample is counted from the block's first pixel a.lo.
SL_GEOM_FN int planes_index_resize(const ResizeAxis& a, int t) {
    return ((int)planes_nearest_index((uint32_t)a.at(t), (uint32_t)a.nw, (uint32_t)a.no) - a.lo) * a.stride;
}

// ---- write side: lanes walk OUTPUT rows, 4 adjacent elements per lane; lanes per row = the power of two that covers the patch's width
// (1 .. 16), so a narrow patch spreads its rows over all the lanes.  Lane tid takes the elements jl .. jl + 3 of rows il0, il0 + rows, ...
struct PlanesLanes {
    int il0, jl, rows;
};
SL_GEOM_FN PlanesLanes planes_lanes(int bw, int tid) {
    const int n4 = (bw + 3) >> 2;                                                // chunks of 4 elements per output row, 1 .. 16
    const int lg = n4 <= 1 ? 0 : 32 - __builtin_clz((unsigned)(n4 - 1));         // log2 of the lanes per row: 0 .. 4
    PlanesLanes l;
    l.il0 = tid >> lg; l.jl = 4 * (tid & ((1 << lg) - 1)); l.rows = kPlanesWG >> lg;
    return l;
}
// the output element (il, jl) of the patch, counted from the first element of the plane's oh x ow output
SL_GEOM_FN size_t planes_out_elem(const ViewPatch& g, int ow, int il, int jl) { return (size_t)(g.i0 + il) * (size_t)ow + (size_t)(g.j0 + jl); }

}  // namespace sl
