// planes_affine_kernels.hpp -- companion planes through the windows of an affine view: label maps, instance maps and masks of any 1-, 2-,
// 4- or 8-byte element type, rotated / zoomed / sheared exactly as their image was, by the NEAREST element.
//
//   k_view_planes_affine<ES>   per plane (tile t = plane / c) and output element (i, j) the element at (Y >> 16, X >> 16) of the plane,
//                              a bit copy, Y and X the image view's (view_affine_geometry.hpp: affine_at); outside the plane the
//                              call's fill element
//
// Shape: ONE workgroup = one plane and one patch -- the image view's patch (AffineTile's edge, affine_patch's decode), so a companion's
// workgroup touches the source footprint its image's workgroup staged, at most 64 x 64 elements.  NO LDS: the kernel is a pure gather
// -- one element in, one element out, nothing computed per SOURCE element and nothing shared between outputs --, so a stage would add
// a barrier and a second address computation to move each element once more.  What LDS buys k_view_affine (the arithmetic per source
// pixel done once, four taps per output) does not exist here; what it would buy here is only row-wise source reads, and the footprint
// of a patch (<= 4096 elements, <= 32 KiB) stays in the CU's vector cache while its 256 lanes walk it: every source line is fetched
// from L2 once per patch either way.  The write side is k_view_planes': output rows, 4 adjacent elements per lane, one vector store.
// The bounds are decided per element from the ABSOLUTE coordinates; the load of an outside element goes to the plane's element 0 (never
// predicated, never outside the plane) and is replaced by the fill.
#pragma once
#include "planes_view_kernels.hpp"   // Planes4, planes_store4, the unaligned vector types; planes_view_geometry.hpp through it
#include "view_affine_geometry.hpp"

namespace sl {

// ES: bytes per element (1, 2, 4, 8).  npatch: the host's upper bound of the patches of a plane.  fill_lo / fill_hi: the fill element's
// low ES bytes (zero-extended) and, at ES = 8, its high half.
template <int ES>
static __global__ __launch_bounds__(kWG) void k_view_planes_affine(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int c, int h,
                                                                   int w, int oh, int ow, int npatch, const int32_t* __restrict__ windows,
                                                                   int max_r, uint32_t fill_lo, uint32_t fill_hi) {
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int tile = plane / c;
    const size_t P = (size_t)h * (size_t)w, PO = (size_t)oh * (size_t)ow;
    SL_GLOBAL const uint8_t* const src = as_global(planes) + (size_t)plane * P * ES;

    const AffineTile vt(windows, tile, h, w, max_r);
    ViewPatch g;
    bool none;
    if (!affine_patch(vt, patch, h, w, oh, ow, g, none)) return;

    const PatchLanes ln = patch_lanes(g.bw, tid, kWG);
    const int jl = ln.jl, bh = g.bh, bw = g.bw;
    if (jl >= bw) return;
    const int nvalid = min(4, bw - jl);
    uint8_t* const dst = out + (size_t)plane * PO * ES;
    for (int il = ln.il0; il < bh; il += ln.rows) {
        Planes4<ES> o;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            o.lo[p] = fill_lo;
            if constexpr (ES == 8) o.hi[p] = fill_hi;
            if (none) continue;                              // (block-uniform: the tile is all fill)
            const AffineYX q = affine_at(vt, g.i0 + il, g.j0 + min(jl + p, bw - 1), oh, ow);
            const int ky = q.Y >> 16, kx = q.X >> 16;
            const bool in = affine_inside(ky, h) && affine_inside(kx, w);
            const size_t e = in ? (size_t)ky * (size_t)w + (size_t)kx : 0;
            SL_GLOBAL const uint8_t* const a = src + e * (size_t)ES;
            uint32_t lo, hi = 0;
            if constexpr (ES == 1) lo = *a;
            else if constexpr (ES == 2) lo = *(SL_GLOBAL const sl_u16u*)a;
            else if constexpr (ES == 4) lo = *(SL_GLOBAL const sl_u32u*)a;
            else { const sl_u32x2u u = *(SL_GLOBAL const sl_u32x2u*)a; lo = u.x; hi = u.y; }
            o.lo[p] = in ? lo : fill_lo;
            if constexpr (ES == 8) o.hi[p] = in ? hi : fill_hi;
        }
        planes_store4<ES>(dst + planes_out_elem(g, ow, il, jl) * (size_t)ES, nvalid, o);
    }
}

}  // namespace sl
