// planes_elastic_kernels.hpp -- companion planes through the windows and the field of an elastic view: label maps, instance maps and masks
// of any 1-, 2-, 4- or 8-byte element type, deformed exactly as their image was, by the NEAREST element.
//
//   k_view_planes_elastic<ES>   k_view_planes_affine (planes_affine_kernels.hpp) with the image view's (Y, X) -- elastic_at
//                               (view_elastic_geometry.hpp) in place of affine_at: per plane (tile t = plane / c) and output element
//                               (i, j) the element at (Y >> 16, X >> 16) of the plane, a bit copy; outside the plane the fill element
//
// Shape: ONE workgroup = one plane and one patch -- the image view's patch (ElasticTile's edge, elastic_patch's decode).  The elements
// are a pure gather with no LDS, as in k_view_planes_affine; the one thing staged is the patch's lattice nodes (98 dwords, clamped once
// per node, one barrier), for the reason view_elastic_kernels.hpp gives: nine nodes per output element, chosen per lane.
#pragma once
#include "planes_affine_kernels.hpp"
#include "view_elastic_geometry.hpp"

namespace sl {

// ES: bytes per element (1, 2, 4, 8).  npatch: the host's upper bound of the patches of a plane.  fill_lo / fill_hi: the fill element's
// low ES bytes (zero-extended) and, at ES = 8, its high half.
template <int ES>
static __global__ __launch_bounds__(kWG) void k_view_planes_elastic(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int c, int h,
                                                                    int w, int oh, int ow, int npatch, const int32_t* __restrict__ windows,
                                                                    int max_r, const int32_t* __restrict__ field, int cell_log2, int max_d,
                                                                    uint32_t fill_lo, uint32_t fill_hi) {
    static_assert(kElasticLds <= kWG, "one slot per lane");
    __shared__ __attribute__((aligned(8))) int32_t s_nodes[kElasticLds];
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int tile = plane / c;
    const size_t P = (size_t)h * (size_t)w, PO = (size_t)oh * (size_t)ow;
    SL_GLOBAL const uint8_t* const src = as_global(planes) + (size_t)plane * P * ES;

    const ElasticTile vt(windows, tile, h, w, max_r, cell_log2, max_d);
    ViewPatch g;
    ElasticNodes e;
    bool none;
    if (!elastic_patch(vt, patch, h, w, oh, ow, g, e, none)) return;
    if (!none) {                                             // (block-uniform)
        const int gh = elastic_grid_side(oh, vt.k), gw = elastic_grid_side(ow, vt.k);
        int v;
        if (tid < kElasticLds && elastic_stage_node(field + (size_t)tile * ((size_t)gh * gw * 2), gw, e, vt.lim, tid, v)) s_nodes[tid] = v;
        __syncthreads();
    }

    const PatchLanes ln = patch_lanes(g.bw, tid, kWG);
    const int jl = ln.jl, bh = g.bh, bw = g.bw;
    if (jl >= bw) return;
    const int nvalid = min(4, bw - jl);
    uint8_t* const dst = out + (size_t)plane * PO * ES;
    for (int il = ln.il0; il < bh; il += ln.rows) {
        Planes4<ES> o;
        const ElasticW wy = elastic_weights(g.i0 + il, vt.k);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            o.lo[p] = fill_lo;
            if constexpr (ES == 8) o.hi[p] = fill_hi;
            if (none) continue;                              // (block-uniform: the tile is all fill, or the patch misses the plane)
            const AffineYX q = elastic_at(vt, e, s_nodes, wy, g.i0 + il, g.j0 + min(jl + p, bw - 1), oh, ow);
            const int ky = q.Y >> 16, kx = q.X >> 16;
            const bool in = affine_inside(ky, h) && affine_inside(kx, w);
            const size_t el = in ? (size_t)ky * (size_t)w + (size_t)kx : 0;
            SL_GLOBAL const uint8_t* const a = src + el * (size_t)ES;
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
