// planes_view_kernels.hpp -- companion planes through the windows of a view pass: label maps, instance maps, masks and distance maps of
// any 1-, 2-, 4- or 8-byte element type, cropped / shrunk / resized, flipped and turned exactly as their image was.
//
//   k_view_planes<ES, MODE>   per plane (tile t = plane / c) the window windows[t] of a crop / shrink view or of a resizing view,
//                             resampled by the centre sample (MODE = nearest: a bit copy of ES-byte elements) or by the images' own box
//                             mean / area average (MODE = area: ES = 1), flipped and turned by the tile's dihedral code
//
// Definition (include/stainlib_hip.h, sl_view_planes): the window is resampled in the TILE's orientation, then flipped and turned.  The
// centre sample ((2 i + 1) nw) // (2 no) does not commute with a reversal when nw / no is even, so the kernel, which samples in OUTPUT
// orientation, mirrors the INDEX (ResizeAxis::at, ViewPatch's affine map plus the half box) and never the formula.
//
// What is shared with k_view / k_view_resize: the decode of a window and its clamp (view_geometry.hpp: Dihedral, ViewTile, ViewPatch,
// ResizeTile, resize_patch), the taps and the exact rounded division of the area average (resize_taps, resize_round).  What is new: the
// element-size read side, the LDS image, the index table and the write side; their lane-to-address arithmetic is in
// planes_view_geometry.hpp, which the CPU check runs lane by lane.
//
// Shape: ONE workgroup = one plane and one patch -- the image views' patch: kViewB / s outputs square for a crop / shrink, the resizing
// view's per-tile edge else, in both cases a source block of at most 64 x 64 elements.  Both sides of the transposition run along rows:
//   read side   SOURCE rows: 16 lanes per row, 4 adjacent elements each (one 4-, 8-, 16-byte load, or two 16-byte loads at ES = 8, at
//               element alignment: rows start at any element), 16 rows per pass, 4 passes, all loads issued before the first LDS write.
//               Never predicated: rows and chunks past the block re-read its last row / chunk and the LDS write is masked.  A vector that
//               would pass the END OF THE PLANE is loaded element by element at clamped addresses instead (at most the last 3 elements
//               of a plane's last row; block-divergent, rare), so no load touches a byte outside the plane.
//   LDS         one DWORD slot per element in SOURCE orientation, row pitch kViewPitch = 65 -- k_view's image; an element of 1 or 2
//               bytes is zero-extended, an element of 8 bytes is TWO dword planes (low halves, high halves) of that same shape.
//   index       threads 0 .. 127 compute once the LDS offset of each of the patch's <= 64 output rows and <= 64 output columns
//               (planes_index_shrink / planes_index_resize): the one division of the centre sample per row and column, none per element.
//   write side  OUTPUT rows, 4 adjacent elements per lane, as many lanes per row as cover the patch's width (a power of two, 1 .. 16):
//               slot = idx[row] + idx[64 + column], one ds_read_b32 per element (two at ES = 8), one 4-, 8-, 16-byte store (two at
//               ES = 8) per lane; the ragged last lane of a row stores element by element.
// LDS banking (ds_write_b32 / ds_read_b32: bank (a / 4) % 32 within each 32-lane half).  Every LDS instruction of this kernel is a
// 4-byte access to a pitch-65 image, whatever ES is, so view_kernels.hpp's picture holds as it stands: the bank of element (r, x) is
// (r + x) % 32; instruction p of a lane touches x = 4 c + p, so row-wise lanes c and c + 8 share a bank and the next row is shifted by
// one: 2-way; column-wise (odd codes) the lane stride is 4 pitches = 4 banks: 2-way again, where an even pitch would be 16-way.  Under a
// shrink or a resize the lane strides grow as in view_kernels.hpp / view_resize_kernels.hpp: 2-way at ratio 2, 4-way at ratio 4.
// 8-byte elements -- two dword planes against ONE 64-bit array of pitch 65 qwords: ds_read_b64 banks are (a / 4) % 64, so element (r, x)
// sits at banks 2 (r + x) % 64 and the next one; row-wise lanes c and c + 8 are 64 banks apart (2-way), column-wise the lane stride is
// 4 x 130 = 8 banks mod 64 (16 lanes on 8 even banks: 2-way) -- the same conflict degree as the two planes.  In LDS cycles per wave one
// ds_read_b64 (2) beats two ds_read_b32 (2 x 2) and one ds_write_b64 (~6) two ds_write_b32 (2 x 4) by a few cycles per element group,
// on a pass that waits for HBM, not for LDS.  Chosen: the two planes -- a lane's high half goes to its low half's bank (the plane offset
// is 65 x 64 dwords) but in an access of its own, so the picture above holds per access (the compiler pairs the two into
// ds_write2st64_b32 / ds_read2st64_b32), and one gather (one index table, one slot) serves every element size.
// LDS per workgroup: 17 152 bytes (ES <= 4), 39 936 as allocated at ES = 8: occupancy 8 and 4 waves per SIMD.
// Not done: under a shrink or a resize the nearest mode still stages every source row of the block, also those no centre falls on.
#pragma once
#include "view_resize_kernels.hpp"   // resize_taps, resize_round, sl_u32x2u / sl_u32x4u; view_geometry.hpp through it
#include "planes_view_geometry.hpp"

namespace sl {

constexpr int kPlanesNearest = 0, kPlanesArea = 1;           // SL_PLANES_NEAREST, SL_PLANES_AREA
constexpr int kPlanesPlane = kViewB * kViewPitch;            // dwords of one LDS plane
static_assert(kPlanesWG == kWG, "planes_view_geometry.hpp counts kWG lanes");

typedef uint32_t sl_u32u __attribute__((aligned(1)));
typedef uint16_t sl_u16u __attribute__((aligned(1)));

// 4 adjacent elements of ES bytes as dwords: lo[k] the (zero-extended) element or its low half, hi[k] its high half (ES = 8 only)
template <int ES>
struct Planes4 {
    uint32_t lo[4];
    uint32_t hi[ES == 8 ? 4 : 1];
};

// the 4 elements of one read-side pass (planes_load): one vector inside the plane, single elements at clamped addresses at its very end
template <int ES>
__device__ __forceinline__ Planes4<ES> planes_load4(const uint8_t* src, size_t P, const PlanesLoad& L) {
    Planes4<ES> v;
    if (L.vec) {
        SL_GLOBAL const uint8_t* const p = as_global(src) + L.e * (size_t)ES;
        if constexpr (ES == 1) {
            const uint32_t u = *(SL_GLOBAL const sl_u32u*)p;
#pragma unroll
            for (int k = 0; k < 4; ++k) v.lo[k] = (u >> (8 * k)) & 0xffu;
        } else if constexpr (ES == 2) {
            const sl_u32x2u u = *(SL_GLOBAL const sl_u32x2u*)p;
            v.lo[0] = u.x & 0xffffu; v.lo[1] = u.x >> 16; v.lo[2] = u.y & 0xffffu; v.lo[3] = u.y >> 16;
        } else if constexpr (ES == 4) {
            const sl_u32x4u u = *(SL_GLOBAL const sl_u32x4u*)p;
            v.lo[0] = u.x; v.lo[1] = u.y; v.lo[2] = u.z; v.lo[3] = u.w;
        } else {
            const sl_u32x4u a = *(SL_GLOBAL const sl_u32x4u*)p, b = *(SL_GLOBAL const sl_u32x4u*)(p + 16);
            v.lo[0] = a.x; v.hi[0] = a.y; v.lo[1] = a.z; v.hi[1] = a.w;
            v.lo[2] = b.x; v.hi[2] = b.y; v.lo[3] = b.z; v.hi[3] = b.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t e = L.e + k < P ? L.e + k : P - 1;
            SL_GLOBAL const uint8_t* const p = as_global(src) + e * (size_t)ES;
            if constexpr (ES == 1) v.lo[k] = *p;
            else if constexpr (ES == 2) v.lo[k] = *(SL_GLOBAL const sl_u16u*)p;
            else if constexpr (ES == 4) v.lo[k] = *(SL_GLOBAL const sl_u32u*)p;
            else { const sl_u32x2u u = *(SL_GLOBAL const sl_u32x2u*)p; v.lo[k] = u.x; v.hi[k] = u.y; }
        }
    }
    return v;
}

// nvalid (1 .. 4) adjacent output elements at byte address p
template <int ES>
__device__ __forceinline__ void planes_store4(uint8_t* p, int nvalid, const Planes4<ES>& v) {
    SL_GLOBAL uint8_t* const g = as_global(p);
    if (nvalid == 4) {
        if constexpr (ES == 1) {
            *(SL_GLOBAL sl_u32u*)g = v.lo[0] | (v.lo[1] << 8) | (v.lo[2] << 16) | (v.lo[3] << 24);
        } else if constexpr (ES == 2) {
            sl_u32x2u u; u.x = v.lo[0] | (v.lo[1] << 16); u.y = v.lo[2] | (v.lo[3] << 16);
            *(SL_GLOBAL sl_u32x2u*)g = u;
        } else if constexpr (ES == 4) {
            sl_u32x4u u; u.x = v.lo[0]; u.y = v.lo[1]; u.z = v.lo[2]; u.w = v.lo[3];
            *(SL_GLOBAL sl_u32x4u*)g = u;
        } else {
            sl_u32x4u a, b;
            a.x = v.lo[0]; a.y = v.hi[0]; a.z = v.lo[1]; a.w = v.hi[1];
            b.x = v.lo[2]; b.y = v.hi[2]; b.z = v.lo[3]; b.w = v.hi[3];
            *(SL_GLOBAL sl_u32x4u*)g = a;
            *(SL_GLOBAL sl_u32x4u*)(g + 16) = b;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < nvalid) {
                SL_GLOBAL uint8_t* const q = g + (size_t)k * ES;
                if constexpr (ES == 1) *q = (uint8_t)v.lo[k];
                else if constexpr (ES == 2) *(SL_GLOBAL sl_u16u*)q = (uint16_t)v.lo[k];
                else if constexpr (ES == 4) *(SL_GLOBAL sl_u32u*)q = v.lo[k];
                else { sl_u32x2u u; u.x = v.lo[k]; u.y = v.hi[k]; *(SL_GLOBAL sl_u32x2u*)q = u; }
            }
        }
    }
}

// ES: bytes per element (1, 2, 4, 8); MODE: kPlanesNearest, or kPlanesArea (ES = 1).  max_wh > 0: a resizing view (n x 5 windows, shrink
// = 1), else a crop / shrink view (n x 3 windows) -- block-uniform kernel arguments, one scalar branch each.  npx: patches per output
// row (crop / shrink), npatch: per plane (the host's upper bound for a resizing view).
template <int ES, int MODE>
static __global__ __launch_bounds__(kWG) void k_view_planes(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int c, int h, int w,
                                                            int oh, int ow, int npx, int npatch, const int32_t* __restrict__ windows,
                                                            int d_mask, int shrink, int max_wh, int max_ww) {
    static_assert(MODE == kPlanesNearest || ES == 1, "the area mode is the uint8 images' own");
    static_assert(kWG == 256 && kViewB == 64, "16 lanes x 4 elements per row, 16 rows per pass, 4 passes");
    __shared__ uint32_t s_el[(ES == 8 ? 2 : 1) * kPlanesPlane];
    __shared__ uint32_t s_idx[kPlanesIdx];                   // nearest: the index table (int); area of a resizing view: resize_taps' table
    const int tid = threadIdx.x;
    const int plane = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int tile = plane / c;
    const size_t P = (size_t)h * (size_t)w, PO = (size_t)oh * (size_t)ow;
    const uint8_t* const src = planes + (size_t)plane * P * ES;

    // the view of this plane's tile (block-uniform) and the source block of this patch -- or none: a resizing grid is sized for the largest window
    const bool resizing = max_wh > 0;
    const int s = resizing ? 1 : __builtin_amdgcn_readfirstlane(shrink);
    ViewPatch g;
    ResizeAxis ai, aj;
    if (resizing) {
        const ResizeTile vt(windows, tile, d_mask, h, w, oh, ow, max_wh, max_ww);
        if (!resize_patch(vt, patch, oh, ow, g, ai, aj)) return;
    } else {
        const ViewTile vt(windows, tile, d_mask, h, w, oh, ow, s);
        g = ViewPatch(vt, patch, npx, oh, ow, s);
    }

    // read side: the four loads of this lane, then the masked LDS writes
    PlanesLoad L[4];
    Planes4<ES> in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        L[q] = planes_load(g, w, P, tid, q);
        in[q] = planes_load4<ES>(src, P, L[q]);
    }
    if (MODE == kPlanesNearest) {
        if (tid < kPlanesIdx) {
            const int t = tid & (kViewB - 1);
            if (t < (tid < kViewB ? g.bh : g.bw))
                s_idx[tid] = (uint32_t)(resizing ? planes_index_resize(tid < kViewB ? ai : aj, t) : planes_index_shrink(g, s, tid));
        }
    } else if (resizing) {
        resize_taps(ai, aj, s_idx, tid);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p < L[q].n) {
                s_el[L[q].slot + p] = in[q].lo[p];
                if constexpr (ES == 8) s_el[kPlanesPlane + L[q].slot + p] = in[q].hi[p];
            }
        }
    }
    __syncthreads();

    // write side: output rows, 4 adjacent elements per lane (nothing below has a barrier)
    const PlanesLanes ln = planes_lanes(g.bw, tid);
    const int jl = ln.jl, bh = g.bh, bw = g.bw;
    if (jl >= bw) return;
    const int nvalid = min(4, bw - jl);
    uint8_t* const dst = out + (size_t)plane * PO * ES;
    const uint32_t D = MODE == kPlanesArea && resizing ? (uint32_t)ai.nw * (uint32_t)aj.nw : 1u;
    const float rden = 1.0f / (float)(2u * D);
    const int sh = s == 1 ? 0 : (s == 2 ? 2 : 4);            // log2 of the elements of a box
    for (int il = ln.il0; il < bh; il += ln.rows) {
        Planes4<ES> o;
        if constexpr (MODE == kPlanesNearest) {
            const int row = (int)s_idx[il];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int at = row + (int)s_idx[kViewB + min(jl + p, bw - 1)];
                o.lo[p] = s_el[at];
                if constexpr (ES == 8) o.hi[p] = s_el[kPlanesPlane + at];
            }
        } else if (!resizing) {                              // the box mean of the shrink: (S + s s / 2) >> (2 log2 s); s = 1: the element
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int at = g.a0 + il * g.ai + min(jl + p, bw - 1) * g.aj;
                uint32_t S = (uint32_t)(s * s) >> 1;
                for (int a = 0; a < s; ++a)
                    for (int b = 0; b < s; ++b) S += s_el[at + a * kViewPitch + b];
                o.lo[p] = S >> sh;
            }
        } else {                                             // the area average: resize_write's tap loops on one channel
            const uint32_t ta = s_idx[il];
            const int na = (int)(ta >> 8), ka = (int)(ta & 0xffu);
            const int elo_a = ai.at(il) * ai.nw, ehi_a = elo_a + ai.nw, c0_a = (ai.lo + ka) * ai.no;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int jj = min(jl + p, bw - 1);
                const uint32_t tb = s_idx[kViewB + jj];
                const int nb = (int)(tb >> 8), kb = (int)(tb & 0xffu);
                const int elo_b = aj.at(jj) * aj.nw, ehi_b = elo_b + aj.nw, c0_b = (aj.lo + kb) * aj.no;
                uint32_t S = 0;
                int ca = c0_a, ra = ka * ai.stride;
                for (int a = 0; a < na; ++a, ca += ai.no, ra += ai.stride) {
                    const uint32_t wa = (uint32_t)(min(ca + ai.no, ehi_a) - max(ca, elo_a));
                    int cb = c0_b, rb = ra + kb * aj.stride;
                    for (int b = 0; b < nb; ++b, cb += aj.no, rb += aj.stride) {
                        const uint32_t wb = (uint32_t)(min(cb + aj.no, ehi_b) - max(cb, elo_b));
                        S += __umul24(__umul24(wa, wb), s_el[rb]);       // weight <= D <= 2^22, S <= 255 D
                    }
                }
                o.lo[p] = resize_round(S, D, rden);
            }
        }
        planes_store4<ES>(dst + planes_out_elem(g, ow, il, jl) * (size_t)ES, nvalid, o);
    }
}

}  // namespace sl
