// view_geometry.hpp -- the geometry of the view passes: the ONE decode of a window and the ONE clamp rule of the tree (Dihedral, ViewTile,
// ViewPatch for the crop / shrink views; ResizeTile, ResizeAxis, resize_patch for the resizing view), moved out of view_kernels.hpp and
// view_resize_kernels.hpp word for word so that k_view_planes (planes_view_kernels.hpp) and the CPU check of its lane arithmetic
// (tests/planes_view_geometry.cpp) take them from here.  Integers only, no AMDGPU builtin outside __HIP_DEVICE_COMPILE__, nothing of HIP
// included: a host compiler can include this header alone.  The kernels that used these pieces are unchanged instruction for
// instruction (tools/isa_diff.py).  Also here: patch_lanes, the lanes-per-row assignment of the affine write sides
// (tests/view_affine_geometry.cpp walks it; resize_write has the same lines written out: DESIGN 4.19.1).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SL_GEOM_FN __host__ __device__ __forceinline__
#else
#define SL_GEOM_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SL_GEOM_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // a block-uniform value read from memory: into a scalar register
#else
#define SL_GEOM_UNIFORM(x) (x)
#endif

namespace sl {

SL_GEOM_FN int geom_min(int a, int b) { return a < b ? a : b; }
SL_GEOM_FN int geom_max(int a, int b) { return a > b ? a : b; }

constexpr int kViewB = 64;                       // patch edge in pixels
constexpr int kViewPitch = kViewB + 1;           // LDS row pitch in dwords (odd: view_kernels.hpp)

// ---- the crop / shrink views (view_kernels.hpp) ---------------------------------------------------------------------------------------
// The view of one tile (block-uniform): the dihedral code as a transposition and two reversals, and the clamped window.  s: the shrink
// (1, 2 or 4; block-uniform, a kernel argument) -- the window is wh x ww BOXES of s x s source pixels at the pixel (y0, x0).
struct Dihedral {                                                                 // the ONE decode of a (masked) code: ViewTile, ResizeTile
    bool tr, ry, rx;
    SL_GEOM_FN explicit Dihedral(int d) {
        const int k = d & 3;
        tr = k & 1; ry = (k >> 1) & 1; rx = ((k >> 1) ^ k ^ (d >> 2)) & 1;
    }
};
struct ViewTile : Dihedral {
    int wh, ww, y0, x0;
    SL_GEOM_FN ViewTile(const int32_t* windows, int tile, int d_mask, int h, int w, int oh, int ow, int s)
        : Dihedral(SL_GEOM_UNIFORM(windows[3 * (size_t)tile + 2]) & d_mask) {
        wh = tr ? ow : oh; ww = tr ? oh : ow;                                     // the window, in boxes of s x s source pixels
        y0 = geom_max(0, geom_min(SL_GEOM_UNIFORM(windows[3 * (size_t)tile + 0]), h - s * wh));
        x0 = geom_max(0, geom_min(SL_GEOM_UNIFORM(windows[3 * (size_t)tile + 1]), w - s * ww));
    }
};
// One patch of the tile's output (i0, j0; bh x bw pixels, at most kViewB / s square), the source block it comes from (ys, xs; nu rows of
// nv pixels, s times the patch) and the affine map from output to LDS pixel: the s x s box of output pixel (il, jl) of the patch has its
// first pixel (lowest row and column) at LDS pixel a0 + il ai + jl aj -- at s = 1 the pixel itself.
struct ViewPatch {
    int i0, j0, bh, bw, nu, nv, ys, xs, a0, ai, aj;
    ViewPatch() = default;                                                        // (filled in by resize_patch below)
    SL_GEOM_FN ViewPatch(const ViewTile& t, int patch, int npx, int oh, int ow, int s) {
        constexpr int PITCH = kViewPitch;
        const int B = kViewB >> (s >> 1);                                         // kViewB / s for s = 1, 2, 4, without a division
        const bool tr = t.tr, ry = t.ry, rx = t.rx;
        i0 = (patch / npx) * B; j0 = (patch % npx) * B;                           // the patch, in output pixels
        bh = geom_min(B, oh - i0); bw = geom_min(B, ow - j0);
        const int u0 = tr ? j0 : i0;                                              // its rows and columns in the (flipped, turned) window
        const int nub = tr ? bw : bh;                                             // (in boxes)
        const int v0 = tr ? i0 : j0;
        const int nvb = tr ? bh : bw;
        nu = s * nub; nv = s * nvb;
        ys = t.y0 + s * (ry ? t.wh - u0 - nub : u0); xs = t.x0 + s * (rx ? t.ww - v0 - nvb : v0);   // the source block: nu rows of nv pixels
        const int su = ry ? -s * PITCH : s * PITCH, sv = rx ? -s : s;
        a0 = (ry ? (nu - s) * PITCH : 0) + (rx ? nv - s : 0);
        ai = tr ? sv : su; aj = tr ? su : sv;
    }
};

// ---- the write side of the affine views (and, written out, of the resizing view): lanes walk OUTPUT rows, 4 adjacent outputs per lane; lanes per row = the power
// of two that covers the patch's width bw (1 .. 16), so a narrow patch spreads its rows over all the lanes (affine_write,
// k_view_planes_affine; resize_write and k_view_planes have the same assignment written out).  Lane tid of `wg` takes the outputs jl .. jl + 3 of rows il0, il0 + rows, ...
struct PatchLanes { int il0, jl, rows; };
SL_GEOM_FN PatchLanes patch_lanes(int bw, int tid, int wg) {
    const int n4 = (bw + 3) >> 2;                                                // chunks of 4 outputs per output row, 1 .. 16
    const int lg = n4 <= 1 ? 0 : 32 - __builtin_clz((unsigned)(n4 - 1));         // log2 of the lanes per row: 0 .. 4
    PatchLanes l;
    l.il0 = tid >> lg; l.jl = 4 * (tid & ((1 << lg) - 1)); l.rows = wg >> lg;
    return l;
}

// ---- the resizing view (view_resize_kernels.hpp) -----------------------------------------------------------------------------------------
constexpr int kResizeMaxRatio = 16;              // wh <= 16 nu, ww <= 16 nv: at most 17 taps per axis
constexpr int kResizeMaxArea = 1 << 22;          // wh ww: 2 S + D < 2^31
constexpr long kResizeMaxProduct = 1L << 30;     // an output side times a window side: the scaled coordinates are 32-bit

// outputs per patch along an axis of `no` outputs from `nw` window pixels (nw <= 16 no): min(64, 63 no / nw), at least 3; does not grow with nw
SL_GEOM_FN int resize_patch_edge(int no, int nw) {
    if (no > nw) return 63L * no >= 64L * nw ? 64 : 63;
    return 63 * no / nw;
}
// the largest window side along an axis of `no` outputs under the call's bound
SL_GEOM_FN int resize_side_max(int no, int bound) { return (int)(16L * no < (long)bound ? 16L * no : (long)bound); }

// The view of one tile (block-uniform): the code (Dihedral), the clamped window and the patch edges along the window's two axes.
struct ResizeTile : Dihedral {
    int nu, nv, wh, ww, y0, x0, bu, bv;
    SL_GEOM_FN ResizeTile(const int32_t* windows, int tile, int d_mask, int h, int w, int oh, int ow, int max_wh, int max_ww)
        : Dihedral(SL_GEOM_UNIFORM(windows[5 * (size_t)tile + 2]) & d_mask) {
        const int32_t* const wv = windows + 5 * (size_t)tile;
        nu = tr ? ow : oh; nv = tr ? oh : ow;                                     // the outputs along the window's rows and columns
        wh = geom_max(1, geom_min(SL_GEOM_UNIFORM(wv[3]), resize_side_max(nu, max_wh)));
        ww = geom_max(1, geom_min(SL_GEOM_UNIFORM(wv[4]), resize_side_max(nv, max_ww)));
        y0 = geom_max(0, geom_min(SL_GEOM_UNIFORM(wv[0]), h - wh));
        x0 = geom_max(0, geom_min(SL_GEOM_UNIFORM(wv[1]), w - ww));
        bu = resize_patch_edge(nu, wh); bv = resize_patch_edge(nv, ww);
    }
};

// One OUTPUT axis of a patch (block-uniform): o0 + t, t = 0 .. nb - 1, are its outputs; the axis has `no` outputs from `nw` window pixels,
// runs backwards through the window when rev, and its source pixels start at window pixel `lo` (= LDS pixel 0 of that axis), `stride`
// dwords apart in LDS.
struct ResizeAxis {
    int o0, nb, no, nw, lo, stride;
    bool rev;
    // the output's index along the window axis
    SL_GEOM_FN int at(int t) const { return rev ? no - 1 - (o0 + t) : o0 + t; }
};

// Patch `patch` of the tile: false when the tile has fewer patches.  g: i0, j0, bh, bw and the source block ys, xs, nu x nv for view_read
// and view_stage; ai, aj: the patch's row and column axis.
SL_GEOM_FN bool resize_patch(const ResizeTile& t, int patch, int oh, int ow, ViewPatch& g, ResizeAxis& ai, ResizeAxis& aj) {
    const int bi = t.tr ? t.bv : t.bu, bj = t.tr ? t.bu : t.bv;                  // the patch edge along output rows and columns
    const int npi = (oh + bi - 1) / bi, npj = (ow + bj - 1) / bj;
    if (patch >= npi * npj) return false;
    g.i0 = (patch / npj) * bi; g.j0 = (patch % npj) * bj;
    g.bh = geom_min(bi, oh - g.i0); g.bw = geom_min(bj, ow - g.j0);
    ai.o0 = g.i0; ai.nb = g.bh; ai.no = oh; ai.nw = t.tr ? t.ww : t.wh; ai.rev = t.tr ? t.rx : t.ry; ai.stride = t.tr ? 1 : kViewPitch;
    aj.o0 = g.j0; aj.nb = g.bw; aj.no = ow; aj.nw = t.tr ? t.wh : t.ww; aj.rev = t.tr ? t.ry : t.rx; aj.stride = t.tr ? kViewPitch : 1;
    int n[2];
    ResizeAxis* const ax[2] = {&ai, &aj};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        ResizeAxis& a = *ax[e];
        const uint32_t first = (uint32_t)(a.rev ? a.no - a.o0 - a.nb : a.o0);    // the patch's outputs along the window axis: first .. first + nb - 1
        a.lo = (int)(first * (uint32_t)a.nw / (uint32_t)a.no);
        n[e] = (int)(((first + (uint32_t)a.nb) * (uint32_t)a.nw + (uint32_t)a.no - 1u) / (uint32_t)a.no) - a.lo;   // <= 64 (resize_patch_edge)
    }
    g.ys = t.y0 + (t.tr ? aj.lo : ai.lo); g.nu = geom_min(t.tr ? n[1] : n[0], kViewB);     // (the min: the LDS block, whatever the arithmetic above)
    g.xs = t.x0 + (t.tr ? ai.lo : aj.lo); g.nv = geom_min(t.tr ? n[0] : n[1], kViewB);
    g.a0 = 0; g.ai = ai.stride; g.aj = aj.stride;
    return true;
}

}  // namespace sl
