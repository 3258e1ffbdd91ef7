// lab_view_kernels.hpp -- the Lab family in the one-pass loader: the Reinhard / luminosity map fused with the crop, flip, quarter turn and
// tensor conversion of the view pass (an extension: behind k_lab_map / k_slab_map a loader otherwise re-reads a full-tile uint8 image whose
// pixels outside the window went through the library's most expensive per-pixel arithmetic for nothing).
//
//   k_lab_view   per tile the window of the image k_lab_map<0>, k_lab_map<1> (lab.hip) or k_slab_map (slide_lab.hip) would write, flipped
//                and turned by the tile's dihedral code, as the uint8 image or the model-ready tensor
//
// Definition (include/stainlib_hip.h, sl_reinhard_view): sl_normalize_view's "the same bits, elsewhere" with that image as `full`.  The
// geometry, the read side, the LDS stage and the write side are view_kernels.hpp's pieces; the arithmetic between the read side and the
// stage is lab_map_chunk on the workgroup's LDS copies of the tables, as k_lab_map / k_slab_map call it.
//
// Shape: the Lab map needs ~14 KB of LDS tables before its first pixel (LabCbrtInv 10 240 B, g 512 B, yf 1 KB, ad and bd 2 KB) -- more than
// the 12 KB of pixels in a 64 x 64 patch -- so ONE workgroup = one tile and a RUN of kLabViewRun consecutive patches of that tile behind one
// table fill (4 patches = 16 Ki pixels, lab_parts' floor per fill).  The next patch's four loads are issued before the current patch's
// write side.  LDS: the tables and s_px (16 640 B), ~31 KB per workgroup.
//
// Tables: (tabs, stride_bytes) -- per-tile calls pass the workspace's LabTileTabs array and sizeof(LabTileTabs), pooled calls the slide's
// one LabMapTabs in the state and 0.  status (pooled; may be NULL): anything but SL_TILE_OK and every window comes from its source bytes,
// as k_slab_map copies the tiles through.
//
// shrink (sl_reinhard_view_shrink and its siblings; block-uniform, 1 / 2 / 4): view_kernels.hpp's box shrink through the shared pieces --
// a patch is 64 / shrink output pixels square, its source block still at most 64 x 64, and view_write averages; nothing of it is restated.
#pragma once
#include "../../include/stainlib_hip.h"        // SL_TILE_OK
#include "lab_device.hpp"
#include "view_kernels.hpp"

namespace sl {

constexpr int kLabViewRun = 4;                   // patches per workgroup and table fill

// DT: kDtU8 or a tensor type; LAYOUT: tensor only; AB_TABLES: lab_map_chunk's (true: the Reinhard map and every pooled map, false: the
// per-tile luminosity map).  npx: patches per output row, npatch: per tile, nrun: workgroups per tile = ceil(npatch / kLabViewRun).
// p_out (per-tile luminosity; may be NULL): p_out[tile] = the tile's LabTileTabs::p, as k_lab_map<1> reports it.
template <int DT, int LAYOUT, bool AB_TABLES>
static __global__ __launch_bounds__(kWG) void k_lab_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                         int npx, int npatch, int nrun, const int32_t* __restrict__ windows, int d_mask,
                                                         int shrink, const LabMapTabs* __restrict__ tabs, size_t stride_bytes,
                                                         const double* __restrict__ status, int mask_background, double thr,
                                                         double* __restrict__ p_out, TensorK fmt) {
    static_assert(kWG == 256 && kViewB == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes; one table entry per thread");
    __shared__ LabCbrtInv s_t;
    __shared__ uint16_t s_g[256];
    __shared__ uint32_t s_yf[256];
    __shared__ int s_ad[256], s_bd[256];
    __shared__ uint32_t s_px[kViewB * kViewPitch];
    __shared__ int s_lim[kWG / 64];
    const int tid = threadIdx.x;
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / nrun, run = blockIdx.x % nrun;
    const int p0 = run * kLabViewRun, p1 = min(npatch, p0 + kLabViewRun);
    const size_t nbytes = (size_t)h * w * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;
    const bool through = status && (int)status[0] != SL_TILE_OK;          // block-uniform: unusable statistics, the source bytes
    const LabMapTabs& tt = *(const LabMapTabs*)((const char*)tabs + (size_t)tile * stride_bytes);
    if (!through) {
        s_t.fill();
        s_g[tid] = tt.g[tid];
        s_yf[tid] = tt.yf[tid];
        if (AB_TABLES) { s_ad[tid] = tt.ad[tid]; s_bd[tid] = tt.bd[tid]; }
    }
    if (p_out && run == 0 && tid == 0) p_out[tile] = static_cast<const LabTileTabs&>(tt).p;
    l8_limit_begin(thr, s_lim);                                           // l8_limit(thr), one test per thread
    const LabBackground bg = lab_background();
    const bool mask_bg = mask_background != 0;

    const int s = __builtin_amdgcn_readfirstlane(shrink);
    const ViewTile vt(windows, tile, d_mask, h, w, oh, ow, s);
    ViewPatch g(vt, p0, npx, oh, ow, s);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);
    __syncthreads();                                                      // the tables
    const int lim = l8_limit_end(s_lim);
    for (int p = p0; p < p1; ++p) {
        if (through) {
            view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) { view_unpack(c, px); });
        } else {
            view_stage(g, s_px, lr, lc, in, [&](const Chunk& c, uint32_t (&px)[4]) {
                view_unpack(lab_map_chunk<AB_TABLES>(s_t, s_g, s_yf, s_ad, s_bd, c, mask_bg, lim, bg), px);
            });
        }
        const ViewPatch cur = g;
        if (p + 1 < p1) {                                                 // the next patch's loads, in flight across this one's write side
            g = ViewPatch(vt, p + 1, npx, oh, ow, s);
            view_read(g, src, nbytes, w, lr, lc, in);
        }
        __syncthreads();
        view_write<DT, LAYOUT>(cur, s_px, out, tile, oh, ow, fmt, lr, lc, s);
        __syncthreads();                                                  // s_px is the next patch's
    }
}

}  // namespace sl
