// hsb_kernels.hpp -- hue / saturation / brightness augmentation (an extension: the sibling of the HED augmenter; the definition and its
// 32-bit arithmetic are in hsb_math.hpp, bytes to bytes in integers).
//
//   k_hsb              the full-tile sweep on the group pipeline of the apply pass (GroupPipe, apply_pass.hpp): 3 B/px read, 3 B/px written
//                      as the uint8 image, or the model-ready tensor through cvt_chunk / store_group behind the map (no uint8 scratch)
//   k_hsb_view         k_view (view_kernels.hpp: view_body) with HedStage<2> between the truncation to bytes and the LDS write: the map
//                      runs per SOURCE pixel, the box shrink of the write side averages mapped pixels
//   k_hsb_view_resize  the same on view_resize_body (view_resize_kernels.hpp)
//
// There is no cutoff test, so no read-only sweep in front of the view: the stage needs the tile's three codes and nothing else.  A tile
// whose fit failed takes the stage on its own bytes (view_body's `raw` compute goes through `stage` like every other).
// Codes outside their ranges are reduced here (hsb_reduce_codes): dhq mod 6 Q, dsq and dvq clamped to +-Q.
#pragma once
#include "view_resize_kernels.hpp"   // view_kernels.hpp, jitter_kernels.hpp (kDtU8), tensor_kernels.hpp and apply_pass.hpp through it
#include "hsb_math.hpp"

namespace sl {

struct HsbViewArgs {
    const int32_t* codes;            // n x 3 (device): dhq, dsq, dvq per tile
};

// the reduced codes of a tile, block-uniform
__device__ __forceinline__ void hsb_tile_codes(const int32_t* __restrict__ codes, int tile, int32_t& dhq, int32_t& dsq, int32_t& dvq) {
    const int32_t c[3] = {__builtin_amdgcn_readfirstlane(codes[3 * (size_t)tile]), __builtin_amdgcn_readfirstlane(codes[3 * (size_t)tile + 1]),
                          __builtin_amdgcn_readfirstlane(codes[3 * (size_t)tile + 2])};
    hsb_reduce_codes(c, dhq, dsq, dvq);
}

// the four pixels of a chunk through the map
__device__ __forceinline__ Chunk hsb_chunk(const Chunk& in, int32_t dhq, int32_t dsq, int32_t dvq) {
    uint32_t px[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) px[p] = hsb_pixel(chunk_pixel(in, p) & 0xffffffu, dhq, dsq, dvq);
    Chunk o;
    o.w0 = px[0] | (px[1] << 24);
    o.w1 = (px[1] >> 8) | (px[2] << 16);
    o.w2 = (px[2] >> 16) | (px[3] << 8);
    return o;
}

// ---- the HSB stage of view_body / view_resize_body ---------------------------------------------------------------------------------------
template <>
struct HedStage<2> {
    int32_t dhq, dsq, dvq;

    __device__ __forceinline__ void init(int, int tile, const HsbViewArgs* hv) { hsb_tile_codes(hv->codes, tile, dhq, dsq, dvq); }

    // four packed pixels r | g << 8 | b << 16 (the truncated bytes of `full`) -> their HSB bytes
    __device__ __forceinline__ void apply(uint32_t (&px)[4]) const {
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = hsb_pixel(px[p], dhq, dsq, dvq);
    }
};

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_hsb_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                         int npx, int npatch, const int32_t* __restrict__ windows, int d_mask, int shrink,
                                                         const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                         const double* M_tgt, const double* maxC_tgt, const double* __restrict__ alpha_beta,
                                                         double lam, float ylimf, TensorK fmt, HsbViewArgs hv) {
    view_body<DT, LAYOUT, MODE, 2>(rgb, out, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam,
                                   ylimf, fmt, &hv);
}

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_hsb_view_resize(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w,
                                                                int oh, int ow, int npatch, const int32_t* __restrict__ windows, int d_mask,
                                                                int max_wh, int max_ww, const double* __restrict__ M_src,
                                                                const double* __restrict__ maxC_src, const double* M_tgt,
                                                                const double* maxC_tgt, const double* __restrict__ alpha_beta, double lam,
                                                                float ylimf, TensorK fmt, HsbViewArgs hv) {
    view_resize_body<DT, LAYOUT, MODE, 2>(rgb, out, h, w, oh, ow, npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                          alpha_beta, lam, ylimf, fmt, &hv);
}

// ---- the full-tile sweep --------------------------------------------------------------------------------------------------------------
// DT: kDtU8 (the uint8 image; LAYOUT and WIDE do not apply) or a tensor type.  One workgroup per (tile, part) of parts_for; a lane owns
// groups of G chunks (1 for uint8 and float32, 2 for the half types: store_group's 16-byte stores), U = kUApply / G groups per trip with
// the next trip in flight (GroupPipe).  Lanes past the end re-read the last group and store nothing; the padding pixels of a ragged last
// chunk are mapped like any other and dropped by store_chunk / store_group.
template <int DT, int LAYOUT, bool ALIGNED, bool WIDE>
static __global__ __launch_bounds__(kWG) void k_hsb(const uint8_t* __restrict__ rgb, void* __restrict__ out, int P, int parts,
                                                    const int32_t* __restrict__ codes, TensorK fmt) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;
    typedef typename Elem<SDT>::type T;
    constexpr int G = group_chunks<SDT>(), U = kUApply / G;
    static_assert(U >= 1, "a group is at most kUApply chunks");
    const int tid = threadIdx.x;
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts;
    int32_t dhq, dsq, dvq;
    hsb_tile_codes(codes, tile, dhq, dsq, dvq);
    const TensorK F = tensor_consts(fmt);
    int g0, g1;
    group_span<G>(P, parts, part, g0, g1);
    if (g0 >= g1) return;
    const size_t nbytes = (size_t)P * 3;
    const int nch = (P + 3) >> 2;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;
    uint8_t* const d_u8 = (uint8_t*)out + (size_t)tile * nbytes;
    T* const d_t = (T*)out + (size_t)tile * nbytes;

    GroupPipe<U, ALIGNED, G> pipe(src, nbytes, nch, g0, g1, tid);
    for (int g = g0 + tid; g < g1; g += kWG * U) {
        pipe.advance(g);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gg = g + u * kWG;
            float v[12 * G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int cc = G * gg + j;
                const Chunk o = hsb_chunk(pipe.in[u][j], dhq, dsq, dvq);
                if (TENSOR) {
                    cvt_chunk(o, F, v + 12 * j);
                } else {
                    if (gg < g1 && cc < nch) store_chunk<ALIGNED, true>(d_u8, nbytes, cc, o);
                }
            }
            if (TENSOR) {
                if (gg < g1) store_group<SDT, LAYOUT, WIDE>(d_t, P, gg, v);
            }
        }
    }
}

}  // namespace sl
