// post_kernels.hpp -- the post stage: a tone curve (one 256-byte table per tile) and additive noise (Philox4x32-10 per OUTPUT pixel) on the
// bytes a call writes (an extension: ToneCurveAugmenter, GaussianNoiseAugmenter; the definition and its 32-bit arithmetic are in
// post_math.hpp, bytes to bytes in integers).
//
//   k_post              the full-tile sweep on the group pipeline of the apply pass (GroupPipe, apply_pass.hpp), exactly as k_hsb: 3 B/px
//                       read, 3 B/px written as the uint8 image, or the model-ready tensor through cvt_chunk / store_group behind the stage
//   k_post_view         k_view (view_kernels.hpp: view_body) with PostStage on the WRITE side: between the four packed pixels of an output
//                       row (behind the box shrink) and their packing into a Chunk, where the tile, the pixel index and the number of
//                       pixels that exist are known.  The stage runs per OUTPUT pixel.
//   k_post_view_resize  the same on view_resize_body (view_resize_kernels.hpp), behind the area resample
//
// Per workgroup: the tile's table into LDS (256 lanes, one byte each; the identity when the call has no tables), filled behind the one
// barrier the kernel has anyway; the tile's four codes read once and made uniform, sq clamped (post_reduce_sq), the key schedule -- twenty
// words, block-uniform -- computed on the scalar side.  Per pixel: three table bytes, then -- under a block-uniform branch on sq != 0 -- ONE
// Philox call (ten rounds, two 32 x 32 -> 64 products each) for the three channels, one v_sad_u8 per word for its byte sum, one multiply,
// shift, add and clamp per channel.  Lanes that hold no output pixel and the pixels of a ragged last lane that do not exist compute and
// store nothing.
#pragma once
#include "view_resize_kernels.hpp"   // view_kernels.hpp, jitter_kernels.hpp (kDtU8), tensor_kernels.hpp and apply_pass.hpp through it
#include "post_math.hpp"

namespace sl {

struct PostViewArgs {
    const uint8_t* tables;           // n x 256 (device) or null: no tone curve
    const int32_t* codes;            // n x 4 (device) or null: no noise -- sq, k0, k1, mono per tile
};

struct PostStage {
    static constexpr bool kOn = true;
    const uint8_t* s_tone;           // LDS: the tile's table
    uint32_t ks[20];                 // the key schedule (uniform)
    int32_t sq;                      // reduced; 0: no noise
    bool mono;

    // s_tab: 256 bytes of LDS; the caller's next barrier stands between this fill and the first apply
    __device__ __forceinline__ void init(int tid, int tile, const PostViewArgs& a, uint8_t* s_tab) {
        s_tab[tid] = a.tables ? a.tables[256 * (size_t)tile + tid] : (uint8_t)tid;
        s_tone = s_tab;
        int32_t c[4] = {0, 0, 0, 0};
        if (a.codes) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = __builtin_amdgcn_readfirstlane(a.codes[4 * (size_t)tile + i]);
        }
        sq = post_reduce_sq(c[0]);
        mono = c[3] != 0;
        philox_schedule((uint32_t)c[1], (uint32_t)c[2], ks);
    }

    // the packed pixel r | g << 8 | b << 16 at pixel index p of the image the stage acts on
    __device__ __forceinline__ uint32_t pixel(uint32_t px, uint32_t p) const {
        const uint32_t t = (uint32_t)s_tone[px & 0xffu] | ((uint32_t)s_tone[(px >> 8) & 0xffu] << 8) | ((uint32_t)s_tone[(px >> 16) & 0xffu] << 16);
        return sq != 0 ? post_noise_pixel(t, p, ks, sq, mono) : t;
    }

    // four pixels at p0 .. p0 + 3, the first nvalid of which exist
    __device__ __forceinline__ void apply4(uint32_t (&px)[4], uint32_t p0, int nvalid) const {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nvalid) px[k] = pixel(px[k], p0 + (uint32_t)k);
    }

    // the hook of the view write sides (ViewNoPost's signature)
    __device__ __forceinline__ void apply(uint32_t (&px)[4], const ViewPatch& g, int il, int jl, int ow) const {
        uint32_t p0 = 0;
        const int nvalid = post_lane(g.i0, g.j0, g.bh, g.bw, ow, il, jl, p0);
        apply4(px, p0, nvalid);
    }
};

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_post_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                          int npx, int npatch, const int32_t* __restrict__ windows, int d_mask, int shrink,
                                                          const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                          const double* M_tgt, const double* maxC_tgt, const double* __restrict__ alpha_beta,
                                                          double lam, float ylimf, TensorK fmt, PostViewArgs pv) {
    __shared__ uint8_t s_tone[256];
    PostStage post;
    post.init(threadIdx.x, blockIdx.x / npatch, pv, s_tone);
    view_body<DT, LAYOUT, MODE, 0>(rgb, out, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam,
                                   ylimf, fmt, nullptr, post);
}

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_post_view_resize(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w,
                                                                 int oh, int ow, int npatch, const int32_t* __restrict__ windows, int d_mask,
                                                                 int max_wh, int max_ww, const double* __restrict__ M_src,
                                                                 const double* __restrict__ maxC_src, const double* M_tgt,
                                                                 const double* maxC_tgt, const double* __restrict__ alpha_beta, double lam,
                                                                 float ylimf, TensorK fmt, PostViewArgs pv) {
    __shared__ uint8_t s_tone[256];
    PostStage post;
    post.init(threadIdx.x, blockIdx.x / npatch, pv, s_tone);
    view_resize_body<DT, LAYOUT, MODE, 0>(rgb, out, h, w, oh, ow, npatch, windows, d_mask, max_wh, max_ww, M_src, maxC_src, M_tgt, maxC_tgt,
                                          alpha_beta, lam, ylimf, fmt, nullptr, post);
}

// ---- the full-tile sweep --------------------------------------------------------------------------------------------------------------
// k_hsb's frame (hsb_kernels.hpp), statement for statement, with the post stage as its map.  DT: kDtU8 (the uint8 image; LAYOUT and WIDE
// do not apply) or a tensor type.  One workgroup per (tile, part) of parts_for; a lane owns groups of G chunks, U = kUApply / G groups per
// trip with the next trip in flight (GroupPipe).  The pixel index of each of a chunk's four pixels is 4 chunk + p; lanes past the end
// re-read the last group and compute and store nothing, nor do the padding pixels of a ragged last chunk.
template <int DT, int LAYOUT, bool ALIGNED, bool WIDE>
static __global__ __launch_bounds__(kWG) void k_post(const uint8_t* __restrict__ rgb, void* __restrict__ out, int P, int parts, PostViewArgs pv,
                                                     TensorK fmt) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;
    typedef typename Elem<SDT>::type T;
    constexpr int G = group_chunks<SDT>(), U = kUApply / G;
    static_assert(U >= 1, "a group is at most kUApply chunks");
    __shared__ uint8_t s_tone[256];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts;
    PostStage post;
    post.init(tid, tile, pv, s_tone);
    __syncthreads();                                             // the table
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
                uint32_t px[4];
                view_unpack(pipe.in[u][j], px);
                const int left = P - 4 * cc;                     // the pixels of this chunk that exist (<= 0: a lane or chunk past the end)
                post.apply4(px, 4u * (uint32_t)cc, gg < g1 ? (left < 4 ? left : 4) : 0);
                Chunk o;
                o.w0 = px[0] | (px[1] << 24);
                o.w1 = (px[1] >> 8) | (px[2] << 16);
                o.w2 = (px[2] >> 16) | (px[3] << 8);
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
