// separate_view_kernels.hpp -- stain separation in the view pass (an extension: segmentation and nuclei-detection training crops, flips
// and turns every tile, often at half the magnification, BEHIND sl_stain_separate -- over three full-tile images and two full-tile float
// planes, most of whose pixels the crop throws away).
//
//   k_separate_view   per tile the window of what k_separate would write -- the normalised image, the haematoxylin-only and eosin-only
//                     images, the two concentration planes --, flipped and turned by the tile's dihedral code; the images as uint8 or as
//                     the model-ready tensor, optionally box-shrunk; the planes in their float type
//
// Definition (include/stainlib_hip.h, sl_stain_separate_view): "the same bits, elsewhere".  The pixel arithmetic is k_separate's
// statement for statement (separate_kernels.hpp: apply_conc on the ApplyK of apply_consts and the table of fill_od_lut, the shared
// e2 = c2 * K.q[1][ch], pack_trunc_fast / pack_trunc_general by the block-uniform K.fast, c_i * s_i for the planes, the failed-fit
// rule); the geometry, read side, LDS stage and image write side are k_view's pieces (view_kernels.hpp: ViewTile, ViewPatch, view_read,
// view_stage, view_write), called as they are.  A dihedral transform is a permutation of elements, of bytes as of floats.
//
// Shape: ONE workgroup = one tile and one patch of the OUTPUT, as in k_view.  What differs from every view kernel before it: there are
// several outputs per pixel, and one of them is not bytes.
//   solve    ONE lasso solve per source pixel of the patch's block: a lane's 4 chunks = 16 pixels, their (c1, c2) kept in 32 registers.
//   rounds   one per wanted output, through ONE s_px (16 640 B, so that several workgroups stay resident per CU): the round's dword per
//            pixel -- the three truncated bytes of that image, or the raw bits of one plane's binary32 value -- is staged in SOURCE
//            orientation, barrier, the write side walks OUTPUT rows, barrier.  Which outputs are wanted is a block-uniform test of the
//            output pointers around a round (a scalar branch); only the image type / layout and the plane type are template parameters:
//            7 x 4 = 28 instantiations.  The rounds are ONE loop that is not unrolled: a code object holds each write side once.
//   planes   view_write_plane: the same affine map (a0, ai, aj) as the image write side, 4 adjacent output pixels per lane -> 16 B
//            (float32) or 8 B (half types) per lane at element alignment, the ragged last lane of a row element by element; the
//            conversion is Elem<CDT>'s (round to nearest even, float16 behind its in_vgpr barrier), as in store_conc.  No shrink: a mean
//            of floats is another definition (the host refuses shrink != 1 with planes).
//   failed   a tile whose fit failed (SL_FIT_FAILED, block-uniform): the rounds stage the source pixels (norm), 0xffffff (h, e), +0.
// Roofline: per SOURCE pixel of the window 3 B read, 9 v_exp_f32 and ~40 VALU as k_separate, plus per round one LDS write and one read;
// issue-bound like k_separate, the five rounds' ten barriers on top.
#pragma once
#include "separate_kernels.hpp"
#include "view_kernels.hpp"

namespace sl {

struct SeparateViewOut {                // device pointers, NULL = not wanted
    void* img[3];                       // norm, haematoxylin only, eosin only: uint8 n x oh x ow x 3, or the tensor of the call's format
    void* conc;                         // n x 2 x oh x ow elements of the plane type
};

// ---- write side of one concentration plane: the raw binary32 bits in s_px (SOURCE orientation) to `base`, the plane's first element
// ---- (oh x ow elements of CDT), along output rows: view_write_s<.., 1>'s walk and ragged rule with one element per pixel
template <int CDT>
__device__ __forceinline__ void view_write_plane(const ViewPatch& g, const uint32_t* s_px, typename Elem<CDT>::type* base, int ow,
                                                 int lr, int lc) {
    typedef Elem<CDT> E;
    const int i0 = g.i0, j0 = g.j0, bh = g.bh, bw = g.bw, a0 = g.a0, ai = g.ai, aj = g.aj;
    const int jl = 4 * lc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int il = 16 * q + lr;
        const int row = a0 + min(il, bh - 1) * ai;
        float v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = __uint_as_float(s_px[row + min(jl + p, bw - 1) * aj]);
        const int nvalid = min(4, bw - jl);
        if (il < bh && nvalid > 0) {
            typename E::type* const p = base + (size_t)(i0 + il) * ow + (j0 + jl);
            if (nvalid == 4) {
                if (CDT == kDtF32) {
                    sl_u32x4u o; o.x = E::word(v); o.y = E::word(v + 1); o.z = E::word(v + 2); o.w = E::word(v + 3);
                    *(SL_GLOBAL sl_u32x4u*)as_global((uint8_t*)p) = o;
                } else {
                    sl_u32x2u o; o.x = E::word(v); o.y = E::word(v + 2);
                    *(SL_GLOBAL sl_u32x2u*)as_global((uint8_t*)p) = o;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < nvalid) as_global(p)[k] = E::one(v[k]);
            }
        }
    }
}

// DT: kDtU8 or a tensor type; LAYOUT: tensor only (the three images); CDT: kDtNone or the planes' type.  npx: patches per output row,
// npatch: per tile.  shrink: 1, 2, 4 (the images; 1 with planes).
template <int DT, int LAYOUT, int CDT>
static __global__ __launch_bounds__(kWG) void k_separate_view(const uint8_t* __restrict__ rgb, SeparateViewOut out, int h, int w, int oh,
                                                              int ow, int npx, int npatch, const int32_t* __restrict__ windows,
                                                              int d_mask, int shrink, const double* __restrict__ M_src,
                                                              const double* __restrict__ maxC_src, const double* M_tgt,
                                                              const double* maxC_tgt, double lam, TensorK fmt) {
    constexpr int B = kViewB, PITCH = kViewPitch;
    constexpr bool CONC = CDT != kDtNone;
    constexpr int SDT = CONC ? CDT : kDtF32;
    typedef typename Elem<SDT>::type T;
    static_assert(kWG == 256 && B == 64, "16 lanes x 4 pixels per row, 16 rows per pass, 4 passes");
    __shared__ float s_od[256 * kRepl];
    __shared__ uint32_t s_px[B * PITCH];
    fill_od_lut(s_od);
    const int tid = threadIdx.x;
    const uint32_t lane32 = tid & (kRepl - 1);
    const int lr = tid >> 4, lc = tid & 15;
    const int tile = blockIdx.x / npatch, patch = blockIdx.x % npatch;
    const int P = h * w;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* const src = rgb + (size_t)tile * nbytes;

    // the view of this tile (block-uniform), the source block of this patch and the four chunks of this lane
    const int s = __builtin_amdgcn_readfirstlane(shrink);
    const ViewTile vt(windows, tile, d_mask, h, w, oh, ow, s);
    const ViewPatch g(vt, patch, npx, oh, ow, s);
    Chunk in[4];
    view_read(g, src, nbytes, w, lr, lc, in);

    const ApplyTile<1> A(blockIdx.x, npatch, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
    const ApplyK& K = A.K;
    float sc[2] = {0.0f, 0.0f};
    if (CONC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) sc[i] = in_vgpr(uni((float)(A.mct[i] / A.mcs[i] * A.unit)));
    }
    __syncthreads();                                                // the table

    // One round per wanted output (r: 0 norm, 1 haematoxylin only, 2 eosin only, 3 / 4 the planes) -- value(r, q, px): the round's dword
    // of the four pixels of this lane's chunk q.  The loop is not unrolled: each write side once per body.
    auto rounds = [&](auto value) {
#pragma nounroll
        for (int r = 0; r < (CONC ? 5 : 3); ++r) {
            if (r < 3 ? out.img[r] == nullptr : out.conc == nullptr) continue;      // (block-uniform)
            int q = 0;                                              // (view_stage calls its functor once per chunk, in order)
            int rl = lr, cl = lc;                                   // (the lane's place, new to the compiler in every round: the two sides'
            asm volatile("" : "+v"(rl), "+v"(cl));                  //  addresses are a few integer instructions, not registers held across rounds)
            view_stage(g, s_px, rl, cl, in, [&](const Chunk&, uint32_t (&px)[4]) { value(r, q, px); ++q; });
            __syncthreads();
            if (r < 3) view_write<DT, LAYOUT>(g, s_px, out.img[r], tile, oh, ow, fmt, rl, cl, s);
            else if (CONC) view_write_plane<SDT>(g, s_px, (T*)out.conc + ((size_t)tile * 2 + (r - 3)) * ((size_t)oh * ow), ow, rl, cl);
            __syncthreads();                                        // s_px is the next round's
        }
    };

    if (SL_FIT_FAILED(A)) {                                         // the source bytes, white, zero concentration
        rounds([&](int r, int q, uint32_t (&px)[4]) {
            uint32_t raw[4];
            view_unpack(in[q], raw);
#pragma unroll
            for (int p = 0; p < 4; ++p) px[p] = r == 0 ? raw[p] : (r < 3 ? 0xffffffu : 0u);
        });
        return;
    }

    auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        // ONE lasso solve per source pixel: pixel px of chunk q (a lane past the block holds a re-read chunk's; the stage masks it)
        float c1[4][4], c2[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                float x, y, z;
                od_of_pixel(s_od, in[q], px, lane32, x, y, z);
                apply_conc<FAST>(K, x, y, z, c1[q][px], c2[q][px]);
            }
        // (The constants of a round go through an empty volatile asm: c1, c2 are the same in every round, and with constants the
        //  compiler can see through it computes all five rounds' products in front of the loop and keeps them -- 256 registers.)
        rounds([&](int r, int q, uint32_t (&px)[4]) {
            float q0[3], q1[3], s0 = sc[0], s1 = sc[1];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                q0[ch] = K.q[0][ch]; q1[ch] = K.q[1][ch];
                asm volatile("" : "+v"(q0[ch]), "+v"(q1[ch]));
            }
            asm volatile("" : "+v"(s0), "+v"(s1));
            if (r < 3) {                                            // k_separate's expressions, the truncated bytes
                float t[12];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float e2 = c2[q][p] * q1[ch];         // shared by norm (apply_px's expression) and stain[1]
                        const float a = r == 0 ? fmaf(c1[q][p], q0[ch], e2) : (r == 1 ? c1[q][p] * q0[ch] : e2);
                        t[3 * p + ch] = 255.0f * __builtin_amdgcn_exp2f(a);
                    }
                }
                view_unpack(FAST ? pack_trunc_fast(t) : pack_trunc_general(t), px);
            } else {                                                // c_i * s_i: one binary32 multiply, its raw bits
#pragma unroll
                for (int p = 0; p < 4; ++p) px[p] = __float_as_uint(r == 3 ? c1[q][p] * s0 : c2[q][p] * s1);
            }
        });
    };
    if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
}

}  // namespace sl
