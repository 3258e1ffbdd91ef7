// separate_kernels.hpp -- stain separation (an extension: the reference ends at normalizer.py:50 with the recombined image).
//
//   k_separate   k_apply's sweep (prologue, failed-fit rule and pipeline of apply_pass.hpp) with up to four outputs per pixel from ONE read of the tile and ONE lasso solve:
//                the normalised image, the haematoxylin-only and eosin-only images, the two concentration planes
//
// Definitions (include/stainlib_hip.h, SlSeparateOut), written so that "separate" equals "compose it yourself", bit for bit.
// For one tile let K be the ApplyK that apply_consts builds from the tile's (M_src, maxC_src) and the target (M_tgt, maxC_tgt), and
// c1, c2 the binary32 concentrations apply_px computes (apply_conc: carried scaled by 2^-k, in the lasso form K.fast selects).
//   norm      k_apply's bytes: 255 * exp2(fmaf(c1, q[0][ch], c2 * q[1][ch])), pack_trunc_fast when K.fast, else pack_trunc_general.
//   stain[i]  t = 255.0f * exp2f(c_i * K.q[i][ch]): one binary32 multiply, the hardware exp2, one multiply; the cast of norm.
//             Wherever sl_normalize_apply, called with the OTHER row of M_tgt replaced by zeros, makes the same K.fast decision, it
//             writes the same bytes: its q of the zeroed row is -0.0f, c >= 0, and fmaf(c1, q0, c2 * (-0.0f)) is c1 * q0 rounded
//             once.  The decisions agree whenever M_tgt has no negative entry (both fast, or both general through g12 < 0), whenever
//             g12 < 0, and for the image of a row that itself holds the negative entry.
//   conc      v = c_i * s_i with s_i = (float)(ratio_i * 2^k), ratio_i = maxC_tgt[i] / maxC_src[i]: one binary32 multiply -- the
//             normalised concentration of normalizer.py:48 -- converted to the output type round-to-nearest-even (Elem<DT>, with
//             its in_vgpr barrier for float16: the multiply and the cast are never one mixed-precision instruction).
//             Planar: plane i of tile t starts at element (2 t + i) P.
//   no target (M_tgt == NULL): every tile is reconstructed under its OWN stain matrix with ratio 1 -- M_tgt := M_src[tile],
//             maxC_tgt := maxC_src[tile], a pointer choice in the prologue.  The stain images are then the tile's own H and E
//             appearance and conc is the raw get_concentrations.
//   a tile whose fit failed (k_apply's block-uniform test: NaN M_src, a non-positive maxC_src): norm = the source bytes, both
//             stain images = 255 in every byte (zero concentration), conc = +0.
//
// Roofline: 3 B read and up to 9 B of images + 8 or 4 B of concentrations written per pixel, against 9 v_exp_f32 (quarter rate)
// and ~40 full-rate VALU instructions per pixel with every output on: more issue-bound than k_apply.  Stores: one
// dwordx3 per image and chunk, as k_apply; the concentration planes in 16-byte stores -- a lane owns a GROUP of G adjacent chunks
// (G = 1 for float32 and for no planes, 2 for the half types: 8 pixels), as in tensor_kernels.hpp.
#pragma once
#include "tensor_kernels.hpp"

namespace sl {

constexpr int kDtNone = -1;             // no concentration planes

struct SeparateOut {                    // device pointers, NULL = not wanted
    uint8_t* norm;
    uint8_t* stain[2];
    void* conc;
};

// Group g of a tile (pixels [4 G g, 4 G (g + 1))), v[i][p] = plane i of its pixel p, to the tile's planes at `base` (element i P + p).
// WIDE (the host checked: every plane of every tile starts on a 16-byte boundary, which makes P a multiple of 4 G -- no ragged
// group): one 16-byte non-temporal store per plane.  Otherwise element stores, each one bounds-checked: nothing is written past
// a plane's end.
template <int DT, bool WIDE>
__device__ __forceinline__ void store_conc(typename Elem<DT>::type* base, int P, int g, const float (&v)[2][4 * group_chunks<DT>()]) {
    typedef Elem<DT> E;
    constexpr int NPX = 4 * group_chunks<DT>(), PW = E::per_word;
    if (WIDE) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sl_u32x4 o;
            o.x = E::word(v[i]); o.y = E::word(v[i] + PW); o.z = E::word(v[i] + 2 * PW); o.w = E::word(v[i] + 3 * PW);
            __builtin_nontemporal_store(o, (SL_GLOBAL sl_u32x4*)as_global(base + (size_t)i * P + (size_t)g * NPX));
        }
    } else {
#pragma unroll
        for (int p = 0; p < NPX; ++p) {
            const size_t pix = (size_t)g * NPX + p;
            if (pix < (size_t)P) {
#pragma unroll
                for (int i = 0; i < 2; ++i) as_global(base)[(size_t)i * P + pix] = E::one(v[i][p]);
            }
        }
    }
}

// ALIGNED: every uint8 tile pointer of the call is 4-byte aligned with P a multiple of 4 (aligned dwordx3 accesses, as in k_apply)
// AND, with planes, every plane starts on a 16-byte boundary (the wide stores).  One flag for both: the tile shapes that miss one
// of the two but not the other are few, and a second flag would double the instantiations.
template <bool NORM, bool STAINS, int CDT, bool ALIGNED>
static __global__ __launch_bounds__(kWG) void k_separate(const uint8_t* __restrict__ rgb, SeparateOut out, int P, int parts,
                                                         const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                         const double* M_tgt, const double* maxC_tgt, double lam) {
    constexpr bool CONC = CDT != kDtNone;
    constexpr int SDT = CONC ? CDT : kDtF32;                    // the group shape (one chunk per lane when there are no planes)
    typedef typename Elem<SDT>::type T;
    constexpr int G = group_chunks<SDT>(), U = kUApply / G;
    static_assert(NORM || STAINS || CONC, "an output");
    static_assert(U >= 1, "a group is at most kUApply chunks");
    __shared__ float s_od[256 * kRepl];
    fill_od_lut(s_od);
    const int tid = threadIdx.x;
    const uint32_t lane32 = tid & (kRepl - 1);
    const ApplyTile<G> A(blockIdx.x, parts, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
    const ApplyK& K = A.K;
    float s[2] = {0.0f, 0.0f};
    if (CONC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) s[i] = in_vgpr(uni((float)(A.mct[i] / A.mcs[i] * A.unit)));
    }
    __syncthreads();
    if (A.empty()) return;

    const size_t nbytes = A.nbytes;
    const int nch = A.nch, g1 = A.g1;
    uint8_t* const d_norm = NORM ? out.norm + (size_t)A.tile * nbytes : nullptr;
    uint8_t* const d_st[2] = {STAINS && out.stain[0] ? out.stain[0] + (size_t)A.tile * nbytes : nullptr,
                              STAINS && out.stain[1] ? out.stain[1] + (size_t)A.tile * nbytes : nullptr};
    T* const d_conc = CONC ? (T*)out.conc + (size_t)A.tile * 2 * P : nullptr;

    if (SL_FIT_FAILED(A)) {                          // the source bytes, zero concentration
        const Chunk white{0xffffffffu, 0xffffffffu, 0xffffffffu};
        const float zero[2][4 * G] = {};
        for (int g = A.g0 + tid; g < g1; g += kWG) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int cc = G * g + j;
                if (cc >= nch) continue;
                if (NORM) store_chunk<ALIGNED>(d_norm, nbytes, cc, load_chunk<ALIGNED>(A.src, nbytes, cc));
                if (STAINS) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        if (d_st[i]) store_chunk<ALIGNED>(d_st[i], nbytes, cc, white);
                }
            }
            if (CONC) store_conc<SDT, ALIGNED>(d_conc, P, g, zero);
        }
        return;
    }

    auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        GroupPipe<U, ALIGNED, G> pipe(A, tid);
        for (int g = A.g0 + tid; g < g1; g += kWG * U) {
            pipe.advance(g);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int gg = g + u * kWG;
                const Chunk (&inu)[G] = pipe.in[u];
                float cv[2][4 * G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int cc = G * gg + j;
                    const bool live = gg < g1 && cc < nch;          // (cc = nch: the second chunk of a ragged last group)
                    float tn[12], th[12], te[12];
#pragma unroll
                    for (int px = 0; px < 4; ++px) {
                        float x, y, z, c1, c2;
                        od_of_pixel(s_od, inu[j], px, lane32, x, y, z);
                        apply_conc<FAST>(K, x, y, z, c1, c2);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            const float e2 = c2 * K.q[1][ch];            // shared by norm (apply_px's expression) and stain[1]
                            if (NORM) tn[3 * px + ch] = 255.0f * __builtin_amdgcn_exp2f(fmaf(c1, K.q[0][ch], e2));
                            if (STAINS) {
                                th[3 * px + ch] = 255.0f * __builtin_amdgcn_exp2f(c1 * K.q[0][ch]);
                                te[3 * px + ch] = 255.0f * __builtin_amdgcn_exp2f(e2);
                            }
                        }
                        if (CONC) { cv[0][4 * j + px] = c1 * s[0]; cv[1][4 * j + px] = c2 * s[1]; }
                    }
                    if (NORM) {
                        const Chunk o = FAST ? pack_trunc_fast(tn) : pack_trunc_general(tn);       // k_apply's bytes, by construction
                        if (live) store_chunk<ALIGNED, true>(d_norm, nbytes, cc, o);
                    }
                    if (STAINS) {                                        // either image alone: a wave-uniform branch
                        if (d_st[0]) {
                            const Chunk o = FAST ? pack_trunc_fast(th) : pack_trunc_general(th);
                            if (live) store_chunk<ALIGNED, true>(d_st[0], nbytes, cc, o);
                        }
                        if (d_st[1]) {
                            const Chunk o = FAST ? pack_trunc_fast(te) : pack_trunc_general(te);
                            if (live) store_chunk<ALIGNED, true>(d_st[1], nbytes, cc, o);
                        }
                    }
                }
                if (CONC) {
                    if (gg < g1) store_conc<SDT, ALIGNED>(d_conc, P, gg, cv);
                }
            }
        }
    };
    if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
}

}  // namespace sl
