// jitter_kernels.hpp -- stain jitter in the apply pass (an extension: the reference normalises, normalizer.py:46-50, and perturbs,
// augmenter.py:428-447, in two passes with a re-fit of the normalised image between them).
//
//   k_apply_jitter   k_apply's sweep (prologue, failed-fit rule and pipeline of apply_pass.hpp) with StainAugmentor.pop's affine map on the concentrations it holds in registers, written
//                    as the uint8 image or, through the converter of tensor_kernels.hpp, as the model-ready tensor
//
// Definition (include/stainlib_hip.h, sl_normalize_jitter), written so that the pass equals its two neighbours bit for bit.  For
// one tile let K be the ApplyK that apply_consts builds from the tile's (M_src, maxC_src) and the target (M_tgt, maxC_tgt),
// 2^k the unit apply_consts reports, ratio_i = maxC_tgt[i] / maxC_src[i], and c1, c2 the binary32 concentrations of apply_conc (carried
// scaled by 2^-k), in the lasso form K.L.g12 >= 0 selects -- k_stain_augment's rule, not K.fast.
//   jitter   al_i = (float)alpha_i, be_i = (float)(beta_i / ratio_i * 2^-k); c_i' = fmaf(c_i, al_i, be_i) on tissue pixels (the
//            luminosity test of the SOURCE pixel, is_tissue_f as k_stain_augment makes it), on every pixel when ALL, else c_i' = c_i:
//            alpha and beta act on the NORMALISED concentration c_i ratio_i, in the target's units
//   value    255.0f * exp2(fmaf(c1', K.q[0][ch], c2' * K.q[1][ch]))
//   cast     pack_trunc_fast always: the saturating truncation, np.clip(., 0, 255).astype(uint8) of augmenter.py:447 (c_i' may be
//            negative, the value then passes 255; it is never taken modulo 256 as k_apply's general path does)
//   tensor   the packed bytes through cvt_chunk / store_group unchanged: equal to "convert afterwards" bit for bit
//   no target (M_tgt == NULL): the tile's own statistics stand in as in k_separate, ratio_i == 1.0 exactly, and the bytes are
//            k_stain_augment's (the same statements on the same constants: q = -log2(e) * 1.0 * M * 2^k, be = beta / 1.0 * 2^-k)
//   alpha = 1, beta = 0: fmaf(c, 1, 0) = c, the bytes are k_apply's wherever its values stay inside [0, 255] (no negative target entry)
//   a tile whose fit failed (k_apply's block-uniform test): its source bytes, converted when a format is given
//
// Tables: ONE 256-entry table of {gamma, od32} pairs (2 KB of LDS; k_apply's own table is 1 KB), one ds_read_b64 per byte -- the
// pair of RowTab layout B without its 32 copies: the sweep keeps k_apply's 256-thread workgroups and occupancy (kRepl = 1 was
// measured fastest there).  The ALL instantiations read the od32 half alone.
// Roofline: HBM, 3 B read + 3 B (uint8) or 6 / 12 B (tensor) written per pixel; per pixel the tissue test adds 3 FMA-class
// instructions and a compare, the jitter 2 FMAs and 2 selects to k_apply's count.
#pragma once
#include "tensor_kernels.hpp"        // the converter; apply_pass.hpp (prologue, driver) through it

namespace sl {

constexpr int kDtU8 = -1;               // the uint8 image instead of a tensor

struct JitterK { float al[2], be[2], ylimf; };      // VGPR-resident; be_i scaled by 2^-k

__device__ __forceinline__ void fill_gam_od_lut(float2* s) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s[i] = make_float2((float)d_gamma[i], d_od_f32[i]);
}

// ALIGNED: every uint8 tile pointer the kernel touches is 4-byte aligned with P a multiple of 4 (rgb; and out for the uint8 image).
// WIDE (tensor only): store_group's 16-byte stores.  LAYOUT and WIDE are ignored for DT = kDtU8.
template <int DT, int LAYOUT, bool ALIGNED, bool WIDE, bool ALL>
static __global__ __launch_bounds__(kWG) void k_apply_jitter(const uint8_t* __restrict__ rgb, void* __restrict__ out, int P, int parts,
                                                             const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                             const double* M_tgt, const double* maxC_tgt,
                                                             const double* __restrict__ alpha_beta, double lam, float ylimf, TensorK fmt) {
    constexpr bool TENSOR = DT != kDtU8;
    constexpr int SDT = TENSOR ? DT : kDtF32;                  // the group shape (one chunk per lane for the uint8 image)
    typedef typename Elem<SDT>::type T;
    constexpr int G = group_chunks<SDT>(), U = kUApply / G;
    static_assert(U >= 1, "a group is at most kUApply chunks");
    __shared__ float2 s_tab[256];
    fill_gam_od_lut(s_tab);
    const int tid = threadIdx.x;
    const ApplyTile<G> A(blockIdx.x, parts, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
    const ApplyK& K = A.K;
    const double sc = 1.0 / A.unit;                            // 2^-k (a power of two: exact)
    JitterK J;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        J.al[i] = in_vgpr(uni((float)alpha_beta[4 * (size_t)A.tile + 2 * i]));
        J.be[i] = in_vgpr(uni((float)(alpha_beta[4 * (size_t)A.tile + 2 * i + 1] / (A.mct[i] / A.mcs[i]) * sc)));
    }
    J.ylimf = in_vgpr(ylimf);
    const TensorK F = tensor_consts(fmt);
    __syncthreads();
    if (A.empty()) return;

    const size_t nbytes = A.nbytes;
    const int nch = A.nch, g1 = A.g1;
    uint8_t* const d_u8 = (uint8_t*)out + (size_t)A.tile * nbytes;
    T* const d_t = (T*)out + (size_t)A.tile * nbytes;

    if (SL_FIT_FAILED(A)) {                          // the source bytes, converted when a format is given
        if (TENSOR) convert_sweep<SDT, LAYOUT, ALIGNED, WIDE>(A.src, d_t, P, A.g0, g1, tid, F);
        else copy_chunks<ALIGNED>(A.src, d_u8, nbytes, A.g0, g1, tid);
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
                float v[12 * G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int cc = G * gg + j;
                    float t[12];
#pragma unroll
                    for (int px = 0; px < 4; ++px) {
                        const float2 er = s_tab[chunk_byte(inu[j], 3 * px + 0)];      // x = gamma, y = od32
                        const float2 eg = s_tab[chunk_byte(inu[j], 3 * px + 1)];
                        const float2 eb = s_tab[chunk_byte(inu[j], 3 * px + 2)];
                        float c1, c2;
                        apply_conc<FAST>(K, er.y, eg.y, eb.y, c1, c2);
                        if (ALL) {
                            c1 = fmaf(c1, J.al[0], J.be[0]);
                            c2 = fmaf(c2, J.al[1], J.be[1]);
                        } else {
                            const bool tissue = is_tissue_f(er.x, eg.x, eb.x, J.ylimf);
                            c1 = tissue ? fmaf(c1, J.al[0], J.be[0]) : c1;
                            c2 = tissue ? fmaf(c2, J.al[1], J.be[1]) : c2;
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch)
                            t[3 * px + ch] = 255.0f * __builtin_amdgcn_exp2f(fmaf(c1, K.q[0][ch], c2 * K.q[1][ch]));
                    }
                    const Chunk o = pack_trunc_fast(t);        // values are >= 0; > 255 saturates = np.clip(.., 0, 255)
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
    };
    if (K.L.g12 >= 0.0f) sweep(std::true_type{}); else sweep(std::false_type{});      // (g12 is wave-uniform: vgpr(K.L))
}

}  // namespace sl
