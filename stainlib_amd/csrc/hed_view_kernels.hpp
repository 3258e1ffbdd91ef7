// hed_view_kernels.hpp -- HED augmentation behind the apply pass, inside the view pass (an extension: a training loader normalises,
// HED-jitters, crops / flips and converts; the HED step used to be a full-tile uint8 image written and read back, most of it thrown away).
//
//   k_sums        the read-only half: the exact byte sum of the image an apply-pass route WOULD write (HedColorAugmenter's cutoff test
//                 needs the mean of its whole input before any pixel is transformed) -- 3 B/px read, one 64-bit atomic per workgroup
//   k_sums_applied  k_hed_fixup's decision on those sums
//   k_hed_view    k_view (view_kernels.hpp: view_body) with HedStage<1> between the truncation to bytes and the LDS write; the box
//                 shrink of sl_normalize_hed_view_shrink is view_body's (the stage runs per SOURCE pixel, the write side averages)
//
// Definition (include/stainlib_hip.h, sl_normalize_sums / sl_normalize_hed_view): with full[t] the image sl_normalize_view defines by its
// pointer pattern, sums[t] = the sum of the 3 h w bytes of full[t], and the view is taken of hed_applied[t] ? HED(full[t]) : full[t] with
// HED(.) = sl_hed_augment under a cutoff that never fails.  HED acts on the TRUNCATED bytes of its input, exactly what `stage` holds in
// px[], so the stage is k_hed<0>'s arithmetic statement for statement (hed.hip: the ln table, the folded A and b in binary64 then
// in_vgpr((float)...), the nested fmaf order, 255.0f * exp2f, pack_trunc_fast) and the result is that chain's bit for bit.
// The sweep of k_sums is the apply-pass frame (ApplyTile, GroupPipe, SL_FIT_FAILED; apply_px / apply_conc and the two casts chosen as
// k_apply and k_apply_jitter choose them) with a byte-sum accumulator where the store is.  The output chunk of a padding pixel (the last
// chunk when P % 4 != 0) or of a lane past the end (it re-reads the last chunk) is NOT zero, so the sum is masked by pixel.
#pragma once
#include "view_kernels.hpp"

namespace sl {

// ---- the HED stage of view_body ----------------------------------------------------------------------------------------------------------
template <>
struct HedStage<1> {
    float A[3][3], b[3];             // k_hed<0>'s folded constants of this tile, VGPR-resident
    const float* s_x;                // ln(max(v / 255, 1e-6)), binary32
    bool on;                         // hed_applied[tile] (block-uniform)

    __device__ __forceinline__ void init(int tid, int tile, const HedViewArgs* hv) {
        __shared__ float s_hx[256];
        static_assert(kWG == 256, "one table entry per thread");
        {
            const double v = tid == 0 ? 1e-6 : fmax((double)tid / 255.0, 1e-6);
            s_hx[tid] = (float)log(v);
        }
        s_x = s_hx;
        on = __builtin_amdgcn_readfirstlane(hv->applied[tile]) != 0;
        const double Ladj = log(1e-6);
        const double* sg = hv->sigma + 3 * (size_t)tile;
        const double* bs = hv->bias + 3 * (size_t)tile;
        const double kL2E = 1.4426950408889634;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double acc = 0;
                for (int j = 0; j < 3; ++j) acc += hv->H[3 * k + j] * (1.0 + sg[j]) * hv->R[3 * j + c];
                A[k][c] = in_vgpr((float)(acc * kL2E));
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double acc = 0;
            for (int j = 0; j < 3; ++j) acc += bs[j] * hv->R[3 * j + c];
            b[c] = in_vgpr((float)(Ladj * acc * kL2E));
        }
    }

    // four packed pixels r | g << 8 | b << 16 (the truncated bytes of `full`) -> their HED bytes
    __device__ __forceinline__ void apply(uint32_t (&px)[4]) const {
        if (!on) return;
        float tv[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float x0 = s_x[px[p] & 0xffu], x1 = s_x[(px[p] >> 8) & 0xffu], x2 = s_x[(px[p] >> 16) & 0xffu];
            float l[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) l[ch] = fmaf(x2, A[2][ch], fmaf(x1, A[1][ch], fmaf(x0, A[0][ch], b[ch])));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) tv[3 * p + ch] = 255.0f * __builtin_amdgcn_exp2f(l[ch]);
        }
        const Chunk o = pack_trunc_fast(tv);
#pragma unroll
        for (int p = 0; p < 4; ++p) px[p] = chunk_pixel(o, p) & 0xffffffu;
    }
};

template <int DT, int LAYOUT, int MODE>
static __global__ __launch_bounds__(kWG) void k_hed_view(const uint8_t* __restrict__ rgb, void* __restrict__ out, int h, int w, int oh, int ow,
                                                         int npx, int npatch, const int32_t* __restrict__ windows, int d_mask, int shrink,
                                                         const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                         const double* M_tgt, const double* maxC_tgt, const double* __restrict__ alpha_beta,
                                                         double lam, float ylimf, TensorK fmt, HedViewArgs hv) {
    view_body<DT, LAYOUT, MODE, 1>(rgb, out, h, w, oh, ow, npx, npatch, windows, d_mask, shrink, M_src, maxC_src, M_tgt, maxC_tgt, alpha_beta, lam,
                                   ylimf, fmt, &hv);
}

// ---- the byte sums ---------------------------------------------------------------------------------------------------------------------
// the bytes of chunk cc that belong to pixels of the tile, as a udot4 operand per word: none for a lane past the end (cc >= c1)
__device__ __forceinline__ void pixel_mask(int cc, int c1, int P, uint32_t (&m)[3]) {
    const int nb = cc < c1 ? 3 * min(4, P - 4 * cc) : 0;             // 0, 3, 6, 9 or 12 bytes
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = max(0, min(4, nb - 4 * i));
        m[i] = k == 0 ? 0u : 0x01010101u >> (8 * (4 - k));
    }
}

// MODE: kView*, which pass `full` is.  One workgroup per (tile, part) of parts_for.
template <bool ALIGNED, int MODE>
static __global__ __launch_bounds__(kWG) void k_sums(const uint8_t* __restrict__ rgb, int P, int parts, const double* __restrict__ M_src,
                                                     const double* __restrict__ maxC_src, const double* M_tgt, const double* maxC_tgt,
                                                     const double* __restrict__ alpha_beta, double lam, float ylimf,
                                                     unsigned long long* __restrict__ sums) {
    __shared__ float2 s_tab[256];
    __shared__ unsigned long long s_sum;
    const int tid = threadIdx.x;
    if (MODE != kViewRaw) fill_gam_od_lut(s_tab);
    if (tid == 0) s_sum = 0;
    uint32_t bsum = 0;
    auto add = [&](const Chunk& o, int cc, int c1) {
        uint32_t m[3];
        pixel_mask(cc, c1, P, m);
        bsum = __builtin_amdgcn_udot4(o.w0, m[0], bsum, false);
        bsum = __builtin_amdgcn_udot4(o.w1, m[1], bsum, false);
        bsum = __builtin_amdgcn_udot4(o.w2, m[2], bsum, false);
    };
    // the source bytes of chunks [c0, c1) (c1 > c0): the raw route, and a tile whose fit failed
    auto source = [&](const uint8_t* src, size_t nbytes, int c0, int c1) {
        for (int c = c0 + tid; c < c1; c += kWG * kU) {
            Chunk in[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) in[u] = load_chunk_clamped<ALIGNED, true>(src, nbytes, c + u * kWG, c1);
#pragma unroll
            for (int u = 0; u < kU; ++u) add(in[u], c + u * kWG, c1);
        }
    };
    int tile;
    if constexpr (MODE == kViewRaw) {
        tile = blockIdx.x / parts;
        int g0, g1;
        group_span<1>(P, parts, blockIdx.x % parts, g0, g1);
        __syncthreads();
        if (g0 < g1) source(rgb + (size_t)tile * P * 3, (size_t)P * 3, g0, g1);
    } else {
        const ApplyTile<1> T(blockIdx.x, parts, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
        const ApplyK& K = T.K;
        tile = T.tile;
        JitterK J;
        if (MODE != kViewApply) {                                   // k_apply_jitter's constants
            const double sc = 1.0 / T.unit;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                J.al[i] = in_vgpr(uni((float)alpha_beta[4 * (size_t)T.tile + 2 * i]));
                J.be[i] = in_vgpr(uni((float)(alpha_beta[4 * (size_t)T.tile + 2 * i + 1] / (T.mct[i] / T.mcs[i]) * sc)));
            }
            J.ylimf = in_vgpr(ylimf);
        }
        __syncthreads();
        if (T.empty()) {
        } else if (SL_FIT_FAILED(T)) {
            source(T.src, T.nbytes, T.g0, T.g1);
        } else if (MODE == kViewApply) {                            // k_apply: K.fast picks the lasso form and the cast
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                GroupPipe<kUApply, ALIGNED, 1> pipe(T, tid);
                for (int c = T.g0 + tid; c < T.g1; c += kWG * kUApply) {
                    pipe.advance(c);
#pragma unroll
                    for (int u = 0; u < kUApply; ++u) {
                        const int cc = c + u * kWG;
                        const Chunk& in = pipe.in[u][0];
                        float t[12];
#pragma unroll
                        for (int px = 0; px < 4; ++px) {
                            const float x = s_tab[chunk_byte(in, 3 * px + 0)].y, y = s_tab[chunk_byte(in, 3 * px + 1)].y,
                                        z = s_tab[chunk_byte(in, 3 * px + 2)].y;
                            float v[3];
                            apply_px<FAST>(K, x, y, z, v);
                            t[3 * px] = v[0]; t[3 * px + 1] = v[1]; t[3 * px + 2] = v[2];
                        }
                        add(FAST ? pack_trunc_fast(t) : pack_trunc_general(t), cc, T.g1);
                    }
                }
            };
            if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
        } else {                                                    // k_apply_jitter: g12 picks the lasso form, the cast saturates
            auto sweep = [&](auto fast_tag) {
                constexpr bool FAST = decltype(fast_tag)::value;
                GroupPipe<kUApply, ALIGNED, 1> pipe(T, tid);
                for (int c = T.g0 + tid; c < T.g1; c += kWG * kUApply) {
                    pipe.advance(c);
#pragma unroll
                    for (int u = 0; u < kUApply; ++u) {
                        const int cc = c + u * kWG;
                        const Chunk& in = pipe.in[u][0];
                        float t[12];
#pragma unroll
                        for (int px = 0; px < 4; ++px) {
                            const float2 er = s_tab[chunk_byte(in, 3 * px + 0)];      // x = gamma, y = od32
                            const float2 eg = s_tab[chunk_byte(in, 3 * px + 1)];
                            const float2 eb = s_tab[chunk_byte(in, 3 * px + 2)];
                            float c1, c2;
                            apply_conc<FAST>(K, er.y, eg.y, eb.y, c1, c2);
                            if (MODE == kViewJitAll) {
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
                        add(pack_trunc_fast(t), cc, T.g1);
                    }
                }
            };
            if (K.L.g12 >= 0.0f) sweep(std::true_type{}); else sweep(std::false_type{});
        }
    }
    // per lane a u32 (a part is ~8 Ki chunks: at most 32 chunks of 12 bytes per lane), then the wave, the workgroup, one atomic
    const unsigned long long ws = wave_sum((unsigned long long)bsum);
    if ((tid & 63) == 0) atomicAdd(&s_sum, ws);
    __syncthreads();
    if (tid == 0) atomicAdd(&sums[tile], s_sum);
}

// HedColorAugmenter's cutoff test on the exact mean (augmenter.py:291-293): k_hed_fixup's expression
static __global__ __launch_bounds__(kWG) void k_sums_applied(const unsigned long long* __restrict__ sums, int n, int P, double lo, double hi,
                                                             int32_t* __restrict__ applied) {
    const int tile = blockIdx.x * kWG + threadIdx.x;
    if (tile >= n) return;
    const double mean = (double)sums[tile] / (3.0 * (double)P) / 255.0;
    const bool ok = (lo <= mean) && (mean <= hi);
    applied[tile] = ok ? 1 : 0;
}

}  // namespace sl
