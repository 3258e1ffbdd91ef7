// tensor_kernels.hpp -- model-ready tensor output (an extension: the reference ends at normalizer.py:50 with a uint8 image).
//
//   k_to_tensor      u8 NHWC -> float32 / float16 / bfloat16, NCHW or NHWC, (b / 255 - mean) / std as ONE FMA per byte
//   k_apply_tensor   k_apply with the converter behind its truncating cast: the uint8 image is never written
//
// Definition (include/stainlib_hip.h, SlTensorFormat): for the TRUNCATED byte b the library produces today and channel c
//     v = fmaf((float)b, scale32[c], shift32[c])        one binary32 rounding
//     out = v converted to the output type, round-to-nearest-even
// so the fused kernel and "convert afterwards" agree to the bit: k_apply_tensor feeds the bytes of the packed chunk
// (pack_trunc_fast / pack_trunc_general, unchanged) to the same cvt_chunk / store_group as k_to_tensor.
//
// Roofline: HBM.  3 B read + 6 or 12 B written per pixel; the write side decides, and narrow stores are priced by
// issue, not by bytes: a lane owns a GROUP of G adjacent chunks (G = 1 for float32, 2 for the half types -- 8 pixels) so
// that every store of the wide path is 16 bytes: one per plane (NCHW), three per group (NHWC).
#pragma once
#include "apply_pass.hpp"

namespace sl {

constexpr int kDtF32 = 0, kDtF16 = 1, kDtBF16 = 2;      // SL_DTYPE_*
constexpr int kLayNCHW = 0, kLayNHWC = 1;               // SL_LAYOUT_*

struct TensorK { float sc[3], sh[3]; };                 // scale32 = 1 / (255 std), shift32 = -mean / std (rounded once on the host)

typedef uint32_t sl_u32x4 __attribute__((ext_vector_type(4)));

// The conversions of the output types, all round-to-nearest-even: v_cvt_f16_f32 under the default MODE (never v_cvt_pkrtz_f16_f32,
// which rounds toward zero), v_cvt_pk_bf16_f32 (RNE on gfx950; no builtin).  They never sit inside pack_trunc_fast's
// toward-zero window: that block is one asm volatile statement which restores the mode before it ends.
template <int DT> struct Elem;
template <> struct Elem<kDtF32> {
    typedef float type;
    static constexpr int per_word = 1;
    static __device__ __forceinline__ type one(float v) { return v; }
    static __device__ __forceinline__ uint32_t word(const float* v) { return __float_as_uint(v[0]); }
};
template <> struct Elem<kDtF16> {
    typedef _Float16 type;
    static constexpr int per_word = 2;
    // (in_vgpr: the value is the ROUNDED binary32 result of the FMA -- without the barrier the compiler folds the FMA and this cast into
    //  one v_fma_mixlo_f16, and the definition's two steps would rest on how that instruction rounds inside)
    static __device__ __forceinline__ type one(float v) { return (_Float16)in_vgpr(v); }
    static __device__ __forceinline__ uint32_t word(const float* v) {
        return (uint32_t)__builtin_bit_cast(uint16_t, one(v[0])) | ((uint32_t)__builtin_bit_cast(uint16_t, one(v[1])) << 16);
    }
};
template <> struct Elem<kDtBF16> {
    typedef uint16_t type;
    static constexpr int per_word = 2;
    static __device__ __forceinline__ uint32_t word(const float* v) {
        uint32_t r;
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(v[0]), "v"(v[1]));
        return r;
    }
    static __device__ __forceinline__ type one(float v) { const float p[2] = {v, v}; return (uint16_t)word(p); }
};

// chunks a lane owns per group: 16 bytes of one plane
template <int DT> constexpr int group_chunks() { return DT == kDtF32 ? 1 : 2; }

__device__ __forceinline__ TensorK tensor_consts(const TensorK& f) {
    TensorK K;
#pragma unroll
    for (int c = 0; c < 3; ++c) { K.sc[c] = in_vgpr(f.sc[c]); K.sh[c] = in_vgpr(f.sh[c]); }   // (an SGPR operand halves the VALU rate)
    return K;
}

// the 12 bytes of a chunk -> 12 values (v_cvt_f32_ubyte0..3 + one v_fma_f32 each), interleaved as the chunk is
__device__ __forceinline__ void cvt_chunk(const Chunk& in, const TensorK& K, float* v) {
    const uint32_t w[3] = {in.w0, in.w1, in.w2};
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = fmaf((float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu), K.sc[i % 3], K.sh[i % 3]);
}

// Group g of a tile (pixels [4 G g, 4 G (g + 1))), v[12 j + 3 px + c] of its chunk j, to the tile's output at `base` (element
// (3 i + c) P + p for NCHW, 3 (i P + p) + c for NHWC; base = the tile's first element).  WIDE (the host checked: `base` of every
// tile and every plane is 16-byte aligned, which makes P a multiple of 4 G -- no ragged group): 16-byte non-temporal stores only.
// Otherwise element stores, each one bounds-checked: nothing is written past a plane's or the tile's end.
template <int DT, int LAYOUT, bool WIDE>
__device__ __forceinline__ void store_group(typename Elem<DT>::type* base, int P, int g, const float* v) {
    typedef Elem<DT> E;
    constexpr int G = group_chunks<DT>(), NPX = 4 * G, PW = E::per_word;
    if (WIDE) {
        if (LAYOUT == kLayNCHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pl[NPX];
#pragma unroll
                for (int p = 0; p < NPX; ++p) pl[p] = v[3 * p + c];       // (12 j + 3 px + c = 3 (4 j + px) + c)
                sl_u32x4 o;
                o.x = E::word(pl); o.y = E::word(pl + PW); o.z = E::word(pl + 2 * PW); o.w = E::word(pl + 3 * PW);
                __builtin_nontemporal_store(o, (SL_GLOBAL sl_u32x4*)as_global(base + (size_t)c * P + (size_t)g * NPX));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float* s = v + 4 * PW * k;
                sl_u32x4 o;
                o.x = E::word(s); o.y = E::word(s + PW); o.z = E::word(s + 2 * PW); o.w = E::word(s + 3 * PW);
                __builtin_nontemporal_store(o, (SL_GLOBAL sl_u32x4*)as_global(base + (size_t)g * (3 * NPX) + (size_t)k * (4 * PW)));
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < NPX; ++p) {
            const size_t pix = (size_t)g * NPX + p;
            if (pix < (size_t)P) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    as_global(base)[LAYOUT == kLayNCHW ? (size_t)c * P + pix : 3 * pix + c] = E::one(v[3 * p + c]);
            }
        }
    }
}

// the groups [g0, g1) of one tile, plain conversion of the source bytes (k_to_tensor; the pass-through of k_apply_tensor)
// (A loop of its own beside GroupPipe of apply_pass.hpp: no prefetch -- there is no arithmetic to hide a load behind -- and
// U = 4 / G groups per trip, kU chunks issued back to back, not kUApply.)
template <int DT, int LAYOUT, bool ALIGNED, bool WIDE>
__device__ __forceinline__ void convert_sweep(const uint8_t* src, typename Elem<DT>::type* dst, int P, int g0, int g1, int tid,
                                              const TensorK& K) {
    constexpr int G = group_chunks<DT>(), U = 4 / G;           // 4 chunk loads per lane issued back to back (kU)
    const size_t nbytes = (size_t)P * 3;
    const int nch = (P + 3) >> 2;
    for (int g = g0 + tid; g < g1; g += kWG * U) {
        Chunk in[U][G];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int gg = g + u * kWG < g1 ? g + u * kWG : g1 - 1;          // lanes past the end re-read the last group (no predicated load)
#pragma unroll
            for (int j = 0; j < G; ++j) in[u][j] = load_chunk_clamped<ALIGNED, true>(src, nbytes, G * gg + j, nch);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float v[12 * G];
#pragma unroll
            for (int j = 0; j < G; ++j) cvt_chunk(in[u][j], K, v + 12 * j);
            if (g + u * kWG < g1) store_group<DT, LAYOUT, WIDE>(dst, P, g + u * kWG, v);
        }
    }
}

template <int DT, int LAYOUT, bool ALIGNED, bool WIDE>
static __global__ __launch_bounds__(kWG) void k_to_tensor(const uint8_t* __restrict__ rgb, void* __restrict__ out, int P, int parts, TensorK fmt) {
    typedef typename Elem<DT>::type T;
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts;
    const TensorK K = tensor_consts(fmt);
    int g0, g1;
    group_span<group_chunks<DT>()>(P, parts, part, g0, g1);
    if (g0 >= g1) return;
    convert_sweep<DT, LAYOUT, ALIGNED, WIDE>(rgb + (size_t)tile * 3 * P, (T*)out + (size_t)tile * 3 * P, P, g0, g1, threadIdx.x, K);
}

// k_apply (apply_pass.hpp) with the converter's store path behind the cast: the same constants, pipelined fetch (kUApply chunks per lane
// and trip), K.fast / general split, apply_px and pack_trunc_*.  A deliberate variant: it keeps its own prologue and its own copy of
// GroupPipe's loop.  On the shared frame float32 NCHW aligned + wide (the same instructions in another order) measured 0.5 % slower on
// an MI355X, outside the run-to-run spread; as written here all 24 instantiations are unchanged function for function (tools/isa_diff.py).
template <int DT, int LAYOUT, bool ALIGNED, bool WIDE>
static __global__ __launch_bounds__(kWG) void k_apply_tensor(const uint8_t* __restrict__ rgb, void* __restrict__ out, int P, int parts,
                                                             const double* __restrict__ M_src, const double* __restrict__ maxC_src,
                                                             const double* __restrict__ M_tgt, const double* __restrict__ maxC_tgt,
                                                             double lam, TensorK fmt) {
    typedef typename Elem<DT>::type T;
    constexpr int G = group_chunks<DT>(), U = kUApply / G;
    static_assert(U >= 1, "a group is at most kUApply chunks");
    __shared__ float s_od[256 * kRepl];
    fill_od_lut(s_od);
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts;
    const int tid = threadIdx.x;
    const uint32_t lane32 = tid & (kRepl - 1);

    ApplyK K;
    apply_consts(M_src + 6 * (size_t)tile, maxC_src + 2 * (size_t)tile, M_tgt, maxC_tgt, lam, K);
    const TensorK F = tensor_consts(fmt);
    __syncthreads();

    const size_t nbytes = (size_t)P * 3;
    const uint8_t* src = rgb + (size_t)tile * nbytes;
    T* dst = (T*)out + (size_t)tile * nbytes;
    const int nch = (P + 3) >> 2;
    int g0, g1;
    group_span<G>(P, parts, part, g0, g1);
    if (g0 >= g1) return;

    // k_apply's pass-through rule (a failed fit: NaN M_src, a non-positive maxC_src): the SOURCE bytes are converted.  (Block-uniform.)
    if (!(M_src[6 * (size_t)tile] == M_src[6 * (size_t)tile]) || !(maxC_src[2 * (size_t)tile] > 0.0) || !(maxC_src[2 * (size_t)tile + 1] > 0.0)) {
        convert_sweep<DT, LAYOUT, ALIGNED, WIDE>(src, dst, P, g0, g1, tid, F);
        return;
    }

    auto fetch = [&](int gg, int j) {
        const int gc = gg < g1 ? gg : g1 - 1;
        return load_chunk_clamped<ALIGNED, true>(src, nbytes, G * gc + j, nch);
    };
    auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        Chunk nxt[U][G];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < G; ++j) nxt[u][j] = fetch(g0 + tid + u * kWG, j);
        for (int g = g0 + tid; g < g1; g += kWG * U) {
            Chunk in[U][G];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    in[u][j] = nxt[u][j];
                    nxt[u][j] = fetch(g + (U + u) * kWG, j);
                }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int gg = g + u * kWG;
                float v[12 * G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    float t[12];
#pragma unroll
                    for (int px = 0; px < 4; ++px) {
                        const float x = lut(s_od, chunk_byte(in[u][j], 3 * px + 0), lane32);       // (od_of_pixel, written out:
                        const float y = lut(s_od, chunk_byte(in[u][j], 3 * px + 1), lane32);       //  through the call 4 of the 24
                        const float z = lut(s_od, chunk_byte(in[u][j], 3 * px + 2), lane32);       //  instantiations change)
                        float r[3];
                        apply_px<FAST>(K, x, y, z, r);
                        t[3 * px] = r[0]; t[3 * px + 1] = r[1]; t[3 * px + 2] = r[2];
                    }
                    const Chunk o = FAST ? pack_trunc_fast(t) : pack_trunc_general(t);       // today's bytes, by construction
                    cvt_chunk(o, F, v + 12 * j);
                }
                if (gg < g1) store_group<DT, LAYOUT, WIDE>(dst, P, gg, v);
            }
        }
    };
    if (K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
}

}  // namespace sl
