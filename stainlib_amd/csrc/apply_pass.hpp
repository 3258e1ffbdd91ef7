// apply_pass.hpp -- what the stand-alone apply-pass kernels share (k_apply, k_separate, k_apply_jitter; k_apply_tensor is the same
// frame in its own words, see tensor_kernels.hpp: one workgroup per (tile, part) of parts_for, a single streaming pass): the tile prologue, the failed-fit rule, the table lookups of a pixel and
// the group pipeline.  Each kernel is its constants, the loop skeleton of GroupPipe and its per-group arithmetic (DESIGN 4.1,
// *The apply-pass pipeline*).  k_apply itself is at the end.  The fused kernels' apply_sweep / augment_sweep (apply_kernels.hpp)
// are a different loop and do not come through here.
#pragma once
#include "apply_kernels.hpp"

namespace sl {

// the tile split of parts_for in groups of G chunks: part `part` of `parts` walks [g0, g1)
template <int G>
__device__ __forceinline__ void group_span(int P, int parts, int part, int& g0, int& g1) {
    const int nch = (P + 3) >> 2;
    const int ngr = (nch + G - 1) / G;
    const int span = (ngr + parts - 1) / parts;
    g0 = part * span;
    g1 = min(ngr, g0 + span);
}

// The prologue of one workgroup: its tile and part, the tile's statistics and the target's -- without a target (M_tgt == NULL; only
// k_separate and k_apply_jitter are ever launched so) the tile's OWN statistics stand in for it, ratio exactly 1 -- the per-tile
// constants (computed redundantly in binary64 by every lane), the tile's bytes and the part's span in groups of G chunks.
template <int G>
struct ApplyTile {
    int tile, nch, g0, g1;
    size_t nbytes;                  // of one uint8 tile
    const uint8_t* src;
    const double *Ms, *mcs, *Mt, *mct;
    ApplyK K;
    double unit;                    // 2^k of K

    __device__ __forceinline__ ApplyTile(int block, int parts, int P, const uint8_t* rgb, const double* M_src, const double* maxC_src,
                                         const double* M_tgt, const double* maxC_tgt, double lam) {
        tile = block / parts;
        Ms = M_src + 6 * (size_t)tile;
        mcs = maxC_src + 2 * (size_t)tile;
        Mt = M_tgt ? M_tgt : Ms;
        mct = M_tgt ? maxC_tgt : mcs;
        unit = apply_consts(Ms, mcs, Mt, mct, lam, K);
        nbytes = (size_t)P * 3;
        src = rgb + (size_t)tile * nbytes;
        nch = (P + 3) >> 2;
        group_span<G>(P, parts, block % parts, g0, g1);
    }
    __device__ __forceinline__ bool empty() const { return g0 >= g1; }
};

// A tile whose fit failed (empty tissue mask / degenerate covariance: M is NaN; a zero 99th-percentile concentration, which the
// reference divides by, normalizer.py:48) is passed through, each kernel in its own output form; the caller sees why in
// status[].  Block-uniform; T is the kernel's ApplyTile.  (A macro, expanded in the kernel's own `if`: as a member function
// returning the same expression, in any spelling tried, both unaligned k_apply and several k_apply_jitter instantiations lost an
// occupancy step -- tools/isa_diff.py.)
#define SL_FIT_FAILED(T) (!((T).Ms[0] == (T).Ms[0]) || !((T).mcs[0] > 0.0) || !((T).mcs[1] > 0.0))

// the optical densities of pixel px of a chunk, from the replicated table of fill_od_lut
__device__ __forceinline__ void od_of_pixel(const float* s_od, const Chunk& in, int px, uint32_t lane32, float& x, float& y, float& z) {
    x = lut(s_od, chunk_byte(in, 3 * px + 0), lane32);
    y = lut(s_od, chunk_byte(in, 3 * px + 1), lane32);
    z = lut(s_od, chunk_byte(in, 3 * px + 2), lane32);
}

// the pass-through of a failed fit for a uint8 image: chunks [c0, c1) copied as they are
template <bool ALIGNED>
__device__ __forceinline__ void copy_chunks(const uint8_t* src, uint8_t* dst, size_t nbytes, int c0, int c1, int tid) {
    for (int c = c0 + tid; c < c1; c += kWG) store_chunk<ALIGNED>(dst, nbytes, c, load_chunk<ALIGNED>(src, nbytes, c));
}

constexpr int kUApply = 2;  // chunks per lane and trip of the apply pass, with the following trip prefetched

// The software pipeline of the apply pass, for thread tid of a kWG workgroup walking the groups [T.g0, T.g1) of tile T (g1 > g0):
// a group is G adjacent chunks, a lane takes U groups per trip, and the next trip's chunks are requested before this trip's
// arithmetic (measured +5 % on k_apply).  Lanes past the end re-read the last group, and the absent second chunk of a ragged last
// group re-reads the last chunk: always a valid address, so no load is predicated and the arithmetic stays free of divergent
// regions (load_chunk_clamped).  Single pass: non-temporal loads.  A kernel's sweep is
//     GroupPipe<U, ALIGNED, G> pipe(T, tid);
//     for (int g = T.g0 + tid; g < T.g1; g += kWG * U) {
//         pipe.advance(g);
//         for u < U (unrolled): group gg = g + u * kWG with its chunks pipe.in[u][0 .. G)
//     }
// and it masks its own stores with gg < T.g1 (and chunk cc = G gg + j with cc < T.nch).
// (The arithmetic stays in the kernel's loop and is not handed over as a functor: as a functor, by value or by reference, the
// two-chunk groups of k_separate and k_apply_jitter lost one or two occupancy steps -- tools/isa_diff.py, DESIGN 4.1.  To see it
// again: give GroupPipe a `template <class Body> void run(int tid, Body body)` holding the loop skeleton and calling
// body(gg, in[u]) with `const Chunk (&in)[G]`, move a kernel's arithmetic into a [&] lambda, and compare separate.s / jitter.s.)
template <int U, bool ALIGNED, int G>
struct GroupPipe {
    const uint8_t* src;
    size_t nbytes;
    int nch, g1;
    Chunk in[U][G], nxt[U][G];
    __device__ __forceinline__ Chunk fetch(int gg, int j) const {
        if (G == 1) return load_chunk_clamped<ALIGNED, true>(src, nbytes, gg, g1);       // (groups are chunks: one clamp)
        const int gc = gg < g1 ? gg : g1 - 1;
        return load_chunk_clamped<ALIGNED, true>(src, nbytes, G * gc + j, nch);
    }
    // [k / G][k % G]: ONE unrolled loop level (with a nested pair the unaligned k_apply loses an occupancy step)
    __device__ __forceinline__ GroupPipe(const ApplyTile<G>& T, int tid) : src(T.src), nbytes(T.nbytes), nch(T.nch), g1(T.g1) {
#pragma unroll
        for (int k = 0; k < U * G; ++k) nxt[k / G][k % G] = fetch(T.g0 + tid + (k / G) * kWG, k % G);
    }
    // the same for a sweep without statistics (k_hsb): the tile's bytes and the part's span [g0, g1) as they are
    __device__ __forceinline__ GroupPipe(const uint8_t* tile, size_t tile_bytes, int tile_chunks, int g0, int g1_, int tid)
        : src(tile), nbytes(tile_bytes), nch(tile_chunks), g1(g1_) {
#pragma unroll
        for (int k = 0; k < U * G; ++k) nxt[k / G][k % G] = fetch(g0 + tid + (k / G) * kWG, k % G);
    }
    __device__ __forceinline__ void advance(int g) {           // in := the trip at g, nxt := the trip after it
#pragma unroll
        for (int k = 0; k < U * G; ++k) {
            in[k / G][k % G] = nxt[k / G][k % G];
            nxt[k / G][k % G] = fetch(g + (U + k / G) * kWG, k % G);
        }
    }
};

// k_apply (normalizer.py:46-50): the G = 1 instance.  HBM-bound: 3 B read + 3 B written per pixel (+ 12 B with PREQ, the values
// before the cast).
template <bool ALIGNED, bool PREQ>
static __global__ __launch_bounds__(kWG) void k_apply(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out,
                                               int P, int parts, const double* __restrict__ M_src,
                                               const double* __restrict__ maxC_src,
                                               const double* __restrict__ M_tgt,
                                               const double* __restrict__ maxC_tgt, double lam,
                                               float* __restrict__ prequant) {
    __shared__ float s_od[256 * kRepl];
    fill_od_lut(s_od);
    const int tid = threadIdx.x;
    const uint32_t lane32 = tid & (kRepl - 1);   // which LDS copy of the table this lane reads
    const ApplyTile<1> T(blockIdx.x, parts, P, rgb, M_src, maxC_src, M_tgt, maxC_tgt, lam);
    __syncthreads();
    if (T.empty()) return;
    uint8_t* dst = out + (size_t)T.tile * T.nbytes;

    if (SL_FIT_FAILED(T)) {
        copy_chunks<ALIGNED>(T.src, dst, T.nbytes, T.g0, T.g1, tid);
        return;
    }

    auto sweep = [&](auto fast_tag) {
        constexpr bool FAST = decltype(fast_tag)::value;
        GroupPipe<kUApply, ALIGNED, 1> pipe(T, tid);
        for (int c = T.g0 + tid; c < T.g1; c += kWG * kUApply) {
            pipe.advance(c);
#pragma unroll
            for (int u = 0; u < kUApply; ++u) {
                const int cc = c + u * kWG;
                float t[12];
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    float x, y, z, v[3];
                    od_of_pixel(s_od, pipe.in[u][0], px, lane32, x, y, z);
                    apply_px<FAST>(T.K, x, y, z, v);
                    t[3 * px] = v[0]; t[3 * px + 1] = v[1]; t[3 * px + 2] = v[2];
                    if (PREQ) {
                        const size_t pix = (size_t)cc * 4 + px;
                        if (cc < T.g1 && pix < (size_t)P) {
                            float* pq = prequant + ((size_t)T.tile * P + pix) * 3;
                            pq[0] = v[0]; pq[1] = v[1]; pq[2] = v[2];
                        }
                    }
                }
                const Chunk o = FAST ? pack_trunc_fast(t) : pack_trunc_general(t);
                if (cc < T.g1) store_chunk<ALIGNED, true>(dst, T.nbytes, cc, o);
            }
        }
    };
    if (T.K.fast) sweep(std::true_type{}); else sweep(std::false_type{});
}

}  // namespace sl
