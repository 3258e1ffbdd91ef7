// sweep_pipeline.hpp -- the canonical hand-scheduled software pipeline the per-pixel sweeps walk a tile with (the deliberate
// variants keep loops of their own and point here), and the two small pieces that go with it (the in-range test of a ragged
// trip, the twelve table gathers of a chunk).
#pragma once
#include "apply_kernels.hpp"
#include "sweep_lookahead.hpp"
#include <type_traits>

namespace sl {

// Pixel px of chunk cc lies inside the part [.., c1) and inside the tile of P pixels.  Only a ragged (TAIL) trip asks.
template <bool ALIGNED>
__device__ __forceinline__ bool in_tile(int cc, int px, int c1, int P) {
    return (cc < c1) & (ALIGNED | ((size_t)cc * 4 + px < (size_t)P));
}

// The twelve table entries of a chunk's bytes: {gamma, od32} rows (layout B), or od32 alone.
struct GatherGamOd { float2 v[12]; };
struct GatherOd { float v[12]; };
template <class TR>
__device__ __forceinline__ GatherGamOd gather_gam_od(const TR& T, const Chunk& ch) {
    GatherGamOd g;
#pragma unroll
    for (int i = 0; i < 12; ++i) g.v[i] = T.gam_odf(T.addr(ch, i));
    return g;
}
template <class TR>
__device__ __forceinline__ GatherOd gather_od(const TR& T, const Chunk& ch) {
    GatherOd g;
#pragma unroll
    for (int i = 0; i < 12; ++i) g.v[i] = T.odf(T.addr(ch, i));
    return g;
}

// Chunks [c0, c1) of one tile of P pixels at `src`, thread t of `nthreads` cooperating ones.  Each lane keeps kTrip chunks plus
// the next trip's kTrip chunks in flight; the table gathers of a chunk (`gather(chunk)`) are issued one chunk ahead of its
// arithmetic, which sits between two scheduling barriers.  The full trips run with a compile-time TAIL = false; at most one
// ragged trip per wave runs with TAIL = true, where lanes past the end hold a re-read of the last chunk (load_chunk_clamped)
// and the arithmetic masks its results with in_tile.
//   compute(tail_tag, chunk, gathered, cc)      the arithmetic of chunk cc; tail_tag is std::true_type / std::false_type
// The functors are taken by value (closures of references): by reference the instruction streams drift further from the copies
// this replaced (tools/isa_diff.py).
// Preconditions: c0 is a multiple of 64 (a wave's 64 lanes then cover one 64-aligned chunk row; for trip sets that do not depend
// on the schedule also of kTrip * nthreads: part_range keeps parts trip-aligned), and c1 >= 1.
template <bool ALIGNED, int kTrip, bool STREAM, class Gather, class Compute>
__device__ __forceinline__ void pipelined_sweep(const uint8_t* src, int P, int c0, int c1, int t, int nthreads,
                                                Gather gather, Compute compute) {
    const size_t nbytes = (size_t)P * 3;
    const int lane = t & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(c0 + (t & ~63));
    auto fetch = [&](int cc) { return load_chunk_clamped<ALIGNED, STREAM>(src, nbytes, cc, c1); };
    Chunk cur[kTrip], nx[kTrip];
#pragma unroll
    for (int k = 0; k < kTrip; ++k) { cur[k] = fetch(w0 + lane + k * nthreads); nx[k] = fetch(w0 + lane + (kTrip + k) * nthreads); }
    decltype(gather(cur[0])) g[2];
    g[0] = gather(cur[0]);
    auto trip = [&](auto tail_tag, int cb) {
#pragma unroll
        for (int k = 0; k < kTrip; ++k) {
            const Chunk ch = cur[k];
            if (k + 1 < kTrip) {
                g[(k + 1) & 1] = gather(cur[k + 1]);
            } else {
#pragma unroll
                for (int j = 0; j < kTrip; ++j) { cur[j] = nx[j]; nx[j] = fetch(cb + lane + (2 * kTrip + j) * nthreads); }
                g[0] = gather(cur[0]);
            }
            __builtin_amdgcn_sched_barrier(0);
            compute(tail_tag, ch, g[k & 1], cb + k * nthreads + lane);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    const int lim = ALIGNED ? c1 : min(c1, P >> 2);          // chunks made of in-range pixels only
    int cb = w0;
    for (; cb + (kTrip - 1) * nthreads + 64 <= lim; cb += nthreads * kTrip) trip(std::false_type{}, cb);
    if (cb < c1) trip(std::true_type{}, cb);                    // at most one ragged trip per wave
}

}  // namespace sl
