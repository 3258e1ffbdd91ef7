// sweep_lookahead.hpp -- the trip loop of the statistics sweeps whose chunks have TWO readers (the merged sweep ts_sweep: the cube
// test of a trip's chunks at the trip's head, then the table gather of each chunk one chunk ahead of its sums).
// (A sibling of lookahead_sweep of apply_kernels.hpp, not an instantiation of it: that loop refills a chunk right behind its one
// reader, the gather, gathers the first chunk of the NEXT trip at the end of a trip and controls the loop per lane with a predicated
// store; here a chunk is refilled only behind its second reader, a trip begins with its own first gather -- the cube test of a chunk
// has to run before the chunk's registers are given away, and in the order the old loop ran it: the ring takes pixels in that
// order -- the loop is controlled per WAVE (the ring and its drain are wave-uniform) and the hot path is a full-trip instantiation
// without range predicates, like pipelined_sweep of sweep_pipeline.hpp.)
// Two register sets X and Y of N chunks each, a loop body of two trips: X is the current set of the first and Y of the second.
// No chunk is ever copied from one set to the other: the rotation `cur = nx; nx = fetch(..)` of pipelined_sweep makes the back-edge
// wait for the loads the same trip has issued (a copy needs the data), one memory round trip per wave and trip.  A chunk's
// registers are refilled with the chunk of the trip two ahead as soon as their last reader has issued, so 2N loads per lane are in
// flight and the only wait of a trip is for loads issued two trips (chunk 0) to one trip and a quarter (chunk N - 1) earlier:
// vmcnt(2N - 1) .. vmcnt(N) at the trip's head.
// The driver clamps every chunk index it hands to `fetch` into [.., c1) itself (lanes and trips past the end re-read the last
// chunk: no predicated load, DESIGN 4.0 hazard 1) and touches no builtin outside __HIP_DEVICE_COMPILE__, so it instantiates on the
// host with counting functors: tests/sweep_lookahead_schedule.cpp checks which lane computes which chunk in which trip.
//   fetch(c)                      chunk c (already clamped)            gather(chunk)   the table entries of a chunk
//   head(tail_tag, chunk, cc)     the first reader of chunk cc         compute(tail_tag, gathered, cc)   its arithmetic
//   end_trip()                    once per trip, behind its last compute
// tail_tag is std::false_type on the hot path (every pixel of every lane's chunks is inside the tile) and std::true_type on the
// at most two trips behind it, where head and compute mask their results (in_tile).  A wave's trips are the ones pipelined_sweep
// gives it -- trip j covers chunks w0 + lane + (j N + k) nthreads, k < N -- only an odd full trip at the end runs with the ragged
// instantiation (its predicates are all true there: the sums and lists are the same).
#pragma once
#include <type_traits>

#if defined(__HIPCC__)
#define SL_LOOKAHEAD_FN __host__ __device__ __forceinline__
#else
#define SL_LOOKAHEAD_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SL_LOOKAHEAD_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define SL_LOOKAHEAD_FENCE() ((void)0)
#endif

namespace sl {

// w0: the wave's first chunk (wave-uniform; a multiple of 64 past c0), lane: 0..63, lim: chunks [.., lim) hold in-range pixels only.
template <int N, class FETCH, class GATHER, class HEAD, class COMPUTE, class ENDTRIP>
SL_LOOKAHEAD_FN void lookahead_wave_sweep(int w0, int lane, int c1, int lim, int nthreads, const FETCH& fetch, const GATHER& gather,
                                          const HEAD& head, const COMPUTE& compute, const ENDTRIP& end_trip) {
    using CH = decltype(fetch(0));
    auto fetch_clamped = [&](int c) { return fetch(c < c1 ? c : c1 - 1); };
    CH X[N], Y[N];
    // (in the order the loop consumes them, a fence behind each: the scheduler otherwise turns them round and the first wait of the
    //  loop covers the youngest load)
#pragma unroll
    for (int k = 0; k < N; ++k) { X[k] = fetch_clamped(w0 + lane + k * nthreads); SL_LOOKAHEAD_FENCE(); }
#pragma unroll
    for (int k = 0; k < N; ++k) { Y[k] = fetch_clamped(w0 + lane + (N + k) * nthreads); SL_LOOKAHEAD_FENCE(); }
    auto trip = [&](auto tail_tag, CH (&cur)[N], int cb) {
        decltype(gather(cur[0])) g[2];
        g[0] = gather(cur[0]);
#pragma unroll
        for (int k = 0; k < N; ++k) head(tail_tag, cur[k], cb + k * nthreads + lane);
        cur[0] = fetch_clamped(cb + lane + 2 * N * nthreads);                    // both readers of chunk 0 are behind
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (k + 1 < N) {
                g[(k + 1) & 1] = gather(cur[k + 1]);
                cur[k + 1] = fetch_clamped(cb + lane + (2 * N + k + 1) * nthreads);
            }
            SL_LOOKAHEAD_FENCE();
            compute(tail_tag, g[k & 1], cb + k * nthreads + lane);
            SL_LOOKAHEAD_FENCE();
        }
        end_trip();
        SL_LOOKAHEAD_FENCE();          // (or the first trip's end_trip sinks behind the second trip and its operands stay live that long)
    };
    const int step = N * nthreads;
    int cb = w0;
    for (; cb + (2 * N - 1) * nthreads + 64 <= lim; cb += 2 * step) {
        trip(std::false_type{}, X, cb);
        trip(std::false_type{}, Y, cb + step);
    }
    if (cb < c1) {                                                   // an odd full trip and / or the ragged one
        trip(std::true_type{}, X, cb);
        if (cb + step < c1) trip(std::true_type{}, Y, cb + step);
    }
}

}  // namespace sl
