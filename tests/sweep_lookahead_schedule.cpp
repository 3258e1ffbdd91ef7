// The index schedule of lookahead_wave_sweep (stainlib_amd/csrc/sweep_lookahead.hpp) on the host, with counting functors: a
// stand-alone program (tests/test_sweep_lookahead_schedule.py builds and runs it with the host compiler; no GPU, no HIP).
// For every lane of a workgroup and a set of ranges [c0, c1) around the trip edges it checks that
//   * every chunk of [c0, c1) is computed exactly once, and its first reader (head) ran exactly once before that;
//   * it is computed by the lane, in the trip and at the place in the lane's sequence that the old loop (the rotation loop of
//     pipelined_sweep / ts_sweep before this driver) gave it -- the order in which pixels reach the ring and the sums;
//   * the registers that reach a reader hold the chunk the reader is told it has (fetch returns its index as the "chunk");
//   * every index handed to fetch lies inside [c0, c1);
//   * a trip that runs without range predicates (tail_tag false) only touches chunks below `lim`.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../stainlib_amd/csrc/sweep_lookahead.hpp"

namespace {

struct Ev { char what; int cc; int trip; bool operator==(const Ev& o) const { return what == o.what && cc == o.cc && trip == o.trip; } };
struct FakeChunk { int idx; };
struct FakeGather { int idx; };

int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++g_fail; } } while (0)

// what the old loop did for one lane: full trips while the wave's last row is below lim, then at most one ragged trip
template <int N>
std::vector<Ev> old_loop(int w0, int lane, int c1, int lim, int nthreads) {
    std::vector<Ev> ev;
    int trip = 0, cb = w0;
    auto one = [&](int cb_) {
        for (int k = 0; k < N; ++k) { const int cc = cb_ + k * nthreads + lane; if (cc < c1) ev.push_back({'H', cc, trip}); }
        for (int k = 0; k < N; ++k) { const int cc = cb_ + k * nthreads + lane; if (cc < c1) ev.push_back({'C', cc, trip}); }
        ev.push_back({'E', 0, trip});
        ++trip;
    };
    for (; cb + (N - 1) * nthreads + 64 <= lim; cb += nthreads * N) one(cb);
    if (cb < c1) one(cb);
    return ev;
}

template <int N>
void check_range(int c0, int c1, int lim, int nthreads, long& n_cases) {
    std::vector<int> computed(c1 - c0, 0), headed(c1 - c0, 0);
    for (int t = 0; t < nthreads; ++t) {
        const int w0 = c0 + (t & ~63), lane = t & 63;
        std::vector<Ev> ev;
        int trip = 0;
        auto clamp = [&](int cc) { return cc < c1 ? cc : c1 - 1; };
        auto fetch = [&](int c) {
            CHECK(c >= c0 && c < c1, "fetch index %d outside [%d, %d) (t %d nthreads %d)", c, c0, c1, t, nthreads);
            return FakeChunk{c};
        };
        auto gather = [&](const FakeChunk& ch) { return FakeGather{ch.idx}; };
        auto head = [&](auto tail_tag, const FakeChunk& ch, int cc) {
            constexpr bool TAIL = decltype(tail_tag)::value;
            CHECK(ch.idx == clamp(cc), "head of chunk %d reads the registers of chunk %d (c1 %d t %d)", cc, ch.idx, c1, t);
            CHECK(TAIL || cc < lim, "chunk %d in a trip without range predicates, lim %d", cc, lim);
            if (cc < c1) { ev.push_back({'H', cc, trip}); ++headed[cc - c0]; CHECK(computed[cc - c0] == 0, "chunk %d computed before its head", cc); }
        };
        auto compute = [&](auto tail_tag, const FakeGather& g, int cc) {
            constexpr bool TAIL = decltype(tail_tag)::value;
            CHECK(g.idx == clamp(cc), "compute of chunk %d gets the gathers of chunk %d (c1 %d t %d)", cc, g.idx, c1, t);
            CHECK(TAIL || cc < lim, "chunk %d in a trip without range predicates, lim %d", cc, lim);
            if (cc < c1) { ev.push_back({'C', cc, trip}); ++computed[cc - c0]; }
        };
        auto end_trip = [&]() { ev.push_back({'E', 0, trip}); ++trip; };
        sl::lookahead_wave_sweep<N>(w0, lane, c1, lim, nthreads, fetch, gather, head, compute, end_trip);
        const std::vector<Ev> want = old_loop<N>(w0, lane, c1, lim, nthreads);
        CHECK(ev == want, "lane %d of %d on [%d, %d) lim %d: %zu events against the old loop's %zu", t, nthreads, c0, c1, lim, ev.size(), want.size());
    }
    for (int c = c0; c < c1; ++c) {
        CHECK(computed[c - c0] == 1, "chunk %d of [%d, %d) computed %d times (nthreads %d)", c, c0, c1, computed[c - c0], nthreads);
        CHECK(headed[c - c0] == 1, "chunk %d of [%d, %d) had %d heads (nthreads %d)", c, c0, c1, headed[c - c0], nthreads);
    }
    ++n_cases;
}

// a tile of P pixels swept whole (c0 = 0) and, where it has that many trips, as the parts part_range would cut (c0 a multiple of the trip)
template <int N>
void check_tile(long P, int nthreads, long& n_cases) {
    const int nch = (int)((P + 3) / 4);
    const int step = N * nthreads;
    for (int aligned = 0; aligned < 2; ++aligned) {
        if (aligned && P % 4) continue;
        const int lim_tile = aligned ? nch : (int)(P >> 2);
        check_range<N>(0, nch, lim_tile < nch ? lim_tile : nch, nthreads, n_cases);
        for (int c0 = step; c0 < nch; c0 += step) {
            check_range<N>(c0, nch, lim_tile, nthreads, n_cases);                                   // the last part
            if (c0 + step < nch) check_range<N>(c0, c0 + step, c0 + step, nthreads, n_cases);       // a middle part of one trip
            if (c0 + 3 * step < nch) check_range<N>(c0, c0 + 3 * step, c0 + 3 * step, nthreads, n_cases);
        }
    }
}

}  // namespace

int main() {
    long n_cases = 0;
    // the shapes of tests/test_gpu_sweep_lookahead.py: under one trip, exactly two, exactly three, three and a ragged one, four and a
    // ragged one, 181x183, 503x527 (and 1024^2, the benchmark's: 128 trips)
    const long shapes[][2] = {{64, 64}, {128, 128}, {128, 192}, {157, 157}, {129, 256}, {181, 183}, {503, 527}, {256, 256}, {512, 512}};
    for (const auto& s : shapes) check_tile<4>(s[0] * s[1], 512, n_cases);
    check_tile<4>(1024L * 1024L, 512, n_cases);
    check_tile<4>(128L * 128L, 1024, n_cases);
    check_tile<4>(157L * 157L, 1024, n_cases);
    // every pixel count around the edges of the first five trips (a trip is 4 chunks x 512 lanes x 4 pixels = 8192 pixels), and the
    // rows of 64 chunks inside a trip
    for (int trips = 0; trips <= 5; ++trips)
        for (int d = -9; d <= 9; ++d) {
            const long P = 8192L * trips + d;
            if (P >= 4) check_tile<4>(P, 512, n_cases);
        }
    for (int rows = 1; rows < 70; rows += 3)
        for (int d = -5; d <= 5; d += 5) check_tile<4>(256L * rows + d, 512, n_cases);
    // other trip sizes and workgroups (the driver is not tied to kFusedTrip = 4 or 512 lanes)
    for (int d = -5; d <= 5; ++d) {
        check_tile<2>(2048L * 3 + d, 256, n_cases);
        check_tile<2>(1024L * 5 + d, 128, n_cases);
        check_tile<4>(16384L * 3 + d, 1024, n_cases);
    }
    std::printf("%ld ranges checked, %d failures\n", n_cases, g_fail);
    return g_fail ? 1 : 0;
}
