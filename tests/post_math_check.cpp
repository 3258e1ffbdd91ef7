// The post stage's arithmetic (stainlib_amd/csrc/post_math.hpp) on the CPU against a plain 64-bit restatement of the definition
// (stainlib_amd/augmentation/noise.py): built with -fsanitize=address,undefined by tests/test_post_host.py.  No GPU, no HIP; the headers
// are included alone.
//   - philox4x32_10 on the three known answers and, on a spread of counters and keys, against a restatement with 64-bit products;
//   - post_g over words whose byte sums cover all of 0 .. 1020;
//   - post_add over all 256 bytes x all 1021 values of G x a dozen sq, the extremes included; sq = 0 must be the identity;
//   - post_reduce_sq on codes out of range;
//   - post_noise_pixel against the restatement, per channel and mono;
//   - the lane-to-pixel-index arithmetic of the write-side hook (post_lane under view_write_s's and resize_write's lane assignment, on
//     view_geometry.hpp's own patches), lane by lane on the shapes of tests/test_gpu_post.py: every output pixel is visited exactly once,
//     with the right p.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../stainlib_amd/csrc/post_math.hpp"
#include "../stainlib_amd/csrc/view_geometry.hpp"

using namespace sl;

static long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

// ---- the 64-bit restatement ---------------------------------------------------------------------------------------------------------------
static void want_philox(const uint64_t ctr[4], uint64_t k0, uint64_t k1, uint64_t out[4]) {
    const uint64_t M = 0xffffffffull;
    uint64_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]};
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint64_t n[4] = {((p1 >> 32) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> 32) ^ c[3] ^ k1) & M, p0 & M};
        for (int i = 0; i < 4; ++i) c[i] = n[i];
        k0 = (k0 + 0x9E3779B9ull) & M;
        k1 = (k1 + 0xBB67AE85ull) & M;
    }
    for (int i = 0; i < 4; ++i) out[i] = c[i];
}
static int64_t want_g(uint64_t w) { return (int64_t)((w & 0xff) + ((w >> 8) & 0xff) + ((w >> 16) & 0xff) + ((w >> 24) & 0xff)) - 510; }
static int64_t floor_shift16(int64_t x) { return x >= 0 ? x / 65536 : -((-x + 65535) / 65536); }       // x >> 16, arithmetic, without a shift
static int64_t want_add(int64_t b1, int64_t G, int64_t sq) {
    const int64_t v = b1 + floor_shift16(G * sq + 32768);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

static void check_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, const uint32_t* known) {
    uint32_t ks[20], got[4];
    philox_schedule(k0, k1, ks);
    philox4x32_10(c0, c1, c2, c3, ks, got);
    const uint64_t ctr[4] = {c0, c1, c2, c3};
    uint64_t want[4];
    want_philox(ctr, k0, k1, want);
    for (int i = 0; i < 4; ++i) {
        CHECK(got[i] == (uint32_t)want[i], "philox(%08x %08x %08x %08x; %08x %08x)[%d] = %08x, want %08x", c0, c1, c2, c3, k0, k1, i, got[i], (uint32_t)want[i]);
        if (known) CHECK(got[i] == known[i], "known answer word %d: %08x, want %08x", i, got[i], known[i]);
    }
}

// ---- the write sides' lane assignment, restated from view_kernels.hpp (view_write_s) and view_resize_kernels.hpp (resize_write) ------------
static void visit(std::vector<int>& seen, int ow, const ViewPatch& g, int il, int jl) {
    uint32_t p0 = 0;
    const int nvalid = post_lane(g.i0, g.j0, g.bh, g.bw, ow, il, jl, p0);
    CHECK(nvalid >= 0 && nvalid <= 4, "nvalid %d", nvalid);
    for (int k = 0; k < nvalid; ++k) {
        const int i = g.i0 + il, j = g.j0 + jl + k;
        CHECK(il < g.bh && jl + k < g.bw, "pixel (%d, %d) outside its patch", il, jl + k);
        CHECK(p0 + (uint32_t)k == (uint32_t)(i * ow + j), "p of (%d, %d): %u, want %d", i, j, p0 + k, i * ow + j);
        if ((size_t)(p0 + k) < seen.size()) ++seen[p0 + k];
        else CHECK(false, "p %u past the output of %zu pixels", p0 + k, seen.size());
    }
}

static void check_fixed(int h, int w, int oh, int ow, int s, int d) {
    const int B = kViewB / s, npx = (ow + B - 1) / B, npatch = npx * ((oh + B - 1) / B);
    const bool tr = d & 1;
    const int32_t win[3] = {(h - s * (tr ? ow : oh)) / 2, (w - s * (tr ? oh : ow)) / 3, d};
    std::vector<int> seen((size_t)oh * ow, 0);
    const ViewTile vt(win, 0, 7, h, w, oh, ow, s);
    for (int patch = 0; patch < npatch; ++patch) {
        const ViewPatch g(vt, patch, npx, oh, ow, s);
        const int LPR = 16 / s, NPASS = s == 1 ? 4 : 1;
        for (int tid = 0; tid < 256; ++tid) {
            const int lr16 = tid >> 4, lc16 = tid & 15;
            const int lr = s == 1 ? lr16 : (16 * lr16 + lc16) / LPR, lc = s == 1 ? lc16 : lc16 % LPR;
            for (int q = 0; q < NPASS; ++q) visit(seen, ow, g, 16 * q + lr, 4 * lc);
        }
    }
    for (size_t p = 0; p < seen.size(); ++p) CHECK(seen[p] == 1, "fixed %dx%d s %d d %d: pixel %zu visited %d times", oh, ow, s, d, p, seen[p]);
}

static void check_resize(int h, int w, int oh, int ow, int wh, int ww, int d) {
    const int32_t win[5] = {1, 2, d, wh, ww};
    const ResizeTile vt(win, 0, 7, h, w, oh, ow, h, w);
    std::vector<int> seen((size_t)oh * ow, 0);
    for (int patch = 0; patch < 4096; ++patch) {
        ViewPatch g;
        ResizeAxis ai, aj;
        if (!resize_patch(vt, patch, oh, ow, g, ai, aj)) break;
        for (int tid = 0; tid < 256; ++tid) {
            const PatchLanes l = patch_lanes(g.bw, tid, 256);          // resize_write's assignment (the same lines written out there)
            if (l.jl >= g.bw) continue;
            for (int il = l.il0; il < g.bh; il += l.rows) visit(seen, ow, g, il, l.jl);
        }
    }
    for (size_t p = 0; p < seen.size(); ++p) CHECK(seen[p] == 1, "resize %dx%d from %dx%d d %d: pixel %zu visited %d times", oh, ow, wh, ww, d, p, seen[p]);
}

int main() {
    // the generator: the known answers, then a spread against the restatement
    const uint32_t ka0[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    const uint32_t ka1[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
    const uint32_t ka2[4] = {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    check_philox(0, 0, 0, 0, 0, 0, ka0);
    check_philox(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, ka1);
    check_philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, ka2);
    uint32_t x = 12345u;
    for (int t = 0; t < 2000; ++t) {
        uint32_t v[6];
        for (int i = 0; i < 6; ++i) { x = x * 1664525u + 1013904223u; v[i] = x; }
        check_philox(t < 1000 ? (uint32_t)t : v[0], t < 1000 ? 0u : v[1], t < 1000 ? 0u : v[2], t < 1000 ? 0u : v[3], v[4], v[5], nullptr);
    }
    // G: every byte sum
    for (uint32_t sum = 0; sum <= 1020; ++sum) {
        uint32_t b[4], left = sum;
        for (int i = 0; i < 4; ++i) { b[i] = left > 255 ? 255 : left; left -= b[i]; }
        const uint32_t wd[2] = {b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[3] | (b[2] << 8) | (b[1] << 16) | (b[0] << 24)};
        for (uint32_t wv : wd) CHECK(post_g(wv) == (int32_t)sum - 510 && want_g(wv) == (int64_t)sum - 510, "post_g(%08x) = %d, want %d", wv, post_g(wv), (int)sum - 510);
    }
    // the scale-and-clamp: all bytes x all G x a dozen sq
    const int32_t sqs[] = {0, 1, 2, 64, 443, 444, 2217, 8868, 16384, 28377, 28378, 12345};
    for (int32_t sq : sqs)
        for (int32_t G = -510; G <= 510; ++G)
            for (uint32_t b = 0; b < 256; ++b) {
                const uint32_t got = post_add(b, G, sq);
                CHECK((int64_t)got == want_add(b, G, sq), "post_add(%u, %d, %d) = %u, want %lld", b, G, sq, got, (long long)want_add(b, G, sq));
                if (sq == 0) CHECK(got == b, "sq = 0 must be the identity: %u -> %u", b, got);
            }
    // the code reduction
    const int32_t wild[] = {-1, -2147483647 - 1, 2147483647, 28379, 65536, 0, 28378, 5};
    for (int32_t c : wild) {
        const int64_t want = c < 0 ? 0 : (c > 28378 ? 28378 : c);
        CHECK(post_reduce_sq(c) == want, "post_reduce_sq(%d) = %d", c, post_reduce_sq(c));
    }
    CHECK(kPostSqMax == 28378, "SQ_MAX");
    // a pixel, per channel and mono
    for (int t = 0; t < 4000; ++t) {
        uint32_t v[4];
        for (int i = 0; i < 4; ++i) { x = x * 1664525u + 1013904223u; v[i] = x; }
        const uint32_t px = v[0] & 0xffffffu, p = t < 2000 ? (uint32_t)t : v[1], k0 = v[2], k1 = v[3];
        const int32_t sq = sqs[1 + t % 11];
        uint32_t ks[20];
        philox_schedule(k0, k1, ks);
        const uint64_t ctr[4] = {p, 0, 0, 0};
        uint64_t W[4];
        want_philox(ctr, k0, k1, W);
        for (int mono = 0; mono < 2; ++mono) {
            uint32_t want = 0;
            for (int c = 0; c < 3; ++c) want |= (uint32_t)want_add((px >> (8 * c)) & 0xff, want_g(W[mono ? 3 : c]), sq) << (8 * c);
            const uint32_t got = post_noise_pixel(px, p, ks, sq, mono != 0);
            CHECK(got == want, "post_noise_pixel(%06x, %u; %08x %08x, %d, %d) = %06x, want %06x", px, p, k0, k1, sq, mono, got, want);
        }
    }
    // the lanes of the write side on the test shapes: tiles 96 x 100
    for (int d = 0; d < 8; ++d) {
        check_fixed(96, 100, 40, 56, 1, d);
        check_fixed(96, 100, 70, 70, 1, d);
        check_fixed(96, 100, 40, 40, 2, d);
        check_fixed(96, 100, 20, 20, 4, d);
        check_fixed(96, 100, (d & 1) ? 96 : 96, (d & 1) ? 96 : 100, 1, d);         // the full tile (a square of it when turned)
        check_resize(96, 100, 40, 56, 50 + 5 * d, 91 - 7 * d, d);
        check_resize(96, 100, 70, 70, 30 + d, 29, d);
        check_resize(96, 100, 40, 56, 96, 100, d);
    }
    check_fixed(5, 7, 5, 7, 1, 0);
    check_fixed(33, 67, 33, 67, 1, 0);
    printf("%ld checks, %ld failures\n", checked, failures);
    return failures ? 1 : 0;
}
