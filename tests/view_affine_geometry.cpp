// The geometry of the affine views (stainlib_amd/csrc/view_affine_geometry.hpp) on the CPU, for every lane of every workgroup: built
// with -fsanitize=address,undefined by tests/test_view_affine_host.py.  No GPU, no HIP; the header is included alone.
//
// Per case (a tile size, an output size, one window row, the call's bound max_r) the program walks what k_view_affine and
// k_view_planes_affine do with the header's functions -- the tile's decode, every patch of the host's grid, the source block, every
// lane's outputs, their coordinates, taps, LDS slots and the blend -- on a model of the LDS block that holds, per slot, WHICH source
// pixel was staged there, and checks that
//   - the patches tile the output exactly once (a workgroup past the tile's own count does nothing);
//   - the source block lies in the tile's buffer and fits the 64 x 64 LDS block;
//   - every tap of a patch lies in that patch's block (its slot holds the tap's own pixel) or outside the tile;
//   - the Y, X the lanes derive, the blended pixel and the nearest element equal the definition's, computed here in 64-bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../stainlib_amd/csrc/view_affine_geometry.hpp"

using namespace sl;

static long failures = 0, checked = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

static const int64_t Q = 65536;
static int64_t fdiv2(int64_t a) { return a >= 0 ? a / 2 : -((-a + 1) / 2); }                 // floor(a / 2) without a shift
static int64_t fdiv(int64_t a, int64_t d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }  // floor(a / d), d > 0

struct Case { int h, w, oh, ow, max_r; int32_t row[6]; };

static uint32_t pixel_of(int y, int x) {                     // three different bytes per pixel, 0 and 255 among them
    const uint32_t r = (uint32_t)(y * 37 + x * 11) & 255u, g = (uint32_t)(y * 5 + x * 101 + 255) & 255u, b = (uint32_t)((y ^ x) * 85) & 255u;
    return r | (g << 8) | (b << 16);
}

static void run(const Case& cs) {
    ++cases;
    const int h = cs.h, w = cs.w, oh = cs.oh, ow = cs.ow;
    const uint32_t fill = 0x00c81e0au;                       // (10, 30, 200)
    // the definition, in 64-bit: the clamped centre, the row-sum rule, Y and X, the blend, the nearest element
    const int64_t cy = std::max<int64_t>(-(1 << 28), std::min<int64_t>(cs.row[0], h * Q + (1 << 28)));
    const int64_t cx = std::max<int64_t>(-(1 << 28), std::min<int64_t>(cs.row[1], w * Q + (1 << 28)));
    const int64_t a00 = cs.row[2], a01 = cs.row[3], a10 = cs.row[4], a11 = cs.row[5];
    const int64_t R = std::max(std::llabs(a00) + std::llabs(a01), std::llabs(a10) + std::llabs(a11));
    const bool all_fill = R > cs.max_r;
    auto tap = [&](int64_t y, int64_t x) { return y >= 0 && y < h && x >= 0 && x < w ? pixel_of((int)y, (int)x) : fill; };
    auto want_px = [&](int i, int j, int64_t& Y, int64_t& X, int64_t& near) {
        const int64_t u = 2 * i + 1 - oh, v = 2 * j + 1 - ow;
        Y = cy + fdiv2(a00 * u + a01 * v); X = cx + fdiv2(a10 * u + a11 * v);
        const int64_t ny = fdiv(Y, Q), nx = fdiv(X, Q);
        near = ny >= 0 && ny < h && nx >= 0 && nx < w ? ny * w + nx : -1;
        if (all_fill) { near = -1; return fill; }
        const int64_t ty = Y - Q / 2, tx = X - Q / 2, ky = fdiv(ty, Q), kx = fdiv(tx, Q);
        const int64_t fy = fdiv(ty, 256) - 256 * ky, fx = fdiv(tx, 256) - 256 * kx;
        uint32_t o = 0;
        for (int c = 0; c < 3; ++c) {
            const int64_t p00 = (tap(ky, kx) >> (8 * c)) & 255, p01 = (tap(ky, kx + 1) >> (8 * c)) & 255;
            const int64_t p10 = (tap(ky + 1, kx) >> (8 * c)) & 255, p11 = (tap(ky + 1, kx + 1) >> (8 * c)) & 255;
            o |= (uint32_t)(((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16) << (8 * c);
        }
        return o;
    };

    // the kernels' walk
    const long npatch = affine_grid_patches(oh, ow, cs.max_r);
    const AffineTile t(cs.row, 0, h, w, cs.max_r);
    CHECK(t.fill == all_fill, "fill %d, expected %d", (int)t.fill, (int)all_fill);
    CHECK(t.b >= 32 && t.b <= 64 && t.b >= affine_patch_edge(cs.max_r), "edge %d", t.b);
    std::vector<int> written((size_t)oh * ow, 0);
    std::vector<int64_t> lds((size_t)kViewB * kViewPitch);
    long own = 0;
    for (long patch = 0; patch < npatch; ++patch) {
        ViewPatch g;
        bool none = false;
        if (!affine_patch(t, (int)patch, h, w, oh, ow, g, none)) {
            CHECK(patch >= own && own > 0, "patch %ld refused below the tile's count", patch);
            continue;
        }
        CHECK(patch == own, "patch %ld accepted behind a refused one", patch);
        ++own;
        CHECK(g.bh >= 1 && g.bw >= 1 && g.bh <= kViewB && g.bw <= kViewB && g.i0 + g.bh <= oh && g.j0 + g.bw <= ow, "patch %ld: %d %d %d %d", patch, g.i0, g.j0, g.bh, g.bw);
        std::fill(lds.begin(), lds.end(), -1);
        if (!none) {                                         // the source block: inside the tile's buffer, inside the LDS block; the stage
            CHECK(g.nu >= 1 && g.nv >= 1 && g.nu <= kViewB && g.nv <= kViewB, "block %d x %d", g.nu, g.nv);
            CHECK(g.ys >= 0 && g.xs >= 0 && g.ys + g.nu <= h && g.xs + g.nv <= w, "block at %d %d, %d x %d, tile %d x %d", g.ys, g.xs, g.nu, g.nv, h, w);
            for (int r = 0; r < g.nu; ++r)
                for (int c = 0; c < g.nv; ++c) lds[(size_t)r * kViewPitch + c] = (int64_t)(g.ys + r) * w + (g.xs + c);
        } else {
            CHECK(g.nu == 0 && g.nv == 0, "an empty block of %d x %d", g.nu, g.nv);
        }
        for (int tid = 0; tid < 256; ++tid) {
            const PatchLanes ln = patch_lanes(g.bw, tid, 256);
            if (ln.jl >= g.bw) continue;
            for (int il = ln.il0; il < g.bh; il += ln.rows) {
                for (int p = 0; p < 4; ++p) {
                    const int jj = geom_min(ln.jl + p, g.bw - 1);
                    const int i = g.i0 + il, j = g.j0 + jj;
                    int64_t Y, X, near;
                    const uint32_t want = want_px(i, j, Y, X, near);
                    uint32_t got = fill;
                    int64_t got_near = -1;
                    if (!none) {
                        const AffineYX q = affine_at(t, i, j, oh, ow);
                        CHECK(q.Y == Y && q.X == X, "(%d, %d): Y, X = %d, %d, expected %lld, %lld", i, j, q.Y, q.X, (long long)Y, (long long)X);
                        const AffineTaps a = affine_taps(q);
                        uint32_t px[4];
                        for (int k = 0; k < 4; ++k) {
                            const int ky = a.ky + (k >> 1), kx = a.kx + (k & 1);
                            const int slot = affine_lds_row(g, ky) + affine_lds_col(g, kx);
                            CHECK(slot >= 0 && slot < kViewB * kViewPitch, "slot %d", slot);
                            const bool in = affine_inside(ky, h) && affine_inside(kx, w);
                            CHECK(in == (ky >= 0 && ky < h && kx >= 0 && kx < w), "inside(%d, %d)", ky, kx);
                            if (in) CHECK(lds[(size_t)slot] == (int64_t)ky * w + kx, "(%d, %d) tap %d at (%d, %d): slot %d holds %lld", i, j, k, ky, kx, slot, (long long)lds[(size_t)slot]);
                            else CHECK(lds[(size_t)slot] >= 0, "(%d, %d) tap %d: an unstaged slot %d is read", i, j, k, slot);
                            px[k] = in ? pixel_of(ky, kx) : fill;
                        }
                        got = affine_blend(px[0], px[1], px[2], px[3], a.fy, a.fx);
                        const int ny = q.Y >> 16, nx = q.X >> 16;
                        got_near = affine_inside(ny, h) && affine_inside(nx, w) ? (int64_t)ny * w + nx : -1;
                    }
                    if (ln.jl + p < g.bw) {
                        ++written[(size_t)i * ow + j];
                        CHECK(got == want, "(%d, %d): pixel %06x, expected %06x", i, j, got, want);
                        CHECK(got_near == near, "(%d, %d): nearest element %lld, expected %lld", i, j, (long long)got_near, (long long)near);
                        ++checked;
                    }
                }
            }
        }
    }
    for (size_t k = 0; k < written.size(); ++k) CHECK(written[k] == 1, "output %zu written %d times", k, written[k]);
}

static Case make(int h, int w, int oh, int ow, double cyp, double cxp, double m00, double m01, double m10, double m11, int max_r = 2 * 65536) {
    Case c;
    c.h = h; c.w = w; c.oh = oh; c.ow = ow; c.max_r = max_r;
    const double v[6] = {cyp, cxp, m00, m01, m10, m11};
    for (int k = 0; k < 6; ++k) c.row[k] = (int32_t)std::llrint(65536.0 * v[k]);
    return c;
}

int main() {
    const double PI = 3.14159265358979323846;
    struct M { double a, b, c, d; };
    std::vector<M> ms;
    for (double deg : {0.0, 30.0, 45.0, 90.0, -45.0, 135.0, 200.0}) ms.push_back({std::cos(deg * PI / 180), -std::sin(deg * PI / 180), std::sin(deg * PI / 180), std::cos(deg * PI / 180)});
    ms.push_back({1, -1, 1, 1});                             // 45 degrees at 1 / z = sqrt 2: the row-sum limit, b = 32
    ms.push_back({2, 0, 0, 2});                              // the 2 x 2 box
    ms.push_back({0, 2, -2, 0});
    ms.push_back({0, 0, 0, 0});                              // a constant
    ms.push_back({1, 1, 0, 0});                              // singular: a line
    ms.push_back({1, 0.4, 0, 1});                            // a shear
    ms.push_back({0.8, 0.3, 0.2, -1.1});                     // negative determinant
    ms.push_back({-1, 0, 0, 1});
    ms.push_back({0, 1, 1, 0});
    ms.push_back({0.37, -0.11, 0.05, 0.41});                 // a magnification
    const int sizes[][4] = {{96, 80, 40, 56}, {96, 80, 70, 70}, {100, 70, 130, 33}, {65, 129, 64, 65}, {1, 1, 5, 3}, {7, 300, 1, 200}};
    for (const auto& s : sizes)
        for (const M& m : ms) {
            const int h = s[0], w = s[1];
            run(make(h, w, s[2], s[3], h / 2.0, w / 2.0, m.a, m.b, m.c, m.d));
            run(make(h, w, s[2], s[3], h / 2.0 + 0.3701, w / 2.0 - 0.2519, m.a, m.b, m.c, m.d));      // a fractional centre
            run(make(h, w, s[2], s[3], 0.25, w + 0.5, m.a, m.b, m.c, m.d));                             // half outside
            run(make(h, w, s[2], s[3], -300.0, w / 2.0, m.a, m.b, m.c, m.d));                           // wholly outside (mostly)
        }
    // the call's bound: a tile beyond it is all fill, a tile below it has fewer patches than the grid
    run(make(96, 80, 70, 70, 48, 40, 1, -1, 1, 1, 65536));
    run(make(96, 80, 70, 70, 48, 40, 1, 0, 0, 1, 65536));
    run(make(96, 80, 70, 70, 48, 40, 0.5, 0, 0, 0.5, 65536));
    run(make(96, 80, 70, 70, 48, 40, 1, 0, 0, 1, 1));
    run(make(96, 80, 70, 70, 48, 40, 0, 0, 0, 0, 1));
    // the 32-bit extremes: sides of 8192, the row-sum limit, centres at and beyond their range, garbage matrices (device windows)
    for (double cyp : {-4096.0, 0.0, 8192.0 + 4096.0, 4096.0}) {
        run(make(8192, 3, 8192, 2, cyp, 1.5, 2, 0, 0, 2));
        run(make(8192, 3, 8192, 2, cyp, 1.5, -1, -1, 1, 1));
        run(make(3, 8192, 2, 8192, 1.5, cyp, 1, 1, -2, 0));
    }
    {
        Case c = make(8192, 3, 8192, 2, 0, 0, 0, 0, 0, 0);
        const int32_t wild[][6] = {{INT32_MAX, INT32_MIN, 65536, 0, 0, 65536}, {INT32_MIN, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX},
                                   {0, 0, INT32_MIN, 0, 0, 1}, {5, 5, 131072, 1, 0, 0}, {5, 5, 0, 0, -131072, -1}};
        for (const auto& r : wild) {
            for (int k = 0; k < 6; ++k) c.row[k] = r[k];
            run(c);
        }
    }
    // random matrices up to the limit
    uint64_t state = 12345;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; };
    for (int k = 0; k < 60; ++k) {
        const double ry = 2 * rnd(), rx = 2 * rnd(), sy = rnd(), sx = rnd();
        run(make(90, 77, 67, 45, 90 * rnd(), 77 * rnd(), (rnd() < 0.5 ? -1 : 1) * ry * sy, (rnd() < 0.5 ? -1 : 1) * ry * (1 - sy),
                 (rnd() < 0.5 ? -1 : 1) * rx * sx, (rnd() < 0.5 ? -1 : 1) * rx * (1 - sx)));
    }
    printf("%ld cases, %ld output elements checked, %ld failures\n", cases, checked, failures);
    return failures ? 1 : 0;
}
