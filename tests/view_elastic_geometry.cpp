// The geometry of the elastic views (stainlib_amd/csrc/view_elastic_geometry.hpp) on the CPU, for every lane of every workgroup: built
// with -fsanitize=address,undefined by tests/test_view_elastic_host.py.  No GPU, no HIP; the header is included alone.
//
// Per case (a tile size, an output size, one window row, one control lattice, the call's cell, max_r and max_d) the program walks what
// k_view_elastic and k_view_planes_elastic do with the header's functions -- the tile's decode, every patch of the host's grid, the source
// block, the staged lattice nodes, every lane's outputs, their coordinates, taps, LDS slots and the blend -- on a model of the LDS block
// that holds, per slot, WHICH source pixel was staged there, and a model of the node block that holds which lattice value, and checks
//   - the patches tile the output exactly once (a workgroup past the tile's own count does nothing);
//   - the source block lies in the tile's buffer and fits the 64 x 64 LDS block; the nodes lie in the lattice and fit their block;
//   - every LDS index is in range; every tap of a patch lies in that patch's block (its slot holds the tap's own pixel) or outside the
//     tile; every node an output reads was staged;
//   - the Y, X the lanes derive, the blended pixel and the nearest element equal the definition's, computed here in 64-bit on the
//     CLAMPED field over the whole tile;
//   - the host's grid bound covers every tile's patches.
// The field is allocated to its exact size, so a read past the lattice is an AddressSanitizer report.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../stainlib_amd/csrc/view_elastic_geometry.hpp"

using namespace sl;

static long failures = 0, checked = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

static const int64_t Q = 65536;
static int64_t fdiv(int64_t a, int64_t d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }  // floor(a / d), d > 0

struct Case { int h, w, oh, ow, max_r, k, max_d; int32_t row[6]; std::vector<int32_t> field; };

static uint32_t pixel_of(int y, int x) {                     // three different bytes per pixel, 0 and 255 among them
    const uint32_t r = (uint32_t)(y * 37 + x * 11) & 255u, g = (uint32_t)(y * 5 + x * 101 + 255) & 255u, b = (uint32_t)((y ^ x) * 85) & 255u;
    return r | (g << 8) | (b << 16);
}

static void run(const Case& cs) {
    ++cases;
    const int h = cs.h, w = cs.w, oh = cs.oh, ow = cs.ow, k = cs.k;
    const uint32_t fill = 0x00c81e0au;                       // (10, 30, 200)
    const int gh = elastic_grid_side(oh, k), gw = elastic_grid_side(ow, k);
    CHECK(gh == (oh + (1 << k) - 1) / (1 << k) + 2 && gw == (ow + (1 << k) - 1) / (1 << k) + 2, "lattice %d x %d", gh, gw);
    CHECK((size_t)gh * gw * 2 == cs.field.size(), "a field of %zu values for a %d x %d lattice", cs.field.size(), gh, gw);
    // the definition, in 64-bit: the clamped centre and field, the row-sum rule, the spline, Y and X, the blend, the nearest element
    const int64_t cy = std::max<int64_t>(-(1 << 28), std::min<int64_t>(cs.row[0], h * Q + (1 << 28)));
    const int64_t cx = std::max<int64_t>(-(1 << 28), std::min<int64_t>(cs.row[1], w * Q + (1 << 28)));
    const int64_t a00 = cs.row[2], a01 = cs.row[3], a10 = cs.row[4], a11 = cs.row[5];
    const int64_t R = std::max(std::llabs(a00) + std::llabs(a01), std::llabs(a10) + std::llabs(a11));
    const bool all_fill = R > cs.max_r;
    const int64_t lim = 256 * cs.max_d;
    auto node = [&](int64_t a, int64_t b, int m) { return std::max<int64_t>(-lim, std::min<int64_t>(cs.field[(size_t)((a * gw + b) * 2 + m)], lim)); };
    auto weights = [&](int o, int64_t& a, int64_t (&wt)[3]) {
        const int64_t t = fdiv((2 * (int64_t)o + 1) * 256, (int64_t)1 << (k + 1)), f = t - 256 * fdiv(t, 256);
        a = fdiv(t, 256); wt[0] = (256 - f) * (256 - f); wt[2] = f * f; wt[1] = 131072 - wt[0] - wt[2];
    };
    auto tap = [&](int64_t y, int64_t x) { return y >= 0 && y < h && x >= 0 && x < w ? pixel_of((int)y, (int)x) : fill; };
    auto want_px = [&](int i, int j, int64_t& Y, int64_t& X, int64_t& near) {
        const int64_t u = 2 * i + 1 - oh, v = 2 * j + 1 - ow;
        int64_t a, b, wy[3], wx[3], d[2];
        weights(i, a, wy); weights(j, b, wx);
        for (int m = 0; m < 2; ++m) {
            int64_t acc = 0;
            for (int q = 0; q < 3; ++q) {
                int64_t r = 0;
                for (int p = 0; p < 3; ++p) r += wx[p] * node(a + q, b + p, m);
                acc += wy[q] * fdiv(r + 65536, 131072);
            }
            d[m] = fdiv(acc + 65536, 131072);
            CHECK(std::llabs(d[m]) <= lim, "(%d, %d): |d| = %lld above %lld", i, j, (long long)std::llabs(d[m]), (long long)lim);
        }
        Y = cy + fdiv(a00 * u + a01 * v, 2) + d[0] * 256; X = cx + fdiv(a10 * u + a11 * v, 2) + d[1] * 256;
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
    const long npatch = elastic_grid_patches(oh, ow, cs.max_r, cs.max_d);
    const ElasticTile t(cs.row, 0, h, w, cs.max_r, k, cs.max_d);
    CHECK(t.fill == all_fill, "fill %d, expected %d", (int)t.fill, (int)all_fill);
    CHECK(t.b >= 24 && t.b <= 64 && t.b >= elastic_patch_edge(cs.max_r, cs.max_d), "edge %d", t.b);
    std::vector<int> written((size_t)oh * ow, 0);
    std::vector<int64_t> lds((size_t)kViewB * kViewPitch);
    const int32_t kUnstaged = INT32_MIN;                     // (a clamped node is never this)
    std::vector<int32_t> nodes((size_t)kElasticLds);
    long own = 0;
    for (long patch = 0; patch < npatch; ++patch) {
        ViewPatch g;
        ElasticNodes e;
        bool none = false;
        if (!elastic_patch(t, (int)patch, h, w, oh, ow, g, e, none)) {
            CHECK(patch >= own && own > 0, "patch %ld refused below the tile's count", patch);
            continue;
        }
        CHECK(patch == own, "patch %ld accepted behind a refused one", patch);
        ++own;
        CHECK(g.bh >= 1 && g.bw >= 1 && g.bh <= kViewB && g.bw <= kViewB && g.i0 + g.bh <= oh && g.j0 + g.bw <= ow, "patch %ld: %d %d %d %d", patch, g.i0, g.j0, g.bh, g.bw);
        std::fill(lds.begin(), lds.end(), -1);
        std::fill(nodes.begin(), nodes.end(), kUnstaged);
        if (!none) {                                         // the source block: inside the tile's buffer, inside the LDS block; the stage
            CHECK(g.nu >= 1 && g.nv >= 1 && g.nu <= kViewB && g.nv <= kViewB, "block %d x %d", g.nu, g.nv);
            CHECK(g.ys >= 0 && g.xs >= 0 && g.ys + g.nu <= h && g.xs + g.nv <= w, "block at %d %d, %d x %d, tile %d x %d", g.ys, g.xs, g.nu, g.nv, h, w);
            for (int r = 0; r < g.nu; ++r)
                for (int c = 0; c < g.nv; ++c) lds[(size_t)r * kViewPitch + c] = (int64_t)(g.ys + r) * w + (g.xs + c);
            // the nodes: inside the lattice, inside their block; one slot per lane of a workgroup of 256
            CHECK(e.nr >= 3 && e.nc >= 3 && e.nr <= kElasticNodes && e.nc <= kElasticNodes, "nodes %d x %d", e.nr, e.nc);
            CHECK(e.na0 >= 0 && e.nb0 >= 0 && e.na0 + e.nr <= gh && e.nb0 + e.nc <= gw, "nodes at %d %d, %d x %d, lattice %d x %d", e.na0, e.nb0, e.nr, e.nc, gh, gw);
            int staged = 0;
            for (int tid = 0; tid < 256; ++tid) {
                int v = 0;
                if (tid < kElasticLds && elastic_stage_node(cs.field.data(), gw, e, t.lim, tid, v)) { nodes[(size_t)tid] = v; ++staged; }
            }
            CHECK(staged == e.nr * e.nc * 2, "%d nodes staged of %d", staged, e.nr * e.nc * 2);
        } else {
            CHECK(g.nu == 0 && g.nv == 0, "an empty block of %d x %d", g.nu, g.nv);
        }
        for (int tid = 0; tid < 256; ++tid) {
            const PatchLanes ln = patch_lanes(g.bw, tid, 256);
            if (ln.jl >= g.bw) continue;
            for (int il = ln.il0; il < g.bh; il += ln.rows) {
                const ElasticW wy = elastic_weights(g.i0 + il, k);
                for (int p = 0; p < 4; ++p) {
                    const int jj = geom_min(ln.jl + p, g.bw - 1);
                    const int i = g.i0 + il, j = g.j0 + jj;
                    int64_t Y, X, near;
                    const uint32_t want = want_px(i, j, Y, X, near);
                    uint32_t got = fill;
                    int64_t got_near = -1;
                    if (!none) {
                        const ElasticW wx = elastic_weights(j, k);
                        CHECK(wy.w0 >= 0 && wy.w1 >= 0 && wy.w2 >= 0 && wy.w0 + wy.w1 + wy.w2 == 131072, "weights of row %d", i);
                        const int n0 = elastic_node_at(e, wy.a, wx.a);
                        CHECK(n0 >= 0 && n0 + 2 * (2 * kElasticNodes) + 5 < kElasticLds, "(%d, %d): node offset %d", i, j, n0);
                        for (int q = 0; q < 3; ++q)
                            for (int c = 0; c < 6; ++c) {
                                const int32_t got_node = nodes[(size_t)(n0 + q * 2 * kElasticNodes + c)];
                                CHECK(got_node == (int32_t)node(wy.a + q, wx.a + (c >> 1), c & 1), "(%d, %d): node (%d, %d, %d) reads %d", i, j, wy.a + q, wx.a + (c >> 1), c & 1, got_node);
                            }
                        const AffineYX q = elastic_at(t, e, nodes.data(), wy, i, j, oh, ow);
                        CHECK(q.Y == Y && q.X == X, "(%d, %d): Y, X = %d, %d, expected %lld, %lld", i, j, q.Y, q.X, (long long)Y, (long long)X);
                        const AffineTaps a = affine_taps(q);
                        uint32_t px[4];
                        for (int kk = 0; kk < 4; ++kk) {
                            const int ky = a.ky + (kk >> 1), kx = a.kx + (kk & 1);
                            const int slot = affine_lds_row(g, ky) + affine_lds_col(g, kx);
                            CHECK(slot >= 0 && slot < kViewB * kViewPitch, "slot %d", slot);
                            const bool in = affine_inside(ky, h) && affine_inside(kx, w);
                            CHECK(in == (ky >= 0 && ky < h && kx >= 0 && kx < w), "inside(%d, %d)", ky, kx);
                            if (in) CHECK(lds[(size_t)slot] == (int64_t)ky * w + kx, "(%d, %d) tap %d at (%d, %d): slot %d holds %lld", i, j, kk, ky, kx, slot, (long long)lds[(size_t)slot]);
                            else CHECK(lds[(size_t)slot] >= 0, "(%d, %d) tap %d: an unstaged slot %d is read", i, j, kk, slot);
                            px[kk] = in ? pixel_of(ky, kx) : fill;
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
    CHECK(own >= 1 && own <= npatch, "%ld patches of the tile, the grid has %ld", own, npatch);
    for (size_t n = 0; n < written.size(); ++n) CHECK(written[n] == 1, "output %zu written %d times", n, written[n]);
}

static uint64_t state = 12345;
static double rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; }

// kind 0: zero; 1: random within the bound; 2: a +- sign pattern at the bound; 3: a "device" field of anything, the int32 extremes among it
static void make_field(Case& c, int kind) {
    const int gh = elastic_grid_side(c.oh, c.k), gw = elastic_grid_side(c.ow, c.k);
    const int lim = 256 * c.max_d;
    c.field.assign((size_t)gh * gw * 2, 0);
    for (size_t n = 0; n < c.field.size(); ++n) {
        if (kind == 1) c.field[n] = (int32_t)std::llrint((2 * rnd() - 1) * lim);
        else if (kind == 2) c.field[n] = rnd() < 0.5 ? -lim : lim;
        else if (kind == 3) {
            const double r = rnd();
            c.field[n] = r < 0.15 ? INT32_MIN : r < 0.3 ? INT32_MAX : r < 0.5 ? (int32_t)std::llrint((2 * rnd() - 1) * 4096) : (int32_t)std::llrint((2 * rnd() - 1) * 2147483647.0);
        }
    }
}

static Case make(int h, int w, int oh, int ow, int k, int max_d, double cyp, double cxp, double m00, double m01, double m10, double m11,
                 int max_r = 2 * 65536) {
    Case c;
    c.h = h; c.w = w; c.oh = oh; c.ow = ow; c.max_r = max_r; c.k = k; c.max_d = max_d;
    const double v[6] = {cyp, cxp, m00, m01, m10, m11};
    for (int n = 0; n < 6; ++n) c.row[n] = (int32_t)std::llrint(65536.0 * v[n]);
    return c;
}

int main() {
    const int tiles[][2] = {{1, 1}, {1, 3}, {9, 11}, {5, 67}, {81, 151}, {96, 80}};
    const int outs[][2] = {{1, 1}, {5, 3}, {13, 66}, {40, 56}, {70, 70}};
    const int ks[] = {4, 6, 8}, mds[] = {0, 1, 3, 8};
    struct M { double a, b, c, d; };
    const M fixed[] = {{1, 0, 0, 1}, {1, -1, 1, 1} /* the row-sum limit */, {0.70710678, -0.70710678, 0.70710678, 0.70710678}, {0, 0, 0, 0}, {0.37, -0.11, 0.05, 0.41}};
    for (const auto& ts : tiles)
        for (const auto& os : outs)
            for (int k : ks)
                for (int md : mds) {
                    const int h = ts[0], w = ts[1];
                    std::vector<M> ms(fixed, fixed + sizeof(fixed) / sizeof(fixed[0]));
                    for (int n = 0; n < 3; ++n) {            // random rows up to the row-sum limit
                        const double ry = 2 * rnd(), rx = 2 * rnd(), sy = rnd(), sx = rnd();
                        ms.push_back({(rnd() < 0.5 ? -1 : 1) * ry * sy, (rnd() < 0.5 ? -1 : 1) * ry * (1 - sy), (rnd() < 0.5 ? -1 : 1) * rx * sx,
                                      (rnd() < 0.5 ? -1 : 1) * rx * (1 - sx)});
                    }
                    int kind = 0;
                    for (const M& m : ms) {
                        Case c = make(h, w, os[0], os[1], k, md, h / 2.0 + 0.3701 * (kind & 1), w * rnd(), m.a, m.b, m.c, m.d);
                        make_field(c, kind++ & 3);
                        run(c);
                    }
                    Case c = make(h, w, os[0], os[1], k, md, h * rnd(), w / 2.0, 1, 0, 0, 1);
                    make_field(c, 3);                        // a device field at the identity
                    run(c);
                    c = make(h, w, os[0], os[1], k, md, -0.25, w + 0.5, 1, 0.4, 0, 1);
                    make_field(c, 2);                        // half outside, a shear
                    run(c);
                }
    // the call's bounds: a tile beyond max_r is all fill, a tile below it has fewer patches than the grid
    for (int md : mds) {
        Case c = make(96, 80, 70, 70, 4, md, 48, 40, 1, -1, 1, 1, 65536);
        make_field(c, 2); run(c);
        c = make(96, 80, 70, 70, 4, md, 48, 40, 0.5, 0, 0, 0.5, 2 * 65536);
        make_field(c, 1); run(c);
        c = make(96, 80, 70, 70, 4, md, 48, 40, 1, 0, 0, 1, 1);
        make_field(c, 3); run(c);
    }
    // the 32-bit extremes: sides of 8192, the row-sum limit, centres at and beyond their range, garbage matrices and fields
    for (double cyp : {-4096.0, 0.0, 8192.0 + 4096.0, 4096.0})
        for (int k : {4, 8}) {
            Case c = make(8192, 3, 8192, 2, k, 8, cyp, 1.5, 2, 0, 0, 2);
            make_field(c, 2); run(c);
            c = make(3, 8192, 2, 8192, k, 8, 1.5, cyp, 1, 1, -2, 0);
            make_field(c, 3); run(c);
        }
    {
        Case c = make(8192, 3, 8192, 2, 4, 8, 0, 0, 0, 0, 0, 0);
        const int32_t wild[][6] = {{INT32_MAX, INT32_MIN, 65536, 0, 0, 65536}, {INT32_MIN, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX},
                                   {0, 0, INT32_MIN, 0, 0, 1}, {5, 5, 131072, 1, 0, 0}};
        for (const auto& r : wild) {
            for (int n = 0; n < 6; ++n) c.row[n] = r[n];
            make_field(c, 3);
            run(c);
        }
    }
    // the patch edge's stated values
    CHECK(elastic_patch_edge(65536, 0) == 63 && elastic_patch_edge(65536, 8) == 47 && elastic_patch_edge(131072, 8) == 24 && elastic_patch_edge(0, 8) == 64,
          "edges %d %d %d", elastic_patch_edge(65536, 0), elastic_patch_edge(65536, 8), elastic_patch_edge(131072, 8));
    printf("%ld cases, %ld output elements checked, %ld failures\n", cases, checked, failures);
    return failures ? 1 : 0;
}
