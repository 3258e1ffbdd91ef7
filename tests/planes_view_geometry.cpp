// The lane-to-address arithmetic of k_view_planes (stainlib_amd/csrc/planes_view_geometry.hpp on the geometry of view_geometry.hpp) on the
// CPU, for every lane of every workgroup: built with -fsanitize=address,undefined by tests/test_planes_view_host.py.  No GPU, no HIP.
//
// Per case the input is a heap buffer of EXACTLY n c h w elem_bytes bytes and the output one of exactly n c oh ow elem_bytes, so the
// sanitizer sees any load or store outside them; every element holds its own index (truncated to its width).  The program walks the
// kernel's steps -- the four loads of a lane, the masked LDS writes, the index table, the gather and the store -- with the header's
// functions, carries the SOURCE ELEMENT INDEX through a model of the LDS image, and asserts that every output element is written exactly
// once, from the source element the definition names: rot90(flip_w_if(f, R), k) with R the centre sample of the clamped window.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stainlib_amd/csrc/planes_view_geometry.hpp"

using namespace sl;

static long failures = 0, checked = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

struct Case {
    int n, c, h, w, es, oh, ow, d_mask, shrink, max_wh, max_ww;
    std::vector<int32_t> win;                    // n x 3 or n x 5
};

// the host's launch geometry (route_host.hpp: view_geometry / view_resize_geometry), restated for the grid only
static long patches_shrink(int oh, int ow, int s, long& npx) {
    const int B = kViewB / s;
    npx = (ow + B - 1) / B;
    return npx * ((oh + B - 1) / B);
}
static long patches_resize(int oh, int ow, int d_mask, int max_wh, int max_ww) {
    auto patches = [&](int nu, int nv) {
        const int bu = resize_patch_edge(nu, resize_side_max(nu, max_wh)), bv = resize_patch_edge(nv, resize_side_max(nv, max_ww));
        return (long)((nu + bu - 1) / bu) * ((nv + bv - 1) / bv);
    };
    long np = patches(oh, ow);
    if (d_mask & 1) { const long t = patches(ow, oh); if (t > np) np = t; }
    return np;
}

// ---- the definition, written without the kernel's pieces: the source element (within the plane) of output element (i, j) of tile t
static size_t expected_source(const Case& k, int t, int i, int j) {
    const bool resizing = k.max_wh > 0;
    const int32_t* wv = &k.win[(resizing ? 5 : 3) * (size_t)t];
    const int d = wv[2] & k.d_mask, q = d & 3;
    const int nu = (q & 1) ? k.ow : k.oh, nv = (q & 1) ? k.oh : k.ow;
    long wh, ww;
    if (resizing) {
        const long hi_h = std::min<long>(16L * nu, k.max_wh), hi_w = std::min<long>(16L * nv, k.max_ww);
        wh = std::max<long>(1, std::min<long>(wv[3], hi_h)); ww = std::max<long>(1, std::min<long>(wv[4], hi_w));
    } else {
        wh = (long)k.shrink * nu; ww = (long)k.shrink * nv;
    }
    const long y0 = std::max<long>(0, std::min<long>(wv[0], k.h - wh)), x0 = std::max<long>(0, std::min<long>(wv[1], k.w - ww));
    // out = rot90(F, q), F = flip_w(R) if d & 4 else R; numpy's rot90 (counter-clockwise) entry by entry, undone:
    int a = i, b = j;                            // (a, b) in rot90(F, q)  ->  in F
    for (int turn = 0; turn < q; ++turn) {       // rot90(m, 1)[a, b] = m[b, ncols - 1 - a]
        const int turns_left = q - turn;         // the matrix we index into next is rot90(F, turns_left - 1)
        const int ncols = ((turns_left - 1) & 1) ? nu : nv;
        const int na = b, nb = ncols - 1 - a;
        a = na; b = nb;
    }
    if (d & 4) b = nv - 1 - b;                   // (a, b) in R: nu x nv
    const long ky = ((2L * a + 1) * wh) / (2L * nu), kx = ((2L * b + 1) * ww) / (2L * nv);
    return (size_t)(y0 + ky) * (size_t)k.w + (size_t)(x0 + kx);
}

static void put(uint8_t* p, int es, uint64_t v) { memcpy(p, &v, (size_t)es); }      // (little endian)
static uint64_t get(const uint8_t* p, int es) { uint64_t v = 0; memcpy(&v, p, (size_t)es); return v; }
static uint64_t trunc_to(uint64_t v, int es) { return es == 8 ? v : v & ((1ull << (8 * es)) - 1); }

static void run(const Case& k) {
    ++cases;
    const bool resizing = k.max_wh > 0;
    const int es = k.es;
    const size_t P = (size_t)k.h * k.w, PO = (size_t)k.oh * k.ow, planes = (size_t)k.n * k.c;
    uint8_t* const in = (uint8_t*)malloc(planes * P * es);
    uint8_t* const out = (uint8_t*)malloc(planes * PO * es);
    memset(out, 0xee, planes * PO * es);
    for (size_t e = 0; e < planes * P; ++e) put(in + e * es, es, e * 0x0000000100000001ull + 0x9e3779b900000000ull);
    std::vector<int> writes(planes * PO, 0);
    std::vector<size_t> from(planes * PO, (size_t)-1);
    long npx = 1;
    const long npatch = resizing ? patches_resize(k.oh, k.ow, k.d_mask, k.max_wh, k.max_ww) : patches_shrink(k.oh, k.ow, k.shrink, npx);
    std::vector<size_t> lds((size_t)kViewB * kViewPitch);          // the source element (within the plane) a slot holds
    std::vector<uint64_t> ldsv((size_t)kViewB * kViewPitch);       // and its bits
    std::vector<char> filled((size_t)kViewB * kViewPitch);
    int idx[kPlanesIdx];
    for (size_t plane = 0; plane < planes; ++plane) {
        const int tile = (int)(plane / k.c);
        const uint8_t* const src = in + plane * P * es;
        for (long patch = 0; patch < npatch; ++patch) {
            ViewPatch g;
            ResizeAxis ai, aj;
            const int s = resizing ? 1 : k.shrink;
            if (resizing) {
                const ResizeTile vt(k.win.data(), tile, k.d_mask, k.h, k.w, k.oh, k.ow, k.max_wh, k.max_ww);
                if (!resize_patch(vt, (int)patch, k.oh, k.ow, g, ai, aj)) continue;
            } else {
                const ViewTile vt(k.win.data(), tile, k.d_mask, k.h, k.w, k.oh, k.ow, s);
                g = ViewPatch(vt, (int)patch, (int)npx, k.oh, k.ow, s);
            }
            CHECK(g.nu >= 1 && g.nu <= kViewB && g.nv >= 1 && g.nv <= kViewB, "block %d x %d", g.nu, g.nv);
            std::fill(filled.begin(), filled.end(), 0);
            for (int tid = 0; tid < kPlanesWG; ++tid)
                for (int q = 0; q < 4; ++q) {
                    const PlanesLoad L = planes_load(g, k.w, P, tid, q);
                    uint8_t v[32];
                    size_t el[4];
                    if (L.vec) {
                        memcpy(v, src + L.e * es, 4 * (size_t)es);                     // the vector load: inside the buffer, or the sanitizer says so
                        for (int p = 0; p < 4; ++p) el[p] = L.e + p;
                    } else {
                        for (int p = 0; p < 4; ++p) {
                            el[p] = L.e + p < P ? L.e + p : P - 1;
                            memcpy(v + p * es, src + el[p] * es, (size_t)es);
                        }
                    }
                    CHECK(L.n >= 0 && L.n <= 4, "n = %d", L.n);
                    for (int p = 0; p < L.n; ++p) {
                        const int slot = L.slot + p;
                        CHECK(slot >= 0 && slot < kViewB * kViewPitch, "LDS slot %d", slot);
                        if (slot < 0 || slot >= kViewB * kViewPitch) continue;
                        CHECK(!filled[slot], "LDS slot %d filled twice", slot);
                        filled[slot] = 1; lds[slot] = el[p]; ldsv[slot] = get(v + p * es, es);
                    }
                }
            for (int e = 0; e < kPlanesIdx; ++e) {
                const int t = e & (kViewB - 1);
                idx[e] = -1000000;
                if (t < (e < kViewB ? g.bh : g.bw)) idx[e] = resizing ? planes_index_resize(e < kViewB ? ai : aj, t) : planes_index_shrink(g, s, e);
            }
            for (int tid = 0; tid < kPlanesWG; ++tid) {
                const PlanesLanes ln = planes_lanes(g.bw, tid);
                if (ln.jl >= g.bw) continue;
                const int nvalid = geom_min(4, g.bw - ln.jl);
                for (int il = ln.il0; il < g.bh; il += ln.rows) {
                    uint8_t v[32];
                    size_t el[4];
                    for (int p = 0; p < 4; ++p) {
                        const int slot = idx[il] + idx[kViewB + geom_min(ln.jl + p, g.bw - 1)];
                        const bool ok = slot >= 0 && slot < kViewB * kViewPitch && filled[slot];
                        CHECK(ok, "gather from slot %d (never filled or outside)", slot);
                        el[p] = ok ? lds[slot] : 0;
                        put(v + p * es, es, ok ? ldsv[slot] : 0);
                    }
                    const size_t o = planes_out_elem(g, k.ow, il, ln.jl);
                    uint8_t* const dst = out + (plane * PO + o) * es;
                    memcpy(dst, v, (size_t)(nvalid == 4 ? 4 : nvalid) * es);           // the vector store, or nvalid single ones
                    for (int p = 0; p < nvalid; ++p) { ++writes[plane * PO + o + p]; from[plane * PO + o + p] = el[p]; }
                }
            }
        }
    }
    for (size_t plane = 0; plane < planes; ++plane)
        for (int i = 0; i < k.oh; ++i)
            for (int j = 0; j < k.ow; ++j) {
                const size_t o = plane * PO + (size_t)i * k.ow + j;
                const size_t want = expected_source(k, (int)(plane / k.c), i, j);
                ++checked;
                CHECK(writes[o] == 1, "es %d tile %dx%d out %dx%d s %d resize %d,%d plane %zu (%d, %d): written %d times", es, k.h, k.w, k.oh, k.ow,
                      k.shrink, k.max_wh, k.max_ww, plane, i, j, writes[o]);
                CHECK(from[o] == want, "es %d tile %dx%d out %dx%d s %d resize %d,%d plane %zu (%d, %d) code %d: from element %zu, the definition says %zu",
                      es, k.h, k.w, k.oh, k.ow, k.shrink, k.max_wh, k.max_ww, plane, i, j,
                      k.win[(k.max_wh > 0 ? 5 : 3) * (plane / k.c) + 2], from[o], want);
                const uint64_t bits = trunc_to((plane * P + want) * 0x0000000100000001ull + 0x9e3779b900000000ull, es);
                CHECK(get(out + o * es, es) == bits, "plane %zu (%d, %d): the bits of another element", plane, i, j);
            }
    free(in);
    free(out);
}

// crop / shrink: 8 tiles = the 8 codes (masked by d_mask), corners by turns
static void crop_case(int h, int w, int oh, int ow, int s, int es, int c, int rot) {
    const int d_mask = 7;
    if (s * oh > h || s * ow > w || s * ow > h || s * oh > w) return;            // (both orientations must fit: d_mask = 7)
    Case k{8, c, h, w, es, oh, ow, d_mask, s, 0, 0, {}};
    for (int t = 0; t < 8; ++t) {
        const int d = t, corner = (t + rot) & 3;
        const int wh = s * ((d & 1) ? ow : oh), ww = s * ((d & 1) ? oh : ow);
        k.win.push_back((corner & 1) ? h - wh : 0);
        k.win.push_back((corner & 2) ? w - ww : 0);
        k.win.push_back(d);
    }
    run(k);
}

// resizing: 8 tiles = the 8 codes; window sides from the ratio (num / den times the output side as the code sees it), corners by turns
static void resize_case(int h, int w, int oh, int ow, int num, int den, int es, int c, int rot) {
    Case k{8, c, h, w, es, oh, ow, 7, 1, h, w, {}};
    if ((long)h * w > (1L << 22)) return;
    for (int t = 0; t < 8; ++t) {
        const int d = t, corner = (t + rot) & 3;
        const int nu = (d & 1) ? ow : oh, nv = (d & 1) ? oh : ow;
        int wh = std::max(1, std::min({h, 16 * nu, (int)((long)nu * num / den)})), ww = std::max(1, std::min({w, 16 * nv, (int)((long)nv * num / den)}));
        k.win.push_back((corner & 1) ? h - wh : 0);
        k.win.push_back((corner & 2) ? w - ww : 0);
        k.win.push_back(d);
        k.win.push_back(wh);
        k.win.push_back(ww);
    }
    run(k);
}

int main() {
    const int tiles[][2] = {{1, 1}, {3, 5}, {70, 131}};
    const int outs[][2] = {{1, 1}, {37, 65}, {64, 64}, {65, 63}};
    const int ratios[][2] = {{1, 1}, {2, 1}, {16, 1}, {5, 3}, {1, 3}};           // 1, 2, 16, a non-integer one, an upsampling one
    int rot = 0;
    for (int es : {1, 2, 4, 8})
        for (int c : {1, 3})
            for (auto& tl : tiles)
                for (auto& o : outs) {
                    for (int s : {1, 2, 4}) crop_case(tl[0], tl[1], o[0], o[1], s, es, c, rot++);
                    for (auto& r : ratios) resize_case(tl[0], tl[1], o[0], o[1], r[0], r[1], es, c, rot++);
                }
    // the crop / shrink sizes that fit a 70 x 131 tile in both orientations, and a tile that holds the large outputs
    for (int es : {1, 2, 4, 8})
        for (int c : {1, 3}) {
            for (int s : {1, 2, 4}) {
                crop_case(70, 131, 70 / s, 70 / s, s, es, c, rot++);
                crop_case(70, 131, 37 / s + 1, 65 / s, s, es, c, rot++);
                crop_case(3, 5, 3 / s, 3 / s, s, es, c, rot++);
            }
            crop_case(131, 140, 65, 63, 2, es, c, rot++);
            crop_case(131, 131, 64, 64, 2, es, c, rot++);
            crop_case(70, 131, 16, 17, 4, es, c, rot++);
        }
    // device windows out of range are clamped, codes outside the mask are masked: nothing outside the buffers
    {
        Case k{4, 1, 70, 131, 2, 16, 24, 6, 2, 0, 0, {-5, -7, 1, 1000, 1000, 7, 30, -1, 13, -2147483647, 2147483647, 4}};
        run(k);
        Case r{4, 3, 70, 131, 1, 33, 21, 7, 1, 50, 60, {-5, -7, 1, 999, 999, 1000, 1000, 7, 0, -3, 30, -1, 13, 2147483647, 1, 0, 0, 4, 20, 2147483647}};
        run(r);
    }
    printf("%ld cases, %ld output elements checked, %ld failures\n", cases, checked, failures);
    return failures ? 1 : 0;
}
