// The geometry and the arithmetic of the blurred view (stainlib_amd/csrc/view_blur_geometry.hpp) on the CPU, for every lane of every
// workgroup: built with -fsanitize=address,undefined by tests/test_blur_host.py.  No GPU, no HIP; the header is included alone.
//
// Per case (a tile size, an output size, a shrink, a window row, the call's bound max_r, a codes row) the program walks what k_view_blur
// does -- the tile's decode, every patch of the host's grid, the read side's byte offsets (view_read / load12, restated), the stage's LDS
// slots (view_stage, restated), the two passes with the header's own lane and tap functions and its own arithmetic, the write side's
// LDS slots and output pixels (view_write_s, restated) -- on LDS buffers of the kernel's sizes that hold, beside the values, WHICH
// pixel each slot holds, and checks that
//   - every global byte offset of the read side lies in the tile, every LDS index of every side in its buffer;
//   - every tap of the two passes reads a slot that holds the tap's own pixel, clamped in TILE space;
//   - every output is written exactly once, from the slots that hold its own box of blurred pixels;
//   - the blurred bytes equal the definition's, computed here in 64-bit from the whole tile.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../stainlib_amd/csrc/view_blur_geometry.hpp"

using namespace sl;

static long failures = 0, checked = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

static uint32_t pixel_of(int y, int x) {                     // three different bytes per pixel, 0 and 255 among them
    const uint32_t r = (uint32_t)(y * 37 + x * 11) & 255u, g = (uint32_t)(y * 5 + x * 101 + 255) & 255u, b = (uint32_t)((y ^ x) * 85) & 255u;
    return r | (g << 8) | (b << 16);
}

struct Case { int h, w, oh, ow, s, max_r, d_mask; int32_t win[3]; int32_t codes[9]; };

// the definition in 64-bit: B of the whole tile under the weights wt (the identity when the codes fail the rule)
static const std::vector<uint32_t>& blur_whole(int h, int w, const int64_t* wt) {
    static std::map<std::vector<int64_t>, std::vector<uint32_t>> cache;          // (the cases share a few tiles and weight rows)
    std::vector<int64_t> key = {h, w};
    key.insert(key.end(), wt, wt + 9);
    const auto hit = cache.find(key);
    if (hit != cache.end()) return hit->second;
    std::vector<int64_t> hs((size_t)h * w * 3);
    std::vector<uint32_t> out((size_t)h * w);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                int64_t sum = 0;
                for (int k = -8; k <= 8; ++k) sum += wt[std::abs(k)] * ((pixel_of(y, std::max(0, std::min(x + k, w - 1))) >> (8 * c)) & 255);
                hs[((size_t)y * w + x) * 3 + c] = sum;
            }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t o = 0;
            for (int c = 0; c < 3; ++c) {
                int64_t sum = 0;
                for (int k = -8; k <= 8; ++k) sum += wt[std::abs(k)] * hs[((size_t)std::max(0, std::min(y + k, h - 1)) * w + x) * 3 + c];
                o |= (uint32_t)((sum + 32768) >> 16) << (8 * c);
            }
            out[(size_t)y * w + x] = o;
        }
    return cache.emplace(key, out).first->second;
}

static void run(const Case& cs) {
    ++cases;
    const int h = cs.h, w = cs.w, oh = cs.oh, ow = cs.ow, s = cs.s, R = cs.max_r;
    const long nbytes = 3L * h * w;
    // the definition: the rule, the clamped window, the blurred tile, the view of it as box corners
    int64_t wt[9];
    bool ok = true;
    int64_t sum = 0;
    for (int k = 0; k < 9; ++k) { wt[k] = cs.codes[k]; ok = ok && wt[k] >= 0 && (k <= R || wt[k] == 0); sum += (k ? 2 : 1) * wt[k]; }
    if (!ok || sum != 256) { wt[0] = 256; for (int k = 1; k < 9; ++k) wt[k] = 0; }
    int want_r = 0;
    for (int k = 0; k < 9; ++k) if (wt[k]) want_r = k;
    const std::vector<uint32_t>& B = blur_whole(h, w, wt);
    const int d = cs.win[2] & cs.d_mask;
    const int wh = (d & 1) ? ow : oh, ww = (d & 1) ? oh : ow;                    // the window, in boxes
    const int y0 = std::max(0, std::min<int>(cs.win[0], h - s * wh)), x0 = std::max(0, std::min<int>(cs.win[1], w - s * ww));
    std::vector<int> cur((size_t)wh * ww);                                      // box index u * ww + v, then flipped and turned
    int ch = wh, cw = ww;
    for (int k = 0; k < wh * ww; ++k) cur[(size_t)k] = k;
    if (d & 4) { std::vector<int> f(cur.size()); for (int u = 0; u < ch; ++u) for (int v = 0; v < cw; ++v) f[(size_t)u * cw + v] = cur[(size_t)u * cw + (cw - 1 - v)]; cur = f; }
    for (int t = 0; t < (d & 3); ++t) {                                         // numpy.rot90: out[i][j] = in[j][cw - 1 - i]
        std::vector<int> f(cur.size());
        for (int i = 0; i < cw; ++i) for (int j = 0; j < ch; ++j) f[(size_t)i * ch + j] = cur[(size_t)j * cw + (cw - 1 - i)];
        cur = f; std::swap(ch, cw);
    }
    CHECK(ch == oh && cw == ow, "the turned window is %d x %d, the output %d x %d", ch, cw, oh, ow);

    // the kernel's walk
    const BlurWeights bw(cs.codes, 0, R);
    CHECK(bw.r == want_r && bw.r <= R, "radius %d, expected %d (max_r %d)", bw.r, want_r, R);
    for (int k = 0; k < 9; ++k) CHECK(bw.w[k] == wt[k], "weight %d: %d, expected %lld", k, bw.w[k], (long long)wt[k]);
    const int b = blur_patch_edge(R, s);
    CHECK(b >= 1 && s * b + 2 * R <= kViewB, "patch edge %d", b);
    const int npx = (ow + b - 1) / b, npatch = npx * ((oh + b - 1) / b);
    const ViewTile vt(cs.win, 0, cs.d_mask, h, w, oh, ow, s);
    CHECK(vt.y0 == y0 && vt.x0 == x0, "window at %d %d, expected %d %d", vt.y0, vt.x0, y0, x0);
    std::vector<int> written((size_t)oh * ow, 0);
    const size_t NLDS = (size_t)kViewB * kViewPitch;
    std::vector<uint32_t> s_px(NLDS);
    std::vector<long> id_px(NLDS), id_h(NLDS);
    std::vector<BlurSum> s_h(NLDS);
    for (int patch = 0; patch < npatch; ++patch) {
        ViewPatch in, gr;
        blur_patch(vt, patch, npx, h, w, oh, ow, s, R, in, gr);
        CHECK(in.bh >= 1 && in.bw >= 1 && in.bh <= b && in.bw <= b && in.i0 + in.bh <= oh && in.j0 + in.bw <= ow, "patch %d: %d %d %d %d", patch, in.i0, in.j0, in.bh, in.bw);
        CHECK(in.ys >= 0 && in.xs >= 0 && in.ys + in.nu <= h && in.xs + in.nv <= w, "inner block at %d %d, %d x %d", in.ys, in.xs, in.nu, in.nv);
        CHECK(gr.nu >= 1 && gr.nv >= 1 && gr.nu <= kViewB && gr.nv <= kViewB, "grown block %d x %d", gr.nu, gr.nv);
        CHECK(gr.ys >= 0 && gr.xs >= 0 && gr.ys + gr.nu <= h && gr.xs + gr.nv <= w, "grown block at %d %d, %d x %d", gr.ys, gr.xs, gr.nu, gr.nv);
        CHECK(gr.ys <= in.ys && gr.xs <= in.xs && gr.ys + gr.nu >= in.ys + in.nu && gr.xs + gr.nv >= in.xs + in.nv, "the grown block does not hold the inner one");
        std::fill(id_px.begin(), id_px.end(), -1L);
        std::fill(id_h.begin(), id_h.end(), -1L);
        // read side and stage (view_read / load12 / view_stage): lane (lr, lc) loads the chunk at column 4 min(lc, (nv - 1) / 4) of the
        // rows min(16 q + lr, nu - 1) and stages its pixels (r, 4 lc + p) that exist
        for (int tid = 0; tid < 256; ++tid) {
            const int lr = tid >> 4, lc = tid & 15, cc = std::min(lc, (gr.nv - 1) >> 2);
            for (int q = 0; q < 4; ++q) {
                const int rr = std::min(16 * q + lr, gr.nu - 1);
                const long base = 3 * ((long)(gr.ys + rr) * w + gr.xs) + 12 * cc;
                CHECK(base >= 0 && base < nbytes, "read side: byte %ld of %ld", base, nbytes);
                if (nbytes >= 12) { const long at = std::min(base, nbytes - 12); CHECK(at >= 0 && at + 12 <= nbytes, "load at %ld", at); }
                const int r = 16 * q + lr;
                for (int p = 0; p < 4; ++p)
                    if (r < gr.nu && 4 * lc + p < gr.nv) {
                        const size_t slot = (size_t)r * kViewPitch + 4 * lc + p;
                        CHECK(slot < NLDS, "stage slot %zu", slot);
                        CHECK(cc == lc, "a staged pixel from a clamped chunk");
                        s_px[slot] = pixel_of(gr.ys + r, gr.xs + 4 * lc + p);
                        id_px[slot] = (long)(gr.ys + r) * w + gr.xs + 4 * lc + p;
                    }
            }
        }
        // horizontal pass
        for (int tid = 0; tid < 256; ++tid)
            for (int q = 0; q < 4; ++q) {
                const int row = blur_lane_row(tid, q);
                if (row >= gr.nu) continue;
                for (int p = 0; p < 4; ++p) {
                    const int c = blur_lane_col(tid, p);
                    if (c >= in.nv) continue;
                    const int X = in.xs + c;
                    const bool cut = blur_cut(gr.nv, in.nv, R);               // the kernel's branch: the clamped pass, or the plain one
                    for (int k = -bw.r; k <= bw.r; ++k) {
                        const int t = cut ? blur_tap_at<true>(X, k, w, gr.xs) : blur_tap_at<false>(X, k, w, gr.xs);
                        CHECK(t >= 0 && t < gr.nv, "row tap %d of column %d: block column %d of %d", k, X, t, gr.nv);
                        const size_t slot = (size_t)row * kViewPitch + (size_t)std::max(0, std::min(t, kViewB - 1));
                        CHECK(id_px[slot] == (long)(gr.ys + row) * w + std::max(0, std::min(X + k, w - 1)), "row tap %d of (%d, %d): slot holds %ld", k, gr.ys + row, X, id_px[slot]);
                    }
                    const size_t slot = (size_t)row * kViewPitch + c;
                    CHECK(slot < NLDS && id_h[slot] == -1, "row-sum slot %zu (written twice?)", slot);
                    s_h[slot] = cut ? blur_row_sum<true>(bw, s_px.data() + (size_t)row * kViewPitch, X, w, gr.xs)
                                    : blur_row_sum<false>(bw, s_px.data() + (size_t)row * kViewPitch, X, w, gr.xs);
                    id_h[slot] = (long)(gr.ys + row) * w + X;
                }
            }
        // vertical pass: into s_px at the inner block's own origin (the staged pixels are dead)
        std::fill(id_px.begin(), id_px.end(), -1L);
        for (int tid = 0; tid < 256; ++tid)
            for (int q = 0; q < 4; ++q) {
                const int y = blur_lane_row(tid, q);
                if (y >= in.nu) continue;
                const int Y = in.ys + y;
                for (int p = 0; p < 4; ++p) {
                    const int c = blur_lane_col(tid, p);
                    if (c >= in.nv) continue;
                    const bool cut = blur_cut(gr.nu, in.nu, R);
                    for (int k = -bw.r; k <= bw.r; ++k) {
                        const int t = cut ? blur_tap_at<true>(Y, k, h, gr.ys) : blur_tap_at<false>(Y, k, h, gr.ys);
                        CHECK(t >= 0 && t < gr.nu, "column tap %d of row %d: block row %d of %d", k, Y, t, gr.nu);
                        const size_t slot = (size_t)std::max(0, std::min(t, kViewB - 1)) * kViewPitch + c;
                        CHECK(id_h[slot] == (long)std::max(0, std::min(Y + k, h - 1)) * w + in.xs + c, "column tap %d of (%d, %d): slot holds %ld", k, Y, in.xs + c, id_h[slot]);
                    }
                    const size_t slot = (size_t)y * kViewPitch + c;
                    CHECK(slot < NLDS && id_px[slot] == -1, "blurred slot %zu (written twice?)", slot);
                    s_px[slot] = cut ? blur_col_px<true>(bw, s_h.data() + c, kViewPitch, Y, h, gr.ys)
                                     : blur_col_px<false>(bw, s_h.data() + c, kViewPitch, Y, h, gr.ys);
                    id_px[slot] = (long)Y * w + in.xs + c;
                    CHECK(s_px[slot] == B[(size_t)Y * w + in.xs + c], "(%d, %d): blurred %06x, expected %06x", Y, in.xs + c, s_px[slot], B[(size_t)Y * w + in.xs + c]);
                    ++checked;
                }
            }
        // write side (view_write_s): 16 / s lanes per output row, 4 adjacent outputs each
        const int LPR = 16 / s, NPASS = s == 1 ? 4 : 1;
        for (int tid = 0; tid < 256; ++tid) {
            const int lr16 = tid >> 4, lc16 = tid & 15;
            const int lr = s == 1 ? lr16 : (16 * lr16 + lc16) / LPR, lc = s == 1 ? lc16 : lc16 % LPR;
            const int jl = 4 * lc;
            for (int q = 0; q < NPASS; ++q) {
                const int il = 16 * q + lr;
                if (il >= in.bh || jl >= in.bw) continue;
                const int nvalid = std::min(4, in.bw - jl);
                for (int p = 0; p < nvalid; ++p) {
                    const int i = in.i0 + il, j = in.j0 + jl + p;
                    const int at = in.a0 + il * in.ai + (jl + p) * in.aj;
                    const int box = cur[(size_t)i * ow + j], u = box / ww, v = box % ww;
                    for (int a = 0; a < s; ++a)
                        for (int bb = 0; bb < s; ++bb) {
                            const long slot = (long)at + a * kViewPitch + bb;
                            CHECK(slot >= 0 && slot < (long)NLDS, "write side: slot %ld", slot);
                            if (slot >= 0 && slot < (long)NLDS)
                                CHECK(id_px[(size_t)slot] == (long)(y0 + s * u + a) * w + x0 + s * v + bb, "output (%d, %d) box (%d, %d): slot holds %ld", i, j, a, bb, id_px[(size_t)slot]);
                        }
                    const long pix = (long)i * ow + j;
                    CHECK(pix >= 0 && pix < (long)oh * ow, "output pixel %ld", pix);
                    ++written[(size_t)pix];
                }
            }
        }
    }
    for (size_t k = 0; k < written.size(); ++k) CHECK(written[k] == 1, "output %zu written %d times", k, written[k]);
}

int main() {
    const int tiles[][2] = {{1, 70}, {3, 70}, {40, 52}, {96, 80}, {130, 129}};
    const int32_t rows[][9] = {{256, 0, 0, 0, 0, 0, 0, 0, 0}, {202, 27, 0, 0, 0, 0, 0, 0, 0}, {40, 38, 30, 20, 11, 6, 2, 1, 0},
                               {16, 15, 15, 15, 15, 15, 15, 15, 15}, {0, 0, 0, 0, 0, 0, 0, 0, 128},
                               {255, 0, 0, 0, 0, 0, 0, 0, 0}, {258, -1, 0, 0, 0, 0, 0, 0, 0}, {INT32_MAX, INT32_MIN, 5, 0, 0, 0, 0, 0, 1}};
    for (const auto& t : tiles)
        for (int s : {1, 2, 4})
            for (int max_r : {0, 1, 8})
                for (int d = 0; d < 8; ++d) {
                    const int h = t[0], w = t[1], m = std::min(h, w);
                    const int sizes[][2] = {{h / s, w / s}, {m / s, m / s}, {std::max(1, h / s / 2), std::max(1, w / s / 3)}, {std::min(h / s, 33), std::min(w / s, 47)}};
                    int nth = 0;
                    for (const auto& z : sizes) {
                        const int oh = z[0], ow = z[1];
                        if (oh < 1 || ow < 1 || s * oh > h || s * ow > w) continue;
                        if ((d & 1) && (s * ow > h || s * oh > w)) continue;
                        const int wh = (d & 1) ? ow : oh, ww = (d & 1) ? oh : ow;
                        const int corners[][2] = {{0, 0}, {h - s * wh, w - s * ww}, {(h - s * wh) / 2, (w - s * ww) / 3}, {-5, 1000000}};
                        for (const auto& c : corners) {
                            Case cs;
                            cs.h = h; cs.w = w; cs.oh = oh; cs.ow = ow; cs.s = s; cs.max_r = max_r; cs.d_mask = 7;
                            cs.win[0] = c[0]; cs.win[1] = c[1]; cs.win[2] = d;
                            const auto& row = rows[(nth++ + d + max_r) % 8];
                            for (int k = 0; k < 9; ++k) cs.codes[k] = row[k];
                            run(cs);
                        }
                    }
                }
    // a masked code: d_mask = 6 drops the transposition, the code's other bits stay
    {
        Case cs = {96, 80, 90, 33, 1, 8, 6, {3, 40, 7}, {40, 38, 30, 20, 11, 6, 2, 1, 0}};
        run(cs);
        cs.win[2] = 0x7ffffff5;
        run(cs);
    }
    printf("%ld cases, %ld blurred pixels checked, %ld failures\n", cases, checked, failures);
    return failures ? 1 : 0;
}
