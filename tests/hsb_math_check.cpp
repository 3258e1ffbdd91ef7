// The per-pixel HSB map (stainlib_amd/csrc/hsb_math.hpp) on the CPU against a plain 64-bit restatement of the definition
// (stainlib_amd/augmentation/hsb.py): built with -fsanitize=address,undefined by tests/test_hsb_host.py.  No GPU, no HIP; the header
// is included alone.
//   - hsb_div over every (num, C) of the hue division, every (C, M) of the saturation division and every M of the value division,
//     with the exact binary32 reciprocal and with reciprocals two units in the last place either side of it (the device's is within one);
//   - hsb_scale over every x in [0, Q] at a spread of codes, the extremes included;
//   - hsb_pixel over a strided colour cube (greys, black, white, the primaries and every channel tie among it) at a dozen code
//     triples, the extremes included; zero codes must be the identity.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../stainlib_amd/csrc/hsb_math.hpp"

using namespace sl;

static long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++failures; } } while (0)

static const int64_t Q = 32768;
static int64_t rdiv(int64_t a, int64_t c) { return (2 * a + c) / (2 * c); }
static int64_t rnd(int64_t x) { return (x + Q / 2) >> 15; }
static int64_t scale(int64_t x, int64_t d) {
    if (d == 0) return x;
    if (d < 0) return rnd(x * (Q + d));
    return rnd(x * (Q + rnd((Q - x) * d)));
}

static uint32_t want_pixel(int r, int g, int b, int64_t dhq, int64_t dsq, int64_t dvq) {
    const int64_t M = r > g ? (r > b ? r : b) : (g > b ? g : b), m = r < g ? (r < b ? r : b) : (g < b ? g : b), C = M - m;
    int64_t hq = 0;
    if (C != 0) {
        int64_t base, num;
        if (M == b) { base = 4; num = r - g; } else if (M == g) { base = 2; num = b - r; } else { base = 0; num = g - b; }
        hq = (base * Q + rdiv((num + C) * Q, C) - Q) % (6 * Q);
        if (hq < 0) hq += 6 * Q;
    }
    const int64_t s = M == 0 ? 0 : rdiv(C * Q, M), v = rdiv(M * Q, 255);
    hq = (hq + dhq) % (6 * Q);
    const int64_t s2 = scale(s, dsq), v2 = scale(v, dvq);
    const int64_t hi = hq / Q, fq = hq - hi * Q;
    const int64_t p = rnd(v2 * (Q - s2)), q = rnd(v2 * (Q - rnd(fq * s2))), t = rnd(v2 * (Q - rnd((Q - fq) * s2)));
    int64_t R, G, B;
    switch (hi) {
        case 0: R = v2; G = t; B = p; break;
        case 1: R = q; G = v2; B = p; break;
        case 2: R = p; G = v2; B = t; break;
        case 3: R = p; G = q; B = v2; break;
        case 4: R = t; G = p; B = v2; break;
        default: R = v2; G = p; B = q; break;
    }
    const int64_t o[3] = {(R * 255 + Q / 2) >> 15, (G * 255 + Q / 2) >> 15, (B * 255 + Q / 2) >> 15};
    for (int k = 0; k < 3; ++k)
        if (o[k] < 0 || o[k] > 255) return 0xffffffffu;          // (never equal to a packed pixel)
    return (uint32_t)(o[0] | (o[1] << 8) | (o[2] << 16));
}

static void check_div(uint32_t num, uint32_t den) {
    const float exact = 1.0f / (float)den;
    float lo = exact, hi = exact;
    for (int k = 0; k < 2; ++k) { lo = std::nextafterf(lo, 0.0f); hi = std::nextafterf(hi, 1.0f); }
    const uint32_t want = num / den;
    const float rs[3] = {exact, lo, hi};
    for (float rden : rs) CHECK(hsb_div(num, den, rden) == want, "hsb_div(%u, %u, %a) = %u, want %u", num, den, (double)rden, hsb_div(num, den, rden), want);
}

int main() {
    // the divisions
    for (int C = 1; C <= 255; ++C)
        for (int num = -C; num <= C; ++num) check_div((uint32_t)((num + C) * 2 * (int)Q + C), (uint32_t)(2 * C));
    for (int M = 1; M <= 255; ++M)
        for (int C = 0; C <= M; ++C) check_div((uint32_t)(2 * C * (int)Q + M), (uint32_t)(2 * M));
    for (int M = 0; M <= 255; ++M) check_div((uint32_t)(2 * M * (int)Q + 255), 510u);
    // the scale
    const int32_t ds[] = {-32768, -32767, -29491, -16384, -3277, -1, 0, 1, 3277, 16384, 21627, 32767, 32768};
    for (int32_t d : ds)
        for (int64_t x = 0; x <= Q; ++x) {
            const uint32_t got = hsb_scale((uint32_t)x, d);
            CHECK((int64_t)got == scale(x, d) && got <= (uint32_t)Q, "hsb_scale(%lld, %d) = %u, want %lld", (long long)x, d, got, (long long)scale(x, d));
        }
    // the pixel
    const int32_t codes[][3] = {{0, 0, 0}, {6 * 32768 - 1, 32768, 32768}, {32768, -32768, -32768}, {2 * 32768, 0, 0}, {3 * 32768, 32768, -32768},
                                {4 * 32768, -32768, 32768}, {5 * 32768, 1, -1}, {1, -1, 1}, {19661, 3277, 0}, {176947, -3277, 0},
                                {98304 + 777, 21627, -29491}, {32768 / 2, 16384, 16384}};
    for (const auto& c : codes) {
        int32_t dhq, dsq, dvq;
        hsb_reduce_codes(c, dhq, dsq, dvq);
        CHECK(dhq == c[0] && dsq == c[1] && dvq == c[2], "codes in range must stay as they are");
        for (int r = 0; r < 256; r += (r < 4 || r >= 250) ? 1 : 3)
            for (int g = 0; g < 256; g += (g < 4 || g >= 250) ? 1 : 3)
                for (int b = 0; b < 256; b += (b < 4 || b >= 250) ? 1 : 3) {
                    const uint32_t px = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
                    const uint32_t got = hsb_pixel(px, dhq, dsq, dvq), want = want_pixel(r, g, b, c[0], c[1], c[2]);
                    CHECK(got == want, "hsb_pixel(%d, %d, %d; %d, %d, %d) = %06x, want %06x", r, g, b, c[0], c[1], c[2], got, want);
                    if (c[0] == 0 && c[1] == 0 && c[2] == 0) CHECK(got == px, "zero codes must be the identity: (%d, %d, %d) -> %06x", r, g, b, got);
                }
    }
    // the reduction of codes out of range
    const int32_t wild[][3] = {{-1, 40000, -40000}, {6 * 32768, 32769, -32769}, {-6 * 32768 - 5, 2147483647, -2147483647 - 1}, {2147483647, 0, 0}};
    for (const auto& c : wild) {
        int32_t dhq, dsq, dvq;
        hsb_reduce_codes(c, dhq, dsq, dvq);
        int64_t h = (int64_t)c[0] % (6 * Q);
        if (h < 0) h += 6 * Q;
        const int64_t s = c[1] < -Q ? -Q : (c[1] > Q ? Q : c[1]), v = c[2] < -Q ? -Q : (c[2] > Q ? Q : c[2]);
        CHECK(dhq == h && dsq == s && dvq == v, "hsb_reduce_codes(%d, %d, %d) = (%d, %d, %d)", c[0], c[1], c[2], dhq, dsq, dvq);
    }
    printf("%ld checks, %ld failures\n", checked, failures);
    return failures ? 1 : 0;
}
