// hsb_math.hpp -- the hue / saturation / brightness map of one pixel in 32-bit integers (an extension: HsbColorAugmenter).  Host and
// device; included alone by tests/hsb_math_check.cpp, which compares it with a 64-bit restatement of the definition.
//
// Definition (stainlib_amd/augmentation/hsb.py: hsb_reference).  Q = 32768, rdiv(a, c) = (2 a + c) / (2 c), rnd(x) = (x + Q / 2) >> 15.
// Per pixel M = max, m = min, C = M - m;  hq = 0 (C == 0) else (base Q + rdiv((num + C) Q, C) - Q) mod 6 Q with (base, num) =
// (4, r - g) if M == b, else (2, b - r) if M == g, else (0, g - b);  s = rdiv(C Q, M) (0 for M == 0);  v = rdiv(M Q, 255);
// scale(x, d) = rnd(x (Q + d)) for d < 0, rnd(x (Q + rnd((Q - x) d))) for d > 0 (either form is x at d == 0: rnd(x Q) = x);
// hq' = (hq + dhq) mod 6 Q, s' = scale(s, dsq), v' = scale(v, dvq), hi = hq' / Q, fq = hq' - hi Q;
// p = rnd(v' (Q - s')), q = rnd(v' (Q - rnd(fq s'))), t = rnd(v' (Q - rnd((Q - fq) s')));  (R, G, B) by hi: 0 (v', t, p), 1 (q, v', p),
// 2 (p, v', t), 3 (p, q, v'), 4 (t, p, v'), 5 (v', p, q);  byte = (X 255 + Q / 2) >> 15.
//
// Ranges: every product is below 2^31 + 2^14 and is computed unsigned (x (Q + ...) reaches Q 2 Q = 2^31); both factors of every product
// are at most 2 Q + 1 < 2^24 (hsb_mul).  The three divisions are by 2 C, 2 M (2 .. 510) and 510, of numerators below 2^25 + 2^9 with quotients at most 2 Q + 1: hsb_div multiplies by a binary32
// reciprocal -- three roundings of 2^-23 relative at most, 0.02 on such a quotient, so the truncated product is within one of the
// quotient -- and one remainder test each way makes it the floor division.  An even sextant uses t and never q, an odd one q and never t,
// so one of the two is computed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SL_HSB_HD __host__ __device__ inline
#else
#define SL_HSB_HD inline
#endif

namespace sl {

constexpr int32_t kHsbQ = 32768;

// 1 / x in binary32, within one unit in the last place (v_rcp_f32 on the device; hsb_div needs no more)
SL_HSB_HD float hsb_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// a b for a, b < 2^24 with a product below 2^32 -- every product of the map: v_mul_u32_u24 on the device (full rate; the 32-bit
// v_mul_lo_u32 issues at a quarter of it), the plain product on the host
SL_HSB_HD uint32_t hsb_mul(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// num / den (floor) for num < 2^25 + 2^9, den in 2 .. 510 and a quotient of at most 2 Q + 1; rden = 1 / float(den) within one unit in
// the last place (the check program goes two units either side)
SL_HSB_HD uint32_t hsb_div(uint32_t num, uint32_t den, float rden) {
    uint32_t q = (uint32_t)((float)num * rden);
    const int32_t r = (int32_t)(num - hsb_mul(q, den));
    q = r < 0 ? q - 1u : (r >= (int32_t)den ? q + 1u : q);
    return q;
}

SL_HSB_HD uint32_t hsb_rnd(uint32_t x) { return (x + (uint32_t)(kHsbQ / 2)) >> 15; }

// x in [0, Q] moved by the code d in [-Q, Q]: towards 0 for d < 0, towards Q and never past it for d > 0
SL_HSB_HD uint32_t hsb_scale(uint32_t x, int32_t d) {
    const uint32_t Q = (uint32_t)kHsbQ;
    const uint32_t up = Q + hsb_rnd(hsb_mul(Q - x, (uint32_t)(d > 0 ? d : 0)));
    const uint32_t e = d < 0 ? (uint32_t)(kHsbQ + d) : up;
    return hsb_rnd(hsb_mul(x, e));
}

// the codes of a tile as the kernels take them: dhq mod 6 Q (non-negative), dsq and dvq clamped to +-Q
SL_HSB_HD void hsb_reduce_codes(const int32_t* in, int32_t& dhq, int32_t& dsq, int32_t& dvq) {
    int32_t h = in[0] % (6 * kHsbQ);
    dhq = h < 0 ? h + 6 * kHsbQ : h;
    dsq = in[1] < -kHsbQ ? -kHsbQ : (in[1] > kHsbQ ? kHsbQ : in[1]);
    dvq = in[2] < -kHsbQ ? -kHsbQ : (in[2] > kHsbQ ? kHsbQ : in[2]);
}

// the packed pixel r | g << 8 | b << 16 under reduced codes -> the packed pixel
SL_HSB_HD uint32_t hsb_pixel(uint32_t px, int32_t dhq, int32_t dsq, int32_t dvq) {
    const int32_t Q = kHsbQ;
    const int32_t r = (int32_t)(px & 0xffu), g = (int32_t)((px >> 8) & 0xffu), b = (int32_t)((px >> 16) & 0xffu);
    const int32_t gb_max = g > b ? g : b, gb_min = g < b ? g : b;
    const int32_t M = r > gb_max ? r : gb_max, m = r < gb_min ? r : gb_min, C = M - m;
    const int32_t Cs = C > 1 ? C : 1, Ms = M > 1 ? M : 1;
    const bool is_b = M == b, is_g = M == g;
    const int32_t base = is_b ? 4 * Q : (is_g ? 2 * Q : 0);
    const int32_t num = is_b ? r - g : (is_g ? b - r : g - b);
    // hue: rdiv((num + C) Q, C) = ((num + C) 2 Q + C) / (2 C)
    const uint32_t dq = hsb_div((uint32_t)((num + C) * 2 * Q + C), (uint32_t)(2 * Cs), hsb_rcp((float)(2 * Cs)));
    int32_t hq = base + (int32_t)dq - Q;
    hq = hq < 0 ? hq + 6 * Q : hq;
    hq = C == 0 ? 0 : hq;
    // saturation (C == 0 gives 0 by itself, M == 0 included) and value
    const uint32_t s = hsb_div((uint32_t)(2 * C * Q + M), (uint32_t)(2 * Ms), hsb_rcp((float)(2 * Ms)));
    const uint32_t v = hsb_div((uint32_t)(2 * M * Q + 255), 510u, 1.0f / 510.0f);
    // the shifts
    hq += dhq;
    hq = hq >= 6 * Q ? hq - 6 * Q : hq;
    const uint32_t s2 = hsb_scale(s, dsq), v2 = hsb_scale(v, dvq);
    const uint32_t hi = (uint32_t)hq >> 15, fq = (uint32_t)hq & (uint32_t)(Q - 1);
    const uint32_t uq = (uint32_t)Q;
    const uint32_t p = hsb_rnd(hsb_mul(v2, uq - s2));
    const uint32_t f = (hi & 1u) ? fq : uq - fq;                    // odd sextant: q; even: t
    const uint32_t qt = hsb_rnd(hsb_mul(v2, uq - hsb_rnd(hsb_mul(f, s2))));
    // (R, G, B) by hi: 0 (v, t, p), 1 (q, v, p), 2 (p, v, t), 3 (p, q, v), 4 (t, p, v), 5 (v, p, q)
    const uint32_t R = (hi == 0u || hi == 5u) ? v2 : ((hi == 1u || hi == 4u) ? qt : p);
    const uint32_t G = (hi == 1u || hi == 2u) ? v2 : ((hi == 0u || hi == 3u) ? qt : p);
    const uint32_t B = (hi == 3u || hi == 4u) ? v2 : ((hi == 2u || hi == 5u) ? qt : p);
    const uint32_t half = (uint32_t)(Q / 2);
    return ((hsb_mul(R, 255u) + half) >> 15) | (((hsb_mul(G, 255u) + half) >> 15) << 8) | (((hsb_mul(B, 255u) + half) >> 15) << 16);
}

}  // namespace sl
