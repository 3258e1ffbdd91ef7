// post_math.hpp -- the post stage of one output pixel in 32-bit integers (an extension: GaussianNoiseAugmenter, ToneCurveAugmenter): the
// counter-based generator, the noise value, the scale-and-clamp, the code reduction and the pixel index of a write-side lane.  Host and
// device, plain C++; included alone by tests/post_math_check.cpp, which compares it with a 64-bit restatement of the definition.
//
// Definition (stainlib_amd/augmentation/noise.py: post_reference).  Pixel p = i ow + j of the image the stage acts on, channel c, byte b:
//   tone    b1 = table[b], the tile's 256 bytes, the same for the three channels
//   noise   W = philox4x32_10(counter (p, 0, 0, 0), key (k0, k1)) -- the published Philox4x32-10: multipliers 0xD2511F53 / 0xCD9E8D57,
//           Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds, the key bumped between rounds;  channel c takes W[c], or W[3] for all
//           three when mono != 0;  G = (the sum of the word's four bytes) - 510, in [-510, 510], mean 0, variance 21845;
//           n = (G sq + 32768) >> 16 (arithmetic),  b2 = clamp(b1 + n, 0, 255);  sq in [0, kPostSqMax], |G sq| < 2^24;  sq == 0: b2 = b1.
// The key schedule (twenty words) depends on the tile alone: the kernels compute it once per workgroup, on uniform values.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SL_POST_HD __host__ __device__ inline
#else
#define SL_POST_HD inline
#endif

namespace sl {

constexpr int32_t kPostSqMax = 28378;            // floor(64 * 65536 / sqrt(21845) + 1/2): sigma = 64 bytes
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// the round keys of key (k0, k1): ks[2 r], ks[2 r + 1] for round r
SL_POST_HD void philox_schedule(uint32_t k0, uint32_t k1, uint32_t (&ks)[20]) {
    for (int r = 0; r < 10; ++r) {
        ks[2 * r] = k0 + (uint32_t)r * kPhiloxW0;
        ks[2 * r + 1] = k1 + (uint32_t)r * kPhiloxW1;
    }
}

// Philox4x32-10 of the counter (c0, c1, c2, c3) under a key schedule
SL_POST_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, const uint32_t (&ks)[20], uint32_t (&out)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ ks[2 * r], n2 = (uint32_t)(p0 >> 32) ^ c3 ^ ks[2 * r + 1];
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the sum of a word's four bytes: one sum of absolute differences against zero on the device
SL_POST_HD uint32_t post_byte_sum(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(w, 0u, 0u);
#else
    return (w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24);
#endif
}

// G of a word: in [-510, 510]
SL_POST_HD int32_t post_g(uint32_t w) { return (int32_t)post_byte_sum(w) - 510; }

// a byte moved by the noise value G under the reduced code sq
SL_POST_HD uint32_t post_add(uint32_t b1, int32_t G, int32_t sq) {
    const int32_t v = (int32_t)b1 + ((G * sq + 32768) >> 16);
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// sq of a tile as the kernels take it: clamped to [0, kPostSqMax]
SL_POST_HD int32_t post_reduce_sq(int32_t sq) { return sq < 0 ? 0 : (sq > kPostSqMax ? kPostSqMax : sq); }

// the noise of the packed pixel r | g << 8 | b << 16 at pixel index p (sq reduced and non-zero)
SL_POST_HD uint32_t post_noise_pixel(uint32_t px, uint32_t p, const uint32_t (&ks)[20], int32_t sq, bool mono) {
    uint32_t W[4];
    philox4x32_10(p, 0u, 0u, 0u, ks, W);
    const int32_t g3 = post_g(W[3]);
    const int32_t g0 = mono ? g3 : post_g(W[0]), g1 = mono ? g3 : post_g(W[1]), g2 = mono ? g3 : post_g(W[2]);
    return post_add(px & 0xffu, g0, sq) | (post_add((px >> 8) & 0xffu, g1, sq) << 8) | (post_add((px >> 16) & 0xffu, g2, sq) << 16);
}

// The pixels a lane of a view's write side holds: the lane has the outputs (il, jl .. jl + 3) of a patch at (i0, j0) of bh x bw pixels in an
// output ow wide.  -> how many of the four exist (0: the lane holds none and the stage does nothing); p0: the pixel index of the first.
SL_POST_HD int post_lane(int i0, int j0, int bh, int bw, int ow, int il, int jl, uint32_t& p0) {
    const int left = bw - jl;
    if (il >= bh || left <= 0) return 0;
    p0 = (uint32_t)(i0 + il) * (uint32_t)ow + (uint32_t)(j0 + jl);
    return left < 4 ? left : 4;
}

}  // namespace sl
