// lab_device.hpp -- device helpers of the OpenCV 8-bit Lab family shared by lab.hip (per tile) and slide_lab.hip (per slide): the
// conversion tables and functions restated from OpenCV's published color_lab.cpp (tables: gen_tables.py), the histogram scratch and
// the numbers the reference derives from it (np.percentile, cv2.meanStdDev), numpy's clip-then-truncate.
#pragma once
#include "apply_kernels.hpp"

namespace sl {

static __device__ const uint16_t d_lab_cbrt[3072] = {SL_LAB_CBRT_VALUES};   // OpenCV LabCbrtTab_b
static __device__ const uint16_t d_lab_yf[512] = {SL_LAB_YF_VALUES};        // OpenCV LabToYF_b: (y, f(y)) per L8
static __device__ const uint8_t d_inv_gamma[4096] = {SL_INV_GAMMA_VALUES};  // OpenCV sRGBInvGammaTab_b

struct LabTabs {
    uint16_t gamma[256];
    uint16_t cbrt[3072];
    uint16_t yf[512];
    uint8_t invg[4096];
    __device__ __forceinline__ void fill() {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) gamma[i] = (uint16_t)d_gamma[i];
        for (int i = threadIdx.x; i < 3072; i += blockDim.x) cbrt[i] = d_lab_cbrt[i];
        for (int i = threadIdx.x; i < 512; i += blockDim.x) yf[i] = d_lab_yf[i];
        for (int i = threadIdx.x; i < 4096; i += blockDim.x) invg[i] = d_inv_gamma[i];
    }
};

// the static tables a sweep needs, without the ones its per-tile tables (LabTileTabs) already contain
struct LabCbrt {              // RGB -> Lab8 behind a per-tile gamma table
    uint16_t cbrt[3072];
    __device__ __forceinline__ void fill() {
        for (int i = threadIdx.x; i < 3072 / 2; i += blockDim.x) ((uint32_t*)cbrt)[i] = ((const uint32_t*)d_lab_cbrt)[i];
    }
};
struct LabCbrtInv {           // ... and back through per-tile yf / a / b tables
    uint16_t cbrt[3072];
    uint8_t invg[4096];
    __device__ __forceinline__ void fill() {
        for (int i = threadIdx.x; i < 3072 / 2; i += blockDim.x) ((uint32_t*)cbrt)[i] = ((const uint32_t*)d_lab_cbrt)[i];
        for (int i = threadIdx.x; i < 4096 / 4; i += blockDim.x) ((uint32_t*)invg)[i] = ((const uint32_t*)d_inv_gamma)[i];
    }
};

// Compiler hazard (hipcc 7.2, gfx950): clamp(x >> n, 0, 255) of two values is selected as ONE v_ashr_pk_u8_i32, whose result the
// compiler then ORs into a word as if bits 31:16 were zero -- on the hardware they are not (found by the exhaustive Lab test:
// bytes 2 of every packed word came out with stray bits).  The empty asm keeps the shift and the clamp apart.
__device__ __forceinline__ int sat8(int v) {
    asm("" : "+v"(v));
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// OpenCV RGB2Lab_b::operator(): coefficients cvRound(4096 * sRGB2XYZ_D65[i][j] / whitePt[i]), lab_shift 12, lab_shift2 15.
// R, G, Bc are the gamma-table values of the three bytes (the sweeps read them from a per-tile table that already
// contains the brightness table: gamma[lut[v]]).
template <class T>
__device__ __forceinline__ void gamma_to_lab8(const T& t, int R, int G, int Bc, int& L, int& A, int& B) {
    // (24-bit multiplies: the gamma values stay below 2^11, the cube-root values below 2^16, every product below 2^31 -- the compiler
    //  cannot see the ranges behind the table reads and would issue twelve full-width multiplies at a quarter of the vector rate)
    const int fX = t.cbrt[(__mul24(R, 1777) + __mul24(G, 1541) + __mul24(Bc, 778) + 2048) >> 12];
    const int fY = t.cbrt[(__mul24(R, 871) + __mul24(G, 2929) + __mul24(Bc, 296) + 2048) >> 12];
    const int fZ = t.cbrt[(__mul24(R, 73) + __mul24(G, 448) + __mul24(Bc, 3575) + 2048) >> 12];
    L = sat8((__mul24(296, fY) - 1336934 + 16384) >> 15);
    A = sat8((__mul24(500, fX - fY) + 128 * 32768 + 16384) >> 15);
    B = sat8((__mul24(200, fY - fZ) + 128 * 32768 + 16384) >> 15);
}
__device__ __forceinline__ void rgb_to_lab8(const LabTabs& t, uint32_t r, uint32_t g, uint32_t b, int& L, int& A, int& B) {
    gamma_to_lab8(t, t.gamma[r], t.gamma[g], t.gamma[b], L, A, B);
}

// OpenCV abToXZ_b[i - minABvalue] evaluated instead of stored (36864 entries): C integer arithmetic, division truncates.
// Both branches are evaluated for every lane; the cubic one only counts for i > 3390, where every operand is positive and
// the two divisions by 16384 are plain shifts (as signed divisions they cost a sign fix-up each).
// The truncating division by 841 (a full-width multiply-high and a multiply-low at a quarter of the vector rate each, plus
// the sign fix-up) is done in binary32 instead: x = 108 i is exact there (|x| < 2^23), x * (1/841) is off by at most
// 1.3e-4 in the range the linear branch is used (|x / 841| < 1100), and exact quotients keep 1/841 = 1.19e-3 away from the
// integers they do not hit -- so truncating x/841 pushed half of 1/841 away from zero gives C's quotient for every x.
__device__ __forceinline__ int ab_to_xz(int i) {
    const float xf = (float)__mul24(i, 108);                  // (|i| < 2^17: a 24-bit multiply, the full-width one runs at quarter rate)
    const int lin = (int)fmaf(xf, 1.0f / 841.0f, copysignf(0.5f / 841.0f, xf)) - 290;     // (i * 108) / 841 - 290;  290 = BASE*16/116*108/841
    const uint32_t u = (uint32_t)i;                       // (i < 2^17, (i*i) >> 14 < 2^20: 24-bit multiplies, the full-width ones run at quarter rate)
    const int cub = (int)(__umul24(__umul24(u, u) >> 14, u) >> 14);
    return i <= 3390 ? lin : cub;
}

// OpenCV Lab2RGBinteger::process: coefficients cvRound(4096 * XYZ2sRGB_D65[i][j] * whitePt[j]), shift 14.
// lab_adiv / lab_bdiv: the a and b bytes on the table's scale (128*BASE/500 = 4194, 128*BASE/200 = 10485).
__device__ __forceinline__ int lab_adiv(int a) { return ((5 * a * 53687 + 128) >> 13) - 4194; }
__device__ __forceinline__ int lab_bdiv(int b) { return ((b * 41943 + 16) >> 9) - 10485 + 1; }
template <class T>
__device__ __forceinline__ void yf_to_rgb(const T& t, int y, int ify, int adiv, int bdiv, uint32_t& r, uint32_t& g, uint32_t& bl) {
    const int x = ab_to_xz(ify + adiv), z = ab_to_xz(ify - bdiv);
    // x, z < 2^17 (ab_to_xz of an argument below 2^15 + 2^14), y < 2^15: 24-bit multiplies (the compiler cannot see the ranges and
    // would issue full-width ones at a quarter of the rate); every sum stays below 2^31 as in OpenCV's int arithmetic
    int ro = (__mul24(12615, x) - __mul24(6296, y) - __mul24(2223, z) + 8192) >> 14;
    int go = (__mul24(-3773, x) + __mul24(7684, y) + __mul24(185, z) + 8192) >> 14;
    int bo = (__mul24(217, x) - __mul24(836, y) + __mul24(4715, z) + 8192) >> 14;
    ro = ro < 0 ? 0 : (ro > 4095 ? 4095 : ro);
    go = go < 0 ? 0 : (go > 4095 ? 4095 : go);
    bo = bo < 0 ? 0 : (bo > 4095 ? 4095 : bo);
    r = t.invg[ro]; g = t.invg[go]; bl = t.invg[bo];
}
__device__ __forceinline__ void lab8_to_rgb(const LabTabs& t, int L, int a, int b, uint32_t& r, uint32_t& g, uint32_t& bl) {
    yf_to_rgb(t, t.yf[2 * L], t.yf[2 * L + 1], lab_adiv(a), lab_bdiv(b), r, g, bl);
}

__device__ __forceinline__ Chunk pack12(const uint32_t (&ob)[12]) {
    Chunk o;
    o.w0 = ob[0] | (ob[1] << 8) | (ob[2] << 16) | (ob[3] << 24);
    o.w1 = ob[4] | (ob[5] << 8) | (ob[6] << 16) | (ob[7] << 24);
    o.w2 = ob[8] | (ob[9] << 8) | (ob[10] << 16) | (ob[11] << 24);
    return o;
}

// uint8(clip(x, 0, 255)) of numpy: clip, then truncate toward zero (NaN -> 0)
__device__ __forceinline__ uint32_t clip_trunc_u8(double x) { return (uint32_t)fmin(fmax(x, 0.0), 255.0); }

// Per-tile scratch (workspace): histograms as uint64 (3 * 2^30 bytes per tile overflow 32 bits)
struct LabScratch {
    unsigned long long bytes[256];      // all byte values of the tile
    unsigned long long lab_l[256];      // L8 of the (optionally brightness-standardised) tile
    unsigned long long ab[4];           // sum a8, sum a8^2, sum b8, sum b8^2 (a - 128 and b - 128 are affine in the byte: no histogram needed)
    unsigned long long tissue;          // pixels of the standardised tile passing the luminosity test
    unsigned long long pad_[3];
};

// np.percentile(values, pct) (linear interpolation) of the integer population described by a 256-bin histogram; one thread
__device__ inline double percentile_of_hist(const unsigned long long* hist, double pct) {
    unsigned long long n = 0;
    for (int v = 0; v < 256; ++v) n += hist[v];
    if (n == 0) return nan("");
    long long k;
    double g;
    percentile_pos((double)n, pct, k, g);
    const unsigned long long k2 = (unsigned long long)k + 1 < n ? (unsigned long long)k + 1 : (unsigned long long)k;
    int va = -1, vb = -1;
    unsigned long long cum = 0;
    for (int v = 0; v < 256; ++v) {
        cum += hist[v];
        if (va < 0 && cum > (unsigned long long)k) va = v;
        if (vb < 0 && cum > k2) { vb = v; break; }
    }
    return np_lerp((double)va, (double)vb, g);
}

// largest L8 that still counts as tissue, +1:  L8 / 255.0 < threshold  (stain_utils.py:42-43)
__device__ __forceinline__ int l8_limit(double thr) {
    int lim = 0;
    for (int v = 0; v < 256; ++v)
        if ((double)v / 255.0 < thr) lim = v + 1;
    return lim;
}

// cv2.meanStdDev of a lab_split plane (stain_utils.py:153-157): sums in binary64, population variance clamped at 0.  One thread.
// L: value(v) = binary32 v / 2.55f as lab_split makes it, from the histogram of L8.  a, b: value = byte - 128, so the two
// sums follow exactly from the integer sums of the byte and its square (every term is an integer below 2^53).
__device__ inline void mean_std_of_scratch(const LabScratch& sc, int channel, double& mean, double& sd) {
    double n = 0, s1 = 0, s2 = 0;
    for (int v = 0; v < 256; ++v) {
        const double c = (double)sc.lab_l[v];
        n += c;
        if (channel == 0) {
            const double x = (double)((float)v / 2.55f);
            s1 += c * x; s2 += c * x * x;
        }
    }
    if (channel != 0) {
        const double sv = (double)sc.ab[2 * (channel - 1)], svv = (double)sc.ab[2 * (channel - 1) + 1];
        s1 = sv - 128.0 * n;
        s2 = svv - 256.0 * sv + 16384.0 * n;
    }
    mean = s1 / n;
    const double var = s2 / n - mean * mean;
    sd = sqrt(var > 0.0 ? var : 0.0);
}

}  // namespace sl
