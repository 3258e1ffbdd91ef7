// lab_device.hpp -- device helpers of the OpenCV 8-bit Lab family shared by lab.hip (per tile) and slide_lab.hip (per slide): the
// conversion tables and functions restated from OpenCV's published color_lab.cpp (tables: gen_tables.py), the histogram scratch and
// the numbers the reference derives from it (np.percentile, cv2.meanStdDev), numpy's clip-then-truncate, and everything the reference
// computes around the conversions: the byte-table formulas, the composed tables, the map of four pixels, the sweep loop.  The two
// files keep their partitions of the pixels (tile x part; one flat span per workgroup), their kernels and their entry points.
// lab_view_kernels.hpp puts the map of four pixels between the read side and the LDS stage of the view pass (tile x run of patches).
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

// the static tables a sweep needs, without the ones its composed tables (LabMapTabs) already contain
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

// The same number by a 256-thread workgroup, one test per thread (thread = L8) instead of 256 per thread: the test is monotone in v, so
// the limit is the count of values that pass.  l8_limit_begin before a barrier, l8_limit_end behind it; s_cnt: one int per wave.
// (For a workgroup that maps 16 Ki pixels the serial loop -- 256 binary64 divisions per thread -- costs as much as its pixels.)
__device__ __forceinline__ void l8_limit_begin(double thr, int* s_cnt) {
    const int v = threadIdx.x;
    const unsigned long long pass = __ballot((double)v / 255.0 < thr);
    if ((v & 63) == 0) s_cnt[v >> 6] = __popcll(pass);
}
__device__ __forceinline__ int l8_limit_end(const int* s_cnt) { return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]; }

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

// ---- the byte tables around the conversions: every per-pixel float expression of the reference has a uint8 argument, so each is
// ---- evaluated once per byte value in binary64, in the reference's operation order, by a 256-thread workgroup (thread = byte) ------
// The composed tables a map sweep looks up: per tile in the workspace (LabTileTabs, lab.hip), once per slide in the state
// (state[SL_SLAB_TABLES ...], slide_lab.hip).  Written once by the two kernels between the sweeps, loaded by every workgroup.
struct LabMapTabs {
    uint32_t yf[256];         // L8 -> (y, f(y)) of the MAPPED L byte, packed
    int ad[256], bd[256];     // a8 / b8 -> the mapped byte on abToXZ's scale
    uint16_t g[256];          // byte -> gamma value, through the brightness table where the op standardises
    uint8_t lut[256];         // the brightness table (identity when the op does not standardise)
};

// Per-tile composed tables (workspace, behind the LabScratch array): written ONCE per tile by k_lab_pre / k_lab_tables and loaded by every
// workgroup of the sweeps that follow.  (Round 5: until then every workgroup of k_lab_hist / k_lab_map rebuilt them -- a serial
// percentile over 256 global counters, three mean/std loops in binary64, five table passes -- before it touched a pixel: ~20 us of a
// workgroup's ~450, which also kept the sweeps from being cut into workgroups small enough to fill the last round.)
struct LabTileTabs : LabMapTabs {
    double p;                 // the percentile the op reports (p90 of the bytes / the L percentile of MODE 1)
    double pad_;
};
static_assert(sizeof(LabTileTabs) == sizeof(LabMapTabs) + 16, "the workspace sizes rest on it");

// standardize_brightness (stain_utils.py:193-194): uint8(clip(v * 255.0 / p, 0, 255)); identity when the op does not standardise
__device__ __forceinline__ uint32_t brightness_byte(int v, double p, int standardize) {
    return standardize ? clip_trunc_u8((double)v * 255.0 / p) : (uint32_t)v;
}
// ReinhardStainNormalizer.transform (normalizer.py:81-83) in binary64: ((x - mean) * (tstd / std)) + tmean; merge_back
// (stain_utils.py:168-171): * 2.55 resp. + 128.0, clip, truncate.  x is the binary32 value lab_split produced, promoted.  Every
// operation rounds on its own, as numpy's do: contracted, (x - mean) * ratio + tmean becomes one v_fma_f64 with one rounding.
__device__ __forceinline__ uint32_t reinhard_byte(int ch, int v, double mean, double sd, double tmean, double tstd) {
#pragma clang fp contract(off)
    const double ratio = tstd / sd;
    const double x = ch == 0 ? (double)((float)v / 2.55f) : (double)((float)v - 128.0f);
    const double nrm = ((x - mean) * ratio) + tmean;
    return clip_trunc_u8(ch == 0 ? nrm * 2.55 : nrm + 128.0);
}
// LuminosityStandardizer (stain_utils.py:65): 255 * L_float / p
__device__ __forceinline__ uint32_t luminosity_byte(int v, double p) { return clip_trunc_u8(255.0 * (double)v / p); }
// a mapped Lab byte triple composed with the conversion tables the pixel path would look up next (lab8_to_rgb's first step)
__device__ __forceinline__ void lab_compose(int L2, int A2, int B2, uint32_t& yf, int& ad, int& bd) {
    yf = (uint32_t)d_lab_yf[2 * L2] | ((uint32_t)d_lab_yf[2 * L2 + 1] << 16);
    ad = lab_adiv(A2);
    bd = lab_bdiv(B2);
}

// After sweep A: the 90th percentile of the byte histogram (NaN when !standardize), the brightness table and the gamma values behind
// it (what sweep B needs).  Returns the percentile to every thread.
__device__ __forceinline__ double lab_begin_tables(LabMapTabs& tt, const unsigned long long* bytes, int standardize) {
    __shared__ double s_p;
    const int v = threadIdx.x;
    if (v == 0) s_p = standardize ? percentile_of_hist(bytes, 90.0) : nan("");
    __syncthreads();
    const uint32_t lut = brightness_byte(v, s_p, standardize);
    tt.lut[v] = (uint8_t)lut;
    tt.g[v] = (uint16_t)d_gamma[lut];
    return s_p;
}
// After sweep B: the map's tables from the statistics.  mode 0 Reinhard (ms = means L, a, b, stds L, a, b), 1 luminosity (p = the L
// percentile; a and b stay).
__device__ __forceinline__ void lab_finish_tables(LabMapTabs& tt, int mode, const double* ms, const double* tmeans, const double* tstds, double p) {
    const int v = threadIdx.x;
    int L2, A2 = v, B2 = v;
    if (mode == 0) {
        L2 = (int)reinhard_byte(0, v, ms[0], ms[3], tmeans[0], tstds[0]);
        A2 = (int)reinhard_byte(1, v, ms[1], ms[4], tmeans[1], tstds[1]);
        B2 = (int)reinhard_byte(2, v, ms[2], ms[5], tmeans[2], tstds[2]);
    } else {
        L2 = (int)luminosity_byte(v, p);
    }
    lab_compose(L2, A2, B2, tt.yf[v], tt.ad[v], tt.bd[v]);
}

// ---- the map: four pixels through the tables ----------------------------------------------------------------------------------
// background of mask_background (normalizer.py:86-90): 254 + 0 on the L/2.55 scale -> clips to 255; a = b = 0 + 128
struct LabBackground { uint32_t yf; int ad, bd; };
__device__ __forceinline__ LabBackground lab_background() {
    LabBackground bg;
    lab_compose(255, 128, 128, bg.yf, bg.ad, bg.bd);
    return bg;
}
// gamma (through the brightness table) -> Lab8 -> the tables -> background -> RGB, packed.  AB_TABLES: a and b are mapped (tables ad,
// bd); otherwise they stay and go straight onto abToXZ's scale (three operations each).  The tables are the workgroup's LDS copies.
template <bool AB_TABLES, class T>
__device__ __forceinline__ Chunk lab_map_chunk(const T& t, const uint16_t* g, const uint32_t* yf_tab, const int* ad_tab, const int* bd_tab,
                                               const Chunk& in, bool mask_bg, int lim, const LabBackground& bg) {
    uint32_t ob[12];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        int L, A, B;
        gamma_to_lab8(t, g[chunk_byte(in, 3 * px)], g[chunk_byte(in, 3 * px + 1)], g[chunk_byte(in, 3 * px + 2)], L, A, B);
        uint32_t yf = yf_tab[L];
        int ad = AB_TABLES ? ad_tab[A] : lab_adiv(A), bd = AB_TABLES ? bd_tab[B] : lab_bdiv(B);
        if (mask_bg) {
            const bool is_bg = !(L < lim);
            yf = is_bg ? bg.yf : yf; ad = is_bg ? bg.ad : ad; bd = is_bg ? bg.bd : bd;
        }
        yf_to_rgb(t, (int)(yf & 0xffffu), (int)(yf >> 16), ad, bd, ob[3 * px], ob[3 * px + 1], ob[3 * px + 2]);
    }
    return pack12(ob);
}

// ---- the sweeps ---------------------------------------------------------------------------------------------------------------
// A run of 12-byte chunks `off` bytes into the batch (`src` points there), `nbytes` long: `nloc` chunks of which only the last can be
// ragged (0 chunks: nothing to do).  slide_lab.hip cuts the shard into one run per workgroup; for lab.hip the run is the tile and a
// workgroup takes the chunks of its part.
struct ChunkSpan { const uint8_t* src; size_t off; size_t nbytes; int nloc; };
// Chunks [c0, nloc) of a run, two per lane in flight: the next trip's are requested before this trip's work (clamped loads, never
// predicated).  body(chunk, c) sees every chunk of the range once.  WG = the workgroup's size.  (The run goes in by reference, as
// slide_lab.hip's loop took it: with src / nbytes / range as scalars the statistics sweeps compile to other, if equivalent, code.)
template <bool ALIGNED, bool STREAM, int WG, class F>
__device__ __forceinline__ void lab_sweep2(const ChunkSpan& s, int c0, F&& body) {
    const int tid = threadIdx.x;
    if (s.nloc <= c0) return;                                           // block-uniform
    Chunk n0 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c0 + tid, s.nloc);
    Chunk n1 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c0 + tid + WG, s.nloc);
    for (int c = c0 + tid; c < s.nloc; c += 2 * WG) {
        const Chunk i0 = n0, i1 = n1;
        n0 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c + 2 * WG, s.nloc);
        n1 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c + 3 * WG, s.nloc);
        body(i0, c);
        if (c + WG < s.nloc) body(i1, c + WG);
    }
}
// the 12 bytes of chunk c counted into one LDS histogram copy (bytes past `nbytes` of a ragged last chunk are not)
template <bool ALIGNED>
__device__ __forceinline__ void count_chunk_bytes(uint32_t* h, const Chunk& in, int c, size_t nbytes) {
#pragma unroll
    for (int i = 0; i < 12; ++i)
        if (ALIGNED || (size_t)c * 12 + i < nbytes) atomicAdd(&h[chunk_byte(in, i)], 1u);
}

}  // namespace sl
