// lab.hip -- the OpenCV 8-bit Lab family: ReinhardStainNormalizer (normalization/normalizer.py:54-94),
// LuminosityStandardizer (utils/stain_utils.py:50-67) and the LAB helpers (utils/stain_utils.py:146-194), plus
// convert_OD_to_RGB (utils/stain_utils.py:114-124).
//
// cv2.cvtColor(uint8, COLOR_RGB2LAB / COLOR_LAB2RGB) is OpenCV's integer RGB2Lab_b / Lab2RGBinteger: table lookups and
// 32-bit integer arithmetic, restated here from the published color_lab.cpp (tables: gen_tables.py).  Everything the
// reference computes AROUND those conversions is a function of 256-entry histograms:
//   np.percentile(I, 90) over all bytes            -> byte histogram                      (standardize_brightness)
//   cv2.meanStdDev of L8/2.55, a8-128, b8-128      -> histograms of the three Lab bytes   (get_mean_std)
//   np.percentile(L8, 95)                          -> histogram of L8                     (LuminosityStandardizer)
// and each per-pixel float expression (I*255.0/p; ((x-mean)*(tstd/std)+tmean)*2.55, clip, truncate; 255*L/p) has a
// uint8 argument, i.e. is a 256-entry table evaluated ONCE per tile in binary64 with the reference's operation order.
// So a tile costs two histogram sweeps (3 B/px read each) and one map sweep (3 B/px read + 3 B/px written); no per-pixel
// floating point at all.  Roofline: HBM; the LDS histogram atomics bound the two statistics sweeps in practice.
#include "lab_host.hpp"

namespace sl {

constexpr int kLabWG = 256;

// ---- sweep A: histogram of all byte values ------------------------------------------------------------------------
// kHistCopies sub-histograms per wave, chosen by the lane (lane & 3): neighbouring lanes read neighbouring pixels, whose bytes are
// often equal, and lanes that hit one counter of one copy serialise (measured: ~13 cycles per wave instruction with one copy).
constexpr int kHistCopies = 4;
template <bool ALIGNED>
static __global__ __launch_bounds__(kLabWG) void k_byte_hist(const uint8_t* __restrict__ rgb, int P, int parts, LabScratch* __restrict__ sc) {
    __shared__ uint32_t s_h[kLabWG / 64][kHistCopies][256];
    for (int i = threadIdx.x; i < (kLabWG / 64) * kHistCopies * 256; i += kLabWG) (&s_h[0][0][0])[i] = 0;
    __syncthreads();
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts, wave = threadIdx.x >> 6;
    uint32_t* h = s_h[wave][threadIdx.x & (kHistCopies - 1)];
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* src = rgb + (size_t)tile * nbytes;
    const int nch = (P + 3) >> 2;
    const int span = (nch + parts - 1) / parts;
    const int c0 = part * span, c1 = min(nch, c0 + span);
    for (int c = c0 + (int)threadIdx.x; c < c1; c += kLabWG)
        count_chunk_bytes<ALIGNED>(h, load_chunk<ALIGNED>(src, nbytes, c), c, nbytes);
    __syncthreads();
    const int v = threadIdx.x;
    unsigned long long t = 0;
    for (int w = 0; w < kLabWG / 64; ++w)
        for (int k = 0; k < kHistCopies; ++k) t += s_h[w][k][v];
    if (t) atomicAdd(&sc[tile].bytes[v], t);
}

// (the per-tile composed tables, LabTileTabs: lab_device.hpp)
// after sweep A: the brightness table and the gamma values behind it (what sweep B needs)
static __global__ __launch_bounds__(256) void k_lab_pre(const LabScratch* __restrict__ sc, int standardize, LabTileTabs* __restrict__ tt) {
    const int tile = blockIdx.x;
    const double p = lab_begin_tables(tt[tile], sc[tile].bytes, standardize);
    if (threadIdx.x == 0) tt[tile].p = p;
}

// ---- sweep B: histograms of the Lab bytes of the (standardised) tile ------------------------------------------------
template <bool ALIGNED>
static __global__ __launch_bounds__(kLabWG) void k_lab_hist(const uint8_t* __restrict__ rgb, int P, int parts, int want_ab, double thr,
                                                            LabScratch* __restrict__ sc, const LabTileTabs* __restrict__ tt) {
    __shared__ LabCbrt s_t;
    __shared__ uint32_t s_h[kLabWG / 64][256];
    __shared__ uint16_t s_g[256];
    __shared__ unsigned long long s_tissue, s_ab[4];
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts, wave = threadIdx.x >> 6;
    s_t.fill();
    for (int i = threadIdx.x; i < (kLabWG / 64) * 256; i += kLabWG) (&s_h[0][0])[i] = 0;
    if (threadIdx.x == 0) s_tissue = 0;
    if (threadIdx.x < 4) s_ab[threadIdx.x] = 0;
    for (int v = threadIdx.x; v < 256; v += kLabWG) s_g[v] = tt[tile].g[v];     // brightness table and gamma table in one lookup (k_lab_pre)
    __syncthreads();
    const int lim = l8_limit(thr);
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* src = rgb + (size_t)tile * nbytes;
    const int nch = (P + 3) >> 2;
    const int span = (nch + parts - 1) / parts;
    const int c0 = part * span, c1 = min(nch, c0 + span);
    uint32_t n_tissue = 0, sa = 0, sb = 0;                       // a thread sees <= 2^30 / 256 pixels: the plain sums fit 32 bits
    unsigned long long saa = 0, sbb = 0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += kLabWG) {
        const Chunk in = load_chunk<ALIGNED>(src, nbytes, c);
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            if (!ALIGNED && (size_t)c * 4 + px >= (size_t)P) break;
            int L, A, B;
            gamma_to_lab8(s_t, s_g[chunk_byte(in, 3 * px)], s_g[chunk_byte(in, 3 * px + 1)], s_g[chunk_byte(in, 3 * px + 2)], L, A, B);
            atomicAdd(&s_h[wave][L], 1u);
            sa += (uint32_t)A; saa += (uint32_t)(A * A); sb += (uint32_t)B; sbb += (uint32_t)(B * B);
            n_tissue += L < lim ? 1u : 0u;
        }
    }
    unsigned long long red[5] = {n_tissue, sa, saa, sb, sbb};
#pragma unroll
    for (int i = 0; i < 5; ++i) red[i] = wave_sum(red[i]);
    if ((threadIdx.x & 63) == 0) {
        if (red[0]) atomicAdd(&s_tissue, red[0]);
        if (want_ab) for (int i = 0; i < 4; ++i) atomicAdd(&s_ab[i], red[1 + i]);
    }
    __syncthreads();
    const int v = threadIdx.x;
    unsigned long long t = 0;
    for (int w = 0; w < kLabWG / 64; ++w) t += s_h[w][v];
    if (t) atomicAdd(&sc[tile].lab_l[v], t);
    if (want_ab && threadIdx.x < 4) atomicAdd(&sc[tile].ab[threadIdx.x], s_ab[threadIdx.x]);
    if (threadIdx.x == 0 && s_tissue) atomicAdd(&sc[tile].tissue, s_tissue);
}

// stats_out[tile] = {p90, mean L, a, b, std L, a, b, tissue}
static __global__ __launch_bounds__(64) void k_lab_stats(const LabScratch* __restrict__ sc, int standardize, double* __restrict__ stats_out) {
    const int tile = blockIdx.x, t = threadIdx.x;
    double* o = stats_out + 8 * (size_t)tile;
    if (t < 3) {
        double m, s;
        mean_std_of_scratch(sc[tile], t, m, s);
        o[1 + t] = m; o[4 + t] = s;
    } else if (t == 3) {
        o[0] = standardize ? percentile_of_hist(sc[tile].bytes, 90.0) : nan("");
        o[7] = (double)sc[tile].tissue;
    }
}

// ---- sweep C: the map.  MODE 0 Reinhard transform, 1 LuminosityStandardizer, 2 standardize_brightness only ----------
struct LabMapArgs {
    const uint8_t* rgb; uint8_t* out; int P, parts;
    const LabScratch* sc;
    LabTileTabs* tt;                                            // [n] per-tile tables (k_lab_pre, k_lab_tables)
    const double* target_means; const double* target_stds;      // MODE 0 (device, 3 each)
    int mask_background; double thr;                            // MODE 0
    double percentile;                                          // MODE 1
    double* p_out;                                              // MODE 1 / 2 (may be NULL)
};

// The per-tile tables of the map sweep, one workgroup per tile (what every workgroup of the sweep used to rebuild): the tile's
// statistics, then lab_finish_tables.  MODE 0: needs k_lab_pre's brightness table; MODE 1: identity brightness.
template <int MODE>
static __global__ __launch_bounds__(256) void k_lab_tables(LabMapArgs a) {
    __shared__ double s_p;
    __shared__ double s_ms[6];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const LabScratch& sc = a.sc[tile];
    LabTileTabs& tt = a.tt[tile];
    if (MODE == 0) {
        if (tid < 3) {
            double m, s;
            mean_std_of_scratch(sc, tid, m, s);
            s_ms[tid] = m; s_ms[3 + tid] = s;
        }
    } else {
        if (tid == 0) tt.p = s_p = percentile_of_hist(sc.lab_l, a.percentile);
        tt.g[tid] = (uint16_t)d_gamma[tid];
        tt.lut[tid] = (uint8_t)tid;
    }
    __syncthreads();
    lab_finish_tables(tt, MODE, s_ms, a.target_means, a.target_stds, s_p);
}

// The sweep: per-tile tables from k_lab_pre / k_lab_tables; two chunks per lane in flight (lab_sweep2).
template <int MODE, bool ALIGNED>
static __global__ __launch_bounds__(kLabWG) void k_lab_map(LabMapArgs a) {
    __shared__ LabCbrtInv s_t;
    __shared__ uint8_t s_lut[256];            // brightness table (MODE 2)
    __shared__ uint16_t s_g[256];
    __shared__ uint32_t s_yf[256];
    __shared__ int s_ad[256], s_bd[256];
    const int tile = blockIdx.x / a.parts, part = blockIdx.x % a.parts, tid = threadIdx.x;
    const LabTileTabs& tt = a.tt[tile];
    if (MODE != 2) {
        s_t.fill();
        s_g[tid] = tt.g[tid];
        s_yf[tid] = tt.yf[tid];
        if (MODE == 0) { s_ad[tid] = tt.ad[tid]; s_bd[tid] = tt.bd[tid]; }
    } else {
        s_lut[tid] = tt.lut[tid];
    }
    if (MODE != 0 && part == 0 && tid == 0 && a.p_out) a.p_out[tile] = tt.p;
    __syncthreads();
    const int lim = MODE == 0 ? l8_limit(a.thr) : 256;
    const LabBackground bg = lab_background();
    const bool mask_bg = MODE == 0 && a.mask_background;
    const size_t nbytes = (size_t)a.P * 3;
    const int nch = (a.P + 3) >> 2;
    const int span = (nch + a.parts - 1) / a.parts;
    const int c0 = part * span;
    const ChunkSpan s{a.rgb + (size_t)tile * nbytes, (size_t)tile * nbytes, nbytes, min(nch, c0 + span)};      // the tile, up to this part's end
    uint8_t* dst = a.out + s.off;
    lab_sweep2<ALIGNED, true, kLabWG>(s, c0, [&](const Chunk& in, int c) {
        if constexpr (MODE != 2) {
            store_chunk<ALIGNED>(dst, s.nbytes, c, lab_map_chunk<MODE == 0>(s_t, s_g, s_yf, s_ad, s_bd, in, mask_bg, lim, bg));
        } else {
            uint32_t ob[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) ob[i] = s_lut[chunk_byte(in, i)];
            store_chunk<ALIGNED>(dst, s.nbytes, c, pack12(ob));
        }
    });
}

// ---- plain conversions -------------------------------------------------------------------------------------------
// DIR 0: RGB -> Lab8 bytes; 1: Lab8 -> RGB bytes
template <int DIR, bool ALIGNED>
static __global__ __launch_bounds__(kLabWG) void k_lab_convert(const uint8_t* __restrict__ in_img, uint8_t* __restrict__ out_img, int P, int parts) {
    __shared__ LabTabs s_t;
    s_t.fill();
    __syncthreads();
    const int tile = blockIdx.x / parts, part = blockIdx.x % parts;
    const size_t nbytes = (size_t)P * 3;
    const uint8_t* src = in_img + (size_t)tile * nbytes;
    uint8_t* dst = out_img + (size_t)tile * nbytes;
    const int nch = (P + 3) >> 2;
    const int span = (nch + parts - 1) / parts;
    const int c0 = part * span, c1 = min(nch, c0 + span);
    for (int c = c0 + (int)threadIdx.x; c < c1; c += kLabWG) {
        const Chunk in = load_chunk<ALIGNED>(src, nbytes, c);
        uint32_t ob[12];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const uint32_t v0 = chunk_byte(in, 3 * px), v1 = chunk_byte(in, 3 * px + 1), v2 = chunk_byte(in, 3 * px + 2);
            if (DIR == 0) {
                int L, A, B;
                rgb_to_lab8(s_t, v0, v1, v2, L, A, B);
                ob[3 * px] = (uint32_t)L; ob[3 * px + 1] = (uint32_t)A; ob[3 * px + 2] = (uint32_t)B;
            } else {
                lab8_to_rgb(s_t, (int)v0, (int)v1, (int)v2, ob[3 * px], ob[3 * px + 1], ob[3 * px + 2]);
            }
        }
        store_chunk<ALIGNED>(dst, nbytes, c, pack12(ob));
    }
}

// lab_split (stain_utils.py:146-158): binary32 planes
static __global__ __launch_bounds__(kLabWG) void k_lab_split(const uint8_t* __restrict__ rgb, size_t n_px, float* __restrict__ I1,
                                                             float* __restrict__ I2, float* __restrict__ I3) {
    __shared__ LabTabs s_t;
    s_t.fill();
    __syncthreads();
    for (size_t p = blockIdx.x * (size_t)kLabWG + threadIdx.x; p < n_px; p += (size_t)gridDim.x * kLabWG) {
        int L, A, B;
        rgb_to_lab8(s_t, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], L, A, B);
        I1[p] = (float)L / 2.55f; I2[p] = (float)A - 128.0f; I3[p] = (float)B - 128.0f;
    }
}

// merge_back (stain_utils.py:160-172)
template <class T>
static __global__ __launch_bounds__(kLabWG) void k_lab_merge(const T* __restrict__ I1, const T* __restrict__ I2, const T* __restrict__ I3,
                                                             size_t n_px, uint8_t* __restrict__ out) {
    __shared__ LabTabs s_t;
    s_t.fill();
    __syncthreads();
    for (size_t p = blockIdx.x * (size_t)kLabWG + threadIdx.x; p < n_px; p += (size_t)gridDim.x * kLabWG) {
        const T l = I1[p] * (T)2.55, a = I2[p] + (T)128.0, b = I3[p] + (T)128.0;      // in the planes' own precision, like numpy
        uint32_t r, g, bl;
        lab8_to_rgb(s_t, (int)clip_trunc_u8((double)l), (int)clip_trunc_u8((double)a), (int)clip_trunc_u8((double)b), r, g, bl);
        out[3 * p] = (uint8_t)r; out[3 * p + 1] = (uint8_t)g; out[3 * p + 2] = (uint8_t)bl;
    }
}

// convert_OD_to_RGB (stain_utils.py:114-124), binary64 like the reference
static __global__ __launch_bounds__(kLabWG) void k_od_to_rgb(const double* __restrict__ od, size_t n, uint8_t* __restrict__ out,
                                                             int32_t* __restrict__ negative) {
    bool neg = false;
    for (size_t i = blockIdx.x * (size_t)kLabWG + threadIdx.x; i < n; i += (size_t)gridDim.x * kLabWG) {
        const double v = od[i];
        neg = neg | (v < 0.0);
        out[i] = (uint8_t)(255.0 * exp(-1.0 * fmax(v, 1e-6)));
    }
    if (negative && __any(neg) && (threadIdx.x & 63) == 0) atomicOr(negative, 1);
}

}  // namespace sl

using namespace sl;

namespace {

// Workgroups per tile of the Lab sweeps: every workgroup merges a 256-bin histogram into the tile's with global atomics (sweeps A, B) or
// fills 14 KB of LDS tables (sweep C) before it touches a pixel, so a tile is split only as far as it takes to put ~8 workgroups on
// every CU.  Measured on 1 250 tiles of 512^2 (round 5, per-tile tables precomputed): 1 250 / 2 500 / 3 750 / 8 750 / 17 500 workgroups:
// k_lab_hist 529 / 526 / 525 / 629 / 882 us, k_lab_map<0> 909 / 903 / 927 / 1 016 / - us.
int lab_parts(int n, long P) {
    const long want = (2048 + n - 1) / n;
    const long nch = (P + 3) >> 2;
    long most = nch / (16L * kLabWG);
    if (most < 1) most = 1;
    return (int)(want < 1 ? 1 : (want < most ? want : most));
}

size_t lab_scratch_bytes(int n) { return (sizeof(LabScratch) * (size_t)n + 255) & ~(size_t)255; }
size_t lab_ws_bytes(int n) { return lab_scratch_bytes(n) + ((sizeof(LabTileTabs) * (size_t)n + 255) & ~(size_t)255); }

// the two statistics sweeps shared by the entry points below (and k_lab_pre between them: the tile's brightness table)
int lab_statistics(const uint8_t* rgb, int n, long P, int standardize, int want_ab, double thr, LabScratch* sc, hipStream_t s) {
    static_assert(sizeof(LabScratch) % 4 == 0, "zero_async clears whole words");
    if (const int rc = zero_async(sc, sizeof(LabScratch) * (size_t)n, s)) return rc;
    LabTileTabs* tt = lab_tabs_of(sc, n);
    const int parts = lab_parts(n, P);
    const dim3 grid((unsigned)((long)n * parts)), block(kLabWG);
    const bool al = aligned4(rgb, P);
    if (standardize) launch_aligned(al, k_byte_hist<true>, k_byte_hist<false>, grid, block, 0, s, rgb, (int)P, parts, sc);
    hipLaunchKernelGGL(k_lab_pre, dim3((unsigned)n), dim3(256), 0, s, sc, standardize, tt);
    if (want_ab >= 0) launch_aligned(al, k_lab_hist<true>, k_lab_hist<false>, grid, block, 0, s, rgb, (int)P, parts, want_ab, thr, sc, tt);
    return launch_status();
}

// the arguments every map shares; the entry points add their mode's
LabMapArgs lab_map_args(const uint8_t* rgb, uint8_t* out, int n, long P, LabScratch* sc) {
    LabMapArgs a{};
    a.rgb = rgb; a.out = out; a.P = (int)P; a.parts = lab_parts(n, P); a.sc = sc; a.tt = lab_tabs_of(sc, n);
    return a;
}

// the per-tile tables of the map (MODE 0, 1), behind the statistics
template <int MODE>
void lab_tables(const LabMapArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL((k_lab_tables<MODE>), dim3((unsigned)n), dim3(256), 0, s, a);
}

template <int MODE>
int lab_map(const LabMapArgs& a, int n, hipStream_t s) {
    if constexpr (MODE != 2) lab_tables<MODE>(a, n, s);
    const dim3 grid((unsigned)((long)n * a.parts)), block(kLabWG);
    launch_aligned(aligned4(a.rgb, a.P) && aligned4(a.out, a.P), k_lab_map<MODE, true>, k_lab_map<MODE, false>, grid, block, 0, s, a);
    return launch_status();
}

// DIR 0: sl_rgb_to_lab8, 1: sl_lab8_to_rgb
template <int DIR>
int lab_convert(const uint8_t* in, uint8_t* out, int n, int h, int w, void* stream) {
    if (const int rc = check_shape(in, out, n, h, w)) return rc;
    const long P = (long)h * w;
    const int parts = parts_for(P);
    const dim3 grid((unsigned)((long)n * parts)), block(kLabWG);
    launch_aligned(aligned4(in, P) && aligned4(out, P), k_lab_convert<DIR, true>, k_lab_convert<DIR, false>, grid, block, 0, (hipStream_t)stream,
                   in, out, (int)P, parts);
    return launch_status();
}

}  // namespace

namespace sl {

size_t lab_workspace_bytes(int n) { return lab_ws_bytes(n); }      // for sl_workspace_bytes (macenko.hip)

// ---- shared with lab_view.hip (lab_host.hpp) ---------------------------------------------------------------------------------------
LabTileTabs* lab_tabs_of(void* ws, int n) { return (LabTileTabs*)((char*)ws + lab_scratch_bytes(n)); }

int lab_check(const void* rgb, const void* out, int n, int h, int w, const void* ws, size_t ws_bytes) {
    if (!rgb || !out || n <= 0 || h <= 0 || w <= 0) return SL_ERR_BADARG;
    if ((long)h * w > (1L << 30) || !grid_fits(n, lab_parts(n, (long)h * w))) return SL_ERR_BADARG;
    if (!ws || ws_bytes < lab_ws_bytes(n) || ((uintptr_t)ws & 7u)) return SL_ERR_WORKSPACE;
    return SL_OK;
}

int lab_reinhard_tables(const uint8_t* rgb, int n, long P, const double* target_means, const double* target_stds, double thr,
                        double* stats_out, void* ws, hipStream_t s) {
    LabScratch* sc = (LabScratch*)ws;
    if (const int rc = lab_statistics(rgb, n, P, 1, 1, thr, sc, s)) return rc;
    if (stats_out) hipLaunchKernelGGL(k_lab_stats, dim3((unsigned)n), dim3(64), 0, s, sc, 1, stats_out);
    LabMapArgs a = lab_map_args(rgb, nullptr, n, P, sc);
    a.target_means = target_means; a.target_stds = target_stds;
    lab_tables<0>(a, n, s);
    return launch_status();
}

int lab_luminosity_tables(const uint8_t* rgb, int n, long P, double percentile, void* ws, hipStream_t s) {
    LabScratch* sc = (LabScratch*)ws;
    if (const int rc = lab_statistics(rgb, n, P, 0, 0, 0.8, sc, s)) return rc;
    LabMapArgs a = lab_map_args(rgb, nullptr, n, P, sc);
    a.percentile = percentile;
    lab_tables<1>(a, n, s);
    return launch_status();
}

}  // namespace sl

extern "C" int sl_rgb_to_lab8(const uint8_t* rgb, uint8_t* lab_out, int n, int h, int w, void* stream) {
    return lab_convert<0>(rgb, lab_out, n, h, w, stream);
}

extern "C" int sl_lab8_to_rgb(const uint8_t* lab, uint8_t* rgb_out, int n, int h, int w, void* stream) {
    return lab_convert<1>(lab, rgb_out, n, h, w, stream);
}

extern "C" int sl_lab_split(const uint8_t* rgb, int n, int h, int w, float* I1, float* I2, float* I3, void* stream) {
    if (!rgb || !I1 || !I2 || !I3 || n <= 0 || h <= 0 || w <= 0) return SL_ERR_BADARG;
    const size_t n_px = (size_t)n * h * w;
    const size_t blocks = (n_px + kLabWG - 1) / kLabWG;
    hipLaunchKernelGGL(k_lab_split, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kLabWG), 0, (hipStream_t)stream, rgb, n_px, I1, I2, I3);
    return launch_status();
}

extern "C" int sl_lab_merge(const void* I1, const void* I2, const void* I3, int is_f64, int n, int h, int w, uint8_t* rgb_out, void* stream) {
    if (!I1 || !I2 || !I3 || !rgb_out || n <= 0 || h <= 0 || w <= 0) return SL_ERR_BADARG;
    const size_t n_px = (size_t)n * h * w;
    const size_t blocks = (n_px + kLabWG - 1) / kLabWG;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192)), block(kLabWG);
    if (is_f64) hipLaunchKernelGGL((k_lab_merge<double>), grid, block, 0, (hipStream_t)stream, (const double*)I1, (const double*)I2, (const double*)I3, n_px, rgb_out);
    else hipLaunchKernelGGL((k_lab_merge<float>), grid, block, 0, (hipStream_t)stream, (const float*)I1, (const float*)I2, (const float*)I3, n_px, rgb_out);
    return launch_status();
}

extern "C" int sl_od_to_rgb(const double* od, size_t n_values, uint8_t* rgb_out, int32_t* negative_flag, void* stream) {
    if (!od || !rgb_out || n_values == 0) return SL_ERR_BADARG;
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(int32_t) % 4 == 0, "zero_async clears whole words");
    if (negative_flag) {
        if (const int rc = zero_async(negative_flag, sizeof(int32_t), s)) return rc;
    }
    const size_t blocks = (n_values + kLabWG - 1) / kLabWG;
    hipLaunchKernelGGL(k_od_to_rgb, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kLabWG), 0, s, od, n_values, rgb_out, negative_flag);
    return launch_status();
}

extern "C" int sl_standardize_brightness(const uint8_t* rgb, uint8_t* out, int n, int h, int w, double* p_out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    int rc = lab_check(rgb, out, n, h, w, workspace, workspace_bytes);
    if (rc) return rc;
    const long P = (long)h * w;
    hipStream_t s = (hipStream_t)stream;
    LabScratch* sc = (LabScratch*)workspace;
    rc = lab_statistics(rgb, n, P, 1, -1, 0.0, sc, s);
    if (rc) return rc;
    LabMapArgs a = lab_map_args(rgb, out, n, P, sc);
    a.p_out = p_out;
    return lab_map<2>(a, n, s);
}

extern "C" int sl_reinhard_stats(const uint8_t* rgb, int n, int h, int w, int standardize, double* stats_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    int rc = lab_check(rgb, stats_out, n, h, w, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    LabScratch* sc = (LabScratch*)workspace;
    rc = lab_statistics(rgb, n, (long)h * w, standardize ? 1 : 0, 1, 0.8, sc, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lab_stats, dim3((unsigned)n), dim3(64), 0, s, sc, standardize ? 1 : 0, stats_out);
    return launch_status();
}

extern "C" int sl_reinhard_transform(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* target_means,
                                     const double* target_stds, int mask_background, double luminosity_threshold,
                                     double* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = lab_check(rgb, out, n, h, w, workspace, workspace_bytes);
    if (rc) return rc;
    if (!target_means || !target_stds) return SL_ERR_BADARG;
    const long P = (long)h * w;
    hipStream_t s = (hipStream_t)stream;
    LabScratch* sc = (LabScratch*)workspace;
    rc = lab_statistics(rgb, n, P, 1, 1, luminosity_threshold, sc, s);
    if (rc) return rc;
    if (stats_out) hipLaunchKernelGGL(k_lab_stats, dim3((unsigned)n), dim3(64), 0, s, sc, 1, stats_out);
    LabMapArgs a = lab_map_args(rgb, out, n, P, sc);
    a.target_means = target_means; a.target_stds = target_stds;
    a.mask_background = mask_background ? 1 : 0; a.thr = luminosity_threshold;
    return lab_map<0>(a, n, s);
}

extern "C" int sl_luminosity_standardize(const uint8_t* rgb, uint8_t* out, int n, int h, int w, double percentile, double* p_out,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    int rc = lab_check(rgb, out, n, h, w, workspace, workspace_bytes);
    if (rc) return rc;
    const long P = (long)h * w;
    hipStream_t s = (hipStream_t)stream;
    LabScratch* sc = (LabScratch*)workspace;
    rc = lab_statistics(rgb, n, P, 0, 0, 0.8, sc, s);
    if (rc) return rc;
    LabMapArgs a = lab_map_args(rgb, out, n, P, sc);
    a.percentile = percentile; a.p_out = p_out;
    return lab_map<1>(a, n, s);
}
