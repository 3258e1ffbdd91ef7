// slide_lab.hip -- the POOLED slide-level Reinhard / luminosity statistics (normalizer.py:70-94 and stain_utils.py:52-67,146-194 on the
// vertical concatenation of every tile of every rank).
//
// Everything the Lab family derives from an image is a function of integer sums (lab.hip): the histogram of all bytes gives the 90th
// percentile, the histogram of L8 with sum a8, sum a8^2, sum b8, sum b8^2 gives the means and standard deviations (and the L percentile
// of LuminosityStandardizer).  Integer sums decompose over tiles and ranks exactly, so the slide is
//   sl_slab_bytes   k_slab_bytes  -> this rank's 256 byte counts                                  -> all-reduce
//   sl_slab_begin   k_slab_begin: p90, the brightness table and the gamma values behind it
//   sl_slab_lab     k_slab_lab    -> this rank's L8 histogram, the four a/b sums, tissue pixels    -> all-reduce
//   sl_slab_finish  k_slab_finish: means / stds (or the L percentile), the composed byte tables of the map, the status
//   sl_slab_map     k_slab_map: the table-driven map of every local tile
// and its result is the reference's on the concatenation, byte for byte: no sample, no bracket, no fallback.  Every rank derives the
// same state from the same reduced sums; nothing is broadcast.
//
// The sweeps run FLAT over the shard: n tiles of one shape are one contiguous run of n*h*w pixels, cut into 12-byte chunks (four whole
// pixels: the run starts on a pixel) and into one contiguous span of chunks per workgroup; only the shard's last chunk can be ragged
// and the alignment case is one decision per shard.  Chunk positions are 64-bit (a workgroup's span offset) plus a 32-bit index inside
// the span.  All tiles share ONE set of tables and ONE scratch, so the workgroups do not merge into it with global atomics (256
// addresses under every workgroup of the chip): each writes one row of partial sums and k_slab_reduce adds the rows.  Integer sums:
// run-to-run identical whatever the order.
#include "lab_device.hpp"
#include "sl_host.hpp"

using namespace sl;

namespace {

enum { kP90 = SL_SLAB_P90, kMeans = SL_SLAB_MEANS, kStds = SL_SLAB_STDS, kLpct = SL_SLAB_LPCT, kTissue = SL_SLAB_TISSUE, kNpx = SL_SLAB_NPX,
       kStatus = SL_SLAB_STATUS, kTables = SL_SLAB_TABLES };

// the composed tables of the slide (state[SL_SLAB_TABLES ...]; what LabTileTabs is per tile)
struct SlabTabs {
    uint32_t yf[256];         // L8 -> (y, f(y)) of the MAPPED L byte, packed
    int ad[256], bd[256];     // a8 / b8 -> the mapped byte on abToXZ's scale
    uint16_t g[256];          // byte -> gamma value through the brightness table
    uint8_t lut[256];         // the brightness table (identity when the chain does not standardise)
};
static_assert(kTables * 8 + sizeof(SlabTabs) <= SL_SLAB_STATE_DOUBLES * 8, "SlabTabs does not fit the state");
static_assert(SL_SLAB_SUMS_A == 256 && SL_SLAB_SUMS_B == 262, "256 counts; 256 counts + 4 sums + tissue pixels + pixels");

__device__ __forceinline__ SlabTabs* tabs_of(double* st) { return reinterpret_cast<SlabTabs*>(st + kTables); }
__device__ __forceinline__ const SlabTabs* tabs_of(const double* st) { return reinterpret_cast<const SlabTabs*>(st + kTables); }

constexpr int kSlabWG = 256;
constexpr int kSlabMinTrips = 16;         // chunks per lane below which a shard is not cut further (a workgroup fills up to 17 KB of tables first)
constexpr int kSlabCopies = 4;            // LDS histogram copies per wave, chosen by the lane: neighbouring pixels are often equal (lab.hip)
constexpr int kSlabCols = SL_SLAB_SUMS_B; // width of a partial row (sweep A uses the first 256 columns)

// The cut of a shard of n tiles of P pixels: `rows` workgroups of `span` chunks each (the last ones may come out short or empty).
struct SlabPlan { long long nch; int rows; long long span; };
SlabPlan slab_plan(int n, long P) {
    SlabPlan p;
    p.nch = ((long long)n * P + 3) >> 2;
    const long long max_rows = 3LL * max_resident_grid();             // 6 per CU (23 KB of LDS, <= 48 VGPRs each): all resident at once, no second round with a tail
    long long want = (p.nch + (long long)kSlabWG * kSlabMinTrips - 1) / ((long long)kSlabWG * kSlabMinTrips);
    want = want < 1 ? 1 : (want > max_rows ? max_rows : want);
    p.rows = (int)want;
    p.span = (p.nch + want - 1) / want;
    return p;
}

// this workgroup's span: where it starts, how many bytes and chunks it holds (0 chunks: nothing to do)
struct SlabSpan { const uint8_t* src; size_t off; size_t nbytes; int nloc; };
__device__ __forceinline__ SlabSpan span_of(const uint8_t* rgb, unsigned long long total_bytes, long long span) {
    SlabSpan s;
    s.off = (size_t)blockIdx.x * (size_t)span * 12;
    s.src = rgb + s.off;
    const size_t left = s.off < total_bytes ? (size_t)total_bytes - s.off : 0;
    s.nbytes = left < (size_t)span * 12 ? left : (size_t)span * 12;
    s.nloc = (int)((s.nbytes + 11) / 12);
    return s;
}

// the chunks of a span, two per lane in flight (the next trip's are requested before this trip's work; clamped loads, never predicated)
template <bool ALIGNED, bool STREAM, class F>
__device__ __forceinline__ void slab_sweep(const SlabSpan& s, F&& body) {
    const int tid = threadIdx.x;
    if (s.nloc <= 0) return;                                            // block-uniform
    Chunk n0 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, tid, s.nloc);
    Chunk n1 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, tid + kSlabWG, s.nloc);
    for (int c = tid; c < s.nloc; c += 2 * kSlabWG) {
        const Chunk i0 = n0, i1 = n1;
        n0 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c + 2 * kSlabWG, s.nloc);
        n1 = load_chunk_clamped<ALIGNED, STREAM>(s.src, s.nbytes, c + 3 * kSlabWG, s.nloc);
        body(i0, c);
        if (c + kSlabWG < s.nloc) body(i1, c + kSlabWG);
    }
}

// ---- sweep A: the byte counts of this rank's shard: partials[blockIdx.x][0 .. 255] ---------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kSlabWG) void k_slab_bytes(const uint8_t* __restrict__ rgb, unsigned long long total_bytes, long long span,
                                                        unsigned long long* __restrict__ partials) {
    __shared__ uint32_t s_h[kSlabWG / 64][kSlabCopies][256];
    for (int i = threadIdx.x; i < (kSlabWG / 64) * kSlabCopies * 256; i += kSlabWG) (&s_h[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t* h = s_h[threadIdx.x >> 6][threadIdx.x & (kSlabCopies - 1)];
    const SlabSpan s = span_of(rgb, total_bytes, span);
    // (a span holds fewer than 2^32 bytes -- sl_slab_bytes checks it --, so the 32-bit counters cannot wrap)
    slab_sweep<ALIGNED, false>(s, [&](const Chunk& in, int c) {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (ALIGNED || (size_t)c * 12 + i < s.nbytes) atomicAdd(&h[chunk_byte(in, i)], 1u);
    });
    __syncthreads();
    const int v = threadIdx.x;
    unsigned long long t = 0;
    for (int w = 0; w < kSlabWG / 64; ++w)
        for (int k = 0; k < kSlabCopies; ++k) t += s_h[w][k][v];
    partials[(size_t)blockIdx.x * kSlabCols + v] = t;
}

// ---- sweep B: the Lab sums of the (standardised) shard: partials[blockIdx.x][0 .. 260] -------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kSlabWG) void k_slab_lab(const uint8_t* __restrict__ rgb, unsigned long long total_bytes, long long span, double thr,
                                                      const double* __restrict__ st, unsigned long long* __restrict__ partials) {
    __shared__ LabCbrt s_t;
    __shared__ uint32_t s_h[kSlabWG / 64][kSlabCopies][256];
    __shared__ uint16_t s_g[256];
    __shared__ unsigned long long s_red[5];
    const int tid = threadIdx.x;
    s_t.fill();
    for (int i = tid; i < (kSlabWG / 64) * kSlabCopies * 256; i += kSlabWG) (&s_h[0][0][0])[i] = 0;
    if (tid < 5) s_red[tid] = 0;
    s_g[tid] = tabs_of(st)->g[tid];                                  // brightness table and gamma table in one lookup (k_slab_begin)
    __syncthreads();
    uint32_t* h = s_h[tid >> 6][tid & (kSlabCopies - 1)];
    const int lim = l8_limit(thr);
    const SlabSpan s = span_of(rgb, total_bytes, span);
    const size_t npx = s.nbytes / 3;
    uint32_t n_tissue = 0, sa = 0, sb = 0;                           // a lane sees < 2^32 / (3 * 256) pixels of its span: the plain sums fit 32 bits
    unsigned long long saa = 0, sbb = 0;
    slab_sweep<ALIGNED, false>(s, [&](const Chunk& in, int c) {
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            int L, A, B;
            gamma_to_lab8(s_t, s_g[chunk_byte(in, 3 * px)], s_g[chunk_byte(in, 3 * px + 1)], s_g[chunk_byte(in, 3 * px + 2)], L, A, B);
            const bool ok = ALIGNED || (size_t)c * 4 + px < npx;
            if (ok) atomicAdd(&h[L], 1u);
            const uint32_t a = ok ? (uint32_t)A : 0u, b = ok ? (uint32_t)B : 0u;
            sa += a; saa += a * a; sb += b; sbb += b * b;
            n_tissue += (ok && L < lim) ? 1u : 0u;
        }
    });
    unsigned long long red[5] = {sa, saa, sb, sbb, n_tissue};
#pragma unroll
    for (int i = 0; i < 5; ++i) red[i] = wave_sum(red[i]);
    if ((tid & 63) == 0)
        for (int i = 0; i < 5; ++i) atomicAdd(&s_red[i], red[i]);
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < kSlabWG / 64; ++w)
        for (int k = 0; k < kSlabCopies; ++k) t += s_h[w][k][tid];
    unsigned long long* row = partials + (size_t)blockIdx.x * kSlabCols;
    row[tid] = t;
    if (tid < 5) row[256 + tid] = s_red[tid];
}

// the rows added up: workgroup b takes columns 64 b .. 64 b + 63, 16 row groups of 64 lanes each, then the groups in a fixed order;
// out[extra_col] = extra (this rank's pixel count, which no row carries)
constexpr int kSlabReduceThreads = 1024;
__global__ __launch_bounds__(kSlabReduceThreads) void k_slab_reduce(const unsigned long long* __restrict__ partials, int rows, int cols, int extra_col,
                                                                    unsigned long long extra, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_red[kSlabReduceThreads / 64][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    unsigned long long t = 0;
    if (col < cols && col != extra_col)
        for (int r = grp; r < rows; r += kSlabReduceThreads / 64) t += partials[(size_t)r * kSlabCols + col];
    s_red[grp][lane] = t;
    __syncthreads();
    if (grp == 0 && col < cols) {
        unsigned long long sum = 0;
        for (int g = 0; g < kSlabReduceThreads / 64; ++g) sum += s_red[g][lane];
        out[col] = col == extra_col ? extra : sum;
    }
}

// ---- after the first all-reduce: p90 of the slide, its brightness table and the gamma values behind it ----------------------------
__global__ __launch_bounds__(256) void k_slab_begin(double* __restrict__ st, const unsigned long long* __restrict__ sums_a, int standardize) {
    __shared__ double s_p;
    const int tid = threadIdx.x;
    if (tid == 0) s_p = standardize ? percentile_of_hist(sums_a, 90.0) : nan("");
    __syncthreads();
    const double p = s_p;
    // stain_utils.py:193-194: uint8(clip(v * 255.0 / p, 0, 255)); identity when the chain does not standardise
    const uint32_t lut = standardize ? clip_trunc_u8((double)tid * 255.0 / p) : (uint32_t)tid;
    SlabTabs* tt = tabs_of(st);
    tt->lut[tid] = (uint8_t)lut;
    tt->g[tid] = (uint16_t)d_gamma[lut];
    if (tid < kTables) st[tid] = tid == kP90 ? p : ((tid >= kMeans && tid <= kLpct) ? nan("") : 0.0);      // (status SL_TILE_OK = 0)
}

// ---- after the second all-reduce: the slide's statistics and the composed tables of the map (k_lab_tables, once per slide) ---------
__global__ __launch_bounds__(256) void k_slab_finish(double* __restrict__ st, const unsigned long long* __restrict__ sums_b, int mode,
                                                     const double* __restrict__ target_means, const double* __restrict__ target_stds,
                                                     double percentile, int mask_background) {
    __shared__ LabScratch s_sc;
    __shared__ uint8_t s_ch[3][256];
    __shared__ double s_p;
    __shared__ double s_ms[6];
    const int tid = threadIdx.x;
    s_sc.lab_l[tid] = sums_b[tid];
    if (tid < 4) s_sc.ab[tid] = sums_b[256 + tid];
    if (tid == 0) s_sc.tissue = sums_b[260];
    __syncthreads();
    if (tid < 3) {
        double m, s;
        mean_std_of_scratch(s_sc, tid, m, s);
        s_ms[tid] = m; s_ms[3 + tid] = s;
    } else if (tid == 64) {
        s_p = mode == 1 ? percentile_of_hist(s_sc.lab_l, percentile) : nan("");
    }
    __syncthreads();
    if (mode == 0) {
        // normalizer.py:81-83 in binary64: ((x - mean) * (tstd / std)) + tmean; merge_back (stain_utils.py:168-171): * 2.55 resp.
        // + 128.0, clip, truncate.  x is the binary32 value lab_split produced, promoted.  Every operation rounds on its own, as numpy's do.
#pragma clang fp contract(off)
        for (int ch = 0; ch < 3; ++ch) {
            const double ratio = target_stds[ch] / s_ms[3 + ch];
            const double x = ch == 0 ? (double)((float)tid / 2.55f) : (double)((float)tid - 128.0f);
            const double nrm = ((x - s_ms[ch]) * ratio) + target_means[ch];
            s_ch[ch][tid] = (uint8_t)clip_trunc_u8(ch == 0 ? nrm * 2.55 : nrm + 128.0);
        }
    } else {
        s_ch[0][tid] = (uint8_t)clip_trunc_u8(255.0 * (double)tid / s_p);          // stain_utils.py:65: 255 * L_float / p
        s_ch[1][tid] = s_ch[2][tid] = (uint8_t)tid;                                // a and b stay
    }
    const int L2 = s_ch[0][tid], A2 = s_ch[1][tid], B2 = s_ch[2][tid];
    SlabTabs* tt = tabs_of(st);
    tt->yf[tid] = (uint32_t)d_lab_yf[2 * L2] | ((uint32_t)d_lab_yf[2 * L2 + 1] << 16);
    tt->ad[tid] = lab_adiv(A2);
    tt->bd[tid] = lab_bdiv(B2);
    if (tid < 6) st[kMeans + tid] = s_ms[tid];
    if (tid == 0) {
        const unsigned long long tissue = sums_b[260], npx = sums_b[261];
        st[kLpct] = s_p;
        st[kTissue] = (double)tissue;
        st[kNpx] = (double)npx;
        // no pixel; with mask_background no tissue pixel either, where the reference raises TissueMaskException (stain_utils.py:46-47)
        st[kStatus] = (npx == 0 || (mode == 0 && mask_background && tissue == 0)) ? SL_TILE_EMPTY_MASK : SL_TILE_OK;
    }
}

// ---- sweep C: the map of this rank's tiles under the slide's tables ---------------------------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kSlabWG) void k_slab_map(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, unsigned long long total_bytes,
                                                      long long span, const double* __restrict__ st, int mask_bg, double thr) {
    __shared__ LabCbrtInv s_t;
    __shared__ uint16_t s_g[256];
    __shared__ uint32_t s_yf[256];
    __shared__ int s_ad[256], s_bd[256];
    const int tid = threadIdx.x;
    const SlabSpan s = span_of(rgb, total_bytes, span);
    uint8_t* dst = out + s.off;
    if (s.nloc <= 0) return;
    if ((int)st[kStatus] != SL_TILE_OK) {                              // unusable statistics: the tiles go through unchanged (k_apply's rule)
        for (int c = tid; c < s.nloc; c += kSlabWG) store_chunk<ALIGNED>(dst, s.nbytes, c, load_chunk<ALIGNED>(s.src, s.nbytes, c));
        return;
    }
    const SlabTabs* tt = tabs_of(st);
    s_t.fill();
    s_g[tid] = tt->g[tid];
    s_yf[tid] = tt->yf[tid];
    s_ad[tid] = tt->ad[tid];
    s_bd[tid] = tt->bd[tid];
    __syncthreads();
    const int lim = l8_limit(thr);
    // background (normalizer.py:86-90): 254 + 0 on the L/2.55 scale -> clips to 255; a = b = 0 + 128
    const uint32_t yf_bg = (uint32_t)d_lab_yf[2 * 255] | ((uint32_t)d_lab_yf[2 * 255 + 1] << 16);
    const int ad_bg = lab_adiv(128), bd_bg = lab_bdiv(128);
    slab_sweep<ALIGNED, true>(s, [&](const Chunk& in, int c) {
        uint32_t ob[12];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            int L, A, B;
            gamma_to_lab8(s_t, s_g[chunk_byte(in, 3 * px)], s_g[chunk_byte(in, 3 * px + 1)], s_g[chunk_byte(in, 3 * px + 2)], L, A, B);
            uint32_t yf = s_yf[L];
            int ad = s_ad[A], bd = s_bd[B];
            if (mask_bg) {
                const bool bg = !(L < lim);
                yf = bg ? yf_bg : yf; ad = bg ? ad_bg : ad; bd = bg ? bd_bg : bd;
            }
            yf_to_rgb(s_t, (int)(yf & 0xffffu), (int)(yf >> 16), ad, bd, ob[3 * px], ob[3 * px + 1], ob[3 * px + 2]);
        }
        store_chunk<ALIGNED>(dst, s.nbytes, c, pack12(ob));
    });
}

// n >= 0 tiles of h x w: the shape checks every entry point with a shard shares
bool slab_shape_ok(int n, int h, int w) {
    if (n < 0 || h <= 0 || w <= 0) return false;
    const long P = (long)h * w;
    return P <= (1L << 30) && (long)n * P <= (1L << 40);
}

size_t slab_ws_bytes(int n, long P) {
    if (n == 0) return 256;
    return ((size_t)slab_plan(n, P).rows * kSlabCols * sizeof(unsigned long long) + 255) & ~(size_t)255;
}

int slab_ws_check(const void* ws, size_t ws_bytes, int n, long P) {
    return (!ws || ((uintptr_t)ws & 7u) || ws_bytes < slab_ws_bytes(n, P)) ? SL_ERR_WORKSPACE : SL_OK;
}

void slab_reduce(const void* ws, int rows, int cols, int extra_col, unsigned long long extra, unsigned long long* out, hipStream_t s) {
    hipLaunchKernelGGL(k_slab_reduce, dim3((unsigned)((cols + 63) / 64)), dim3(kSlabReduceThreads), 0, s, (const unsigned long long*)ws, rows, cols,
                       extra_col, extra, out);
}

}  // namespace

extern "C" size_t sl_slab_workspace_bytes(int n, int h, int w) {
    if (!slab_shape_ok(n, h, w)) return 0;
    return slab_ws_bytes(n, (long)h * w);
}

extern "C" int sl_slab_bytes(const uint8_t* rgb, int n, int h, int w, void* workspace, size_t workspace_bytes, unsigned long long* sums_a_out,
                             void* stream) {
    if (!sums_a_out || !slab_shape_ok(n, h, w) || (n > 0 && !rgb)) return SL_ERR_BADARG;
    const long P = (long)h * w;
    if (const int rc = slab_ws_check(workspace, workspace_bytes, n, P)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int rows = 0;
    if (n > 0) {
        const SlabPlan pl = slab_plan(n, P);
        if (pl.span * 12 >= (1LL << 32)) return SL_ERR_BADARG;            // (a device with a handful of CUs and a 2^40-pixel shard)
        rows = pl.rows;
        launch_aligned(aligned4(rgb, (long)n * P), k_slab_bytes<true>, k_slab_bytes<false>, dim3((unsigned)rows), dim3(kSlabWG), 0, s, rgb,
                       (unsigned long long)n * (unsigned long long)P * 3ull, pl.span, (unsigned long long*)workspace);
    }
    slab_reduce(workspace, rows, SL_SLAB_SUMS_A, -1, 0ull, sums_a_out, s);
    return launch_status();
}

extern "C" int sl_slab_begin(double* state, const unsigned long long* sums_a_reduced, int standardize, void* stream) {
    if (!state || (standardize && !sums_a_reduced)) return SL_ERR_BADARG;
    hipLaunchKernelGGL(k_slab_begin, dim3(1), dim3(256), 0, (hipStream_t)stream, state, sums_a_reduced, standardize ? 1 : 0);
    return launch_status();
}

extern "C" int sl_slab_lab(const uint8_t* rgb, int n, int h, int w, const double* state, double luminosity_threshold, void* workspace,
                           size_t workspace_bytes, unsigned long long* sums_b_out, void* stream) {
    if (!state || !sums_b_out || !slab_shape_ok(n, h, w) || (n > 0 && !rgb)) return SL_ERR_BADARG;
    const long P = (long)h * w;
    if (const int rc = slab_ws_check(workspace, workspace_bytes, n, P)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int rows = 0;
    if (n > 0) {
        const SlabPlan pl = slab_plan(n, P);
        if (pl.span * 12 >= (1LL << 32)) return SL_ERR_BADARG;
        rows = pl.rows;
        launch_aligned(aligned4(rgb, (long)n * P), k_slab_lab<true>, k_slab_lab<false>, dim3((unsigned)rows), dim3(kSlabWG), 0, s, rgb,
                       (unsigned long long)n * (unsigned long long)P * 3ull, pl.span, luminosity_threshold, state, (unsigned long long*)workspace);
    }
    slab_reduce(workspace, rows, SL_SLAB_SUMS_B, SL_SLAB_SUMS_B - 1, (unsigned long long)n * (unsigned long long)P, sums_b_out, s);
    return launch_status();
}

extern "C" int sl_slab_finish(double* state, const unsigned long long* sums_b_reduced, int mode, const double* target_means,
                              const double* target_stds, double percentile, int mask_background, void* stream) {
    if (!state || !sums_b_reduced || (mode != 0 && mode != 1)) return SL_ERR_BADARG;
    if (mode == 0 && (!target_means || !target_stds)) return SL_ERR_BADARG;
    hipLaunchKernelGGL(k_slab_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, state, sums_b_reduced, mode, target_means, target_stds, percentile,
                       mask_background ? 1 : 0);
    return launch_status();
}

extern "C" int sl_slab_map(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* state, int mode, int mask_background,
                           double luminosity_threshold, void* stream) {
    if (!rgb || !out || !state || n <= 0 || !slab_shape_ok(n, h, w) || (mode != 0 && mode != 1)) return SL_ERR_BADARG;
    const long P = (long)h * w;
    const SlabPlan pl = slab_plan(n, P);
    if (pl.span * 12 >= (1LL << 32)) return SL_ERR_BADARG;
    launch_aligned(aligned4(rgb, (long)n * P) && aligned4(out, (long)n * P), k_slab_map<true>, k_slab_map<false>, dim3((unsigned)pl.rows),
                   dim3(kSlabWG), 0, (hipStream_t)stream, rgb, out, (unsigned long long)n * (unsigned long long)P * 3ull, pl.span, state,
                   (mode == 0 && mask_background) ? 1 : 0, luminosity_threshold);
    return launch_status();
}
