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
#include "lab_host.hpp"          // slab_shape_ok

using namespace sl;

namespace {

enum { kP90 = SL_SLAB_P90, kMeans = SL_SLAB_MEANS, kStds = SL_SLAB_STDS, kLpct = SL_SLAB_LPCT, kTissue = SL_SLAB_TISSUE, kNpx = SL_SLAB_NPX,
       kStatus = SL_SLAB_STATUS, kTables = SL_SLAB_TABLES };

// the composed tables of the slide fill state[SL_SLAB_TABLES ...] (what LabTileTabs holds per tile)
static_assert(kTables * 8 + sizeof(LabMapTabs) == SL_SLAB_STATE_DOUBLES * 8, "LabMapTabs is the rest of the state");
static_assert(SL_SLAB_SUMS_A == 256 && SL_SLAB_SUMS_B == 262, "256 counts; 256 counts + 4 sums + tissue pixels + pixels");

__device__ __forceinline__ LabMapTabs* tabs_of(double* st) { return reinterpret_cast<LabMapTabs*>(st + kTables); }
__device__ __forceinline__ const LabMapTabs* tabs_of(const double* st) { return reinterpret_cast<const LabMapTabs*>(st + kTables); }

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

// this workgroup's span: where it starts, how many bytes and chunks it holds
__device__ __forceinline__ ChunkSpan span_of(const uint8_t* rgb, unsigned long long total_bytes, long long span) {
    ChunkSpan s;
    s.off = (size_t)blockIdx.x * (size_t)span * 12;
    s.src = rgb + s.off;
    const size_t left = s.off < total_bytes ? (size_t)total_bytes - s.off : 0;
    s.nbytes = left < (size_t)span * 12 ? left : (size_t)span * 12;
    s.nloc = (int)((s.nbytes + 11) / 12);
    return s;
}

// ---- sweep A: the byte counts of this rank's shard: partials[blockIdx.x][0 .. 255] ---------------------------------------------
template <bool ALIGNED>
__global__ __launch_bounds__(kSlabWG) void k_slab_bytes(const uint8_t* __restrict__ rgb, unsigned long long total_bytes, long long span,
                                                        unsigned long long* __restrict__ partials) {
    __shared__ uint32_t s_h[kSlabWG / 64][kSlabCopies][256];
    for (int i = threadIdx.x; i < (kSlabWG / 64) * kSlabCopies * 256; i += kSlabWG) (&s_h[0][0][0])[i] = 0;
    __syncthreads();
    uint32_t* h = s_h[threadIdx.x >> 6][threadIdx.x & (kSlabCopies - 1)];
    const ChunkSpan s = span_of(rgb, total_bytes, span);
    // (a span holds fewer than 2^32 bytes -- sl_slab_bytes checks it --, so the 32-bit counters cannot wrap)
    lab_sweep2<ALIGNED, false, kSlabWG>(s, 0, [&](const Chunk& in, int c) { count_chunk_bytes<ALIGNED>(h, in, c, s.nbytes); });
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
    const ChunkSpan s = span_of(rgb, total_bytes, span);
    const size_t npx = s.nbytes / 3;
    uint32_t n_tissue = 0, sa = 0, sb = 0;                           // a lane sees < 2^32 / (3 * 256) pixels of its span: the plain sums fit 32 bits
    unsigned long long saa = 0, sbb = 0;
    lab_sweep2<ALIGNED, false, kSlabWG>(s, 0, [&](const Chunk& in, int c) {
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
    const int tid = threadIdx.x;
    const double p = lab_begin_tables(*tabs_of(st), sums_a, standardize);
    if (tid < kTables) st[tid] = tid == kP90 ? p : ((tid >= kMeans && tid <= kLpct) ? nan("") : 0.0);      // (status SL_TILE_OK = 0)
}

// ---- after the second all-reduce: the slide's statistics and the composed tables of the map (what k_lab_tables does per tile) ---------
__global__ __launch_bounds__(256) void k_slab_finish(double* __restrict__ st, const unsigned long long* __restrict__ sums_b, int mode,
                                                     const double* __restrict__ target_means, const double* __restrict__ target_stds,
                                                     double percentile, int mask_background) {
    __shared__ LabScratch s_sc;
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
    lab_finish_tables(*tabs_of(st), mode, s_ms, target_means, target_stds, s_p);
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
    const ChunkSpan s = span_of(rgb, total_bytes, span);
    uint8_t* dst = out + s.off;
    if (s.nloc <= 0) return;
    if ((int)st[kStatus] != SL_TILE_OK) {                              // unusable statistics: the tiles go through unchanged (k_apply's rule)
        for (int c = tid; c < s.nloc; c += kSlabWG) store_chunk<ALIGNED>(dst, s.nbytes, c, load_chunk<ALIGNED>(s.src, s.nbytes, c));
        return;
    }
    const LabMapTabs* tt = tabs_of(st);
    s_t.fill();
    s_g[tid] = tt->g[tid];
    s_yf[tid] = tt->yf[tid];
    s_ad[tid] = tt->ad[tid];
    s_bd[tid] = tt->bd[tid];
    __syncthreads();
    const int lim = l8_limit(thr);
    const LabBackground bg = lab_background();
    lab_sweep2<ALIGNED, true, kSlabWG>(s, 0, [&](const Chunk& in, int c) {
        store_chunk<ALIGNED>(dst, s.nbytes, c, lab_map_chunk<true>(s_t, s_g, s_yf, s_ad, s_bd, in, mask_bg, lim, bg));
    });
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

// A statistics sweep of the shard and the reduce of its partial rows: sl_slab_bytes (cols SL_SLAB_SUMS_A) and sl_slab_lab (cols
// SL_SLAB_SUMS_B, whose last column is the pixel count no row carries).  `args`: what the kernel takes between the span and the partials.
template <class K, class... Args>
int slab_sums(K k_aligned, K k_unaligned, const uint8_t* rgb, int n, int h, int w, void* workspace, size_t workspace_bytes, int cols, int extra_col,
              unsigned long long* out, void* stream, Args... args) {
    if (!out || !slab_shape_ok(n, h, w) || (n > 0 && !rgb)) return SL_ERR_BADARG;
    const long P = (long)h * w;
    if (const int rc = slab_ws_check(workspace, workspace_bytes, n, P)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int rows = 0;
    if (n > 0) {
        const SlabPlan pl = slab_plan(n, P);
        if (pl.span * 12 >= (1LL << 32)) return SL_ERR_BADARG;            // (a device with a handful of CUs and a 2^40-pixel shard)
        rows = pl.rows;
        launch_aligned(aligned4(rgb, (long)n * P), k_aligned, k_unaligned, dim3((unsigned)rows), dim3(kSlabWG), 0, s, rgb,
                       (unsigned long long)n * (unsigned long long)P * 3ull, pl.span, args..., (unsigned long long*)workspace);
    }
    slab_reduce(workspace, rows, cols, extra_col, (unsigned long long)n * (unsigned long long)P, out, s);
    return launch_status();
}

}  // namespace

extern "C" size_t sl_slab_workspace_bytes(int n, int h, int w) {
    if (!slab_shape_ok(n, h, w)) return 0;
    return slab_ws_bytes(n, (long)h * w);
}

extern "C" int sl_slab_bytes(const uint8_t* rgb, int n, int h, int w, void* workspace, size_t workspace_bytes, unsigned long long* sums_a_out,
                             void* stream) {
    return slab_sums(k_slab_bytes<true>, k_slab_bytes<false>, rgb, n, h, w, workspace, workspace_bytes, SL_SLAB_SUMS_A, -1, sums_a_out, stream);
}

extern "C" int sl_slab_begin(double* state, const unsigned long long* sums_a_reduced, int standardize, void* stream) {
    if (!state || (standardize && !sums_a_reduced)) return SL_ERR_BADARG;
    hipLaunchKernelGGL(k_slab_begin, dim3(1), dim3(256), 0, (hipStream_t)stream, state, sums_a_reduced, standardize ? 1 : 0);
    return launch_status();
}

extern "C" int sl_slab_lab(const uint8_t* rgb, int n, int h, int w, const double* state, double luminosity_threshold, void* workspace,
                           size_t workspace_bytes, unsigned long long* sums_b_out, void* stream) {
    if (!state) return SL_ERR_BADARG;
    return slab_sums(k_slab_lab<true>, k_slab_lab<false>, rgb, n, h, w, workspace, workspace_bytes, SL_SLAB_SUMS_B, SL_SLAB_SUMS_B - 1, sums_b_out,
                     stream, luminosity_threshold, state);
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
