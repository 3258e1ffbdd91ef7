// slide_dict.hip -- the POOLED slide-level Vahadane dictionary (vahadane_stain_extractor.py:28-43 on the vertical concatenation of
// every tile of every rank).
//
// The per-tile fit (stats_dict.hpp) learns the dictionary by CLASS MOMENTS: under a fixed dictionary D the exact code of a pixel is
// affine in its OD vector once its active set is known, so one sweep reduces a tile to 31 sums (3 classes x {n, sum x, sum x x^T}
// and the tissue count) and the block-coordinate update runs on those alone.  Sums decompose over tiles and ranks: the slide is
// "sweep every local tile under ONE shared D -> this rank's 31 sums -> all-reduce -> update", repeated.  The update is the per-tile
// one (dict_iter_update / dict_advance: the sample stage from the Ruifrok start, the a-posteriori stop, the step-back and 2-cycle
// safeguards), run by one workgroup on the all-reduced sums: every rank reaches the same state, bit for bit, without a broadcast.
//   sl_sdict_begin   DictIter at the Ruifrok start, mode 1 (sample)
//   sl_sdict_sweep   k_sd_sweep: persistent grid over the (tile, part) items of the local tiles, per-workgroup binary64 rows
//                    -> k_sd_reduce: one workgroup adds the rows in a fixed order (+ this rank's pixel count)
//   sl_sdict_step    k_sd_step: dict_iter_update + dict_advance on the reduced sums; at the end the stain matrix and a status
// The parts of a tile are a function of its pixel count alone (whole kDictAlignTrips spans, as in the per-tile k_dict), and the
// sample is placed by a sub-row's position inside its tile: the binary32 bursts of a tile do not depend on the shard it sits in.
#include "stats_kernels.hpp"
#include "sl_host.hpp"
#include <cmath>

using namespace sl;

namespace {

// ---- the state (doubles; include/stainlib_hip.h SL_SDICT_*) -------------------------------------------------------------------
enum { kM = SL_SDICT_M, kStatus = SL_SDICT_STATUS, kSweeps = SL_SDICT_SWEEPS, kRounds = SL_SDICT_ROUNDS, kMode = SL_SDICT_MODE,
       kD = SL_SDICT_D, kNpx = SL_SDICT_NPX, kSlog = 17, kCore = 24 };
struct SDictCore {
    DictIter it;
    DictProgress pr;
    int dead;                 // the last reduced sums left an atom without a pixel
    int pad_;
};
static_assert(kCore * 8 + sizeof(SDictCore) <= SL_SDICT_STATE_DOUBLES * 8, "SDictCore does not fit the state");
static_assert(SL_SDICT_SUMS == 32, "31 sums + the pixel count");

constexpr int kSdSpanChunks = kSweepThreads * kPhaseTrip * kDictAlignTrips;    // one part: the per-tile k_dict's alignment unit (64 Ki pixels)
constexpr int kSdSampleFlush = 16;                                            // sampled rounds: wave iterations per binary32 burst (64 pixels per lane)

inline int sd_parts(long P) {
    const long nch = (P + 3) >> 2;
    const long p = (nch + kSdSpanChunks - 1) / kSdSpanChunks;
    return (int)(p < 1 ? 1 : p);
}
inline int sd_grid(int n, long P) {
    const long items = (long)n * sd_parts(P);
    const long mg = max_resident_grid();
    return (int)(items < mg ? items : mg);
}

__device__ __forceinline__ SDictCore* core_of(double* st) { return reinterpret_cast<SDictCore*>(st + kCore); }

__global__ void k_sd_begin(double* st, int slog) {
    if (threadIdx.x != 0) return;
    SDictCore c;
    dict_iter_init(c.it);
    c.pr = DictProgress{1, 0, 0, 0};
    c.dead = 0; c.pad_ = 0;
    *core_of(st) = c;
    for (int i = 0; i < 6; ++i) { st[kM + i] = nan_d(); st[kD + i] = c.it.D[i]; }
    st[kStatus] = SL_TILE_OK; st[kSweeps] = 0; st[kRounds] = 0; st[kMode] = 1; st[kNpx] = 0; st[kSlog] = slog;
}

// The sampled round: in every 2^slog consecutive 64-pixel sub-rows of a tile (sub-row = 16 chunks) the one at offset
// hash(block) & mask.  One lane per chunk, four sub-rows per wave and iteration.
template <bool ALIGNED>
__device__ __forceinline__ void sd_sample_item(const uint8_t* src, int P, int c0, int c1, int slog, int tid, const TabReaderB& T,
                                               float ylimf, const DictK& L, DictWaveAcc& acc) {
    const size_t nbytes = (size_t)P * 3;
    const int lane = tid & 63, wave = tid >> 6, grp = lane >> 4, sub = lane & 15;
    const uint32_t mask = (1u << slog) - 1u;
    const uint32_t r0 = (uint32_t)c0 >> 4, rend = ((uint32_t)c1 + 15u) >> 4;
    const uint32_t b0 = r0 >> slog, b1 = ((rend - 1u) >> slog) + 1u;              // blocks touching [r0, rend)
    int its = 0;
    for (uint32_t j0 = b0 + (uint32_t)wave * 4u; j0 < b1; j0 += (kSweepThreads / 64) * 4u) {        // wave-uniform
        const uint32_t b = j0 + (uint32_t)grp;
        const uint32_t r16 = (b << slog) | ((sample_hash(b) >> 9) & mask);
        const bool live_row = b < b1 && r16 >= r0 && r16 < rend;
        const int cc = (int)(r16 * 16u) + sub;
        const bool live = live_row & (cc < c1);
        const Chunk ch = load_chunk_clamped<ALIGNED>(src, nbytes, live ? cc : c0, c1);
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const float2 er = T.gam_odf(T.addr(ch, 3 * px)), eg = T.gam_odf(T.addr(ch, 3 * px + 1)), eb = T.gam_odf(T.addr(ch, 3 * px + 2));
            const bool ok = live & (ALIGNED | ((size_t)cc * 4 + px < (size_t)P));
            acc.pixel(L, ok & is_tissue_f(er.x, eg.x, eb.x, ylimf), er.y, eg.y, eb.y);
        }
        if (++its == kSdSampleFlush) { acc.flush(lane); its = 0; }
    }
    if (its) acc.flush(lane);
}

// One round over this rank's tiles under the dictionary of the state: mode 1 the sample, 2 every pixel, 0 nothing (zeros).
// Each workgroup accumulates its items into its waves' binary64 rows and writes the sum of its rows: partials[blockIdx.x][32].
template <bool ALIGNED>
__global__ __launch_bounds__(kSweepThreads, 4) void k_sd_sweep(const uint8_t* rgb, int P, int parts, int n_items, int slog, float ylimf,
                                                               double lam, const double* st, double* partials) {
    __shared__ RowTab s_tab;
    __shared__ double s_red[kSweepThreads / 64][32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int mode = (int)st[kMode];                                         // uniform
    DictWaveAcc acc;
    acc.begin(s_red[tid >> 6], lane);
    if (mode == 1 || mode == 2) {
        s_tab.fill_b();
        __syncthreads();
        const TabReaderB T = TabReaderB::make(s_tab);
        DictK Ld;
        dict_consts(st + kD, lam, Ld);
        const int nch = (P + 3) >> 2;
        const bool stream = (size_t)P * 3 >= kStreamBytes;
        for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
            const int tile = item / parts, part = item % parts;
            const uint8_t* src = rgb + (size_t)tile * P * 3;
            int c0, c1;
            part_range(nch, parts, part, c0, c1, kDictAlignTrips);
            if (c0 >= c1) continue;                                          // block-uniform
            if (mode == 1) sd_sample_item<ALIGNED>(src, P, c0, c1, slog, tid, T, ylimf, Ld, acc);
            else if (stream) dict_sweep_b<ALIGNED, kDictTrip, true>(src, P, c0, c1, tid, kSweepThreads, T, ylimf, Ld, acc);
            else dict_sweep_b<ALIGNED, kDictTrip, false>(src, P, c0, c1, tid, kSweepThreads, T, ylimf, Ld, acc);
        }
    }
    __syncthreads();
    if (tid < 32) {
        double t = 0;
        if (tid < 31)
            for (int w = 0; w < kSweepThreads / 64; ++w) t += s_red[w][tid];
        partials[(size_t)blockIdx.x * 32 + tid] = t;
    }
}

// rows summed in a fixed order (run-to-run identical): wave v adds columns v and v + 16, lane l rows l, l + 64, ..., then a butterfly;
// out[31] = this rank's pixel count.  One workgroup of kSdReduceThreads.
constexpr int kSdReduceThreads = 1024;
__global__ __launch_bounds__(kSdReduceThreads) void k_sd_reduce(const double* partials, int rows, double npx, double* out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int col = wave; col < 32; col += kSdReduceThreads / 64) {        // wave-uniform
        double t = 0;
        if (col < 31)
            for (int r = lane; r < rows; r += 64) t += partials[(size_t)r * 32 + col];
        t = wave_sum(t);
        if (lane == 0) out[col] = col == 31 ? npx : t;
    }
}

// the update from the all-reduced sums (the body of dict_learn's loop / k_dict_finish, on the slide)
constexpr int kSdStepThreads = 64;
__global__ __launch_bounds__(kSdStepThreads) void k_sd_step(double* st, const double* sums, double lam, double tol, int max_sweeps) {
    __shared__ SDictCore s_c;
    __shared__ double s_sum[32];
    const int tid = threadIdx.x;
    if ((int)st[kMode] == 0) return;                                        // settled: every rank's later rounds are no-ops
    if (tid == 0) s_c = *core_of(st);
    if (tid < 32) s_sum[tid] = sums[tid];
    __syncthreads();
    DictProgress pr = s_c.pr;
    if (tid == 0) {
        if (st[kRounds] == 0.0) st[kNpx] = s_sum[31];                    // (the first round: the pixel count of the slide)
        if (s_sum[30] >= 1.0) s_c.dead = (s_sum[0] + s_sum[10] <= 0.0 || s_sum[0] + s_sum[20] <= 0.0) ? 1 : 0;
        dict_iter_update(s_c.it, s_sum, lam, pr.stage, pr.outer, pr.stage == 1 ? kDictSampleTol : tol);
    }
    __syncthreads();
    const bool go = dict_advance(s_c.it, pr, tol, tid) && pr.sweeps_used < max_sweeps;
    __syncthreads();
    if (tid == 0) {
        s_c.pr = pr;
        st[kRounds] += 1.0;
        st[kSweeps] = pr.sweeps_used;
        for (int i = 0; i < 6; ++i) st[kD + i] = s_c.it.D[i];
        if (go) {
            st[kMode] = pr.stage;
        } else {                                                            // dict_finalize of the per-tile schedule, plus the dead-atom rule
            int status = s_c.it.status;
            double M[6];
            if (status == SL_TILE_OK) {
                dict_iter_stain_matrix(s_c.it, M);                          // vahadane_stain_extractor.py:40-43
                if (stain_matrix_singular(M) || s_c.dead) status = SL_TILE_DEGENERATE_COV;
            }
            for (int i = 0; i < 6; ++i) st[kM + i] = status == SL_TILE_OK ? M[i] : nan_d();
            st[kStatus] = status;
            st[kMode] = 0;
        }
        *core_of(st) = s_c;
    }
}

}  // namespace

extern "C" size_t sl_sdict_workspace_bytes(int n, int h, int w) {
    if (n < 0 || h <= 0 || w <= 0 || (long)h * w > (1L << 30)) return 0;
    if (n == 0) return 256;
    const int g = sd_grid(n, (long)h * w);
    return ((size_t)g * 32 * sizeof(double) + 255) & ~(size_t)255;
}

extern "C" int sl_sdict_begin(const SlParams* params, int sample_log2, double* state, void* stream) {
    if (!state || sample_log2 < 0 || sample_log2 > 12 || !params_ok(params)) return SL_ERR_BADARG;
    hipLaunchKernelGGL(k_sd_begin, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sample_log2);
    return launch_status();
}

extern "C" int sl_sdict_sweep(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int sample_log2, const double* state,
                              void* workspace, size_t workspace_bytes, double* sums_out, void* stream) {
    if (!state || !sums_out || n < 0 || h <= 0 || w <= 0 || (n > 0 && !rgb)) return SL_ERR_BADARG;
    if (sample_log2 < 0 || sample_log2 > 12 || !params_ok(params)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    const long P = (long)h * w;
    if (P > (1L << 30) || (long)n * P > (1L << 40)) return SL_ERR_BADARG;
    const size_t need = sl_sdict_workspace_bytes(n, h, w);
    if (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < need) return SL_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int rows = 0;
    if (n > 0) {
        const int parts = sd_parts(P);
        const int items = n * parts;
        rows = sd_grid(n, P);
        const float ylimf = tissue_ylimf(p);
        const dim3 g((unsigned)rows), b(kSweepThreads);
        launch_aligned(aligned4(rgb, P), k_sd_sweep<true>, k_sd_sweep<false>, g, b, 0, s, rgb, (int)P, parts, items, sample_log2, ylimf, p.dl_lambda,
                       state, (double*)workspace);
    }
    hipLaunchKernelGGL(k_sd_reduce, dim3(1), dim3(kSdReduceThreads), 0, s, (const double*)workspace, rows, (double)n * (double)P, sums_out);
    return launch_status();
}

extern "C" int sl_sdict_step(double* state, const double* sums_reduced, const SlParams* params, void* stream) {
    if (!state || !sums_reduced || !params_ok(params)) return SL_ERR_BADARG;
    const SlParams p = params_or_defaults(params);
    if (!(p.dl_lambda >= 0.0) || !(p.dl_tol > 0.0) || p.dl_max_sweeps < 1) return SL_ERR_BADARG;
    hipLaunchKernelGGL(k_sd_step, dim3(1), dim3(kSdStepThreads), 0, (hipStream_t)stream, state, sums_reduced, p.dl_lambda, p.dl_tol,
                       p.dl_max_sweeps);
    return launch_status();
}
