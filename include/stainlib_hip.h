/*
 * stainlib_hip.h -- C ABI of the MI355X-native H&E stain-normalization engine.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json.  The
 * reference (sebastianffx/stainlib v0.6.1) has no FFI: its "operator API" is a
 * handful of Python classes whose arithmetic lives in numpy / OpenCV / spams /
 * scikit-image.  Each entry point below replaces one reference call chain
 * (cited as file:line, relative to the reference checkout) and is what a
 * ctypes binding inside stainlib would call (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer (HBM), e.g. torch tensor.data_ptr();
 *     SlParams, SlTensorFormat and SlSeparateOut are the only host structs (a few pooled-mode calls take small host arrays, named where
 *     they are declared).
 *   - images: n tiles, each h x w x 3 interleaved RGB uint8, tiles contiguous
 *     (NHWC).  Stain matrices: row-major 2x3 double, row 0 = haematoxylin.
 *   - the caller owns every buffer including the workspace; the library keeps
 *     no state, allocates nothing, and is re-entrant per stream.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and returns without synchronising the host.
 *   - return value: 0 on success, SL_ERR_* (<0) otherwise.  No C++ exception
 *     crosses this boundary.  Per-tile conditions are reported in status[i].
 */
#ifndef STAINLIB_HIP_H
#define STAINLIB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_VERSION 600 /* 0.6.0: sl_pool2_* (the pooled slide statistics in one full sweep), two_sweep validated; 0.5.0: SlParams starts with struct_size (checked by every entry point), two_sweep / twosweep_out; 0.4.0: prefilter, prefilter_out; 0.3.0: fused_min_tiles, sl_pool_*, resweeps_out carries reasons */

/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#if defined(__GNUC__)
#define SL_API __attribute__((visibility("default")))
#else
#define SL_API
#endif

/* return codes */
#define SL_OK 0
#define SL_ERR_BADARG (-1)    /* null pointer, n/h/w <= 0, unknown op/mode; on every per-tile entry point also h w > 2^30 and a batch
                                 whose (tile, part) grid does not fit 31 bits: n * ceil(h w / 32768) > 2^31 - 1 (the views: n times
                                 the 64 x 64 patches of an output) */
#define SL_ERR_WORKSPACE (-2) /* workspace missing or smaller than sl_workspace_bytes() */
#define SL_ERR_NODEVICE (-3)  /* no HIP device / wrong architecture */
#define SL_ERR_HIP_BASE (-1000) /* HIP runtime error e is returned as SL_ERR_HIP_BASE - e */

/* per-tile status[i] */
#define SL_TILE_OK 0
#define SL_TILE_EMPTY_MASK 1     /* stain_utils.py:46-47 -> TissueMaskException */
#define SL_TILE_DEGENERATE_COV 2 /* fewer than 2 tissue pixels (np.cov is NaN in the reference), or tissue of a single colour:
                                    two parallel stain vectors, inf/NaN concentrations in the reference */
#define SL_TILE_ZERO_MAXC 3      /* 99th percentile of a concentration is 0: normalizer.py:48 divides by it (inf / NaN cast to uint8
                                    in the reference).  A tile with any non-zero status is passed through unchanged by the transforms. */

/* ops for sl_workspace_bytes */
#define SL_OP_MACENKO_FIT 1
#define SL_OP_MACENKO_TRANSFORM 2
#define SL_OP_VAHADANE_FIT 3
#define SL_OP_VAHADANE_TRANSFORM 4
#define SL_OP_HED_AUGMENT 5
#define SL_OP_STAIN_AUGMENT 6
#define SL_OP_TILE_MOMENTS 7
#define SL_OP_LAB_STATS 8        /* sl_reinhard_stats, sl_reinhard_transform, sl_luminosity_standardize, sl_standardize_brightness */

/* selection key sets of the pooled slide-level mode (sl_slide_key_*): each set carries TWO targets */
#define SL_KEYSET_ANGLE 0 /* both targets: pseudo-angle of the projected OD, tissue pixels only (macenko_stain_extractor.py:29-34) */
#define SL_KEYSET_CONC 1  /* target i: lasso concentration of stain i, all pixels (normalizer.py:36,47) */

/* skimage semantics selector for sl_hed_augment.  Only 0.18 is pinned by vectors from a real scikit-image
 * (0.18.3); the other three are restated from memory and checked against the CPU restatement only -- no source or wheel
 * of those releases exists in the build environment. */
#define SL_HED_SKIMAGE_018 0 /* ln(max(rgb,1e-6))/ln(1e-6) @ hed_from_rgb  (golden-pinned) */
#define SL_HED_SKIMAGE_019 1 /* as 0.18 + stains clamped at 0 after separation  (unpinned) */
#define SL_HED_SKIMAGE_017 2 /* presumed <= 0.17 (environment.yml:107 pins 0.17.2): -ln(rgb + 2) @ hed_from_rgb,
                                exp(-stains @ rgb_from_hed) - 2, clipped  (natural logarithm; unpinned) */
#define SL_HED_EXPERIMENTAL_LOG10 3 /* the same with a base-10 logarithm (round 1's reading of 0.17; kept as an experiment, unpinned) */

/* Optional kernel timing.  When SlParams.profile is non-NULL, sl_*_fit / sl_*_transform bracket every
 * launch of the selected kernel classes with two caller-created hipEvent_t from events[] (start, stop),
 * on the same stream as the kernels, and record which class each pair belongs to.  The library only
 * records; the caller synchronises and reads hipEventElapsedTime.  Launches beyond `capacity` are
 * simply not bracketed. */
#define SL_PROF_MOMENTS 1
#define SL_PROF_SELECT_ANGLE 2
#define SL_PROF_SELECT_CONC 4
#define SL_PROF_FINISH 8
#define SL_PROF_APPLY 16
#define SL_PROF_DICT 32
#define SL_PROF_FUSED_FIT 64       /* the persistent one-workgroup-per-tile kernel, fit only */
#define SL_PROF_FUSED_TRANSFORM 128 /* the same including the apply sweep */
typedef struct SlProfile {
    void** events;      /* capacity caller-owned hipEvent_t */
    int32_t* tags;      /* capacity/2 ints, out: SL_PROF_* class of pair i */
    int32_t* tiles;     /* capacity/2 ints, out: tiles covered by the launch of pair i */
    int32_t capacity;   /* number of events available (even) */
    int32_t used;       /* in/out: events consumed so far (start at 0) */
    int32_t mask;       /* OR of SL_PROF_* classes to bracket */
    int32_t reserved;
} SlProfile;

/* Extractor constants.  The reference never forwards these from fit/transform, so the
 * defaults are effectively constants (macenko_stain_extractor.py:7,
 * vahadane_stain_extractor.py:19, stain_utils.py:69). */
#define SL_RESWEEP_NO_BOX 1         /* the sample's brackets left no usable box of stain matrices (open, or too wide) */
#define SL_RESWEEP_OUTSIDE_BOX 2    /* the exact stain matrix fell outside the box the sweep assumed */
#define SL_RESWEEP_BRACKET_MISSED 3 /* a concentration bracket did not hold the wanted rank */
#define SL_RESWEEP_LIST_FULL 4      /* the candidate list overflowed */
/* what became of a tile's two-sweep attempt (SlParams.twosweep_out) */
#define SL_TWOSWEEP_DIRECT 1        /* the tile's stain matrix came out of two read sweeps (moments + candidates in one, then the apply pass) */
#define SL_TWOSWEEP_OFF 0           /* not attempted (SlParams.two_sweep == 1, a schedule without it, or the workgroup was backing off after a decline) */
#define SL_TWOSWEEP_NO_ESTIMATE (-1) /* the cluster sample gave no usable estimate (few tissue entries, an ill-defined plane, open brackets) */
#define SL_TWOSWEEP_SHARE (-2)      /* too many of the sample's pixels in colour-cube cells the mask could not prove plain: not worth it */
#define SL_TWOSWEEP_PLANE (-3)      /* the exact eigenvector plane left the tilt the sweep allowed for: three-sweep route from the exact moments */
#define SL_TWOSWEEP_BRACKET (-4)    /* an angular bracket carried over from the estimate missed its rank (or a list overflowed): likewise */
#define SL_TWOSWEEP_LISTS (-5)      /* the sample predicts more bracket members than the candidate lists hold: not attempted */
typedef struct SlParams {
    uint32_t struct_size;        /* sizeof(SlParams) of the header the CALLER was compiled against: set by sl_default_params, checked by every
                                    entry point that takes an SlParams (SL_ERR_BADARG on a mismatch) -- a caller built against another
                                    version of this struct is refused instead of being read past its end */
    uint32_t reserved0;
    double luminosity_threshold; /* 0.8  (binary64 like the Python float the reference compares with).  ANY value: the tissue test is
                                    L8 / 255.0 < threshold as the reference writes it -- at 0 and below, and for NaN, no pixel is tissue
                                    (every tile SL_TILE_EMPTY_MASK); above 1 every pixel is, saturated white included */
    double angular_percentile;   /* 99.  [0, 100]; outside it, or NaN: SL_ERR_BADARG (np.percentile raises there).  The pair the reference
                                    takes is (100 - p, p) and it orders the two stain vectors afterwards, so p and 100 - p give the same
                                    matrix: the kernels run with max(p, 100 - p).  50 makes the two vectors one: SL_TILE_DEGENERATE_COV */
    double lasso_lambda;        /* 0.01.  >= 0; negative or NaN: SL_ERR_BADARG -- from every entry point that takes an SlParams and from those
                                   that take lasso_lambda as a bare double (sl_normalize_apply, sl_normalize_apply_tensor, sl_concentrations,
                                   sl_stain_separate).  0 is plain non-negative least squares; a penalty above every pixel's projection
                                   zeroes all concentrations: SL_TILE_ZERO_MAXC */
    double dl_lambda;           /* 0.1  (Vahadane) */
    int32_t dl_max_sweeps;      /* 200  (Vahadane; the reference is wall-clock budgeted) */
    int32_t schedule;           /* 0 = automatic; 1 = one launch per phase; 2 = persistent fused kernel (two 512-thread workgroups per CU);
                                   3 = Macenko only: the fused kernel with one 1024-thread workgroup per CU where the batch has no more tiles
                                   than the device has CUs (else as 2) */
    double dl_tol;              /* 1e-7 the dictionary iteration stops when a full sweep moves D by less than this (max-abs), or
                                        when the a-posteriori estimate of its distance to the fixed point (the step the next sweep would
                                        take, predicted from the last two) is below it */
    SlProfile* profile;         /* NULL (default): no timing events */
    int32_t* fallbacks_out;     /* NULL (default) or DEVICE pointer to n ints: per tile, how many of its four order statistics
                                   (two angular, two concentration percentiles) needed the slow exact selection over the whole
                                   tile because the sampled bracket missed or its candidate list overflowed (diagnostics;
                                   results never depend on it).  Written by sl_macenko_* / sl_vahadane_*. */
    int32_t* resweeps_out;      /* NULL (default) or DEVICE pointer to n ints: nonzero (an SL_RESWEEP_* reason, below) for a tile whose concentration percentiles needed a
                                   selection sweep of their own (the persistent Macenko kernel collects the angular and the
                                   concentration candidates in ONE sweep under a sample estimate of the stain matrix and repeats
                                   the concentration part when the exact matrix falls outside the assumed box; diagnostics).
                                   Written by the fused schedule of sl_macenko_*; left untouched otherwise. */
    int32_t fused_min_tiles;    /* schedule == 0 only: batches of at least this many tiles run the persistent fused kernel, smaller ones
                                   one launch per phase.  0 (default) = the library's measured crossovers on an MI355X at its 1400 W
                                   power state (tools/crossover.py, profiles/r04_crossover*.txt): Macenko 352 tiles (320 for tiles below 512 Ki
                                   pixels, 288 up to 256 Ki), Vahadane 640 (192 below 512 Ki pixels; 704 when the batch exceeds one resident grid).  A Macenko batch larger than the fused
                                   kernel's resident grid (2 x compute units) is split: whole fused rounds, and a remainder below this
                                   number of tiles one launch per phase (default: 208 / 224 / 192 tiles by the same tile sizes, never for
                                   tiles up to 64 Ki pixels).  Results do not depend on the schedule. */
    int32_t prefilter;          /* the colour-cube pre-filter of the fused Macenko kernel's selection sweep (a 32^3-cell mask of colours that are
                                   provably "plain", built per tile by finish 1; pixels of the other cells are re-tested exactly):
                                   0 (default) = per tile, wherever the tile's pixel sample says it pays; 1 = never (the per-pixel sweep);
                                   2 = wherever the mask can be built, whatever the sample says (tests).  Results do not depend on it. */
    int32_t* prefilter_out;     /* NULL (default) or DEVICE pointer to n ints: bit 0 set for a tile whose selection sweep ran behind the mask,
                                   bits 8.. the share (percent) of the tile's sample pixels that fell into cells the mask could not
                                   prove plain (0 when no mask was built; diagnostics).  Written by the fused schedule of sl_macenko_*;
                                   left untouched otherwise. */
    int32_t two_sweep;          /* the two-read-sweep schedule of the fused Macenko kernel (the candidates of all four order statistics are
                                   collected in the moments sweep, under eigenvectors estimated from a cluster sample gathered before it, and
                                   the finish verifies the estimate against the exact eigenvectors; a tile that fails takes the three-sweep
                                   route): 0 (default) = per tile, wherever the sample says it pays (a workgroup whose tile declined skips the attempt on its next
                                   three tiles); 1 = never; 2 = wherever an estimate
                                   exists (tests); 3 = as 2 with the verification forced to fail, 4 = as 2 with the sample's plane tilted
                                   (tests of the fallback).  Any other value: SL_ERR_BADARG.  The test modes 2-4 run the merged sweep behind
                                   the colour-cube mask even under prefilter == 1 (that sweep has no per-pixel form); in the automatic mode
                                   prefilter == 1 rules the route out.  Results do not depend on it.  On real tissue the automatic mode
                                   mostly declines after its sample's eigen-solve (+2-3 % against two_sweep = 1 on such batches, -6-10 % on
                                   synthetic ones: DESIGN 4.1). */
    int32_t reserved1;
    int32_t* twosweep_out;      /* NULL (default) or DEVICE pointer to n ints: SL_TWOSWEEP_* per tile (diagnostics).  Written by the fused
                                   schedule of sl_macenko_*; left untouched otherwise. */
} SlParams;

/* sl_version() == SL_VERSION must be checked BEFORE any other call: sl_default_params writes sizeof(SlParams) of THIS library's
 * header into the caller's struct -- a caller compiled against a header with a smaller SlParams would be written past its end before
 * any struct_size check could run (the ctypes binding refuses a library of another version: stainlib_amd/_ffi.py). */
SL_API int sl_version(void);
SL_API const char* sl_error_string(int code);
SL_API void sl_default_params(SlParams* p);

/* Bytes of device workspace an op needs for n tiles of h x w.  0 for ops that need none.
 * The layout depends on the number of compute units of the CURRENT HIP device (persistent grids are sized to it): call this
 * with the device current on which the operator will be launched (same partition mode); a workspace sized under another
 * device may be refused with SL_ERR_WORKSPACE, never overrun. */
SL_API size_t sl_workspace_bytes(int op, int n_tiles, int h, int w);
/* sl_workspace_bytes is the maximum over every SlParams (a workspace of that size serves any call of the op at this batch shape).
 * What ONE call needs -- the schedule its SlParams (NULL: the defaults) select: the one-launch-per-phase schedule has no angular
 * candidate list, 28 % less per tile -- is sl_workspace_bytes_for; the entry points check against this figure.  0: bad arguments. */
SL_API size_t sl_workspace_bytes_for(int op, int n_tiles, int h, int w, const SlParams* params);

/* MacenkoStainExtractor.get_stain_matrix (extraction/macenko_stain_extractor.py:7-44)
 * + get_concentrations (utils/stain_utils.py:69-78) + np.percentile(C, 99, axis=0)
 * (normalization/normalizer.py:34-36), for each of n tiles.
 *   M_out    n x 2 x 3 double   unit-norm rows, H first
 *   maxC_out n x 2 double
 *   status   n int32 */
SL_API int sl_macenko_fit(const uint8_t* rgb, int n, int h, int w, const SlParams* params,
                   double* M_out, double* maxC_out, int32_t* status,
                   void* workspace, size_t workspace_bytes, void* stream);

/* VahadaneStainExtractor.get_stain_matrix (extraction/vahadane_stain_extractor.py:19-43) with
 * spams.trainDL replaced by the converged optimum of the same objective, then as above.  "The" optimum of this
 * non-convex problem is the point plain full-batch block-coordinate descent reaches from Ruifrok's H and E vectors
 * (oracle/stain_oracle.py vahadane_dictionary); the device iteration is an acceleration of that scheme that takes a
 * step back whenever the objective rose or an atom lost all its pixels, so that it stays on the plain scheme's path.
 *   sweeps_out  n int32 (may be NULL): dictionary sweeps used per tile */
SL_API int sl_vahadane_fit(const uint8_t* rgb, int n, int h, int w, const SlParams* params,
                    double* M_out, double* maxC_out, int32_t* status, int32_t* sweeps_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The OD + reconstruction pass: get_concentrations on every pixel with the tile's own
 * stain matrix, rescale by maxC_tgt / maxC_src, 255*exp(-C @ M_tgt), truncating uint8 cast
 * (utils/stain_utils.py:69-78,101-112 ; normalization/normalizer.py:46-50).
 *   M_src n x 2 x 3, maxC_src n x 2 (per tile); M_tgt 2 x 3, maxC_tgt 2 (shared)
 *   prequant  optional n x P x 3 float: the values before the uint8 cast (parity tests) */
SL_API int sl_normalize_apply(const uint8_t* rgb, uint8_t* out, int n, int h, int w,
                       const double* M_src, const double* maxC_src,
                       const double* M_tgt, const double* maxC_tgt,
                       double lasso_lambda, float* prequant, void* stream);

/* ExtractiveStainNormalizer('macenko').transform (normalization/normalizer.py:39-50) for a
 * batch: per-tile fit stages + the apply pass in one cache-friendly schedule.
 *   M_src_out n x 2 x 3 / maxC_src_out n x 2 may be NULL. */
SL_API int sl_macenko_transform(const uint8_t* rgb, uint8_t* out, int n, int h, int w,
                         const SlParams* params, const double* M_tgt, const double* maxC_tgt,
                         double* M_src_out, double* maxC_src_out, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ExtractiveStainNormalizer('vahadane').transform, same shape. */
SL_API int sl_vahadane_transform(const uint8_t* rgb, uint8_t* out, int n, int h, int w,
                          const SlParams* params, const double* M_tgt, const double* maxC_tgt,
                          double* M_src_out, double* maxC_src_out, int32_t* status,
                          void* workspace, size_t workspace_bytes, void* stream);

/* HedColorAugmenter.transform (augmentation/augmenter.py:276-331) for uint8 tiles:
 * cutoff test on the tile mean, rgb2hed, per-channel x*(1+sigma)+bias, hed2rgb, clip, *255,
 * truncate.  sigma, bias: n x 3 double (H, E, D).  applied[i] (may be NULL) = 0 when tile i failed
 * cutoff_lo <= mean/255 <= cutoff_hi; such a tile is copied through unchanged.
 * workspace: sl_workspace_bytes(SL_OP_HED_AUGMENT, n, h, w) = 8 n bytes. */
SL_API int sl_hed_augment(const uint8_t* rgb, uint8_t* out, int n, int h, int w,
                   const double* sigma, const double* bias, double cutoff_lo, double cutoff_hi,
                   int skimage_mode, int32_t* applied,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The float branch of HedColorAugmenter.transform (augmentation/augmenter.py:288-289, 319-320): patches of
 * binary64 values in [0,1], n x h x w x 3; cutoff on np.mean(patch); binary64 arithmetic; clipped output.
 * workspace: 8 n bytes. */
SL_API int sl_hed_augment_f64(const double* rgb, double* out, int n, int h, int w,
                       const double* sigma, const double* bias, double cutoff_lo, double cutoff_hi,
                       int skimage_mode, int32_t* applied,
                       void* workspace, size_t workspace_bytes, void* stream);

/* convert_RGB_to_OD (utils/stain_utils.py:101-112) materialised: od_out n x h x w x 3 double. */
SL_API int sl_rgb_to_od(const uint8_t* rgb, int n, int h, int w, double* od_out, void* stream);

/* convert_OD_to_RGB (utils/stain_utils.py:114-124): rgb_out[i] = uint8(255 * exp(-max(od[i], 1e-6))) for n_values doubles.
 * negative_flag (device int32, may be NULL) is set to 1 when any od[i] < 0 (the reference asserts "Negative optical density."). */
SL_API int sl_od_to_rgb(const double* od, size_t n_values, uint8_t* rgb_out, int32_t* negative_flag, void* stream);

/* StainAugmentor.pop (augmentation/augmenter.py:428-449): concentrations with the tile's
 * stain matrix M (n x 2 x 3), C[:,i] = C[:,i]*alpha_i + beta_i on tissue pixels (all pixels
 * when augment_background), 255*exp(-C @ M), clip to [0,255], truncate.
 *   alpha_beta n x 4 double: alpha0, beta0, alpha1, beta1 (the reference's draw order) */
SL_API int sl_stain_augment(const uint8_t* rgb, uint8_t* out, int n, int h, int w,
                     const double* M, const double* alpha_beta, int augment_background,
                     const SlParams* params, void* stream);

/* LuminosityThresholdTissueLocator.get_tissue_mask (utils/stain_utils.py:32-48):
 * mask_out n x P uint8 (0/1, may be NULL), counts n int64 (may be NULL). */
SL_API int sl_tissue_mask(const uint8_t* rgb, int n, int h, int w, double luminosity_threshold,
                   uint8_t* mask_out, int64_t* counts, void* stream);

/* get_concentrations (utils/stain_utils.py:69-78) materialised: C_out n x P x 2 float. */
SL_API int sl_concentrations(const uint8_t* rgb, int n, int h, int w, const double* M,
                      double lasso_lambda, float* C_out, void* stream);

/* GrayscaleAugmentor.pop (augmentation/augmenter.py:390-401): out = 3 x uint8(255 * clip(rgb2gray * alpha +
 * beta, 0, 1)), binary64 arithmetic like the reference.  alpha_beta: n x 2 doubles (device). */
SL_API int sl_grayscale_augment(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* alpha_beta,
                         void* stream);

/* ---- OpenCV 8-bit Lab family: ReinhardStainNormalizer, LuminosityStandardizer, LAB helpers.
 * cv2.cvtColor on uint8 images is restated from OpenCV's published RGB2Lab_b / Lab2RGBinteger (integer tables); no cv2 exists in
 * the build environment, so this family is PARITY UNPINNED against OpenCV itself (tools/pin_cv2.py checks it wherever cv2 is
 * installed).  The reference's own arithmetic around it (percentiles, binary32/binary64 promotion, clip-then-truncate, masking)
 * is golden-pinned.  Workspace of the four entry points that take one: sl_workspace_bytes(SL_OP_LAB_STATS, n, h, w). */

/* cv2.cvtColor(I, COLOR_RGB2LAB), uint8 (utils/stain_utils.py:62,152): lab_out n x h x w x 3 = L*255/100, a+128, b+128. */
SL_API int sl_rgb_to_lab8(const uint8_t* rgb, uint8_t* lab_out, int n, int h, int w, void* stream);
/* cv2.cvtColor(LAB, COLOR_LAB2RGB), uint8 (utils/stain_utils.py:66,172). */
SL_API int sl_lab8_to_rgb(const uint8_t* lab, uint8_t* rgb_out, int n, int h, int w, void* stream);
/* lab_split (utils/stain_utils.py:146-158): three n x h x w binary32 planes L8/2.55, a8-128, b8-128. */
SL_API int sl_lab_split(const uint8_t* rgb, int n, int h, int w, float* I1, float* I2, float* I3, void* stream);
/* merge_back (utils/stain_utils.py:160-172): I1*2.55, I2+128, I3+128 in the planes' own precision (is_f64: binary64 planes,
 * else binary32), clip [0,255], truncate, LAB2RGB.  The planes are not modified (the reference scales them in place). */
SL_API int sl_lab_merge(const void* I1, const void* I2, const void* I3, int is_f64, int n, int h, int w, uint8_t* rgb_out, void* stream);

/* standardize_brightness (utils/stain_utils.py:188-194): p = 90th percentile (np.percentile, linear) of ALL byte values of the
 * tile, out = uint8(clip(I * 255.0 / p, 0, 255)).  p_out: n doubles (may be NULL). */
SL_API int sl_standardize_brightness(const uint8_t* rgb, uint8_t* out, int n, int h, int w, double* p_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* get_mean_std (utils/stain_utils.py:174-186; cv2.meanStdDev of the lab_split planes: population std), optionally of the
 * brightness-standardised tile (standardize != 0: what ReinhardStainNormalizer.fit / transform feed it, normalizer.py:65-66,78-80).
 *   stats_out n x 8 double: p90 (NaN when !standardize), mean L, a, b, std L, a, b, and the number of tissue pixels of the
 *   (standardised) tile at luminosity threshold 0.8 (what transform(mask_background=True) tests for emptiness) */
SL_API int sl_reinhard_stats(const uint8_t* rgb, int n, int h, int w, int standardize, double* stats_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ReinhardStainNormalizer.transform (normalization/normalizer.py:70-94): standardize_brightness, lab_split, per-channel
 * (x - mean) * (target_std / std) + target_mean in binary64, optional background masking with the luminosity test of the
 * standardised tile (background -> L 254, a = b = 0 before merge_back), merge_back.
 *   target_means / target_stds: 3 doubles each (DEVICE), shared by all tiles
 *   stats_out n x 8 (may be NULL): as sl_reinhard_stats(standardize = 1), last entry = tissue pixels of the standardised tile
 *                                  (0 with mask_background -> the reference raises TissueMaskException) */
SL_API int sl_reinhard_transform(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* target_means,
                          const double* target_stds, int mask_background, double luminosity_threshold, double* stats_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* LuminosityStandardizer.standardize (utils/stain_utils.py:52-67): p = np.percentile(L8, percentile),
 * L8 <- uint8(clip(255 * L8 / p, 0, 255)), LAB2RGB.  p_out: n doubles (may be NULL). */
SL_API int sl_luminosity_standardize(const uint8_t* rgb, uint8_t* out, int n, int h, int w, double percentile, double* p_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- pooled slide-level mode (BASELINE.json configs[4]; an extension: the reference has no notion of a slide).
 * Every tile of a slide gets the statistics the reference would compute from the vertical concatenation of all
 * the tiles.  Each call reduces THIS process's tiles; the host sums / all-reduces the small results over ranks
 * (stainlib_amd/distributed.py: PooledSlideStatistics).
 *
 * sl_tile_moments: per tile {n, sum od[3], sum od od^T [xx,xy,xz,yy,yz,zz]} over the tissue pixels, binary64,
 * run-to-run identical.  workspace: sl_workspace_bytes(SL_OP_TILE_MOMENTS, n, h, w). */
SL_API int sl_tile_moments(const uint8_t* rgb, int n, int h, int w, const SlParams* params,
                    double* moments_out /* n x 10 */, void* workspace, size_t workspace_bytes, void* stream);

/* Keys are compared as order-preserving uint32 images of their binary32 value: ord(f) = bits(f) ^ 0x80000000 for
 * f >= 0, ~bits(f) for f < 0.  `basis` is a HOST pointer to 6 doubles: V (3x2, V[c*2+k]) for SL_KEYSET_ANGLE, the
 * stain matrix M (2x3) for SL_KEYSET_CONC.  Both targets of the key set are served by the same sweep: hist
 * (device, 2 x 256 uint64) is ACCUMULATED into, target t counting bin = the 8 key bits below the top `prefix_bits`
 * bits over the keys whose top `prefix_bits` (0, 8, 16 or 24) bits equal prefixes[t] (HOST pointer, 2 values). */
SL_API int sl_slide_key_histogram(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset,
                           const double* basis, const uint32_t* prefixes, int prefix_bits,
                           unsigned long long* hist, void* stream);
/* The last two rounds in one sweep: hist16 (device, 2 x 65536 uint64, ACCUMULATED into) counts the LOW 16 key bits
 * over the keys whose top 16 bits equal prefixes16[t] (HOST pointer, 2 values). */
SL_API int sl_slide_key_histogram16(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset,
                             const double* basis, const uint32_t* prefixes16, unsigned long long* hist16, void* stream);
/* sl_slide_key_histogram over a stratified pixel sample: one 64-chunk row in 2^sample_log2 (0 <= sample_log2 <= 12). */
SL_API int sl_slide_key_histogram_sampled(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset,
                                   const double* basis, const uint32_t* prefixes, int prefix_bits, int sample_log2,
                                   unsigned long long* hist, void* stream);
/* One sweep for an order statistic whose neighbourhood is known: hist_below (device, 2 x 65536 + 2 uint64, ACCUMULATED
 * into) = per target the histogram of key - window_lo[t] over the keys in [window_lo[t], window_lo[t] + 65536), followed
 * by the two counts of keys below window_lo[t] (HOST pointer, 2 ordered-uint32 values). */
SL_API int sl_slide_key_window(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset,
                        const double* basis, const uint32_t* window_lo, unsigned long long* hist_below, void* stream);
/* min_out[t] (device uint32 x 2, set to 0xffffffff by the caller) = min(min_out[t], smallest key of target t
 * above key_ords[t]) (key_ords: HOST pointer, 2 values). */
SL_API int sl_slide_key_next_above(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset,
                            const double* basis, const uint32_t* key_ords, uint32_t* min_out, void* stream);

/* ---- the same pooled statistics, DEVICE-DRIVEN: no host read-back between the steps ----------------------------
 * `state` is SL_POOL_STATE_DOUBLES doubles of device memory owned by the caller.  One computation is the chain
 *     [sum of sl_tile_moments over the local tiles, pixel count appended: 11 doubles]  -> all-reduce ->  sl_pool_begin
 *     for keyset in (SL_KEYSET_ANGLE, SL_KEYSET_CONC):
 *         for round in 0, 1, 2:  sl_pool_histogram (sampled, 2 x 256)  -> all-reduce ->  sl_pool_pick
 *         sl_pool_window (2 x 65536 + 2)  -> all-reduce ->  sl_pool_resolve
 * enqueued on one stream; every decision (eigenvectors, which bin holds the rank, where the window sits, whether it caught the
 * ranks, the stain matrix, maxC) is taken on the device from all-reduced data, so every rank reaches the same state.  Afterwards
 * state[SL_POOL_M .. +5] is the slide's stain matrix, state[SL_POOL_MAXC .. +1] its 99th-percentile concentrations,
 * state[SL_POOL_STATUS] a SL_TILE_* code and state[SL_POOL_MISS] != 0 says a window missed its rank (an estimate off by more than
 * 32768 consecutive binary32 values, or an empty sample): the caller then takes the host-driven radix rounds above.  ONE read-back,
 * at the end.  The sweeps are the kernels of sl_slide_key_histogram_sampled / sl_slide_key_window reading their basis, prefixes
 * and windows from `state`. */
#define SL_POOL_STATE_DOUBLES 64
#define SL_POOL_M 0
#define SL_POOL_MAXC 6
#define SL_POOL_STATUS 8
#define SL_POOL_MISS 9
SL_API int sl_pool_begin(const double* moments11, const SlParams* params, double* state, void* stream);
SL_API int sl_pool_histogram(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset, const double* state,
                      int round, int sample_log2, unsigned long long* hist, void* stream);
SL_API int sl_pool_pick(double* state, int keyset, int round, const unsigned long long* hist_reduced, void* stream);
SL_API int sl_pool_window(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int keyset, const double* state,
                   unsigned long long* hist_below, void* stream);
SL_API int sl_pool_resolve(double* state, int keyset, const unsigned long long* window_reduced, const SlParams* params, void* stream);

/* ---- the pooled statistics in ONE full sweep (round 6; stainlib_amd/csrc/slide_merged.hip) ---------------------------------------
 * The moments sweep also collects the raw candidates of all four order statistics, against an estimate of the eigenvectors, the angular
 * brackets and the stain matrix taken from a stratified pixel sample of the whole slide (one 64-pixel sub-row in 2^sample_log2; the same
 * sample_log2 on every rank); once the exact moments are all-reduced the estimate is CHECKED, and the exact order statistics of the
 * binary32 keys are those of the candidates at shifted ranks.  Results never depend on the sample: when a check fails
 * (state[SL_POOL_MISS] != 0 at the end) the caller takes the three-sweep chain above.  One computation is the chain
 *     sl_pool2_sample                          -> all-reduce moments16 (16 doubles, SUM)  -> sl_pool2_begin
 *     sl_pool2_hist(0, ANGLE, 0)               -> all-reduce hist (SL_POOL2_HIST_WORDS uint64)  -> sl_pool2_bands(ANGLE)
 *     sl_pool2_hist(0, CONC, 0)                -> all-reduce                              -> sl_pool2_bands(CONC)
 *     sl_pool2_sweep  (THE full sweep)         -> all-reduce totals16 (16 doubles)        -> sl_pool2_exact
 *     for keyset in (ANGLE, CONC):  SL_POOL2_LEVELS times:  sl_pool2_hist(1, keyset, 1) -> all-reduce -> sl_pool2_step
 *         (a radix descent in the ordered binary32 domain, one target per wanted RANK -- k and k + 1 of each of the two order statistics share
 *          a window until they fall into different bins: SL_POOL2_WINDOW_BINS coarse bins, 11 key bits, per level, the last level
 *          SL_POOL2_KEY_BINS single keys; two levels settle a bracket of up to 2^23 values, three every bracket; sparse and heavily tied keys
 *          are settled like dense ones; a settled key set turns the remaining passes and steps into no-ops)
 * on one stream; state[SL_POOL_M / _MAXC / _STATUS / _MISS] as for sl_pool_*;
 * state[SL_POOL2_WHY] != 0 says the sample gave no usable estimate (the sweep then returns at once and the chain ends in a miss).
 * `workspace` (sl_pool2_workspace_bytes, 256-byte aligned) carries the sample list, the candidate list (up to 1/8 of the pixels) and
 * the per-workgroup partial sums from sl_pool2_sample to the last sl_pool2_hist.  Every step consumes all-reduced data only: the ranks
 * reach the same state without a broadcast.  Reference: macenko_stain_extractor.py:18-44, normalizer.py:36,45-47 on the concatenation.
 * Limits: h w <= 2^30 and n h w <= 2^40 pixels, AND both lists must count their blocks in 32 bits -- the sample list holds about
 * n h w / (256 * 2^sample_log2) blocks, so the densest samples are not accepted for the largest shards (2^40 pixels need
 * sample_log2 >= 1 or so; the Python layer's own choice for that size is 9).  Where they do not fit, sl_pool2_workspace_bytes returns 0 and every
 * sl_pool2_* entry point that takes the shape returns SL_ERR_BADARG before anything is launched. */
#define SL_POOL2_STATE_DOUBLES 256
#define SL_POOL2_TAIL_SLOTS 32
#define SL_POOL2_GRID_BINS 8192
#define SL_POOL2_WINDOW_BINS 2048 /* coarse bins per target of a window pass (mode 1) */
#define SL_POOL2_KEY_BINS 4096    /* single keys per target at the last level of a window pass: 4 targets x SL_POOL2_KEY_BINS = 2 x SL_POOL2_GRID_BINS */
/* a histogram buffer: 8 x SL_POOL2_TAIL_SLOTS tail words, then 2 x SL_POOL2_GRID_BINS bins (mode 0: two grids; mode 1: four targets of
 * SL_POOL2_KEY_BINS); every pass WRITES it whole */
#define SL_POOL2_HIST_WORDS (8 * SL_POOL2_TAIL_SLOTS + 2 * SL_POOL2_GRID_BINS)
#define SL_POOL2_WHY 33
SL_API size_t sl_pool2_workspace_bytes(int n, int h, int w, int sample_log2);
SL_API int sl_pool2_sample(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int sample_log2, void* workspace,
                    size_t workspace_bytes, double* moments16_out, void* stream);
SL_API int sl_pool2_begin(const double* moments16_reduced, const SlParams* params, int sample_log2, double* state, void* stream);
/* which: 0 the sample list (mode 0: a uniform grid of SL_POOL2_GRID_BINS bins per order statistic), 1 the candidate list (mode 1: per target a
 * window of bins of 2^sh consecutive binary32 values, position and sh from `state`); hist (SL_POOL2_HIST_WORDS uint64) is written whole */
SL_API int sl_pool2_hist(int which, int keyset, int mode, int n, int h, int w, const SlParams* params, int sample_log2, const double* state,
                  void* workspace, size_t workspace_bytes, unsigned long long* hist, void* stream);
SL_API int sl_pool2_bands(double* state, int keyset, const unsigned long long* hist_reduced, void* stream);
SL_API int sl_pool2_sweep(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int sample_log2, const double* state,
                   void* workspace, size_t workspace_bytes, double* totals16_out, void* stream);
SL_API int sl_pool2_exact(const double* totals16_reduced, double* state, void* stream);
SL_API int sl_pool2_step(double* state, int keyset, const unsigned long long* hist_reduced, void* stream);
/* the whole chain above on ONE process (no all-reduce between the steps), enqueued by one call; state as above */
#define SL_POOL2_LEVELS 3
SL_API int sl_pool2_local(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int sample_log2, void* workspace,
                   size_t workspace_bytes, double* state, void* stream);

/* ---- the pooled slide-level VAHADANE dictionary (stainlib_amd/csrc/slide_dict.hip) ----------------------------------------------------
 * The stain matrix vahadane_stain_extractor.py:28-43 computes from the vertical concatenation of every tile of every rank (tissue mask :30,
 * OD :31-32, dictionary learning :35-36 -- run to the fixed point full-batch block-coordinate descent reaches from the Ruifrok start, as
 * for the per-tile sl_vahadane_fit --, H first :40-41, unit rows :43).  Under ONE shared dictionary a sweep reduces the slide to 31 sums
 * (3 classes x {count, sum x, sum x x^T} + the tissue count); the update runs on those alone, so a round is
 *     sl_sdict_sweep -> all-reduce sums (SL_SDICT_SUMS doubles, SUM) -> sl_sdict_step
 * repeated until state[SL_SDICT_MODE] reads 0 (settled).  One computation is sl_sdict_begin, then rounds; every rank issues the same
 * rounds (a settled state turns a sweep into zeros and a step into a no-op, so ranks may enqueue a fixed number of rounds between two
 * read-backs).  Rounds of mode 1 sweep a stratified sample of the slide (one 64-pixel sub-row in 2^sample_log2 of every tile, placed by
 * the sub-row's position in its tile alone: the same sample_log2 on every rank), rounds of mode 2 every pixel.  SlParams: dl_lambda,
 * dl_tol, dl_max_sweeps (full sweeps), luminosity_threshold.  n == 0 is legal (a rank with an empty shard writes zero sums and its
 * pixel count 0).  The 99th-percentile concentrations (normalizer.py:36,47) are then those of the key set SL_KEYSET_CONC under
 * basis = state[SL_SDICT_M .. +5] (sl_slide_key_*). */
#define SL_SDICT_STATE_DOUBLES 64
#define SL_SDICT_SUMS 32          /* sums of a sweep: [0, 30) class moments, [30] tissue pixels, [31] pixels (the slide's pixel count once reduced) */
#define SL_SDICT_M 0              /* the slide's stain matrix (2 x 3, H first, unit rows) once settled with status 0; NaN otherwise */
#define SL_SDICT_STATUS 6         /* SL_TILE_OK, SL_TILE_EMPTY_MASK (no tissue pixel), SL_TILE_DEGENERATE_COV (a dead atom or parallel atoms) */
#define SL_SDICT_SWEEPS 7         /* full sweeps used */
#define SL_SDICT_ROUNDS 8         /* updates taken (sampled and full) */
#define SL_SDICT_MODE 9           /* what the next round sweeps: 1 the sample, 2 every pixel, 0 nothing (settled) */
#define SL_SDICT_D 10             /* the current dictionary (2 x 3, rows = atoms) */
#define SL_SDICT_NPX 16           /* the slide's pixel count (from the first reduced sums) */
/* workspace bytes of sl_sdict_sweep (per-workgroup partial rows); 0 for bad arguments */
SL_API size_t sl_sdict_workspace_bytes(int n, int h, int w);
/* the Ruifrok start, mode 1 (vahadane_stain_extractor.py:35: the dictionary learning starts) */
SL_API int sl_sdict_begin(const SlParams* params, int sample_log2, double* state, void* stream);
/* this rank's sums (SL_SDICT_SUMS doubles, written whole, fixed order: run-to-run identical) of the round state[SL_SDICT_MODE] names, under
 * the dictionary state[SL_SDICT_D] (vahadane_stain_extractor.py:35-36, one pass of the codes over the rank's tissue pixels) */
SL_API int sl_sdict_sweep(const uint8_t* rgb, int n, int h, int w, const SlParams* params, int sample_log2, const double* state,
                          void* workspace, size_t workspace_bytes, double* sums_out, void* stream);
/* the dictionary update from the ALL-REDUCED sums, the stopping rule, and at the end the stain matrix (vahadane_stain_extractor.py:36-43) */
SL_API int sl_sdict_step(double* state, const double* sums_reduced, const SlParams* params, void* stream);

/* ---- the pooled slide-level REINHARD / LUMINOSITY statistics (stainlib_amd/csrc/slide_lab.hip) ----------------------------------------
 * ReinhardStainNormalizer.transform (normalization/normalizer.py:70-94) and LuminosityStandardizer.standardize with the LAB helpers
 * (utils/stain_utils.py:52-67,146-194) on the concatenation: every tile of every rank is mapped with the statistics the reference computes
 * from the vertical concatenation of all of them.  Everything those statistics need is a sum of integers -- the histogram of all bytes
 * (p90, np.percentile linear), the histogram of L8 with sum a8, sum a8^2, sum b8, sum b8^2 (cv2.meanStdDev of the lab_split planes; the L
 * percentile) -- so the pooled result is the reference's on the concatenation byte for byte: no sample, no bracket, no fallback route and
 * no tolerance.  One computation is the chain
 *     sl_slab_bytes                 -> all-reduce sums_a (SL_SLAB_SUMS_A uint64, SUM)  -> sl_slab_begin
 *     sl_slab_lab                   -> all-reduce sums_b (SL_SLAB_SUMS_B uint64, SUM)  -> sl_slab_finish
 *     sl_slab_map
 * enqueued on one stream; every decision is taken on the device from all-reduced sums, so every rank reaches the same state without a
 * broadcast.  LuminosityStandardizer (mode 1) does not standardise the brightness: no bytes sweep, sl_slab_begin(standardize = 0).
 * n == 0 is legal in the two sum calls (a rank with an empty shard writes zeros).  A zero standard deviation follows numpy's inf / NaN
 * arithmetic as the per-tile kernel does; it is not a status.
 * Like the per-tile Lab family, OpenCV's 8-bit Lab conversions are RESTATED here (from the published RGB2Lab_b / Lab2RGBinteger), not
 * pinned against a real cv2: PARITY UNPINNED against OpenCV itself; the reference's own arithmetic around them is what the tests pin.
 * `state`: SL_SLAB_STATE_DOUBLES doubles of device memory owned by the caller. */
#define SL_SLAB_STATE_DOUBLES 512
#define SL_SLAB_SUMS_A 256        /* counts of the byte values 0 .. 255 over all three channels */
#define SL_SLAB_SUMS_B 262        /* [0, 256) counts of L8 of the (standardised) pixels, [256] sum a8, [257] sum a8^2, [258] sum b8, [259] sum b8^2,
                                     [260] tissue pixels at the threshold of sl_slab_lab, [261] pixels */
#define SL_SLAB_P90 0             /* 90th percentile of all bytes of the slide (NaN when the chain does not standardise) */
#define SL_SLAB_MEANS 1           /* mean L, a, b of the (standardised) slide as get_mean_std gives them */
#define SL_SLAB_STDS 4            /* population standard deviations L, a, b */
#define SL_SLAB_LPCT 7            /* mode 1: the percentile of L8 (NaN in mode 0) */
#define SL_SLAB_TISSUE 8          /* the slide's tissue-pixel count at the threshold of sl_slab_lab */
#define SL_SLAB_NPX 9             /* the slide's pixel count */
#define SL_SLAB_STATUS 10         /* SL_TILE_OK; SL_TILE_EMPTY_MASK: the slide has no pixel, or (mode 0 with mask_background) no tissue pixel,
                                     where the reference raises TissueMaskException (stain_utils.py:46-47) */
#define SL_SLAB_TABLES 32         /* from here: the composed byte tables of the sweeps (private layout) */
/* workspace bytes of sl_slab_bytes / sl_slab_lab (per-workgroup partial rows); 0 for bad arguments */
SL_API size_t sl_slab_workspace_bytes(int n, int h, int w);
/* this rank's byte counts (stain_utils.py:193: np.percentile(I, 90) needs the counts of the whole slide) */
SL_API int sl_slab_bytes(const uint8_t* rgb, int n, int h, int w, void* workspace, size_t workspace_bytes,
                         unsigned long long* sums_a_out, void* stream);
/* p90 (np.percentile, linear) from the ALL-REDUCED counts, the brightness table uint8(clip(v * 255.0 / p90, 0, 255)) (stain_utils.py:194)
 * and the gamma values behind it; standardize == 0: identity brightness, sums_a_reduced may be NULL.  Writes the whole state header. */
SL_API int sl_slab_begin(double* state, const unsigned long long* sums_a_reduced, int standardize, void* stream);
/* this rank's Lab sums of the (standardised) tiles (stain_utils.py:146-158,174-186; the luminosity test of stain_utils.py:42-43) */
SL_API int sl_slab_lab(const uint8_t* rgb, int n, int h, int w, const double* state, double luminosity_threshold, void* workspace,
                       size_t workspace_bytes, unsigned long long* sums_b_out, void* stream);
/* from the ALL-REDUCED sums.  mode 0 (Reinhard): means / stds, the three byte tables of normalizer.py:81-83 -- the lookup index is the
 * binary32 v / 2.55f (resp. v - 128.0f) promoted to binary64, ((x - mean) * (tstd / std)) + tmean in binary64 -- composed with merge_back
 * (* 2.55 resp. + 128.0, clip, truncate) and the Lab -> RGB tables; target_means / target_stds: 3 doubles each (DEVICE).  mode 1
 * (luminosity): the `percentile` of L8 and the table uint8(clip(255 * L8 / p, 0, 255)) (stain_utils.py:64-65).  Sets the status. */
SL_API int sl_slab_finish(double* state, const unsigned long long* sums_b_reduced, int mode, const double* target_means,
                          const double* target_stds, double percentile, int mask_background, void* stream);
/* the map of this rank's tiles under the slide's tables; mode 0 with mask_background: pixels failing the luminosity test become L 254,
 * a = b = 0 before merge_back (normalizer.py:86-90).  With a status other than SL_TILE_OK the tiles are copied through unchanged. */
SL_API int sl_slab_map(const uint8_t* rgb, uint8_t* out, int n, int h, int w, const double* state, int mode, int mask_background,
                       double luminosity_threshold, void* stream);

/* ---- model-ready tensor output (stainlib_amd/csrc/tensor_out.hip; an extension: the reference ends at normalizer.py:50 with a uint8
 * image, and every consumer then writes ((out.permute(0, 3, 1, 2).float() / 255) - mean) / std in its framework) -------------------------
 * One definition everywhere, so that the fused pass and "convert afterwards" agree to the bit.  For channel c and a result byte b --
 * the TRUNCATED uint8 the library produces today, never the value before the cast --
 *     scale32[c] = (float)(1.0 / (255.0 * std[c]))        binary64 on the host, rounded to binary32 once
 *     shift32[c] = (float)(-mean[c] / std[c])
 *     v          = fmaf((float)b, scale32[c], shift32[c])   ONE fused multiply-add: one binary32 rounding
 *     out        = v converted to the output type, round-to-nearest-even
 * Layouts of `out` (n x 3 x h x w elements): SL_LAYOUT_NCHW -- plane c of tile i starts at element (3 i + c) h w; SL_LAYOUT_NHWC --
 * interleaved like the input (torch's channels_last).  `out` needs the alignment of its element type only; stores are 16 bytes wide
 * where `out` is 16-byte aligned and h w is a multiple of 4 (float32) or 8 (the half types) pixels, element-wise otherwise.
 * SlTensorFormat is a HOST pointer, like SlParams. */
#define SL_DTYPE_F32 0
#define SL_DTYPE_F16 1
#define SL_DTYPE_BF16 2
#define SL_LAYOUT_NCHW 0
#define SL_LAYOUT_NHWC 1
typedef struct SlTensorFormat {
    uint32_t struct_size;        /* sizeof(SlTensorFormat) of the caller's header: set by sl_default_tensor_format, checked by both entry
                                    points (SL_ERR_BADARG on a mismatch) */
    int32_t dtype;               /* SL_DTYPE_* */
    int32_t layout;              /* SL_LAYOUT_* */
    int32_t reserved;
    double mean[3];              /* per channel, in units of [0, 1]; finite, else SL_ERR_BADARG */
    double std[3];               /* finite and > 0, else SL_ERR_BADARG */
} SlTensorFormat;
/* float32, NCHW, mean 0, std 1 (the plain b / 255) */
SL_API void sl_default_tensor_format(SlTensorFormat* f);
/* Replaces the consumer's permute / cast / scale / shift passes behind any uint8 result: one streaming sweep, 3 B read and 6 or 12 B
 * written per pixel.  rgb: n x h x w x 3 uint8; out: n x 3 x h x w elements of fmt->dtype in fmt->layout. */
SL_API int sl_to_tensor(const uint8_t* rgb, void* out, int n, int h, int w, const SlTensorFormat* fmt, void* stream);
/* sl_normalize_apply (normalization/normalizer.py:46-50) followed by sl_to_tensor in ONE pass: the bytes of the truncating cast are
 * converted in registers and the uint8 image is never written; equal to sl_to_tensor(sl_normalize_apply(...)) bit for bit.  A tile whose
 * fit failed (NaN M_src, maxC_src <= 0) is passed through as in sl_normalize_apply: its SOURCE bytes are converted. */
SL_API int sl_normalize_apply_tensor(const uint8_t* rgb, void* out, int n, int h, int w, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlTensorFormat* fmt, void* stream);

/* ---- stain separation (stainlib_amd/csrc/separate.hip; an extension: what torchstain's normalize(..., stains=True), staintools and
 * HistomicsTK hand out beside the normalised image) ---------------------------------------------------------------------------------
 * sl_normalize_apply's sweep with up to four outputs per pixel from ONE read of the tile and ONE lasso solve.  With c1, c2 the binary32
 * concentrations of a pixel as sl_normalize_apply computes them under the tile's (M_src, maxC_src) -- carried scaled by 2^-k, k per
 * tile -- and q[i][ch] = (float)(-log2(e) * ratio_i * M_tgt[i][ch] * 2^k), ratio_i = maxC_tgt[i] / maxC_src[i]:
 *     norm      n x h x w x 3 uint8: the bytes of sl_normalize_apply, byte for byte
 *     stain[i]  n x h x w x 3 uint8, i = 0 haematoxylin only, 1 eosin only: 255.0f * exp2f(c_i * q[i][ch]) through the cast of norm --
 *               the bytes of sl_normalize_apply called with the OTHER row of M_tgt zeroed, wherever that call takes the same lasso
 *               form (always when M_tgt has no negative entry or the source rows are negatively correlated; for the image of a row
 *               that itself holds the negative entry)
 *     conc      n x 2 x h x w elements of conc_dtype, planar, H plane first: c_i * (float)(ratio_i * 2^k), the normalised
 *               concentration of normalizer.py:48, one binary32 multiply, converted round-to-nearest-even
 * Without a target (M_tgt == NULL and maxC_tgt == NULL) every tile is reconstructed under its OWN stain matrix with ratio 1: norm is
 * the tile's reconstruction, the stain images are its own H and E appearance, conc is the raw get_concentrations.
 * A tile whose fit failed (NaN M_src, maxC_src <= 0): norm = its source bytes, both stain images 255 in every byte, conc +0.
 * `conc` needs the alignment of its element type only; its stores are 16 bytes wide where it is 16-byte aligned and h w is a multiple
 * of 4 (float32) or 8 (the half types) pixels and every uint8 pointer of the call is 4-byte aligned, element-wise otherwise.
 * No workspace.  SlSeparateOut is a HOST struct; the pointers in it are DEVICE pointers. */
typedef struct SlSeparateOut {
    uint32_t struct_size;        /* sizeof(SlSeparateOut) of the caller's header: set by sl_default_separate_out, checked (SL_ERR_BADARG
                                    on a mismatch) */
    int32_t conc_dtype;          /* SL_DTYPE_F32 (default) / _F16 / _BF16; checked even when conc is NULL */
    uint8_t* norm;               /* n x h x w x 3, or NULL */
    uint8_t* stain[2];           /* H-only, E-only image, each n x h x w x 3, or NULL */
    void* conc;                  /* n x 2 x h x w elements of conc_dtype, or NULL */
} SlSeparateOut;
/* all outputs NULL, float32 */
SL_API void sl_default_separate_out(SlSeparateOut* o);
/* SL_ERR_BADARG before anything is launched: a NULL rgb / M_src / maxC_src / outs; exactly one of M_tgt, maxC_tgt NULL; n, h or w <= 0
 * or h w > 2^30; a struct_size mismatch; an unknown conc_dtype; no output requested; two outputs at one address or an output at rgb;
 * conc not aligned to its element size. */
SL_API int sl_stain_separate(const uint8_t* rgb, int n, int h, int w, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlSeparateOut* outs, void* stream);

/* ---- stain jitter in the apply pass (stainlib_amd/csrc/jitter.hip; an extension: a training loader normalises, normalization/normalizer.py:46-50,
 * and then perturbs the stains, augmentation/augmenter.py:428-447 -- which re-fits the NORMALISED image to learn what the apply pass already
 * holds: after normalisation the stain basis of every tile is the target's and its concentrations are C * maxC_tgt / maxC_src) ---------------
 * sl_normalize_apply's sweep with StainAugmentor.pop's affine map on the concentrations, ONE pass: 3 B/px read, the uint8 image or the
 * model-ready tensor written.  Per tile t, with K the constants sl_normalize_apply builds from (M_src[t], maxC_src[t]) and (M_tgt, maxC_tgt),
 * 2^k its per-tile scale, ratio_i = maxC_tgt[i] / maxC_src[t][i], and c1, c2 the binary32 concentrations of a pixel (carried scaled by 2^-k; the
 * lasso form is chosen by the sign of the source rows' correlation alone, as in sl_stain_augment):
 *     al_i = (float)alpha_i,  be_i = (float)(beta_i / ratio_i * 2^-k)
 *     c_i' = fmaf(c_i, al_i, be_i) on tissue pixels (all pixels when augment_background), else c_i
 *            -- alpha and beta act on the NORMALISED concentration c_i ratio_i, in the target's units: the same beta means the same on every tile
 *     value = 255.0f * exp2(fmaf(c1', q[0][ch], c2' * q[1][ch])),  q[i][ch] = (float)(-log2(e) * ratio_i * M_tgt[i][ch] * 2^k)
 *     byte  = the SATURATING truncation, np.clip(., 0, 255).astype(uint8) of augmenter.py:447 -- never modulo 256
 * "Tissue" is the luminosity test of the SOURCE pixel under params->luminosity_threshold (utils/stain_utils.py:32-48), as in sl_stain_augment.
 * Without a target (M_tgt == NULL and maxC_tgt == NULL) every tile is perturbed under its OWN stain matrix with ratio exactly 1: the bytes of
 * sl_stain_augment, byte for byte (StainAugmentor.pop's definition).  With alpha = 1 and beta = 0 the bytes are sl_normalize_apply's wherever
 * its values stay in [0, 255] (M_tgt without a negative entry).
 *   alpha_beta  n x 4 double (device): alpha0, beta0, alpha1, beta1 per tile (the reference's draw order, augmenter.py:435-437)
 *   params      NULL (defaults) or an SlParams: lasso_lambda and luminosity_threshold are read
 *   fmt         NULL: out is the n x h x w x 3 uint8 image.  Otherwise out is the tensor of sl_normalize_apply_tensor in that format, equal to
 *               sl_to_tensor of the uint8 result bit for bit
 * A tile whose fit failed (NaN M_src, maxC_src <= 0) is passed through: its source bytes, converted when a format is given.
 * SL_ERR_BADARG before anything is launched: a NULL rgb / out / M_src / maxC_src / alpha_beta; exactly one of M_tgt, maxC_tgt NULL; n, h or
 * w <= 0 or h w > 2^30; an SlParams of another struct_size; a format sl_to_tensor refuses (struct_size, dtype, layout, a non-finite value,
 * std <= 0).  out == rgb is not supported.  No workspace; capture-safe like the rest (no allocation, no synchronisation, no memset). */
SL_API int sl_normalize_jitter(const uint8_t* rgb, void* out, int n, int h, int w, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);

/* ---- random crop, flip and quarter turn in the apply pass (stainlib_amd/csrc/view.hip; an extension: the geometric half of a training
 * loader's augmentation -- 224^2 out of 256^2, a flip, a turn, different for every tile -- otherwise runs behind the call, on the widest
 * data type, over pixels that were computed and written for nothing) ---------------------------------------------------------------------
 * For tile t let full[t] be the h x w x 3 uint8 image an existing pass writes:
 *     alpha_beta != NULL                   sl_normalize_jitter with the same augment_background, params and target (or no target)
 *     alpha_beta == NULL, M_src != NULL    sl_normalize_apply with lasso_lambda = params->lasso_lambda, its general cast included
 *     M_src == NULL                        none: the source bytes themselves
 * (a tile whose fit failed -- NaN M_src, maxC_src <= 0 --: its source bytes, as in both passes).  The statistics are those of the WHOLE
 * tile; only the apply is restricted to the window: "normalise, then crop".
 * A view is windows[t] = (y0, x0, d), three int32 per tile on the device; the output size (oh, ow) is one for the whole call:
 *     d' = d & d_mask,  k = d' & 3 quarter turns,  f = d' & 4 flip
 *     (wh, ww) = (oh, ow) for even k, (ow, oh) for odd k: the window in the tile
 *     y0' = clamp(y0, 0, h - wh),  x0' = clamp(x0, 0, w - ww), clamped on the device: no window can leave the tile
 *     view[t] = rot90(flip_w_if(f, full[t][y0' : y0' + wh, x0' : x0' + ww]), k)
 * with rot90 = torch.rot90(., k, dims=(0, 1)) (counter-clockwise) and the flip = torch.flip(., dims=(1,)), applied BEFORE the turn.
 *   out   fmt == NULL: n x oh x ow x 3 uint8.  Otherwise the n x 3 x oh x ow tensor sl_to_tensor makes of view, bit for bit, in fmt->dtype
 *         and fmt->layout; `out` needs the alignment of its element type only
 * Only window pixels are read (3 B), computed and written.
 * SL_ERR_BADARG before anything is launched: what sl_normalize_jitter refuses of rgb, out, n, h, w, a one-sided target, params and fmt;
 * NULL windows; oh or ow < 1, oh > h or ow > w; d_mask outside 0..7; d_mask & 1 with ow > h or oh > w (the transposed window must fit
 * too); M_src == NULL with a non-NULL M_tgt, maxC_src or alpha_beta; M_src without maxC_src; M_src without both a target and alpha_beta
 * (sl_normalize_apply needs a target); more than 2^31 - 1 (tile, 64 x 64 patch) pairs.  out == rgb is not supported.  No workspace;
 * capture-safe like the rest (no allocation, no synchronisation, no memset). */
SL_API int sl_normalize_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);

/* ---- HED augmentation behind the apply pass, inside the view pass (stainlib_amd/csrc/hed_view.hip; an extension: a loader that normalises,
 * HED-jitters (HedColorAugmenter, augmentation/augmenter.py:276-331), crops / flips and converts otherwise writes and re-reads two full-tile
 * uint8 images, most of whose pixels the crop throws away) ---------------------------------------------------------------------------------
 * In both calls full[t] is what sl_normalize_view defines by its pointer pattern: the h x w x 3 uint8 image that nothing (M_src == NULL: the
 * source bytes), sl_normalize_apply (M_src and a target, no alpha_beta) or sl_normalize_jitter (alpha_beta, with or without a target,
 * augment_background) writes for the WHOLE tile; a tile whose fit failed (NaN M_src, maxC_src <= 0) is its own bytes.
 *
 * sl_normalize_sums: HedColorAugmenter's cutoff test needs the mean of its whole input before any pixel is transformed; behind
 * normalisation that input is an image nobody wants to write.  One read-only sweep (3 B/px read, n words written):
 *     sums[t]    = the exact integer sum of the 3 h w bytes of full[t]   (uint64, device, 8-byte aligned; cleared by the call itself)
 *     applied[t] = (cutoff_lo <= m && m <= cutoff_hi), m = (double)sums[t] / (3.0 * h w) / 255.0   (int32, device; may be NULL)
 * -- sl_hed_augment's own test on its own sums, so applied equals what sl_hed_augment(full, ..) reports.  Integer atomics: the result does not
 * depend on the order of the workgroups.  No workspace; capture-safe (no allocation, no synchronisation, no memset).
 * SL_ERR_BADARG before anything is launched: what sl_normalize_view refuses of rgb, n, h, w, the statistics pattern and params; a NULL or
 * misaligned sums; cutoff_lo <= cutoff_hi false (a NaN too; infinities are fine: -inf, +inf never fails). */
SL_API int sl_normalize_sums(const uint8_t* rgb, int n, int h, int w, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, double cutoff_lo, double cutoff_hi, uint64_t* sums, int32_t* applied, void* stream);

/* sl_normalize_hed_view: sl_normalize_view's parameters and its result -- the window, flip and quarter turn per tile, as the uint8 image or
 * the tensor -- taken of
 *     hed_applied[t] ? HED(full[t]) : full[t]
 * where HED(.) is sl_hed_augment with hed_sigma[t], hed_bias[t] (n x 3 double each, device: H, E, D), skimage_mode and a cutoff that never
 * fails: the bytes of that chain, bit for bit, without a pixel outside the window being read, computed or written.  The decision
 * hed_applied (n int32, device) is an INPUT: sl_normalize_sums gives it, and a caller may overrule it between the two calls (the Python
 * layer does, for a tile whose mean lies on a cutoff bound).
 * skimage_mode: SL_HED_SKIMAGE_018 only.  The other three SL_HED_* modes are refused with SL_ERR_BADARG; use the chain for them.
 * SL_ERR_BADARG before anything is launched: what sl_normalize_view refuses; a NULL hed_sigma, hed_bias or hed_applied; a skimage_mode
 * outside the SL_HED_* range or other than SL_HED_SKIMAGE_018.  out == rgb is not supported.  No workspace; capture-safe like the rest. */
SL_API int sl_normalize_hed_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode, void* stream);

/* ---- the Lab family in the one-pass loader (stainlib_amd/csrc/lab_view.hip; an extension: behind sl_reinhard_transform,
 * sl_luminosity_standardize or sl_slab_map a training loader otherwise converts, crops, flips and turns a full-tile uint8 image, most of
 * whose pixels went through the library's most expensive per-pixel arithmetic to be thrown away) ---------------------------------------
 * sl_normalize_view's definition -- windows[t] = (y0, x0, d), d_mask, the clamp, the flip BEFORE the turn, (oh, ow), `out` as the
 * n x oh x ow x 3 uint8 image (fmt == NULL) or the n x 3 x oh x ow tensor sl_to_tensor makes of it, bit for bit -- with full[t] the
 * h x w x 3 uint8 image the existing call with the same arguments writes:
 *     sl_reinhard_view      sl_reinhard_transform  (target_means, target_stds, mask_background, luminosity_threshold; stats_out as there)
 *     sl_luminosity_view    sl_luminosity_standardize  (percentile; p_out as there)
 *     sl_slab_view          sl_slab_map  (state, mode, mask_background, luminosity_threshold; with a status other than SL_TILE_OK the
 *                           view of the SOURCE bytes, as sl_slab_map copies the tiles through)
 * The statistics are those of the WHOLE tile (the whole slide): the per-tile calls run the unchanged statistics sweeps and table kernels
 * of the existing calls in the same workspace (SL_OP_LAB_STATS), then ONE sweep that reads, maps and writes window pixels only.
 * sl_slab_view: n == 0 is legal (SL_OK, nothing is launched; rgb, out and windows may then be NULL).
 * SL_ERR_BADARG / SL_ERR_WORKSPACE before anything is enqueued: what the existing call refuses of rgb, out, n, h, w, the workspace, the
 * state and the mode; NULL target_means / target_stds; what sl_normalize_view refuses of windows, oh, ow, d_mask, fmt and the number of
 * (tile, patch) pairs; out == rgb.  Capture-safe like the rest (no allocation, no synchronisation, no memset). */
SL_API int sl_reinhard_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, const double* target_means, const double* target_stds, int mask_background, double luminosity_threshold, double* stats_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_luminosity_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, double percentile, double* p_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_slab_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, const double* state, int mode, int mask_background, double luminosity_threshold, const SlTensorFormat* fmt, void* stream);

/* ---- magnification change in the one-pass loader: a 2x / 4x box shrink inside the view (view.hip, hed_view.hip, lab_view.hip; an extension:
 * slides are tiled at 40x and most networks train at 20x or 10x, so a loader otherwise runs avg_pool2d(2) or (4) behind the call, on the
 * widest data type, over a full-resolution tensor of which three quarters or fifteen sixteenths are averaged away) ------------------------
 * Each call is its parent -- sl_normalize_view, sl_normalize_hed_view, sl_reinhard_view, sl_luminosity_view, sl_slab_view -- with
 * `int shrink` = s in {1, 2, 4} after d_mask; the parent is the call with s = 1, by forwarding.  (oh, ow) stays the size of the OUTPUT:
 *     (wh, ww) = (oh, ow) for an even number of quarter turns, (ow, oh) for an odd one: the window in BOXES of s x s source pixels
 *     y0' = clamp(y0, 0, h - s wh),  x0' = clamp(x0, 0, w - s ww), clamped on the device; any pixel, not only a multiple of s
 * With full[t] the h x w x 3 uint8 image the parent defines -- at SOURCE resolution: normalised, jittered, HED-transformed, Lab-mapped per
 * source pixel, the statistics (fits, cutoff sums, Lab and pooled statistics) those of the whole tile at source resolution -- per channel
 *     S[i, j] = sum of full[t][y0' + s i + a, x0' + s j + b] over a, b in 0 .. s-1          (an integer, at most 16 x 255 = 4080)
 *     b[i, j] = (S[i, j] + s s / 2) >> (2 log2 s)                                           (the mean, round half up; a uint8)
 *     view[t] = rot90(flip_w_if(f, b), k)                                                   (the parent's dihedral rule)
 * The boxes start at the window's corner and the window is a whole number of them, so shrinking commutes with the flip and the turn.  The
 * tensor is defined on b as it is on a byte everywhere else: fma(float32(b), 1 / (255 std), -mean / std), rounded to fmt->dtype.  A tile
 * whose fit failed, and every tile of a pooled slide whose status is not SL_TILE_OK: the shrunk view of its own bytes.  Averaging happens
 * AFTER normalisation, in byte space; "shrink first, normalise a quarter of the pixels" is another image and not offered.  Neither are
 * other factors, arbitrary or per-tile ratios, bilinear or antialiased filters.
 * Every source pixel of the window is read and computed (s s times the output's); only the output is written.
 * SL_ERR_BADARG (SL_ERR_WORKSPACE) before anything is launched: what the parent refuses, with s oh, s ow in place of oh, ow in its tests
 * against h and w (s oh > h, s ow > w; d_mask & 1 with s ow > h or s oh > w); shrink other than 1, 2, 4; more than 2^31 - 1 (tile, patch)
 * pairs, a patch being 64 / s output pixels square.  out == rgb is not supported.  Capture-safe like the parents. */
SL_API int sl_normalize_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);
SL_API int sl_normalize_hed_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode, void* stream);
SL_API int sl_reinhard_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, const double* target_means, const double* target_stds, int mask_background, double luminosity_threshold, double* stats_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_luminosity_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, double percentile, double* p_out, void* workspace, size_t workspace_bytes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_slab_view_shrink(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, const double* state, int mode, int mask_background, double luminosity_threshold, const SlTensorFormat* fmt, void* stream);

/* ---- random-resized crop in the one-pass loader: a per-tile window of any size, area-resampled to the output inside the view (view.hip,
 * hed_view.hip, view_resize_kernels.hpp; an extension: RandomResizedCrop(224, scale=(0.08, 1)) is the one augmentation every training
 * recipe otherwise runs behind the call -- on the full-tile tensor, in a per-tile loop, because the windows differ in size) -----------
 * Each call is its parent -- sl_normalize_view, sl_normalize_hed_view -- with `int max_wh, int max_ww` after d_mask and windows of
 * n x 5 int32 on the device: windows[t] = (y0, x0, d, wh, ww), a window of wh rows and ww columns in the TILE's orientation at (y0, x0).
 * (oh, ow) stays the size of the OUTPUT, one for the call.  On the device, per tile:
 *     d' = d & d_mask;  (nu, nv) = (oh, ow) for an even number of quarter turns, (ow, oh) for an odd one
 *     wh' = clamp(wh, 1, min(max_wh, 16 nu)),  ww' = clamp(ww, 1, min(max_ww, 16 nv))
 *     y0' = clamp(y0, 0, h - wh'),  x0' = clamp(x0, 0, w - ww')
 * With full[t] the h x w x 3 uint8 image the parent defines (at SOURCE resolution; every statistic the whole tile's) and
 * win = full[t][y0' : y0' + wh', x0' : x0' + ww'], the window is resampled to nu x nv by exact pixel-area averaging (OpenCV's INTER_AREA
 * for shrinking, in integers).  Along an axis of nw window pixels and no outputs, in coordinates scaled by no, source pixel k covers
 * [k no, (k + 1) no), output i covers [i nw, (i + 1) nw) and c(i, k) is the length of their overlap: an integer, every row of c sums to
 * nw, every column to no.  Per channel
 *     S[i, j] = sum_k sum_l cy(i, k) cx(j, l) win[k, l]                                    (an integer, at most 255 wh' ww')
 *     b[i, j] = (2 S[i, j] + D) / (2 D),  D = wh' ww', integer division                     (the mean, round half up; a uint8)
 *     view[t] = rot90(flip_w_if(f, b), k)                                                   (the parent's dihedral rule)
 * wh' = nu and ww' = nv: the window itself (the parent's result).  wh' = s nu and ww' = s nv: the s x s box mean of the _shrink calls.
 * The resample commutes with the flip and the turn.  wh' < nu (upscaling) is the same formula: piecewise constant with blended edges where
 * an output straddles two source pixels -- not bilinear.  The tensor is defined on b as on a byte everywhere else.  A tile whose fit
 * failed: the resampled view of its own bytes.  Bilinear, bicubic or antialiased-triangle filters are other definitions and not offered.
 * (max_wh, max_ww): an upper bound of the window sides of this call; the launch is sized from it (the windows are never read back), and
 * a window beyond it is clamped to it.  Limits: wh ww <= 2^22 (2 S + D < 2^31), wh <= 16 nu and ww <= 16 nv (at most 17 source pixels
 * per output and axis).
 * SL_ERR_BADARG before anything is launched: what the parent refuses of rgb, out, n, h, w, d_mask, the statistics pattern, params, fmt
 * (and the HED arguments); a NULL windows; oh < 1 or ow < 1; max_wh outside [1, h] or max_ww outside [1, w]; max_wh max_ww > 2^22;
 * max(oh, ow) max(max_wh, max_ww) > 2^30; more (tile, patch) pairs than 2^31 - 1.  Unlike the parents, (oh, ow) need not fit in the
 * tile.  out == rgb is not supported.  Capture-safe like the parents. */
SL_API int sl_normalize_view_resize(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);
SL_API int sl_normalize_hed_view_resize(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const double* hed_sigma, const double* hed_bias, const int32_t* hed_applied, int skimage_mode, void* stream);

/* ---- stain separation in the view pass (stainlib_amd/csrc/separate_view.hip; an extension: segmentation and nuclei-detection training
 * consumes the haematoxylin image, the eosin image and the concentration planes -- cropped, flipped, turned and often at half the
 * magnification; behind sl_stain_separate a loader re-reads up to 9 B/px of images and 8 B/px of planes of the FULL tile to do so) -----
 * "The same bits, elsewhere".  Let full = what sl_stain_separate writes for the same rgb, statistics, target (or none), lasso_lambda and
 * outs->conc_dtype: full.norm, full.stain[0], full.stain[1] (h x w x 3 uint8 per tile) and full.conc (2 x h x w per tile).  With
 * sl_normalize_view_shrink's view -- windows[t] = (y0, x0, d), d_mask, (oh, ow) the size of the OUTPUT, shrink = s, the clamp on the
 * device, the flip BEFORE the turn --:
 *     an image X, s = 1    rot90(flip_w_if(f, full.X[t][y0' : y0' + wh, x0' : x0' + ww]), k)
 *     an image X, s = 2, 4 the box shrink of sl_normalize_view_shrink on those bytes: (S + s s / 2) >> (2 log2 s) of every s x s box,
 *                          boxes counted from the window's corner, then the flip and the turn
 *     conc, s = 1 only     the same slice, flip and turn of each of the two h x w planes of full.conc[t]: a permutation of elements of
 *                          conc_dtype, bit for bit.  (A mean of floats is another definition and not offered.)
 * A tile whose fit failed (NaN M_src, maxC_src <= 0): norm = the view of its source bytes, both stain images 255 in every byte,
 * conc +0 -- sl_stain_separate's rule under the view.  Without a target (M_tgt == NULL and maxC_tgt == NULL): as there.
 *   outs  SlSeparateOut as for sl_stain_separate (same struct, same size), NULL = not wanted.  fmt == NULL: each image is
 *         n x oh x ow x 3 uint8.  Otherwise its three image pointers are read as pointers to elements of fmt->dtype, and each image is
 *         the n x 3 x oh x ow tensor sl_to_tensor makes of the uint8 view, bit for bit, in fmt->layout.  conc: n x 2 x oh x ow
 *         elements of conc_dtype, planar, H plane first; fmt does not apply to it.
 * Only window pixels are read (3 B), solved (ONE lasso solve per source pixel) and written.
 * SL_ERR_BADARG before anything is launched: what sl_stain_separate refuses (a NULL rgb / M_src / maxC_src / outs; a one-sided target;
 * n, h or w <= 0 or h w > 2^30; a negative or NaN lasso_lambda; a struct_size mismatch; an unknown conc_dtype; no output requested; two
 * outputs at one address or an output at rgb; conc not aligned to its element size); what sl_normalize_view_shrink refuses of windows,
 * oh, ow, d_mask, shrink and the number of (tile, patch) pairs; shrink != 1 with a non-NULL conc; a format sl_to_tensor refuses; an
 * image pointer not aligned to its element size.  No workspace; capture-safe like the rest (no allocation, no synchronisation, no
 * memset). */
SL_API int sl_stain_separate_view(const uint8_t* rgb, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, double lasso_lambda, const SlSeparateOut* outs, const SlTensorFormat* fmt, void* stream);

/* ---- companion planes through the windows of a view (stainlib_amd/csrc/planes_view.hip; an extension: segmentation and nuclei-detection
 * training carries per-pixel companions of every tile -- class map, instance map, loss mask, tissue mask, distance map -- which have to
 * go through the window, the flip, the turn and the change of magnification of their image) -------------------------------------------
 * planes: n x c x h x w elements of elem_bytes bytes (1, 2, 4 or 8; any type, only bits are moved), contiguous; out: n x c x oh x ow of
 * the same.  windows: the ones the image call took -- max_wh == max_ww == 0: n x 3 int32 (y0, x0, d) of sl_normalize_view_shrink under
 * shrink = s in {1, 2, 4}; both above 0: n x 5 int32 (y0, x0, d, wh, ww) of sl_normalize_view_resize under that bound (shrink = 1).  d is
 * masked with d_mask and the window is clamped on the device by those calls' own rules, so a companion sees the window its image saw.
 * Per tile t and plane ch, with k = d & 3, f = d & 4, (nu, nv) = (ow, oh) for odd k, else (oh, ow), and the source window
 * win = planes[t, ch][y0' : y0' + s nu, x0' : x0' + s nv] (a resizing view: [y0' : y0' + wh', x0' : x0' + ww']):
 *     SL_PLANES_NEAREST   R[i, j] = win[ky(i), kx(j)], a bit copy; along an axis of nw window pixels and no outputs
 *                         k(i) = ((2 i + 1) nw) / (2 no), the pixel under the output's centre (i itself for the plain view, s i + s / 2
 *                         under a shrink); the product stays below 2^31 under the resizing view's limits
 *     SL_PLANES_AREA      elem_bytes = 1 only: the images' own definition on one channel -- (S + s s / 2) >> (2 log2 s) of every s x s box,
 *                         or the exact area average (2 S + D) / (2 D) of sl_normalize_view_resize
 *     out[t, ch] = rot90(flip_w_if(f, R), k)
 * The order matters: the centre sample does NOT commute with a reversal when nw / no is even (nw = 10, no = 5: 1 3 5 7 9 against
 * 0 2 4 6 8 after the reversal); R is sampled in the TILE's orientation.  Without a shrink or a resize both modes are the same permutation.
 * SL_ERR_BADARG before anything is launched: a NULL planes, out or windows; n, c, h, w, oh or ow <= 0; h w > 2^30; elem_bytes not 1, 2, 4
 * or 8; planes or out not aligned to elem_bytes; an unknown mode; SL_PLANES_AREA with elem_bytes != 1; exactly one of the two bounds
 * zero, or a negative bound; what sl_normalize_view_shrink / sl_normalize_view_resize refuse of h, w, oh, ow, d_mask, shrink and the
 * bounds; more (plane, patch) pairs than 2^31 - 1.  n c h w elem_bytes may pass 2^32: all byte offsets are size_t.  out == planes is
 * not supported.  No workspace; capture-safe like the rest. */
#define SL_PLANES_NEAREST 0
#define SL_PLANES_AREA    1
SL_API int sl_view_planes(const void* planes, void* out, int n, int c, int h, int w, int elem_bytes, int oh, int ow,
                          const int32_t* windows, int d_mask, int shrink, int max_wh, int max_ww, int mode, void* stream);

/* ---- arbitrary rotation, zoom, shear and translation in the one-pass loader: an affine view, bilinear for the images and nearest for
 * their companion planes (stainlib_amd/csrc/view_affine.hip; an extension: segmentation and nuclei-detection recipes rotate every tile by
 * any angle, zoom 0.8 - 1.2, shear and translate, image and label maps alike -- behind the call that is affine_grid / grid_sample on
 * the widest data type, once per image and once per label plane, on pixels the rotation then pushes out of the frame) ----------------
 * The definition is in integers, so "bit for bit" applies.  windows: n x 6 int32 on the device, windows[t] = (cy, cx, a00, a01, a10, a11),
 * all in units of 2^-16 source pixel (Q = 65536); pixel k of an axis covers [k, k + 1).  (cy, cx) is the source position of the CENTRE of
 * the output, a.. the source displacement per output pixel.  (oh, ow) is the size of the OUTPUT, one for the call.  For output pixel
 * (i, j), with u = 2 i + 1 - oh and v = 2 j + 1 - ow:
 *     Y = cy + ((a00 u + a01 v) >> 1)        X = cx + ((a10 u + a11 v) >> 1)                 (arithmetic shift = floor)
 * Images (sl_normalize_view_affine; bilinear, 8-bit weights): ty = Y - Q/2, ky = ty >> 16, fy = (ty >> 8) & 255, the same for x; with
 * p00, p01, p10, p11 the bytes of full[t] at (ky, kx), (ky, kx + 1), (ky + 1, kx), (ky + 1, kx + 1), per channel
 *     b = ((256 - fy) ((256 - fx) p00 + fx p01) + fy ((256 - fx) p10 + fx p11) + 32768) >> 16
 * full[t] is, as for every other view, the h x w x 3 uint8 image the statistics pattern names (sl_normalize_view's rule: the tile's
 * own bytes, sl_normalize_apply's image or sl_normalize_jitter's): normalised / jittered per SOURCE pixel, every statistic the whole
 * tile's, a tile whose fit failed gives its own bytes.  A tap outside [0, h) x [0, w) is the fill byte of its channel, fill_rgb =
 * r | g << 8 | b << 16 in OUTPUT space (it is not normalised).  fmt != NULL: the tensor sl_to_tensor makes of b, as everywhere else.
 * Planes (sl_view_planes_affine; nearest): out[t, ch][i, j] = planes[t, ch][Y >> 16, X >> 16], a bit copy of an elem_bytes element;
 * outside the plane the low elem_bytes bytes of fill_bits.  planes / out: n x c x h x w and n x c x oh x ow, as for sl_view_planes.
 * What follows from the definition: A = Q I with c = (h Q / 2, w Q / 2) and (oh, ow) = (h, w) is the identity; the eight signed
 * permutation matrices (entries 0, +-Q) with the centre on a window's centre are sl_normalize_view's rot90(flip(window)), bit for bit;
 * A = 2 Q I is (S + 2) >> 2 of every 2 x 2 box, the shrink = 2 rule.  A = 4 Q I is NOT the 4 x 4 box: bilinear takes four taps, the
 * middle 2 x 2 of each box -- beyond two source pixels per output it aliases, and downsampling further is shrink / the resizing view.
 * Limits, so that every quantity above is 32-bit: h, w, oh, ow <= 8192; the row sums Ry = |a00| + |a01| and Rx = |a10| + |a11| each
 * <= 2 Q; cy in [-2^28, h Q + 2^28], cx in [-2^28, w Q + 2^28].  Zero and singular matrices are legal (a constant, a line).
 * max_r (Q16, 1 <= max_r <= 2 Q): an upper bound of max(Ry, Rx) over the windows of this call; the launch is sized from it (the windows
 * are never read back).  On the device cy and cx are clamped to their range; a tile with max(Ry, Rx) > max_r is written as fill
 * EVERYWHERE -- there is no sensible clamp of a matrix.
 * SL_ERR_BADARG before anything is launched: what sl_normalize_view / sl_view_planes refuse of rgb / planes, out, n, c, h, w,
 * elem_bytes, alignment, the statistics pattern, params and fmt; a NULL windows; oh < 1 or ow < 1; h, w, oh or ow > 8192; max_r outside
 * [1, 2 Q]; fill_rgb >= 2^24; more (tile, patch) or (plane, patch) pairs than 2^31 - 1 (a patch is min(64, 1 + 62 Q / max_r) outputs
 * square).  No workspace; capture-safe like the rest (no allocation, no synchronisation, no memset).  out == rgb / out == planes is
 * not supported.  Bicubic and antialiased filters, perspective warps (elastic ones: sl_normalize_view_elastic below), reflect / replicate borders and bilinear planes are
 * other definitions and not offered. */
SL_API int sl_normalize_view_affine(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, uint32_t fill_rgb, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);
SL_API int sl_view_planes_affine(const void* planes, void* out, int n, int c, int h, int w, int elem_bytes, int oh, int ow, const int32_t* windows, int max_r, uint64_t fill_bits, void* stream);

/* ---- elastic deformation in the one-pass loader: the affine view plus a smooth per-pixel displacement, for the images and their
 * companion planes alike (stainlib_amd/csrc/view_elastic.hip; an extension: the U-Net recipe of segmentation and nuclei-detection
 * loaders -- random displacements on a coarse grid, interpolated smoothly -- behind the call that is a per-pixel float field of
 * N x H x W x 2 and grid_sample once for the image and once more per label plane) ------------------------------------------------------
 * The definition is in integers, so "bit for bit" applies.  windows: sl_normalize_view_affine's n x 6 rows.  field: n x gh x gw x 2 int32
 * on the device, a control lattice per tile of displacements (dy, dx) in units of 1/256 SOURCE pixel (the resolution of the 8-bit
 * bilinear weights) on cells of 2^k OUTPUT pixels, k = cell_log2 in 4 .. 8, one for the call:
 *     gh = ((oh + 2^k - 1) >> k) + 2        gw = ((ow + 2^k - 1) >> k) + 2
 * max_d in 0 .. 8 (source pixels), one for the call, bounds the field: every control value is CLAMPED to +-256 max_d by the kernel (any
 * int32 is safe).  The displacement of output pixel (i, j) is the uniform quadratic B-spline of the lattice -- C1-smooth, weights exact
 * integers:
 *     along i:  t = ((2 i + 1) << 8) >> (k + 1);   a = t >> 8;   f = t & 255
 *               wy = ((256 - f)^2,  131072 - (256 - f)^2 - f^2,  f^2)                          (>= 0, sum 2^17)
 *     along j:  b, wx likewise from j
 *     r[q]  = (sum_{p=0..2} wx[p] field[a + q][b + p][m] + 65536) >> 17                        (q = 0, 1, 2; arithmetic shift)
 *     d[m]  = (sum_{q=0..2} wy[q] r[q] + 65536) >> 17                                          (m = 0: y, 1: x)
 *     Y = cy + ((a00 u + a01 v) >> 1) + (d[0] << 8)        X = cx + ((a10 u + a11 v) >> 1) + (d[1] << 8)
 * with the affine view's u = 2 i + 1 - oh, v = 2 j + 1 - ow.  From (Y, X) on everything is the affine view's: the taps, the fill outside
 * the tile and the blend of the images (sl_normalize_view_elastic), the element at (Y >> 16, X >> 16) or the fill of the planes
 * (sl_view_planes_elastic) -- a label plane and its image go through the same (Y, X).  What follows: |d| <= max |field| (a convex
 * combination, rounded to nearest); a zero field is the affine view bit for bit; a constant field (c_y, c_x) is the affine view with
 * the centre moved by (c_y << 8, c_x << 8).  Every intermediate is 32-bit.
 * max_r: sl_normalize_view_affine's bound of the row sums; a tile beyond it is written as fill.  The grid is sized on the host from max_r
 * and max_d: a workgroup takes min(64, 1 + (62 - 2 max_d) Q / R) outputs a side and stages the box of its four affine corners grown by
 * max_d pixels, cut to the tile.
 * Returns SL_ERR_BADARG before anything is launched for whatever the affine entry point refuses, a NULL or misaligned field, cell_log2
 * outside 4 .. 8 and max_d outside 0 .. 8; n == 0 is SL_OK and launches nothing.  No workspace; capture-safe like the rest.  out == rgb
 * / out == planes is not supported.  Displacements above 8 pixels, cells below 16, cubic or Gaussian-smoothed fields, perspective warps
 * and bilinear planes are other definitions and not offered. */
SL_API int sl_normalize_view_elastic(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, const int32_t* field, int cell_log2, int max_d, uint32_t fill_rgb, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, void* stream);
SL_API int sl_view_planes_elastic(const void* planes, void* out, int n, int c, int h, int w, int elem_bytes, int oh, int ow, const int32_t* windows, int max_r, const int32_t* field, int cell_log2, int max_d, uint64_t fill_bits, void* stream);

/* ---- hue / saturation / brightness augmentation (stainlib_amd/csrc/hsb.hip; an extension: the HSV half of the Tellez et al. colour
 * augmenters, the sibling of sl_hed_augment).  Defined in INTEGERS on bytes, so every route below computes the same bits.
 * Q = 32768; rdiv(a, c) = (2 a + c) / (2 c), rnd(x) = (x + Q / 2) >> 15, integer division.  codes: n x 3 int32 on the device,
 * (dhq, dsq, dvq) per tile -- from float shifts dh (turns, any real) and ds, dv in [-1, 1]: dhq = floor((dh mod 1) 6 Q + 1/2) mod 6 Q,
 * dsq = floor(ds Q + 1/2), dvq = floor(dv Q + 1/2).  Codes outside their ranges are reduced by the kernel: dhq mod 6 Q (non-negative),
 * dsq and dvq clamped to +-Q.  Per pixel (r, g, b): M = max, m = min, C = M - m;
 *     hq = 0 when C == 0, else (base Q + rdiv((num + C) Q, C) - Q) mod 6 Q with (base, num) = (4, r - g) if M == b, else (2, b - r) if
 *          M == g, else (0, g - b)              (blue wins ties over green, green over red, as in scikit-image's rgb2hsv)
 *     s = 0 when M == 0, else rdiv(C Q, M);   v = rdiv(M Q, 255)
 *     scale(x, d) = x if d == 0;  rnd(x (Q + d)) if d < 0;  rnd(x (Q + rnd((Q - x) d))) if d > 0       (towards Q, never past it)
 *     hq' = (hq + dhq) mod 6 Q,  s' = scale(s, dsq),  v' = scale(v, dvq),  hi = hq' / Q,  fq = hq' - hi Q
 *     p = rnd(v' (Q - s')),  q = rnd(v' (Q - rnd(fq s'))),  t = rnd(v' (Q - rnd((Q - fq) s')))
 *     (R, G, B) by hi: 0 (v', t, p), 1 (q, v', p), 2 (p, v', t), 3 (p, q, v'), 4 (t, p, v'), 5 (v', p, q);  byte = (X 255 + Q / 2) >> 15
 * Zero codes are the identity.  (stainlib_amd/augmentation/hsb.py holds the same in numpy; csrc/hsb_math.hpp in 32 bits.)
 *
 * sl_hsb_augment: out = HSB(rgb) per tile, one sweep, 3 B/px read.  fmt == NULL: out is the n x h x w x 3 uint8 image; else the tensor
 * SlTensorFormat describes, bit for bit sl_to_tensor of that image, written directly.  SL_ERR_BADARG: what sl_to_tensor refuses of rgb,
 * out, n, h, w and a non-NULL fmt; a NULL or misaligned codes.  out == rgb is not supported.
 *
 * sl_normalize_hsb_view: the view of HSB(full[t]) in ONE pass, full[t] the image the statistics pattern names as in sl_normalize_view
 * (the tiles' own bytes, sl_normalize_apply's image, the jitter of tissue pixels or of all pixels).  max_wh == 0 (then max_ww == 0): the
 * fixed-size view of sl_normalize_view_shrink -- windows n x 3, shrink 1, 2 or 4, the box mean taken of the HSB-mapped pixels.
 * Otherwise the resizing view of sl_normalize_view_resize -- windows n x 5, shrink == 1, the area resample of the mapped pixels.  A tile
 * whose fit failed: the view of HSB(its own bytes).  SL_ERR_BADARG before anything is launched: what those two calls refuse; max_wh == 0
 * with max_ww != 0; a resizing view with shrink != 1; a NULL or misaligned codes.  Capture-safe like them. */
SL_API int sl_hsb_augment(const uint8_t* rgb, void* out, int n, int h, int w, const int32_t* codes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_normalize_hsb_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const int32_t* codes, void* stream);

/* ---- Gaussian blur in the view pass (stainlib_amd/csrc/view_blur.hip; an extension: the blur of the usual histopathology augmentation
 * set, a per-tile separable filter in INTEGERS, so every route computes the same bits).  R = 8 is the largest radius, Q = 256 the weight
 * sum per axis.  codes: n x 9 int32 on the device, (w_0 .. w_8) per tile: every w_k >= 0, w_0 + 2 (w_1 + .. + w_8) == 256; the tile's
 * radius r is the largest k with w_k != 0; (256, 0, .., 0) is the identity.  Let full[t] be the h x w x 3 uint8 image the statistics
 * pattern names as in sl_normalize_view (the tile's own bytes, sl_normalize_apply's image, the jitter of tissue pixels or of all pixels;
 * a tile whose fit failed: its own bytes), normalised and jittered per source pixel with the WHOLE tile's statistics.  Per channel
 *     Hs[y, x] = sum_{k=-8..8} w_|k| full[y, clamp(x + k, 0, w - 1)]                         (<= 65280, exact)
 *     B[y, x]  = (sum_{k=-8..8} w_|k| Hs[clamp(y + k, 0, h - 1), x] + 32768) >> 16            (rounded once)
 * The border replicates the TILE's edge, not the window's: the blur is of the whole image, and the view then cuts it.  The output is
 * sl_normalize_view_shrink's view of B: windows[t] = (y0, x0, d), d_mask, (oh, ow), the clamp of the window into the tile, the flip and
 * the quarter turns; with shrink = 2, 4 the box rule (S + s s / 2) >> (2 log2 s) on the bytes of B; fmt as there (the tensor is
 * sl_to_tensor of those bytes).  Identity codes give sl_normalize_view_shrink's bits; a constant image stays constant.
 * max_r (0 .. 8): the call's bound of the radii -- the launch is sized from it (patches of (64 - 2 max_r) / shrink outputs square), the
 * codes themselves are not read on the host.  A tile whose codes fail the rule -- a negative weight, a sum other than 256, a non-zero w_k
 * with k > max_r -- gets the identity; nothing is read out of bounds.  (stainlib_amd/augmentation/blur.py holds the same in numpy, and the
 * rule from sigma to codes: r = min(8, ceil(3 sigma)), g_k = exp(-k k / (2 sigma sigma)) normalised over |k| <= r in binary64,
 * w_k = floor(256 g_k + 1/2) for k >= 1, w_0 = 256 - 2 sum_{k >= 1} w_k; sigma <= 0: the identity.)
 * SL_ERR_BADARG before anything is launched: what sl_normalize_view_shrink refuses; a NULL or misaligned codes; max_r outside 0 .. 8.
 * out == rgb is not supported.  Capture-safe like sl_normalize_view. */
SL_API int sl_normalize_blur_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, int max_r, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const int32_t* codes, void* stream);

/* ---- the post stage: a tone curve and additive noise on the bytes a call WRITES (stainlib_amd/csrc/post.hip; an extension: brightness /
 * contrast / gamma and the Gaussian-noise item of the Tellez et al. / HoVer-Net augmentation set).  Defined in INTEGERS on bytes, so every
 * route below computes the same bits.  The stage acts on a uint8 image n x oh x ow x 3 -- the OUTPUT: behind the view, the box shrink or the
 * area resample, in front of the tensor conversion.  Per tile, pixel p = i ow + j, channel c, byte b:
 *     tone   b1 = tables[256 t + b]: 256 bytes per tile, the same for the three channels; any 256 bytes are a table, 0 .. 255 the identity
 *     noise  codes[4 t ..] = (sq, k0, k1, mono), int32; k0, k1 the bit patterns of two uint32.  W = Philox4x32-10 of the counter
 *            (p, 0, 0, 0) under the key (k0, k1) (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds, the
 *            key bumped between rounds).  Channel c takes W[c], or W[3] for all three when mono != 0.  G = (the sum of the word's four
 *            bytes) - 510 (mean 0, variance 21845: a four-fold Irwin-Hall sum, tails cut at 3.45 sigma).  n = (G sq + 32768) >> 16
 *            (arithmetic), b2 = clamp(b1 + n, 0, 255).  sq = floor(sigma 65536 / sqrt(21845) + 1/2) for a sigma of 0 .. 64 bytes, so
 *            0 <= sq <= 28378; values outside are clamped by the kernel; sq == 0 is the identity.
 * tables, codes: device pointers; each may be NULL (that half is absent), not both; codes 4-byte aligned.  A tile's noise depends on its
 * key and on p, never on its position in the batch.  (stainlib_amd/augmentation/noise.py holds the same in numpy; csrc/post_math.hpp in
 * 32 bits.)
 *
 * sl_post_augment: out = post(rgb) per tile, the full tile (oh x ow = h x w), one sweep, 3 B/px read.  fmt == NULL: out is the n x h x w x 3
 * uint8 image; else the tensor SlTensorFormat describes, bit for bit sl_to_tensor of that image, written directly.  SL_ERR_BADARG: what
 * sl_to_tensor refuses of rgb, out, n, h, w and a non-NULL fmt; tables and codes both NULL; misaligned codes.  out == rgb is not supported.
 *
 * sl_normalize_post_view: post(view of full[t]) in ONE pass, full[t] the image the statistics pattern names as in sl_normalize_view (the
 * tiles' own bytes, sl_normalize_apply's image, the jitter of tissue pixels or of all pixels); p counts in the view's OUTPUT.  max_wh == 0
 * (then max_ww == 0): the fixed-size view of sl_normalize_view_shrink -- windows n x 3, shrink 1, 2 or 4, the stage behind the box mean.
 * Otherwise the resizing view of sl_normalize_view_resize -- windows n x 5, shrink == 1, the stage behind the area resample.  A tile whose
 * fit failed: post(the view of its own bytes).  SL_ERR_BADARG before anything is launched: what those two calls refuse; max_wh == 0 with
 * max_ww != 0; a resizing view with shrink != 1; tables and codes both NULL; misaligned codes.  Capture-safe like them. */
SL_API int sl_post_augment(const uint8_t* rgb, void* out, int n, int h, int w, const uint8_t* tables, const int32_t* codes, const SlTensorFormat* fmt, void* stream);
SL_API int sl_normalize_post_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const uint8_t* tables, const int32_t* codes, void* stream);

/* ---- the one-pass recipe: a colour stage, a view and the post stage TOGETHER (stainlib_amd/csrc/recipe.hip; nothing new is defined,
 * the stages above are composed).  With full[t] the uint8 image the statistics pattern names as in sl_normalize_view:
 *     out[t] = convert( post( view( colour(full[t]) ) ) )
 *   colour  on SOURCE pixels, at most one: sl_hed_augment under hed_applied[t] (sl_normalize_hed_view's stage: hed_sigma, hed_bias n x 3
 *           binary64, hed_applied n int32, skimage_mode 0 only), or the HSB map of sl_normalize_hsb_view (hsb_codes n x 3 int32)
 *   view    the definition of its entry point: the window, flip and turn and the box shrink of sl_normalize_view_shrink, the area resample
 *           of sl_normalize_view_resize, the bilinear sample of sl_normalize_view_affine or sl_normalize_view_elastic
 *   post    on WRITTEN pixels: sl_normalize_post_view's stage (tone_tables n x 256 or NULL, then noise_codes n x 4 int32 or NULL), with
 *           p = i ow + j counted in the view's output
 * All arrays are device pointers; an absent stage is NULL and is the identity, so a recipe with one stage is bit for bit that stage's own
 * call.  Consequences of the order: the fill byte of an affine / elastic view is in output space -- it does NOT take the colour stage and
 * it DOES take the post stage; so does a tile written entirely as fill (a row of windows beyond max_r) and a patch whose source box misses
 * the tile.  A tile whose fit failed is the recipe applied to its own bytes.
 * struct_size must be sizeof(SlViewStages).
 *
 * sl_normalize_stages_view: sl_normalize_post_view's geometry (max_wh == 0: fixed-size with shrink 1, 2, 4; else resizing).  A call whose
 * stages one existing entry point covers -- a colour stage alone, or the post stage alone -- is forwarded to it.
 * sl_normalize_stages_view_affine, sl_normalize_stages_view_elastic: the arguments of sl_normalize_view_affine / _view_elastic.
 * SL_ERR_BADARG before anything is launched: what the parent entry point refuses; stages NULL or of another struct_size; no stage at all;
 * HED and HSB both; an incomplete HED triple; skimage_mode != 0; hsb_codes or noise_codes not 4-byte aligned.  n == 0: SL_OK, nothing
 * launched.  No workspace; capture-safe like the parents.  out == rgb is not supported. */
typedef struct SlViewStages {
    uint32_t struct_size;
    const double *hed_sigma, *hed_bias;   /* n x 3 each */
    const int32_t* hed_applied;           /* n */
    int skimage_mode;                     /* 0 only */
    const int32_t* hsb_codes;             /* n x 3; not together with HED */
    const uint8_t* tone_tables;           /* n x 256 or NULL */
    const int32_t* noise_codes;           /* n x 4 or NULL */
} SlViewStages;
SL_API int sl_normalize_stages_view(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int d_mask, int shrink, int max_wh, int max_ww, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const SlViewStages* stages, void* stream);
SL_API int sl_normalize_stages_view_affine(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, uint32_t fill_rgb, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const SlViewStages* stages, void* stream);
SL_API int sl_normalize_stages_view_elastic(const uint8_t* rgb, void* out, int n, int h, int w, int oh, int ow, const int32_t* windows, int max_r, const int32_t* field, int cell_log2, int max_d, uint32_t fill_rgb, const double* M_src, const double* maxC_src, const double* M_tgt, const double* maxC_tgt, const double* alpha_beta, int augment_background, const SlParams* params, const SlTensorFormat* fmt, const SlViewStages* stages, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STAINLIB_HIP_H */
