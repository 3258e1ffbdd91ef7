/* Argument checks of the three entry points of the one-pass recipe (include/stainlib_hip.h: sl_normalize_stages_view,
 * sl_normalize_stages_view_affine, sl_normalize_stages_view_elastic) on the HOST side, no GPU needed: every refused call must return
 * SL_ERR_BADARG before anything is launched or dereferenced, and an empty batch (n == 0) is SL_OK with nothing launched -- also where the
 * call would be forwarded to an existing entry point.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-recipe`
 * (tests/test_recipe_host.py).  Every refusal of the parent's arguments is made with each valid set of stages (ST below), so that what is
 * refused is the other argument; every refusal of the stages is made on each entry point and route.
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.  SlViewStages,
 * SlParams and SlTensorFormat are host pointers: the undersized copies sit at the very end of their heap blocks, so a library that read a
 * caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

#define Q 65536

static uint8_t* rgb = (uint8_t*)0x100000;
static void* out = (void*)0x200000;
static double* d6 = (double*)0x300000;
static double* d2 = (double*)0x300100;
static double* ab = (double*)0x300200;
static int32_t* win = (int32_t*)0x300300;
static int32_t* fld = (int32_t*)0x500100;
static SlParams prm;
static SlTensorFormat fmt;

static SlViewStages stages(const double* sg, const double* bs, const int32_t* ap, const int32_t* hsb, const uint8_t* tb, const int32_t* cd) {
    SlViewStages s;
    memset(&s, 0, sizeof s);
    s.struct_size = sizeof s;
    s.hed_sigma = sg; s.hed_bias = bs; s.hed_applied = ap; s.hsb_codes = hsb; s.tone_tables = tb; s.noise_codes = cd;
    return s;
}

/* the three calls on a route r (0: the tiles' own bytes, 1: apply, 2: the jitter of tissue pixels with params and a format, 3: the jitter
 * of all pixels under the tile's own matrix) */
static int fixed(const uint8_t* in, void* o, int n, int h, int w, int oh, int ow, const int32_t* wn, int dm, int s, int mh, int mw, int r,
                 const SlViewStages* st) {
    switch (r) {
    case 0: return sl_normalize_stages_view(in, o, n, h, w, oh, ow, wn, dm, s, mh, mw, 0, 0, 0, 0, 0, 0, 0, &fmt, st, 0);
    case 1: return sl_normalize_stages_view(in, o, n, h, w, oh, ow, wn, dm, s, mh, mw, d6, d2, d6, d2, 0, 0, &prm, 0, st, 0);
    case 2: return sl_normalize_stages_view(in, o, n, h, w, oh, ow, wn, dm, s, mh, mw, d6, d2, d6, d2, ab, 0, &prm, &fmt, st, 0);
    default: return sl_normalize_stages_view(in, o, n, h, w, oh, ow, wn, dm, s, mh, mw, d6, d2, 0, 0, ab, 1, 0, 0, st, 0);
    }
}
static int affine(const uint8_t* in, void* o, int n, int h, int w, int oh, int ow, const int32_t* wn, int mr, uint32_t fill, int r,
                  const SlViewStages* st) {
    switch (r) {
    case 0: return sl_normalize_stages_view_affine(in, o, n, h, w, oh, ow, wn, mr, fill, 0, 0, 0, 0, 0, 0, 0, &fmt, st, 0);
    case 1: return sl_normalize_stages_view_affine(in, o, n, h, w, oh, ow, wn, mr, fill, d6, d2, d6, d2, 0, 0, &prm, 0, st, 0);
    case 2: return sl_normalize_stages_view_affine(in, o, n, h, w, oh, ow, wn, mr, fill, d6, d2, d6, d2, ab, 0, &prm, &fmt, st, 0);
    default: return sl_normalize_stages_view_affine(in, o, n, h, w, oh, ow, wn, mr, fill, d6, d2, 0, 0, ab, 1, 0, 0, st, 0);
    }
}
static int elastic(const uint8_t* in, void* o, int n, int h, int w, int oh, int ow, const int32_t* wn, int mr, const int32_t* fd, int k,
                   int md, uint32_t fill, int r, const SlViewStages* st) {
    switch (r) {
    case 0: return sl_normalize_stages_view_elastic(in, o, n, h, w, oh, ow, wn, mr, fd, k, md, fill, 0, 0, 0, 0, 0, 0, 0, &fmt, st, 0);
    case 1: return sl_normalize_stages_view_elastic(in, o, n, h, w, oh, ow, wn, mr, fd, k, md, fill, d6, d2, d6, d2, 0, 0, &prm, 0, st, 0);
    case 2: return sl_normalize_stages_view_elastic(in, o, n, h, w, oh, ow, wn, mr, fd, k, md, fill, d6, d2, d6, d2, ab, 0, &prm, &fmt, st, 0);
    default: return sl_normalize_stages_view_elastic(in, o, n, h, w, oh, ow, wn, mr, fd, k, md, fill, d6, d2, 0, 0, ab, 1, 0, 0, st, 0);
    }
}

int main(void) {
    double* sg = (double*)0x600000;    double* bs = (double*)0x600100;
    int32_t* ap = (int32_t*)0x600200;  int32_t* hc = (int32_t*)0x600300;   int32_t* cd = (int32_t*)0x600400;
    uint8_t* tb = (uint8_t*)0x600501;                          /* the tables need no alignment */
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    sl_default_params(&prm);
    sl_default_tensor_format(&fmt);
    EXPECT(sl_version(), SL_VERSION);

    /* every valid set of stages: a colour stage alone, the post stage alone (its three forms), both */
    SlViewStages ST[11];
    int nst = 0;
    ST[nst++] = stages(sg, bs, ap, 0, 0, 0);
    ST[nst++] = stages(0, 0, 0, hc, 0, 0);
    ST[nst++] = stages(0, 0, 0, 0, tb, cd);
    ST[nst++] = stages(0, 0, 0, 0, tb, 0);
    ST[nst++] = stages(0, 0, 0, 0, 0, cd);
    ST[nst++] = stages(sg, bs, ap, 0, tb, cd);
    ST[nst++] = stages(sg, bs, ap, 0, 0, cd);
    ST[nst++] = stages(0, 0, 0, hc, tb, cd);
    ST[nst++] = stages(0, 0, 0, hc, tb, 0);

/* a refusal of the parent's arguments: with every set of stages on every route */
#define FIXED(in_, o_, n_, h_, w_, oh_, ow_, wn_, dm_, s_, mh_, mw_) do { for (int i_ = 0; i_ < nst; ++i_) for (int r_ = 0; r_ < 4; ++r_) \
        EXPECT(fixed(in_, o_, n_, h_, w_, oh_, ow_, wn_, dm_, s_, mh_, mw_, r_, &ST[i_]), SL_ERR_BADARG); } while (0)
#define AFF(in_, o_, n_, h_, w_, oh_, ow_, wn_, mr_, fill_) do { for (int i_ = 0; i_ < nst; ++i_) for (int r_ = 0; r_ < 4; ++r_) \
        EXPECT(affine(in_, o_, n_, h_, w_, oh_, ow_, wn_, mr_, fill_, r_, &ST[i_]), SL_ERR_BADARG); } while (0)
#define ELA(in_, o_, n_, h_, w_, oh_, ow_, wn_, mr_, fd_, k_, md_, fill_) do { for (int i_ = 0; i_ < nst; ++i_) for (int r_ = 0; r_ < 4; ++r_) \
        EXPECT(elastic(in_, o_, n_, h_, w_, oh_, ow_, wn_, mr_, fd_, k_, md_, fill_, r_, &ST[i_]), SL_ERR_BADARG); } while (0)
/* a refusal of the stages: on the three entry points (the fixed-size and the resizing view), on every route */
#define STAGES(st_) do { for (int r_ = 0; r_ < 4; ++r_) { \
        EXPECT(fixed(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, r_, st_), SL_ERR_BADARG); \
        EXPECT(fixed(rgb, out, n, h, w, 20, 16, win, 6, 2, 0, 0, r_, st_), SL_ERR_BADARG); \
        EXPECT(fixed(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w, r_, st_), SL_ERR_BADARG); \
        EXPECT(fixed(rgb, out, 0, h, w, oh, ow, win, 7, 1, 0, 0, r_, st_), SL_ERR_BADARG); \
        EXPECT(affine(rgb, out, n, h, w, oh, ow, win, Q, 0xffffff, r_, st_), SL_ERR_BADARG); \
        EXPECT(affine(rgb, out, 0, h, w, oh, ow, win, Q, 0, r_, st_), SL_ERR_BADARG); \
        EXPECT(elastic(rgb, out, n, h, w, oh, ow, win, Q, fld, 5, 4, 0, r_, st_), SL_ERR_BADARG); \
        EXPECT(elastic(rgb, out, 0, h, w, oh, ow, win, Q, fld, 5, 4, 0, r_, st_), SL_ERR_BADARG); } } while (0)

    /* ---- the stages ---- */
    STAGES(0);                                                                   /* no struct */
    {
        SlViewStages s = ST[5];
        s.struct_size = 0;                              STAGES(&s);
        s.struct_size = sizeof(SlViewStages) - 8;       STAGES(&s);
        s.struct_size = sizeof(SlViewStages) + 8;       STAGES(&s);
        void* blk = undersized(&ST[5]);
        STAGES((const SlViewStages*)blk);
        free(blk);
        s = stages(0, 0, 0, 0, 0, 0);                   STAGES(&s);              /* no stage at all */
        s = stages(sg, bs, ap, hc, 0, 0);               STAGES(&s);              /* HED and HSB */
        s = stages(sg, bs, ap, hc, tb, cd);             STAGES(&s);
        s = stages(sg, 0, 0, 0, 0, 0);                  STAGES(&s);              /* an incomplete HED triple: each of the six */
        s = stages(0, bs, 0, 0, tb, 0);                 STAGES(&s);
        s = stages(0, 0, ap, 0, 0, cd);                 STAGES(&s);
        s = stages(sg, bs, 0, 0, tb, cd);               STAGES(&s);
        s = stages(sg, 0, ap, 0, 0, 0);                 STAGES(&s);
        s = stages(0, bs, ap, 0, 0, 0);                 STAGES(&s);
        s = stages(0, bs, 0, hc, 0, 0);                 STAGES(&s);              /* (and beside an HSB stage) */
        const int modes[] = {1, 2, 3, 4, -1, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(modes) / sizeof(modes[0]); ++i) {        /* skimage_mode: 0 only, with or without a HED stage */
            s = ST[0]; s.skimage_mode = modes[i];       STAGES(&s);
            s = ST[5]; s.skimage_mode = modes[i];       STAGES(&s);
            s = ST[7]; s.skimage_mode = modes[i];       STAGES(&s);
        }
        for (int off = 1; off < 4; ++off) {                                      /* misaligned codes */
            s = stages(0, 0, 0, (int32_t*)((char*)hc + off), 0, 0);         STAGES(&s);
            s = stages(0, 0, 0, (int32_t*)((char*)hc + off), tb, cd);       STAGES(&s);
            s = stages(0, 0, 0, 0, 0, (int32_t*)((char*)cd + off));         STAGES(&s);
            s = stages(0, 0, 0, 0, tb, (int32_t*)((char*)cd + off));        STAGES(&s);
            s = stages(sg, bs, ap, 0, 0, (int32_t*)((char*)cd + off));      STAGES(&s);
            s = stages(0, 0, 0, hc, 0, (int32_t*)((char*)cd + off));        STAGES(&s);
        }
    }

    /* ---- what sl_normalize_post_view refuses: the fixed-size and the resizing view ---- */
    FIXED(0, out, n, h, w, oh, ow, win, 7, 1, 0, 0);          FIXED(0, out, n, h, w, oh, ow, win, 7, 1, h, w);
    FIXED(rgb, 0, n, h, w, oh, ow, win, 7, 1, 0, 0);          FIXED(rgb, 0, n, h, w, oh, ow, win, 7, 1, h, w);
    FIXED(rgb, out, n, h, w, oh, ow, 0, 7, 1, 0, 0);          FIXED(rgb, out, n, h, w, oh, ow, 0, 7, 1, h, w);
    FIXED(rgb, out, -1, h, w, oh, ow, win, 7, 1, 0, 0);       FIXED(rgb, out, -2147483647 - 1, h, w, oh, ow, win, 7, 1, h, w);
    FIXED(rgb, out, n, 0, w, oh, ow, win, 7, 1, 0, 0);        FIXED(rgb, out, n, h, -5, oh, ow, win, 7, 1, h, w);
    FIXED(rgb, out, n, 65536, 65536, oh, ow, win, 7, 1, 0, 0);                   /* more than 2^30 pixels */
    FIXED(rgb, out, n, 32768, 32769, oh, ow, win, 6, 1, 0, 0);                   /* just over */
    FIXED(rgb, out, n, h, w, 0, ow, win, 7, 1, 0, 0);         FIXED(rgb, out, n, h, w, 0, ow, win, 7, 1, h, w);
    FIXED(rgb, out, n, h, w, oh, 0, win, 7, 1, 0, 0);         FIXED(rgb, out, n, h, w, oh, -1, win, 7, 1, h, w);
    FIXED(rgb, out, n, h, w, h + 1, ow, win, 6, 1, 0, 0);
    FIXED(rgb, out, n, h, w, oh, w + 1, win, 6, 1, 0, 0);
    FIXED(rgb, out, n, h, w, oh, ow, win, -1, 1, 0, 0);       FIXED(rgb, out, n, h, w, oh, ow, win, -1, 1, h, w);
    FIXED(rgb, out, n, h, w, oh, ow, win, 8, 1, 0, 0);        FIXED(rgb, out, n, h, w, oh, ow, win, 8, 1, h, w);
    FIXED(rgb, out, n, h, w, h, w, win, 7, 1, 0, 0);                             /* 64 x 48 does not fit into 64 x 48 turned */
    FIXED(rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 7, 1, 0, 0);       /* more (tile, patch) pairs than a grid holds */
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0);                           /* the shrink */
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 3, 0, 0);
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, -2, 0, 0);
    FIXED(rgb, out, n, h, w, oh, ow, win, 6, 2, 0, 0);                           /* 80 x 64 > 64 x 48 */
    FIXED(rgb, out, n, h, w, 16, 16, win, 6, 4, 0, 0);                           /* 64 x 64: too wide */
    FIXED(rgb, out, n, h, w, 16, 12, win, 6, 2, h, w);                           /* a shrink on a resizing view */
    FIXED(rgb, out, n, h, w, 16, 12, win, 6, 4, h, w);
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, w);                           /* the bound of a resizing view */
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 1, h, 0);
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 1, -1, w);
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 1, h + 1, w);
    FIXED(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w + 1);
    FIXED(rgb, out, n, 4096, 4096, oh, ow, win, 7, 1, 2049, 2048);               /* more than 2^22 pixels */

    /* ---- what sl_normalize_view_affine and sl_normalize_view_elastic refuse ---- */
    AFF(0, out, n, h, w, 8, 8, win, Q, 0);                    ELA(0, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0);
    AFF(rgb, 0, n, h, w, 8, 8, win, Q, 0);                    ELA(rgb, 0, n, h, w, 8, 8, win, Q, fld, 5, 4, 0);
    AFF(rgb, out, n, h, w, 8, 8, 0, Q, 0);                    ELA(rgb, out, n, h, w, 8, 8, 0, Q, fld, 5, 4, 0);
    ELA(rgb, out, n, h, w, 8, 8, win, Q, 0, 5, 4, 0);
    for (int off = 1; off < 4; ++off) ELA(rgb, out, n, h, w, 8, 8, win, Q, (int32_t*)((char*)fld + off), 5, 4, 0);
    {
        const int bad[] = {0, -1, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            if (bad[i] < 0) { AFF(rgb, out, bad[i], h, w, 8, 8, win, Q, 0);   ELA(rgb, out, bad[i], h, w, 8, 8, win, Q, fld, 5, 4, 0); }
            AFF(rgb, out, n, bad[i], w, 8, 8, win, Q, 0);     ELA(rgb, out, n, bad[i], w, 8, 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, n, h, bad[i], 8, 8, win, Q, 0);     ELA(rgb, out, n, h, bad[i], 8, 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, n, h, w, bad[i], 8, win, Q, 0);     ELA(rgb, out, n, h, w, bad[i], 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, n, h, w, 8, bad[i], win, Q, 0);     ELA(rgb, out, n, h, w, 8, bad[i], win, Q, fld, 5, 4, 0);
        }
        const int big[] = {8193, 65536, 2147483647};                             /* h, w, oh, ow > 8192 */
        for (unsigned i = 0; i < sizeof(big) / sizeof(big[0]); ++i) {
            AFF(rgb, out, 1, big[i], w, 8, 8, win, Q, 0);     ELA(rgb, out, 1, big[i], w, 8, 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, 1, h, big[i], 8, 8, win, Q, 0);     ELA(rgb, out, 1, h, big[i], 8, 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, 1, h, w, big[i], 8, win, Q, 0);     ELA(rgb, out, 1, h, w, big[i], 8, win, Q, fld, 5, 4, 0);
            AFF(rgb, out, 1, h, w, 8, big[i], win, Q, 0);     ELA(rgb, out, 1, h, w, 8, big[i], win, Q, fld, 5, 4, 0);
        }
        const int mr[] = {0, -1, 2 * Q + 1, 4 * Q, 2147483647, -2147483647 - 1};  /* max_r outside [1, 2 Q] */
        for (unsigned i = 0; i < sizeof(mr) / sizeof(mr[0]); ++i) {
            AFF(rgb, out, n, h, w, 8, 8, win, mr[i], 0);      ELA(rgb, out, n, h, w, 8, 8, win, mr[i], fld, 5, 4, 0);
        }
        const int cl[] = {3, 0, -1, 9, 32, 2147483647, -2147483647 - 1};         /* cell_log2 outside 4 .. 8 */
        for (unsigned i = 0; i < sizeof(cl) / sizeof(cl[0]); ++i) ELA(rgb, out, n, h, w, 8, 8, win, Q, fld, cl[i], 4, 0);
        const int md[] = {-1, 9, 32, 2147483647, -2147483647 - 1};               /* max_d outside 0 .. 8 */
        for (unsigned i = 0; i < sizeof(md) / sizeof(md[0]); ++i) ELA(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, md[i], 0);
    }
    AFF(rgb, out, n, h, w, 8, 8, win, Q, 0x1000000u);         ELA(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0x1000000u);
    AFF(rgb, out, n, h, w, 8, 8, win, Q, 0xffffffffu);        ELA(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0x80000000u);
    AFF(rgb, out, 2147483647, 8, 8, 65, 65, win, Q, 0);                          /* more (tile, patch) pairs than 2^31 - 1 */
    ELA(rgb, out, 2147483647, 8, 8, 65, 65, win, Q, fld, 5, 0, 0);
    ELA(rgb, out, 1073741824, 8, 8, 48, 48, win, Q, fld, 5, 8, 0);
    AFF(rgb, out, 131072, 8, 8, 8192, 8192, win, Q / 2, 0);
    ELA(rgb, out, 131072, 8, 8, 8192, 8192, win, Q / 2, fld, 4, 0, 0);

    /* ---- the statistics pattern, SlParams and SlTensorFormat: sl_normalize_view's rules, on the three entry points ---- */
    for (int i = 0; i < nst; ++i) {
        const SlViewStages* s = &ST[i];
#define ROUTE(ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) do { \
        EXPECT(sl_normalize_stages_view(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, s, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_stages_view(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, s, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_stages_view_affine(rgb, out, n, h, w, oh, ow, win, Q, 0, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, s, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_stages_view_elastic(rgb, out, n, h, w, oh, ow, win, Q, fld, 5, 4, 0, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, s, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_stages_view_elastic(rgb, out, 0, h, w, oh, ow, win, Q, fld, 5, 4, 0, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, s, 0), SL_ERR_BADARG); \
        } while (0)
        ROUTE(d6, 0, d6, d2, ab, 0, 0, 0);                    /* M_src without maxC_src */
        ROUTE(d6, d2, 0, d2, ab, 0, 0, 0);                    /* a one-sided target */
        ROUTE(d6, d2, d6, 0, ab, 0, 0, &fmt);
        ROUTE(d6, d2, 0, 0, 0, 0, 0, 0);                      /* the apply route has no "no target" */
        ROUTE(0, d2, 0, 0, 0, 0, 0, 0);                       /* the source bytes: nothing else may be given */
        ROUTE(0, 0, d6, d2, 0, 0, 0, 0);
        ROUTE(0, 0, 0, 0, ab, 1, &prm, &fmt);
        SlParams q = prm;
        q.struct_size = 0;                         ROUTE(d6, d2, d6, d2, ab, 0, &q, 0);
        q.struct_size = sizeof(SlParams) - 8;      ROUTE(d6, d2, d6, d2, 0, 0, &q, &fmt);
        q.struct_size = sizeof(SlParams) + 8;      ROUTE(0, 0, 0, 0, 0, 0, &q, 0);
        q = prm; q.two_sweep = 9;                  ROUTE(d6, d2, 0, 0, ab, 1, &q, 0);
        void* blk = undersized(&prm);
        ROUTE(d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0);
        free(blk);
        SlTensorFormat g = fmt;
        g.struct_size = 0;                               ROUTE(d6, d2, d6, d2, ab, 0, 0, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      ROUTE(0, 0, 0, 0, 0, 0, 0, &g);
        blk = undersized(&fmt);
        ROUTE(0, 0, 0, 0, 0, 0, 0, (const SlTensorFormat*)blk);
        free(blk);
        g = fmt; g.dtype = 3;                            ROUTE(d6, d2, d6, d2, ab, 0, 0, &g);
        g = fmt; g.layout = -1;                          ROUTE(0, 0, 0, 0, 0, 0, 0, &g);
        g = fmt; g.std[1] = 0.0;                         ROUTE(d6, d2, d6, d2, ab, 0, 0, &g);
        g = fmt; g.mean[2] = NAN;                        ROUTE(d6, d2, 0, 0, ab, 1, &prm, &g);
    }

    /* ---- an empty batch is fine and launches nothing -- with every set of stages, forwarded ones included, on every route ---- */
    for (int i = 0; i < nst; ++i)
        for (int r = 0; r < 4; ++r) {
            EXPECT(fixed(rgb, out, 0, h, w, oh, ow, win, 7, 1, 0, 0, r, &ST[i]), SL_OK);
            EXPECT(fixed(rgb, out, 0, h, w, 20, 16, win, 6, 2, 0, 0, r, &ST[i]), SL_OK);
            EXPECT(fixed(rgb, out, 0, h, w, oh, ow, win, 7, 1, h, w, r, &ST[i]), SL_OK);
            EXPECT(affine(rgb, out, 0, h, w, oh, ow, win, Q, 0xffffff, r, &ST[i]), SL_OK);
            EXPECT(elastic(rgb, out, 0, h, w, oh, ow, win, Q, fld, 4, 0, 0, r, &ST[i]), SL_OK);
        }
    /* -- but only a call that is right otherwise */
    FIXED(rgb, out, 0, h, w, oh, ow, win, 9, 1, 0, 0);
    FIXED(rgb, out, 0, h, w, oh, ow, 0, 7, 1, h, w);
    AFF(rgb, out, 0, h, w, 8, 8, win, 0, 0);
    ELA(rgb, out, 0, h, w, 8, 8, win, Q, fld, 3, 4, 0);
    ELA(rgb, out, 0, h, w, 8, 8, win, Q, 0, 5, 4, 0);
    return report();
}
