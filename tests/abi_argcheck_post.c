/* Argument checks of the two entry points of the post stage, the tone curve and the additive noise (include/stainlib_hip.h:
 * sl_post_augment, sl_normalize_post_view) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything
 * is launched or dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-post` (tests/test_post_host.py).
 * Every call is made three times: with tables and codes, with the tables alone and with the codes alone (each may be NULL, not both).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlParams and SlTensorFormat are host pointers: the undersized copies below sit at the very end of their heap blocks, so a library
 * that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    int32_t* cd = (int32_t*)0x300400;
    uint8_t* tb = (uint8_t*)0x300501;                          /* the tables need no alignment */
    int32_t* odd = (int32_t*)0x300402;                         /* not 4-byte aligned */
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

    /* ---- sl_post_augment ---- */
#define AUG1(rgb_, out_, n_, h_, w_, tb_, cd_, f_) EXPECT(sl_post_augment(rgb_, out_, n_, h_, w_, tb_, cd_, f_, 0), SL_ERR_BADARG)
/* cd_ == cd: the three forms; else the codes as given, with the tables */
#define AUG(rgb_, out_, n_, h_, w_, cd_, f_) do { AUG1(rgb_, out_, n_, h_, w_, tb, cd_, f_); \
        if ((cd_) == cd) { AUG1(rgb_, out_, n_, h_, w_, 0, cd_, f_); AUG1(rgb_, out_, n_, h_, w_, tb, 0, f_); } } while (0)
#define AUG2(rgb_, out_, n_, h_, w_, cd_) do { AUG(rgb_, out_, n_, h_, w_, cd_, 0); AUG(rgb_, out_, n_, h_, w_, cd_, &f); } while (0)
    AUG2(0, out, n, h, w, cd);
    AUG2(rgb, 0, n, h, w, cd);
    EXPECT(sl_post_augment(rgb, out, n, h, w, 0, 0, 0, 0), SL_ERR_BADARG);      /* neither tables nor codes */
    EXPECT(sl_post_augment(rgb, out, n, h, w, 0, 0, &f, 0), SL_ERR_BADARG);
    EXPECT(sl_post_augment(rgb, out, n, h, w, 0, odd, 0, 0), SL_ERR_BADARG);
    AUG2(rgb, out, n, h, w, odd);
    AUG2(rgb, out, 0, h, w, cd);
    AUG2(rgb, out, -1, h, w, cd);
    AUG2(rgb, out, n, 0, w, cd);
    AUG2(rgb, out, n, h, -5, cd);
    AUG2(rgb, out, n, 65536, 65536, cd);                       /* more than 2^30 pixels */
    AUG2(rgb, out, n, 32768, 32769, cd);                       /* just over */
    AUG2(rgb, out, 2147483647, 32768, 32768, cd);              /* more (tile, part) pairs than a grid holds */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                               AUG(rgb, out, n, h, w, cd, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      AUG(rgb, out, n, h, w, cd, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      AUG(rgb, out, n, h, w, cd, &g);
        void* blk = undersized(&f);
        AUG(rgb, out, n, h, w, cd, (const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     AUG(rgb, out, n, h, w, cd, &g);
            g = f; g.layout = bad[i];                    AUG(rgb, out, n, h, w, cd, &g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       AUG(rgb, out, n, h, w, cd, &g);
            g = f; g.std[c] = NAN;                       AUG(rgb, out, n, h, w, cd, &g);
            g = f; g.mean[c] = -INFINITY;                AUG(rgb, out, n, h, w, cd, &g);
        }
    }

    /* ---- sl_normalize_post_view ---- */
#define HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd_) \
        do { EXPECT(sl_normalize_post_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, tb, cd_, 0), SL_ERR_BADARG); \
        if ((cd_) == cd) { \
        EXPECT(sl_normalize_post_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, 0, cd_, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_post_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, tb, 0, 0), SL_ERR_BADARG); } } while (0)
/* a refusal of the geometry or of the codes on every route, with and without a format and an SlParams */
#define GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, cd_) do { \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, d6, d2, d6, d2, ab, 0, 0, 0, cd_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, d6, d2, 0, 0, ab, 1, &p, &f, cd_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, d6, d2, d6, d2, 0, 0, &p, 0, cd_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mh_, mw_, 0, 0, 0, 0, 0, 0, 0, &f, cd_); } while (0)
/* the fixed-size view (shrink 1) and the resizing view whose bound is the tile */
#define FIXED(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_) GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 1, 0, 0, cd)
#define RESIZE(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_) GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 1, mh_, mw_, cd)
#define VIEWOK(ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) do { \
        HVIEW(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd); \
        HVIEW(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd); } while (0)

    /* required pointers, the codes */
    FIXED(0, out, n, h, w, oh, ow, win, 7);           RESIZE(0, out, n, h, w, oh, ow, win, 7, h, w);
    FIXED(rgb, 0, n, h, w, oh, ow, win, 7);           RESIZE(rgb, 0, n, h, w, oh, ow, win, 7, h, w);
    FIXED(rgb, out, n, h, w, oh, ow, 0, 7);           RESIZE(rgb, out, n, h, w, oh, ow, 0, 7, h, w);
    EXPECT(sl_normalize_post_view(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, d6, d2, d6, d2, ab, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);   /* neither */
    EXPECT(sl_normalize_post_view(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, 0, 0, 0, 0, 0, 0, &p, &f, 0, 0, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_post_view(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, odd, 0), SL_ERR_BADARG);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0, odd);
    EXPECT(sl_normalize_post_view(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w, d6, d2, d6, d2, ab, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);   /* neither */
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, h, w, odd);
    /* shapes */
    FIXED(rgb, out, 0, h, w, oh, ow, win, 7);         RESIZE(rgb, out, 0, h, w, oh, ow, win, 7, h, w);
    FIXED(rgb, out, -1, h, w, oh, ow, win, 7);
    FIXED(rgb, out, n, 0, w, oh, ow, win, 7);         RESIZE(rgb, out, n, h, -5, oh, ow, win, 7, h, w);
    FIXED(rgb, out, n, 65536, 65536, oh, ow, win, 7); /* more than 2^30 pixels */
    FIXED(rgb, out, n, 32768, 32769, oh, ow, win, 6); /* just over */
    /* the output size, the mask, the transposed window */
    FIXED(rgb, out, n, h, w, 0, ow, win, 7);          RESIZE(rgb, out, n, h, w, 0, ow, win, 7, h, w);
    FIXED(rgb, out, n, h, w, oh, 0, win, 7);          RESIZE(rgb, out, n, h, w, oh, -1, win, 7, h, w);
    FIXED(rgb, out, n, h, w, h + 1, ow, win, 6);
    FIXED(rgb, out, n, h, w, oh, w + 1, win, 6);
    FIXED(rgb, out, n, h, w, oh, ow, win, -1);        RESIZE(rgb, out, n, h, w, oh, ow, win, -1, h, w);
    FIXED(rgb, out, n, h, w, oh, ow, win, 8);         RESIZE(rgb, out, n, h, w, oh, ow, win, 8, h, w);
    FIXED(rgb, out, n, h, w, h, w, win, 7);           /* 64 x 48 does not fit into 64 x 48 turned */
    FIXED(rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 7);      /* more (tile, patch) pairs than a grid holds */
    /* the shrink: a value that is none, a window larger than the tile, a shrink on a resizing view */
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 3, 0, 0, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, -2, 0, 0, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 6, 2, 0, 0, cd);               /* 80 x 64 > 64 x 48 */
    GEOM(rgb, out, n, h, w, 16, 16, win, 6, 4, 0, 0, cd);               /* 64 x 64: too wide */
    GEOM(rgb, out, n, h, w, 16, 12, win, 6, 2, h, w, cd);
    GEOM(rgb, out, n, h, w, 16, 12, win, 6, 4, h, w, cd);
    /* the bound of a resizing view: one side alone, outside the tile, too many pixels */
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, w, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, h, 0, cd);
    RESIZE(rgb, out, n, h, w, oh, ow, win, 7, -1, w);
    RESIZE(rgb, out, n, h, w, oh, ow, win, 7, h + 1, w);
    RESIZE(rgb, out, n, h, w, oh, ow, win, 7, h, w + 1);
    RESIZE(rgb, out, n, 4096, 4096, oh, ow, win, 7, 2049, 2048);         /* more than 2^22 pixels */
    /* the statistics */
    VIEWOK(d6, 0, d6, d2, ab, 0, 0, 0);               /* M_src without maxC_src */
    VIEWOK(d6, d2, 0, d2, ab, 0, 0, 0);               /* a one-sided target */
    VIEWOK(d6, d2, d6, 0, ab, 0, 0, &f);
    VIEWOK(d6, d2, 0, 0, 0, 0, 0, 0);                 /* the apply route has no "no target" */
    VIEWOK(0, d2, 0, 0, 0, 0, 0, 0);                  /* the source bytes: nothing else may be given */
    VIEWOK(0, 0, d6, d2, 0, 0, 0, 0);
    VIEWOK(0, 0, 0, 0, ab, 1, &p, &f);
    /* SlParams.struct_size, two_sweep */
    {
        SlParams q = p;
        q.struct_size = 0;                         VIEWOK(d6, d2, d6, d2, ab, 0, &q, 0);
        q.struct_size = sizeof(SlParams) - 8;      VIEWOK(d6, d2, d6, d2, 0, 0, &q, &f);
        q.struct_size = sizeof(SlParams) + 8;      VIEWOK(0, 0, 0, 0, 0, 0, &q, 0);
        q = p; q.two_sweep = 9;                    VIEWOK(d6, d2, 0, 0, ab, 1, &q, 0);
        void* blk = undersized(&p);
        VIEWOK(d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0);
        VIEWOK(0, 0, 0, 0, 0, 0, (const SlParams*)blk, &f);
        free(blk);
    }
    /* SlTensorFormat: struct_size, dtype, layout, std, non-finite values (the checks of sl_to_tensor) */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                               VIEWOK(d6, d2, d6, d2, ab, 0, 0, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      VIEWOK(d6, d2, d6, d2, 0, 0, &p, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      VIEWOK(0, 0, 0, 0, 0, 0, 0, &g);
        void* blk = undersized(&f);
        VIEWOK(d6, d2, d6, d2, ab, 0, 0, (const SlTensorFormat*)blk);
        VIEWOK(0, 0, 0, 0, 0, 0, 0, (const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     VIEWOK(d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.layout = bad[i];                    VIEWOK(0, 0, 0, 0, 0, 0, 0, &g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       VIEWOK(d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = NAN;                       VIEWOK(0, 0, 0, 0, 0, 0, 0, &g);
            g = f; g.mean[c] = -INFINITY;                VIEWOK(d6, d2, 0, 0, ab, 1, &p, &g);
        }
    }
    return report();
}
