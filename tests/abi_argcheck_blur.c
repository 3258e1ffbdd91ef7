/* Argument checks of the blurred view (include/stainlib_hip.h: sl_normalize_blur_view) on the HOST side, no GPU needed: every refused
 * call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under AddressSanitizer by
 * `make -C stainlib_amd/csrc asan-blur` (tests/test_blur_host.py).
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
    int32_t* odd = (int32_t*)0x300402;                         /* not 4-byte aligned */
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

#define BVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd_) \
        EXPECT(sl_normalize_blur_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd_, 0), SL_ERR_BADARG)
/* a refusal of the geometry, the bound or the codes on every route, with and without a format and an SlParams */
#define GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, cd_) do { \
        BVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, d6, d2, d6, d2, ab, 0, 0, 0, cd_); \
        BVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, d6, d2, 0, 0, ab, 1, &p, &f, cd_); \
        BVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, d6, d2, d6, d2, 0, 0, &p, 0, cd_); \
        BVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, s_, mr_, 0, 0, 0, 0, 0, 0, 0, &f, cd_); } while (0)
/* at shrink 1 under the bounds 0 and 8 */
#define FIXED(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_) do { \
        GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 1, 0, cd); GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 1, 8, cd); } while (0)
#define VIEWOK(ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) do { \
        BVIEW(rgb, out, n, h, w, oh, ow, win, 7, 1, 8, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd); \
        BVIEW(rgb, out, n, h, w, 16, 12, win, 7, 2, 3, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, cd); } while (0)

    /* required pointers, the codes, the bound */
    FIXED(0, out, n, h, w, oh, ow, win, 7);
    FIXED(rgb, 0, n, h, w, oh, ow, win, 7);
    FIXED(rgb, out, n, h, w, oh, ow, 0, 7);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 8, 0);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 0, 0);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 8, odd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, -1, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 9, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 32, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, 2147483647, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 1, -2147483647 - 1, cd);
    GEOM(rgb, out, n, h, w, 16, 12, win, 7, 4, 9, cd);
    /* shapes */
    FIXED(rgb, out, 0, h, w, oh, ow, win, 7);
    FIXED(rgb, out, -1, h, w, oh, ow, win, 7);
    FIXED(rgb, out, n, 0, w, oh, ow, win, 7);
    FIXED(rgb, out, n, h, -5, oh, ow, win, 7);
    FIXED(rgb, out, n, 65536, 65536, oh, ow, win, 7); /* more than 2^30 pixels */
    FIXED(rgb, out, n, 32768, 32769, oh, ow, win, 6); /* just over */
    /* the output size, the mask, the transposed window */
    FIXED(rgb, out, n, h, w, 0, ow, win, 7);
    FIXED(rgb, out, n, h, w, oh, 0, win, 7);
    FIXED(rgb, out, n, h, w, oh, -1, win, 7);
    FIXED(rgb, out, n, h, w, h + 1, ow, win, 6);
    FIXED(rgb, out, n, h, w, oh, w + 1, win, 6);
    FIXED(rgb, out, n, h, w, oh, ow, win, -1);
    FIXED(rgb, out, n, h, w, oh, ow, win, 8);
    FIXED(rgb, out, n, h, w, h, w, win, 7);           /* 64 x 48 does not fit into 64 x 48 turned */
    FIXED(rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 7);      /* more (tile, patch) pairs than a grid holds */
    GEOM(rgb, out, 8191, 32768, 32768, 32768, 32768, win, 7, 1, 8, cd);      /* ... than a grid holds with the patches of the bound 8 */
    /* the shrink: a value that is none, a window larger than the tile */
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 0, 8, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 3, 8, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, -2, 0, cd);
    GEOM(rgb, out, n, h, w, oh, ow, win, 6, 2, 8, cd);                  /* 80 x 64 > 64 x 48 */
    GEOM(rgb, out, n, h, w, 16, 16, win, 6, 4, 2, cd);                  /* 64 x 64: too wide */
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
