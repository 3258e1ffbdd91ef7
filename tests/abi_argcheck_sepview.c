/* Argument checks of the stain separation in the view pass (include/stainlib_hip.h: sl_stain_separate_view) on the HOST side, no GPU
 * needed: every refused call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under
 * AddressSanitizer by `make -C stainlib_amd/csrc asan-sepview` (tests/test_separate_view_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlSeparateOut and SlTensorFormat are host pointers: the undersized copies below sit at the very end of their heap blocks, so a
 * library that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    uint8_t* o1 = (uint8_t*)0x200000;  uint8_t* o2 = (uint8_t*)0x210000;  uint8_t* o3 = (uint8_t*)0x220000;
    void* cc = (void*)0x230000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;
    int32_t* win = (int32_t*)0x400000;
    const int n = 4, h = 64, w = 48, oh = 32, ow = 24;
    SlSeparateOut f;
    SlTensorFormat t;
    sl_default_separate_out(&f);
    sl_default_tensor_format(&t);
    EXPECT(sl_version(), SL_VERSION);
    EXPECT(sizeof(SlSeparateOut), 40);
    f.norm = o1; f.stain[0] = o2; f.stain[1] = o3; f.conc = cc;      /* a complete request: every refusal below is its own */

#define SV(rgb_, n_, h_, w_, oh_, ow_, win_, dm_, s_, ms_, cs_, mt_, ct_, lam_, outs_, fmt_) \
        EXPECT(sl_stain_separate_view(rgb_, n_, h_, w_, oh_, ow_, win_, dm_, s_, ms_, cs_, mt_, ct_, lam_, outs_, fmt_, 0), SL_ERR_BADARG)
#define SEP(rgb_, n_, h_, w_, ms_, cs_, mt_, ct_, outs_) SV(rgb_, n_, h_, w_, oh, ow, win, 7, 1, ms_, cs_, mt_, ct_, 0.01, outs_, 0)
#define VIEW(oh_, ow_, win_, dm_, s_, outs_, fmt_) SV(rgb, n, h, w, oh_, ow_, win_, dm_, s_, d6, d2, d6, d2, 0.01, outs_, fmt_)

    /* ---- what sl_stain_separate refuses ---- */
    /* required pointers */
    SEP(0, n, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, h, w, 0, d2, d6, d2, &f);
    SEP(rgb, n, h, w, d6, 0, d6, d2, &f);
    SEP(rgb, n, h, w, d6, d2, d6, d2, 0);
    SEP(rgb, n, h, w, d6, d2, 0, 0, 0);
    /* a one-sided target */
    SEP(rgb, n, h, w, d6, d2, 0, d2, &f);
    SEP(rgb, n, h, w, d6, d2, d6, 0, &f);
    /* shapes */
    SEP(rgb, 0, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, -1, h, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, 0, w, d6, d2, d6, d2, &f);
    SEP(rgb, n, h, -5, d6, d2, d6, d2, &f);
    SEP(rgb, n, 65536, 65536, d6, d2, d6, d2, &f);      /* more than 2^30 pixels */
    SEP(rgb, n, 32768, 32769, d6, d2, 0, 0, &f);        /* just over, no target */
    /* lasso_lambda: negative, NaN */
    SV(rgb, n, h, w, oh, ow, win, 7, 1, d6, d2, d6, d2, -0.5, &f, 0);
    SV(rgb, n, h, w, oh, ow, win, 7, 1, d6, d2, d6, d2, (double)NAN, &f, 0);
    SV(rgb, n, h, w, oh, ow, win, 7, 1, d6, d2, 0, 0, -1e-300, &f, &t);
    /* struct_size */
    {
        SlSeparateOut g = f;
        g.struct_size = 0;                         SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.struct_size = sizeof(SlSeparateOut) - 8; SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.struct_size = sizeof(SlSeparateOut) + 8; SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        void* blk = undersized(&f);                /* (the header fields and one pointer) */
        SEP(rgb, n, h, w, d6, d2, d6, d2, (const SlSeparateOut*)blk);
        SEP(rgb, n, h, w, d6, d2, 0, 0, (const SlSeparateOut*)blk);
        free(blk);
    }
    /* conc_dtype: checked with and without planes */
    {
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            SlSeparateOut g = f;
            g.conc_dtype = bad[i];  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
            g.conc = 0;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        }
    }
    /* no output */
    {
        SlSeparateOut g;
        sl_default_separate_out(&g);
        SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        SEP(rgb, n, h, w, d6, d2, 0, 0, &g);
        g.conc_dtype = SL_DTYPE_BF16;  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        VIEW(oh, ow, win, 7, 2, &g, &t);
    }
    /* two outputs at one address; an output at rgb */
    {
        SlSeparateOut g;
        g = f; g.stain[0] = g.norm;          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = g.norm;          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = g.stain[0];      SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.norm;              SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.stain[0];          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = g.stain[1];          SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.norm = rgb;                 SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[0] = rgb;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.stain[1] = rgb;             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g = f; g.conc = rgb;                 SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        sl_default_separate_out(&g); g.stain[1] = rgb;   SEP(rgb, n, h, w, d6, d2, 0, 0, &g);
        g = f; g.stain[0] = g.norm;          VIEW(oh, ow, win, 7, 1, &g, &t);          /* under a format too */
        g = f; g.norm = rgb;                 VIEW(oh, ow, win, 7, 1, &g, &t);
    }
    /* conc aligned to its element size */
    {
        SlSeparateOut g = f;
        g.conc = (char*)cc + 1;  g.conc_dtype = SL_DTYPE_F16;   SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc_dtype = SL_DTYPE_BF16;                            SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc_dtype = SL_DTYPE_F32;                             SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
        g.conc = (char*)cc + 2;                                  SEP(rgb, n, h, w, d6, d2, d6, d2, &g);
    }

    /* ---- what the view refuses (view_geometry) ---- */
    VIEW(oh, ow, 0, 7, 1, &f, 0);                        /* NULL windows */
    VIEW(0, ow, win, 7, 1, &f, 0);                       /* size */
    VIEW(oh, 0, win, 7, 1, &f, 0);
    VIEW(-1, ow, win, 7, 1, &f, 0);
    VIEW(h + 1, ow, win, 6, 1, &f, 0);
    VIEW(oh, w + 1, win, 6, 1, &f, 0);
    VIEW(h, w, win, 7, 1, &f, 0);                        /* 64 x 48 does not fit transposed in 64 x 48 */
    VIEW(49, 48, win, 1, 1, &f, 0);
    VIEW(oh, ow, win, -1, 1, &f, 0);                     /* d_mask */
    VIEW(oh, ow, win, 8, 1, &f, 0);
    {
        SlSeparateOut g = f;                             /* images only: a shrink is legal, these are not */
        g.conc = 0;
        VIEW(oh, ow, win, 7, 0, &g, 0);                  /* shrink */
        VIEW(oh, ow, win, 7, 3, &g, 0);
        VIEW(oh, ow, win, 7, 8, &g, 0);
        VIEW(oh, ow, win, 7, -2, &g, 0);
        VIEW(33, ow, win, 6, 2, &g, 0);                  /* 2 x 33 > 64 */
        VIEW(oh, 25, win, 6, 2, &g, 0);                  /* 2 x 25 > 48 */
        VIEW(17, 12, win, 6, 4, &g, 0);
        VIEW(oh, ow, win, 7, 2, &g, 0);                  /* 2 x 32 = 64 rows do not fit in 48 columns, transposed */
        VIEW(16, 13, win, 7, 4, &g, &t);
    }
    /* shrink != 1 with planes */
    VIEW(16, 12, win, 6, 2, &f, 0);
    VIEW(8, 8, win, 7, 4, &f, 0);
    VIEW(8, 8, win, 7, 2, &f, &t);
    {
        SlSeparateOut g;
        sl_default_separate_out(&g); g.conc = cc;        VIEW(8, 8, win, 7, 2, &g, 0);
    }
    /* more (tile, patch) pairs than a grid holds */
    SV(rgb, 2147483647, 128, 128, 65, 65, win, 7, 1, d6, d2, d6, d2, 0.01, &f, 0);

    /* ---- a bad format ---- */
    {
        SlTensorFormat u = t;
        u.struct_size = 0;                               VIEW(oh, ow, win, 7, 1, &f, &u);
        u.struct_size = sizeof(SlTensorFormat) + 8;      VIEW(oh, ow, win, 7, 1, &f, &u);
        void* blk = undersized(&t);
        VIEW(oh, ow, win, 7, 1, &f, (const SlTensorFormat*)blk);
        free(blk);
        u = t; u.dtype = -1;                             VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.dtype = 3;                              VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.layout = 2;                             VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.layout = -1;                            VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.std[1] = 0.0;                           VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.std[2] = -1.0;                          VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.std[0] = (double)NAN;                   VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.mean[0] = (double)INFINITY;             VIEW(oh, ow, win, 7, 1, &f, &u);
        u = t; u.mean[2] = (double)NAN;                  VIEW(oh, ow, win, 7, 1, &f, &u);
    }
    /* ---- an image pointer aligned to its element size ---- */
    {
        SlTensorFormat u = t;
        SlSeparateOut g;
        u.dtype = SL_DTYPE_F32;
        g = f; g.norm = o1 + 1;                          VIEW(oh, ow, win, 7, 1, &g, &u);
        g = f; g.stain[0] = o2 + 2;                      VIEW(oh, ow, win, 7, 1, &g, &u);
        g = f; g.stain[1] = o3 + 3;                      VIEW(oh, ow, win, 7, 1, &g, &u);
        u.dtype = SL_DTYPE_F16;
        g = f; g.norm = o1 + 1;                          VIEW(oh, ow, win, 7, 1, &g, &u);
        g = f; g.stain[0] = o2 + 1;                      VIEW(oh, ow, win, 7, 1, &g, &u);
        u.dtype = SL_DTYPE_BF16;
        g = f; g.stain[1] = o3 + 1;                      VIEW(oh, ow, win, 7, 1, &g, &u);
        sl_default_separate_out(&g); g.stain[1] = o3 + 1;  VIEW(oh, ow, win, 7, 2, &g, &u);
    }
    return report();
}
