/* Argument checks of the elastic views' entry points of the C ABI (include/stainlib_hip.h: sl_normalize_view_elastic,
 * sl_view_planes_elastic) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything is launched or
 * dereferenced, and an empty batch (n == 0) is SL_OK with nothing launched.  Built and run under AddressSanitizer by
 * `make -C stainlib_amd/csrc asan-elastic` (tests/test_view_elastic_host.py).  The data pointers are DEVICE pointers the host side never
 * reads through: the non-null ones below are deliberately wild -- the windows and the field too, which are clamped on the device and
 * never read back. */
#include "abi_argcheck.h"

#define Q 65536

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    int32_t* win = (int32_t*)0x300300;
    int32_t* fld = (int32_t*)0x500100;
    const double* st = (const double*)0x400000;              /* any statistic */
    const int n = 4, c = 3, h = 64, w = 48;
    SlParams prm;
    SlTensorFormat fmt;
    sl_default_params(&prm);
    sl_default_tensor_format(&fmt);
    EXPECT(sl_version(), SL_VERSION);

/* an image call on the raw route and on the jitter route, as the uint8 image and as a tensor */
#define IMG(rgb_, out_, n_, h_, w_, oh_, ow_, win_, mr_, fld_, k_, md_, fill_) do { \
        EXPECT(sl_normalize_view_elastic(rgb_, out_, n_, h_, w_, oh_, ow_, win_, mr_, fld_, k_, md_, fill_, 0, 0, 0, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_view_elastic(rgb_, out_, n_, h_, w_, oh_, ow_, win_, mr_, fld_, k_, md_, fill_, st, st, st, st, st, 1, &prm, &fmt, 0), SL_ERR_BADARG); } while (0)
/* a planes call at every element size */
#define PL(pl_, out_, n_, c_, h_, w_, oh_, ow_, win_, mr_, fld_, k_, md_) do { \
        const int eb_[] = {1, 2, 4, 8}; \
        for (int i_ = 0; i_ < 4; ++i_) \
            EXPECT(sl_view_planes_elastic(pl_, out_, n_, c_, h_, w_, eb_[i_], oh_, ow_, win_, mr_, fld_, k_, md_, 7, 0), SL_ERR_BADARG); } while (0)

    /* NULL pointers */
    IMG(0, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0);
    IMG(rgb, 0, n, h, w, 8, 8, win, Q, fld, 5, 4, 0);
    IMG(rgb, out, n, h, w, 8, 8, 0, Q, fld, 5, 4, 0);
    IMG(rgb, out, n, h, w, 8, 8, win, Q, 0, 5, 4, 0);
    PL(0, out, n, c, h, w, 8, 8, win, Q, fld, 5, 4);
    PL(rgb, 0, n, c, h, w, 8, 8, win, Q, fld, 5, 4);
    PL(rgb, out, n, c, h, w, 8, 8, 0, Q, fld, 5, 4);
    PL(rgb, out, n, c, h, w, 8, 8, win, Q, 0, 5, 4);
    /* a field that is not aligned to its int32 */
    for (int off = 1; off < 4; ++off) {
        IMG(rgb, out, n, h, w, 8, 8, win, Q, (int32_t*)((char*)fld + off), 5, 4, 0);
        PL(rgb, out, n, c, h, w, 8, 8, win, Q, (int32_t*)((char*)fld + off), 5, 4);
    }
    /* n < 0; c, h, w, oh, ow <= 0 */
    {
        const int bad[] = {0, -1, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            if (bad[i] < 0) {
                IMG(rgb, out, bad[i], h, w, 8, 8, win, Q, fld, 5, 4, 0);
                PL(rgb, out, bad[i], c, h, w, 8, 8, win, Q, fld, 5, 4);
            }
            IMG(rgb, out, n, bad[i], w, 8, 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, n, h, bad[i], 8, 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, n, h, w, bad[i], 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, n, h, w, 8, bad[i], win, Q, fld, 5, 4, 0);
            PL(rgb, out, n, bad[i], h, w, 8, 8, win, Q, fld, 5, 4);
            PL(rgb, out, n, c, bad[i], w, 8, 8, win, Q, fld, 5, 4);
            PL(rgb, out, n, c, h, bad[i], 8, 8, win, Q, fld, 5, 4);
            PL(rgb, out, n, c, h, w, bad[i], 8, win, Q, fld, 5, 4);
            PL(rgb, out, n, c, h, w, 8, bad[i], win, Q, fld, 5, 4);
        }
    }
    /* h, w, oh, ow > 8192: the coordinates would leave 32 bits */
    {
        const int bad[] = {8193, 16384, 65536, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            IMG(rgb, out, 1, bad[i], w, 8, 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, 1, h, bad[i], 8, 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, 1, h, w, bad[i], 8, win, Q, fld, 5, 4, 0);
            IMG(rgb, out, 1, h, w, 8, bad[i], win, Q, fld, 5, 4, 0);
            PL(rgb, out, 1, 1, bad[i], w, 8, 8, win, Q, fld, 5, 4);
            PL(rgb, out, 1, 1, h, bad[i], 8, 8, win, Q, fld, 5, 4);
            PL(rgb, out, 1, 1, h, w, bad[i], 8, win, Q, fld, 5, 4);
            PL(rgb, out, 1, 1, h, w, 8, bad[i], win, Q, fld, 5, 4);
        }
    }
    /* max_r outside [1, 2 Q] */
    {
        const int bad[] = {0, -1, 2 * Q + 1, 4 * Q, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            IMG(rgb, out, n, h, w, 8, 8, win, bad[i], fld, 5, 4, 0);
            PL(rgb, out, n, c, h, w, 8, 8, win, bad[i], fld, 5, 4);
        }
    }
    /* cell_log2 outside 4 .. 8 */
    {
        const int bad[] = {3, 0, -1, 9, 16, 31, 32, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            IMG(rgb, out, n, h, w, 8, 8, win, Q, fld, bad[i], 4, 0);
            PL(rgb, out, n, c, h, w, 8, 8, win, Q, fld, bad[i], 4);
        }
    }
    /* max_d outside 0 .. 8 */
    {
        const int bad[] = {-1, 9, 31, 32, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            IMG(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, bad[i], 0);
            PL(rgb, out, n, c, h, w, 8, 8, win, Q, fld, 5, bad[i]);
        }
    }
    /* fill_rgb >= 2^24 */
    IMG(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0x1000000u);
    IMG(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0x80000000u);
    IMG(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0xffffffffu);
    /* elem_bytes; planes or out not aligned to it */
    {
        const int bad[] = {0, -1, 3, 5, 6, 7, 9, 16, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i)
            EXPECT(sl_view_planes_elastic(rgb, out, n, c, h, w, bad[i], 8, 8, win, Q, fld, 5, 4, 0, 0), SL_ERR_BADARG);
        const int eb[] = {2, 4, 8};
        for (int i = 0; i < 3; ++i)
            for (int off = 1; off < eb[i]; ++off) {
                EXPECT(sl_view_planes_elastic((char*)rgb + off, out, n, c, h, w, eb[i], 8, 8, win, Q, fld, 5, 4, 0, 0), SL_ERR_BADARG);
                EXPECT(sl_view_planes_elastic(rgb, (char*)out + off, n, c, h, w, eb[i], 8, 8, win, Q, fld, 5, 4, 0, 0), SL_ERR_BADARG);
            }
    }
    /* the statistics pattern, params and fmt: sl_normalize_view's rules */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, st, 0, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);      /* maxC_src without M_src */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, st, st, 0, 0, 0, 0, 0), SL_ERR_BADARG);     /* a target without M_src */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, st, 0, 0, 0, 0), SL_ERR_BADARG);      /* alpha_beta without M_src */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, st, 0, st, st, 0, 0, 0, 0, 0), SL_ERR_BADARG);    /* M_src without maxC_src */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, st, st, st, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);    /* a one-sided target */
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, st, st, 0, st, 0, 0, 0, 0, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, st, st, 0, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);     /* apply has no "no target" */
    {
        SlParams* small = (SlParams*)undersized(&prm);
        EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, st, st, st, st, st, 0, small, 0, 0), SL_ERR_BADARG);
        free(small);
        SlTensorFormat* fsmall = (SlTensorFormat*)undersized(&fmt);
        EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, fsmall, 0), SL_ERR_BADARG);
        free(fsmall);
        SlTensorFormat f2 = fmt;
        f2.dtype = 3;
        EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, &f2, 0), SL_ERR_BADARG);
        f2 = fmt;
        f2.layout = 2;
        EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, &f2, 0), SL_ERR_BADARG);
        f2 = fmt;
        f2.std[1] = 0.0;
        EXPECT(sl_normalize_view_elastic(rgb, out, n, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, &f2, 0), SL_ERR_BADARG);
    }
    /* more (tile, patch) / (plane, patch) pairs than 2^31 - 1: a patch is 63 outputs square at the identity with max_d = 0, 47 with
     * max_d = 8, 24 at 2 Q with max_d = 8 */
    IMG(rgb, out, 2147483647, 8, 8, 65, 65, win, Q, fld, 5, 0, 0);               /* 4 patches each */
    IMG(rgb, out, 1073741824, 8, 8, 48, 48, win, Q, fld, 5, 8, 0);               /* 2^30 tiles x 4 patches of 47 */
    IMG(rgb, out, 1073741824, 8, 8, 25, 25, win, 2 * Q, fld, 5, 8, 0);           /* 2^30 tiles x 4 patches of 24 */
    IMG(rgb, out, 131072, 8, 8, 8192, 8192, win, Q / 2, fld, 4, 0, 0);           /* 2^17 tiles x 2^14 patches */
    PL(rgb, out, 65536, 32768, h, w, 8, 8, win, Q, fld, 5, 4);                   /* n c = 2^31 */
    PL(rgb, out, 2147483647, 2147483647, h, w, 8, 8, win, Q, fld, 5, 4);
    PL(rgb, out, 32768, 32768, 8, 8, 48, 48, win, Q, fld, 5, 8);                 /* 2^30 planes x 4 patches */
    PL(rgb, out, 1073741824, 1, 8, 8, 25, 25, win, 2 * Q, fld, 5, 8);
    /* an empty batch is fine and launches nothing -- but only a call that is right otherwise */
    EXPECT(sl_normalize_view_elastic(rgb, out, 0, h, w, 8, 8, win, Q, fld, 5, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), SL_OK);
    EXPECT(sl_normalize_view_elastic(rgb, out, 0, h, w, 8, 8, win, Q, fld, 4, 0, 0xffffff, st, st, st, st, st, 1, &prm, &fmt, 0), SL_OK);
    EXPECT(sl_view_planes_elastic(rgb, out, 0, c, h, w, 8, 8, 8, win, Q, fld, 8, 8, 0, 0), SL_OK);
    IMG(rgb, out, 0, h, w, 8, 8, win, Q, fld, 3, 4, 0);
    IMG(rgb, out, 0, h, w, 8, 8, win, Q, 0, 5, 4, 0);
    PL(rgb, out, 0, c, h, w, 8, 8, win, Q, fld, 5, 9);
    return report();
}
