/* Argument checks of the resizing-view entry points of the C ABI (include/stainlib_hip.h: sl_normalize_view_resize,
 * sl_normalize_hed_view_resize) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything is launched
 * or dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-resize` (tests/test_view_resize_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild -- the windows
 * too, whose sides are clamped on the device and never read back. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    double* sg = (double*)0x300400;    int32_t* ap = (int32_t*)0x300500;
    const int n = 4, h = 64, w = 48;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

/* one call of each export (the view's on two routes) */
#define NV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, f_) do { \
        EXPECT(sl_normalize_view_resize(rgb_, out_, n, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, d6, d2, d6, d2, ab, 0, &p, f_, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_view_resize(rgb_, out_, n, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, 0, 0, 0, 0, 0, 0, 0, f_, 0), SL_ERR_BADARG); } while (0)
#define HV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, f_) \
        EXPECT(sl_normalize_hed_view_resize(rgb_, out_, n, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, d6, d2, d6, d2, 0, 0, 0, f_, sg, sg, ap, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG)
#define ALL(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_) do { \
        NV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, 0); NV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, &f); \
        HV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, 0); HV(rgb_, out_, h_, w_, oh_, ow_, win_, dm_, mh_, mw_, &f); } while (0)

    /* max_wh outside [1, h], max_ww outside [1, w] */
    {
        const int bad[] = {0, -1, -64, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            ALL(rgb, out, h, w, 8, 8, win, 7, bad[i], 8);
            ALL(rgb, out, h, w, 8, 8, win, 7, 8, bad[i]);
            ALL(rgb, out, h, w, 8, 8, win, 0, bad[i], bad[i]);
        }
    }
    ALL(rgb, out, h, w, 8, 8, win, 7, 65, 48);
    ALL(rgb, out, h, w, 8, 8, win, 7, 64, 49);
    ALL(rgb, out, h, w, 8, 8, win, 6, 48, 64);           /* the bound is in the TILE's orientation, whatever the mask */
    /* max_wh max_ww > 2^22 (tiles that hold such a window) */
    ALL(rgb, out, 4096, 4096, 224, 224, win, 7, 2049, 2048);
    ALL(rgb, out, 4096, 4096, 224, 224, win, 7, 4096, 1025);
    ALL(rgb, out, 4096, 4096, 224, 224, win, 0, 4096, 4096);
    ALL(rgb, out, 16384, 16384, 1024, 1024, win, 0, 16384, 16384);      /* the product overflows an int: refused, not wrapped */
    /* the output size: below 1; an output side times a window side above 2^30 */
    ALL(rgb, out, h, w, 0, 8, win, 7, 8, 8);
    ALL(rgb, out, h, w, 8, 0, win, 7, 8, 8);
    ALL(rgb, out, h, w, -1, -1, win, 0, 8, 8);
    ALL(rgb, out, h, w, 2147483647, 8, win, 0, 64, 48);
    ALL(rgb, out, h, w, 8, 33554432, win, 6, 64, 48);    /* 2^25 x 64 */
    /* what the parents refuse: the pointers, the mask */
    ALL(0, out, h, w, 8, 8, win, 7, 8, 8);
    ALL(rgb, 0, h, w, 8, 8, win, 7, 8, 8);
    ALL(rgb, out, h, w, 8, 8, 0, 7, 8, 8);
    ALL(rgb, out, h, w, 8, 8, win, 8, 8, 8);
    ALL(rgb, out, h, w, 8, 8, win, -1, 8, 8);
    ALL(rgb, out, 0, w, 8, 8, win, 7, 8, 8);
    ALL(rgb, out, h, -3, 8, 8, win, 7, 8, 8);
    /* the rest of each parent's arguments, once each */
    EXPECT(sl_normalize_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, d6, 0, d6, d2, ab, 0, 0, 0, 0), SL_ERR_BADARG);        /* M_src without maxC_src */
    EXPECT(sl_normalize_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, ab, 0, 0, &f, 0), SL_ERR_BADARG);          /* alpha_beta without M_src */
    EXPECT(sl_normalize_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, d6, d2, d6, 0, 0, 0, 0, 0, 0), SL_ERR_BADARG);         /* M_tgt without maxC_tgt */
    EXPECT(sl_normalize_hed_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, sg, ap, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0, sg, 0, ap, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, 0, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, ap, SL_HED_SKIMAGE_019, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, ap, -1, 0), SL_ERR_BADARG);
    {
        SlTensorFormat bad = f;
        bad.dtype = 99;
        EXPECT(sl_normalize_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, &bad, 0), SL_ERR_BADARG);
        void* small = undersized(&f);
        EXPECT(sl_normalize_view_resize(rgb, out, n, h, w, 8, 8, win, 7, 8, 8, 0, 0, 0, 0, 0, 0, 0, (const SlTensorFormat*)small, 0), SL_ERR_BADARG);
        free(small);
    }
    return report();
}
