/* Argument checks of the box-shrink entry points of the C ABI (include/stainlib_hip.h: sl_normalize_view_shrink,
 * sl_normalize_hed_view_shrink, sl_reinhard_view_shrink, sl_luminosity_view_shrink, sl_slab_view_shrink) on the HOST side, no GPU needed:
 * every refused call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under AddressSanitizer by
 * `make -C stainlib_amd/csrc asan-shrink` (tests/test_view_shrink_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.  What the
 * parents refuse of everything else (routes, params, formats, workspaces) is their own drivers' business: the shrink exports are the
 * parents' code, which forward to them with shrink = 1. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    double* sg = (double*)0x300400;    int32_t* ap = (int32_t*)0x300500;  double* st = (double*)0x300600;
    double* state = (double*)0x400000;
    void* ws = (void*)0x500000;
    const int n = 4, h = 64, w = 48;
    const size_t wsb = sl_workspace_bytes(SL_OP_LAB_STATS, n, h, w);
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);
    EXPECT(wsb > 0, 1);

/* one call of each of the five exports (the view's on two routes), with and without a format */
#define NV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) do { \
        EXPECT(sl_normalize_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, d6, d2, d6, d2, ab, 0, &p, f_, 0), SL_ERR_BADARG); \
        EXPECT(sl_normalize_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, 0, 0, 0, 0, 0, 0, 0, f_, 0), SL_ERR_BADARG); } while (0)
#define HV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) \
        EXPECT(sl_normalize_hed_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, d6, d2, d6, d2, 0, 0, 0, f_, sg, sg, ap, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG)
#define RV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) \
        EXPECT(sl_reinhard_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, d6, d6, 1, 0.8, st, ws, wsb, f_, 0), SL_ERR_BADARG)
#define LV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) \
        EXPECT(sl_luminosity_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, 95.0, st, ws, wsb, f_, 0), SL_ERR_BADARG)
#define SV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) do { \
        EXPECT(sl_slab_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, state, 0, 1, 0.8, f_, 0), SL_ERR_BADARG); \
        EXPECT(sl_slab_view_shrink(rgb_, out_, n, h, w, oh_, ow_, win_, dm_, s_, state, 1, 0, 0.8, f_, 0), SL_ERR_BADARG); } while (0)
#define ALL5(rgb_, out_, oh_, ow_, win_, dm_, s_, f_) do { NV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_); HV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_); \
        RV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_); LV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_); SV(rgb_, out_, oh_, ow_, win_, dm_, s_, f_); } while (0)
#define ALL(rgb_, out_, oh_, ow_, win_, dm_, s_) do { ALL5(rgb_, out_, oh_, ow_, win_, dm_, s_, 0); ALL5(rgb_, out_, oh_, ow_, win_, dm_, s_, &f); } while (0)

    /* shrink is 1, 2 or 4 (sizes that fit under every one of them) */
    {
        const int bad[] = {0, 3, 5, 8, 16, -1, -2, -4, 2147483647, -2147483647 - 1};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            ALL(rgb, out, 8, 8, win, 7, bad[i]);
            ALL(rgb, out, 1, 1, win, 0, bad[i]);
        }
    }
    /* s oh > h, s ow > w: each fits at the shrink below (64 x 48 tiles, no quarter turns) */
    ALL(rgb, out, 33, 24, win, 6, 2);          /* 66 x 48 */
    ALL(rgb, out, 32, 25, win, 6, 2);          /* 64 x 50 */
    ALL(rgb, out, 17, 12, win, 6, 4);          /* 68 x 48 */
    ALL(rgb, out, 16, 13, win, 6, 4);          /* 64 x 52 */
    ALL(rgb, out, 64, 48, win, 0, 2);          /* the full tile is a shrink = 1 view only */
    ALL(rgb, out, 32, 24, win, 0, 4);
    ALL(rgb, out, 2147483647, 1, win, 0, 2);   /* s oh overflows an int: refused, not wrapped */
    ALL(rgb, out, 1, 1073741824, win, 0, 4);
    ALL(rgb, out, 1073741824, 1073741824, win, 0, 4);
    /* d_mask & 1: the transposed window must fit too */
    ALL(rgb, out, 32, 24, win, 7, 2);          /* 64 x 48 turned is 48 x 64: does not fit in 64 x 48 */
    ALL(rgb, out, 32, 24, win, 1, 2);
    ALL(rgb, out, 25, 24, win, 3, 2);          /* 50 x 48 fits; 48 x 50 does not */
    ALL(rgb, out, 13, 12, win, 5, 4);          /* 52 x 48 fits; 48 x 52 does not */
    ALL(rgb, out, 16, 8, win, 7, 4);           /* 64 x 32 fits; 32 x 64 fits in height, 64 > 48 in width */
    /* what the parents refuse is refused under a shrink too: the pointers, the output size, the mask */
    ALL(0, out, 8, 8, win, 7, 2);
    ALL(rgb, 0, 8, 8, win, 7, 4);
    ALL(rgb, out, 8, 8, 0, 7, 2);
    ALL(rgb, out, 0, 8, win, 7, 2);
    ALL(rgb, out, 8, 0, win, 7, 4);
    ALL(rgb, out, -1, -1, win, 0, 2);
    ALL(rgb, out, 8, 8, win, 8, 2);
    ALL(rgb, out, 8, 8, win, -1, 4);
    /* out == rgb (the Lab family refuses it by name) */
    RV(rgb, (void*)rgb, 8, 8, win, 7, 2, 0);
    LV(rgb, (void*)rgb, 8, 8, win, 7, 4, &f);
    SV(rgb, (void*)rgb, 8, 8, win, 7, 2, 0);
    /* the rest of each parent's arguments, once each under a shrink */
    EXPECT(sl_normalize_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, d6, 0, d6, d2, ab, 0, 0, 0, 0), SL_ERR_BADARG);        /* M_src without maxC_src */
    EXPECT(sl_normalize_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 4, 0, 0, 0, 0, ab, 0, 0, &f, 0), SL_ERR_BADARG);          /* alpha_beta without M_src */
    EXPECT(sl_normalize_hed_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, sg, ap, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, 0, SL_HED_SKIMAGE_018, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 4, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, ap, SL_HED_SKIMAGE_019, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 4, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, ap, SL_HED_EXPERIMENTAL_LOG10 + 1, 0), SL_ERR_BADARG);
    EXPECT(sl_normalize_hed_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, 0, 0, 0, 0, 0, 0, 0, 0, sg, sg, ap, -1, 0), SL_ERR_BADARG);
    EXPECT(sl_reinhard_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, 0, d6, 1, 0.8, st, ws, wsb, 0, 0), SL_ERR_BADARG);       /* no target means */
    EXPECT(sl_reinhard_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, d6, d6, 1, 0.8, st, 0, wsb, 0, 0), SL_ERR_WORKSPACE);
    EXPECT(sl_luminosity_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 4, 95.0, st, ws, wsb - 1, &f, 0), SL_ERR_WORKSPACE);
    EXPECT(sl_slab_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 2, 0, 0, 1, 0.8, 0, 0), SL_ERR_BADARG);                        /* no state */
    EXPECT(sl_slab_view_shrink(rgb, out, n, h, w, 8, 8, win, 7, 4, state, 2, 1, 0.8, 0, 0), SL_ERR_BADARG);                    /* the mode */
    /* an empty pooled shard: SL_OK and nothing launched -- with a legal shrink only */
    EXPECT(sl_slab_view_shrink(0, 0, 0, h, w, 8, 8, 0, 7, 2, state, 0, 0, 0.8, 0, 0), SL_OK);
    EXPECT(sl_slab_view_shrink(0, 0, 0, h, w, 16, 12, 0, 6, 4, state, 1, 0, 0.8, &f, 0), SL_OK);
    EXPECT(sl_slab_view_shrink(0, 0, 0, h, w, 8, 8, 0, 7, 3, state, 0, 0, 0.8, 0, 0), SL_ERR_BADARG);
    EXPECT(sl_slab_view_shrink(0, 0, 0, h, w, 33, 24, 0, 6, 2, state, 0, 0, 0.8, 0, 0), SL_ERR_BADARG);
    return report();
}
