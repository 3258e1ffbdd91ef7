/* Argument checks of the Lab family's view entry points of the C ABI (include/stainlib_hip.h: sl_reinhard_view, sl_luminosity_view,
 * sl_slab_view) on the HOST side, no GPU needed: every refused call must return its error code before anything is enqueued or
 * dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-labview` (tests/test_lab_view_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlTensorFormat is a host pointer: the undersized copy below sits at the very end of its heap block, so a library that read a caller's
 * struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* tm = (double*)0x300000;    double* ts = (double*)0x300100;    double* st = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    double* state = (double*)0x400000;
    void* ws = (void*)0x500000;
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    const size_t wsb = sl_workspace_bytes(SL_OP_LAB_STATS, n, h, w);
    SlTensorFormat f;
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);
    EXPECT(wsb > 0, 1);

#define RV(want_, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, tm_, ts_, ws_, wsb_, f_) \
        EXPECT(sl_reinhard_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, tm_, ts_, 1, 0.8, st, ws_, wsb_, f_, 0), want_)
#define LV(want_, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ws_, wsb_, f_) \
        EXPECT(sl_luminosity_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 95.0, st, ws_, wsb_, f_, 0), want_)
#define SV(want_, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, state_, mode_, f_) \
        EXPECT(sl_slab_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, state_, mode_, 1, 0.8, f_, 0), want_)
/* a refusal every entry point shares, with and without a format, in both pooled modes */
#define ALL(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_) do { \
        RV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, tm, ts, ws, wsb, 0); RV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, tm, ts, ws, wsb, &f); \
        LV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ws, wsb, 0);         LV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ws, wsb, &f); \
        SV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, state, 0, 0);        SV(SL_ERR_BADARG, rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, state, 1, &f); } while (0)

    /* required pointers; out == rgb */
    ALL(0, out, n, h, w, oh, ow, win, 7);
    ALL(rgb, 0, n, h, w, oh, ow, win, 7);
    ALL(rgb, out, n, h, w, oh, ow, 0, 7);
    ALL(rgb, (void*)rgb, n, h, w, oh, ow, win, 7);
    /* shapes (n == 0 is an empty shard for sl_slab_view: below) */
    ALL(rgb, out, -1, h, w, oh, ow, win, 7);
    ALL(rgb, out, n, 0, w, oh, ow, win, 7);
    ALL(rgb, out, n, h, -5, oh, ow, win, 7);
    ALL(rgb, out, n, 65536, 65536, oh, ow, win, 7);      /* more than 2^30 pixels */
    ALL(rgb, out, n, 32768, 32769, oh, ow, win, 6);      /* just over */
    RV(SL_ERR_BADARG, rgb, out, 0, h, w, oh, ow, win, 7, tm, ts, ws, wsb, 0);
    LV(SL_ERR_BADARG, rgb, out, 0, h, w, oh, ow, win, 7, ws, wsb, &f);
    SV(SL_ERR_BADARG, rgb, out, 1 << 11, 32768, 32768, oh, ow, win, 7, state, 0, 0);      /* a shard of more than 2^40 pixels */
    /* the output size */
    ALL(rgb, out, n, h, w, 0, ow, win, 7);
    ALL(rgb, out, n, h, w, oh, 0, win, 7);
    ALL(rgb, out, n, h, w, -1, -1, win, 0);
    ALL(rgb, out, n, h, w, h + 1, ow, win, 6);
    ALL(rgb, out, n, h, w, oh, w + 1, win, 6);
    ALL(rgb, out, n, h, w, 2147483647, 2147483647, win, 0);
    /* the mask */
    ALL(rgb, out, n, h, w, oh, ow, win, -1);
    ALL(rgb, out, n, h, w, oh, ow, win, 8);
    ALL(rgb, out, n, h, w, oh, ow, win, -2147483647 - 1);
    /* quarter turns: the transposed window must fit too (64 x 48 does not fit into 64 x 48 turned) */
    ALL(rgb, out, n, h, w, h, w, win, 7);
    ALL(rgb, out, n, h, w, h, w, win, 1);
    ALL(rgb, out, n, h, w, w + 1, w, win, 5);
    ALL(rgb, out, n, w, h, oh, h, win, 3);                /* a 48 x 64 tile, 40 x 64 out: ow > h */
    /* more (tile, patch) pairs than a grid holds (behind the workspace check; a shard of at most 2^40 pixels cannot get there) */
    RV(SL_ERR_BADARG, rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 6, tm, ts, ws, (size_t)-1, 0);
    LV(SL_ERR_BADARG, rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 6, ws, (size_t)-1, &f);
    /* the workspace of the per-tile calls */
    RV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, tm, ts, 0, wsb, 0);
    RV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, tm, ts, ws, wsb - 1, &f);
    RV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, tm, ts, (char*)ws + 4, wsb, 0);
    LV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, 0, wsb, 0);
    LV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, ws, 0, &f);
    LV(SL_ERR_WORKSPACE, rgb, out, n, h, w, oh, ow, win, 7, (char*)ws + 1, wsb, 0);
    /* the targets */
    RV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, 0, ts, ws, wsb, 0);
    RV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, tm, 0, ws, wsb, &f);
    RV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, 0, 0, ws, wsb, 0);
    /* the state and the mode */
    SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0);
    SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, 0, 1, &f);
    SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, state, -1, 0);
    SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, state, 2, &f);
    SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, state, 2147483647, 0);
    /* an empty shard: SL_OK, nothing launched, no data pointer needed -- but the rest is still checked */
    SV(SL_OK, 0, 0, 0, h, w, oh, ow, 0, 7, state, 0, 0);
    SV(SL_OK, rgb, out, 0, h, w, oh, ow, win, 6, state, 1, &f);
    SV(SL_ERR_BADARG, 0, 0, 0, h, w, oh, ow, 0, 7, 0, 0, 0);
    SV(SL_ERR_BADARG, 0, 0, 0, h, w, oh, ow, 0, 7, state, 3, 0);
    SV(SL_ERR_BADARG, 0, 0, 0, h, w, h + 1, ow, 0, 6, state, 0, 0);
    SV(SL_ERR_BADARG, 0, 0, 0, h, w, oh, ow, 0, 9, state, 0, 0);
    /* SlTensorFormat: struct_size, dtype, layout, std, non-finite values (the checks of sl_to_tensor) */
    {
#define FMT(g_) do { RV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, tm, ts, ws, wsb, g_); LV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, ws, wsb, g_); \
        SV(SL_ERR_BADARG, rgb, out, n, h, w, oh, ow, win, 7, state, 0, g_); SV(SL_ERR_BADARG, 0, 0, 0, h, w, oh, ow, 0, 7, state, 1, g_); } while (0)
        SlTensorFormat g = f;
        g.struct_size = 0;                               FMT(&g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      FMT(&g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      FMT(&g);
        void* blk = undersized(&f);
        FMT((const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     FMT(&g);
            g = f; g.layout = bad[i];                    FMT(&g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       FMT(&g);
            g = f; g.std[c] = -1.0;                      FMT(&g);
            g = f; g.std[c] = NAN;                       FMT(&g);
            g = f; g.std[c] = INFINITY;                  FMT(&g);
            g = f; g.mean[c] = NAN;                      FMT(&g);
            g = f; g.mean[c] = -INFINITY;                FMT(&g);
        }
    }
    return report();
}
