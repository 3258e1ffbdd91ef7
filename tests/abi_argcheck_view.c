/* Argument checks of the crop / flip / rot90 entry point of the C ABI (include/stainlib_hip.h: sl_normalize_view) on the HOST side, no
 * GPU needed: every refused call must return SL_ERR_BADARG before anything is launched or dereferenced.  Built and run under
 * AddressSanitizer by `make -C stainlib_amd/csrc asan-view` (tests/test_view_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlParams and SlTensorFormat are host pointers: the undersized copies below sit at the very end of their heap blocks, so a library
 * that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

#define VIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) \
        EXPECT(sl_normalize_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, 0), SL_ERR_BADARG)
/* a refusal of the geometry on every route (jitter with a target, jitter under the tile's own matrix, apply, the source bytes), with and
 * without a format and an SlParams */
#define GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_) do { \
        VIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, d6, d2, ab, 0, 0, 0); VIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, 0, 0, ab, 1, &p, &f); \
        VIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, d6, d2, 0, 0, &p, 0); VIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 0, 0, 0, 0, 0, 0, 0, &f); } while (0)

    /* required pointers */
    GEOM(0, out, n, h, w, oh, ow, win, 7);
    GEOM(rgb, 0, n, h, w, oh, ow, win, 7);
    GEOM(rgb, out, n, h, w, oh, ow, 0, 7);
    /* shapes */
    GEOM(rgb, out, 0, h, w, oh, ow, win, 7);
    GEOM(rgb, out, -1, h, w, oh, ow, win, 7);
    GEOM(rgb, out, n, 0, w, oh, ow, win, 7);
    GEOM(rgb, out, n, h, -5, oh, ow, win, 7);
    GEOM(rgb, out, n, 65536, 65536, oh, ow, win, 7);      /* more than 2^30 pixels */
    GEOM(rgb, out, n, 32768, 32769, oh, ow, win, 6);      /* just over */
    /* the output size */
    GEOM(rgb, out, n, h, w, 0, ow, win, 7);
    GEOM(rgb, out, n, h, w, oh, 0, win, 7);
    GEOM(rgb, out, n, h, w, -1, -1, win, 0);
    GEOM(rgb, out, n, h, w, h + 1, ow, win, 6);
    GEOM(rgb, out, n, h, w, oh, w + 1, win, 6);
    GEOM(rgb, out, n, h, w, 2147483647, 2147483647, win, 0);
    /* the mask */
    GEOM(rgb, out, n, h, w, oh, ow, win, -1);
    GEOM(rgb, out, n, h, w, oh, ow, win, 8);
    GEOM(rgb, out, n, h, w, oh, ow, win, -2147483647 - 1);
    /* quarter turns: the transposed window must fit too (64 x 48 does not fit into 64 x 48 turned) */
    GEOM(rgb, out, n, h, w, h, w, win, 7);
    GEOM(rgb, out, n, h, w, h, w, win, 1);
    GEOM(rgb, out, n, h, w, w + 1, w, win, 5);
    GEOM(rgb, out, n, w, h, oh, h, win, 3);                /* a 48 x 64 tile, 40 x 64 out: ow > h */
    /* more (tile, patch) pairs than a grid holds */
    GEOM(rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 7);
    /* the statistics */
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, 0, d6, d2, ab, 0, 0, 0);         /* M_src without maxC_src */
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, d2, ab, 0, 0, 0);         /* a one-sided target */
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, 0, ab, 0, 0, &f);
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, 0, 0, 0, 0);           /* the apply route has no "no target" */
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, d2, 0, 0, 0, 0, 0, 0);            /* the source bytes: nothing else may be given */
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, d6, d2, 0, 0, 0, 0);
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, ab, 1, &p, &f);
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, d6, 0, 0, 0, 0, 0);
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, d2, 0, 0, 0, 0);
    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, d2, d6, d2, ab, 0, 0, 0);
    /* SlParams.struct_size, two_sweep */
    {
        SlParams q = p;
        q.struct_size = 0;                         VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, &q, 0);
        q.struct_size = sizeof(SlParams) - 8;      VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, 0, 0, &q, &f);
        q.struct_size = sizeof(SlParams) + 8;      VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, &q, 0);
        q = p; q.two_sweep = 9;                    VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, ab, 1, &q, 0);
        void* blk = undersized(&p);
        VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0);
        VIEW(rgb, out, n, h, w, oh, ow, win, 6, 0, 0, 0, 0, 0, 0, (const SlParams*)blk, &f);
        free(blk);
    }
    /* SlTensorFormat: struct_size, dtype, layout, std, non-finite values (the checks of sl_to_tensor) */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                               VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, 0, 0, &p, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
        void* blk = undersized(&f);
        VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, (const SlTensorFormat*)blk);
        VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, (const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.layout = bad[i];                    VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = -1.0;                      VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, 0, 0, 0, &g);
            g = f; g.std[c] = NAN;                       VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
            g = f; g.std[c] = INFINITY;                  VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, ab, 1, &p, &g);
            g = f; g.mean[c] = NAN;                      VIEW(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.mean[c] = -INFINITY;                VIEW(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
        }
    }
    return report();
}
