/* Argument checks of the two entry points of HED augmentation behind the apply pass (include/stainlib_hip.h: sl_normalize_sums,
 * sl_normalize_hed_view) on the HOST side, no GPU needed: every refused call must return SL_ERR_BADARG before anything is launched or
 * dereferenced.  Built and run under AddressSanitizer by `make -C stainlib_amd/csrc asan-hedview` (tests/test_hed_view_host.py).
 * The data pointers are DEVICE pointers the host side never reads through: the non-null ones below are deliberately wild.
 * SlParams and SlTensorFormat are host pointers: the undersized copies below sit at the very end of their heap blocks, so a library
 * that read a caller's struct before checking struct_size would be caught reading past it. */
#include "abi_argcheck.h"

int main(void) {
    uint8_t* rgb = (uint8_t*)0x100000;
    void* out = (void*)0x200000;
    double* d6 = (double*)0x300000;    double* d2 = (double*)0x300100;    double* ab = (double*)0x300200;
    int32_t* win = (int32_t*)0x300300;
    double* sg = (double*)0x300400;    double* bs = (double*)0x300500;
    int32_t* ap = (int32_t*)0x300600;
    uint64_t* sums = (uint64_t*)0x300700;
    const int n = 4, h = 64, w = 48, oh = 40, ow = 32;
    SlParams p;
    SlTensorFormat f;
    sl_default_params(&p);
    sl_default_tensor_format(&f);
    EXPECT(sl_version(), SL_VERSION);

    /* ---- sl_normalize_sums ---- */
#define SUMS(rgb_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, bg_, p_, lo_, hi_, sums_, ap_) \
        EXPECT(sl_normalize_sums(rgb_, n_, h_, w_, ms_, cs_, mt_, ct_, ab_, bg_, p_, lo_, hi_, sums_, ap_, 0), SL_ERR_BADARG)
/* a refusal of the shape, the sums or the cutoff on every route (jitter with a target, jitter under the tile's own matrix, apply, the
 * source bytes), with and without applied and an SlParams */
#define SGEOM(rgb_, n_, h_, w_, lo_, hi_, sums_) do { \
        SUMS(rgb_, n_, h_, w_, d6, d2, d6, d2, ab, 0, 0, lo_, hi_, sums_, ap); SUMS(rgb_, n_, h_, w_, d6, d2, 0, 0, ab, 1, &p, lo_, hi_, sums_, 0); \
        SUMS(rgb_, n_, h_, w_, d6, d2, d6, d2, 0, 0, &p, lo_, hi_, sums_, ap); SUMS(rgb_, n_, h_, w_, 0, 0, 0, 0, 0, 0, 0, lo_, hi_, sums_, 0); } while (0)
    SGEOM(0, n, h, w, 0.05, 0.95, sums);
    SGEOM(rgb, n, h, w, 0.05, 0.95, 0);
    SGEOM(rgb, n, h, w, 0.05, 0.95, (uint64_t*)0x300704);      /* not 8-byte aligned */
    SGEOM(rgb, 0, h, w, 0.05, 0.95, sums);
    SGEOM(rgb, -1, h, w, 0.05, 0.95, sums);
    SGEOM(rgb, n, 0, w, 0.05, 0.95, sums);
    SGEOM(rgb, n, h, -5, 0.05, 0.95, sums);
    SGEOM(rgb, n, 65536, 65536, 0.05, 0.95, sums);              /* more than 2^30 pixels */
    SGEOM(rgb, n, 32768, 32769, 0.05, 0.95, sums);              /* just over */
    SGEOM(rgb, n, h, w, 0.95, 0.05, sums);                      /* lo > hi */
    SGEOM(rgb, n, h, w, NAN, 0.95, sums);
    SGEOM(rgb, n, h, w, 0.05, NAN, sums);
    SGEOM(rgb, n, h, w, INFINITY, -INFINITY, sums);
    /* the statistics */
    SUMS(rgb, n, h, w, d6, 0, d6, d2, ab, 0, 0, 0.05, 0.95, sums, ap);           /* M_src without maxC_src */
    SUMS(rgb, n, h, w, d6, d2, 0, d2, ab, 0, 0, 0.05, 0.95, sums, ap);           /* a one-sided target */
    SUMS(rgb, n, h, w, d6, d2, d6, 0, ab, 0, 0, 0.05, 0.95, sums, 0);
    SUMS(rgb, n, h, w, d6, d2, 0, 0, 0, 0, 0, 0.05, 0.95, sums, ap);             /* the apply route has no "no target" */
    SUMS(rgb, n, h, w, 0, d2, 0, 0, 0, 0, 0, 0.05, 0.95, sums, ap);              /* the source bytes: nothing else may be given */
    SUMS(rgb, n, h, w, 0, 0, d6, d2, 0, 0, 0, 0.05, 0.95, sums, ap);
    SUMS(rgb, n, h, w, 0, 0, 0, 0, ab, 1, &p, -INFINITY, INFINITY, sums, ap);
    SUMS(rgb, n, h, w, 0, d2, d6, d2, ab, 0, 0, 0.05, 0.95, sums, ap);
    {
        SlParams q = p;
        q.struct_size = 0;                         SUMS(rgb, n, h, w, d6, d2, d6, d2, ab, 0, &q, 0.05, 0.95, sums, ap);
        q.struct_size = sizeof(SlParams) - 8;      SUMS(rgb, n, h, w, d6, d2, d6, d2, 0, 0, &q, 0.05, 0.95, sums, ap);
        q.struct_size = sizeof(SlParams) + 8;      SUMS(rgb, n, h, w, 0, 0, 0, 0, 0, 0, &q, 0.05, 0.95, sums, 0);
        q = p; q.two_sweep = 9;                    SUMS(rgb, n, h, w, d6, d2, 0, 0, ab, 1, &q, 0.05, 0.95, sums, ap);
        void* blk = undersized(&p);
        SUMS(rgb, n, h, w, d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0.05, 0.95, sums, ap);
        SUMS(rgb, n, h, w, 0, 0, 0, 0, 0, 0, (const SlParams*)blk, 0.05, 0.95, sums, 0);
        free(blk);
    }

    /* ---- sl_normalize_hed_view ---- */
#define HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, sg_, bs_, ap_, mode_) \
        EXPECT(sl_normalize_hed_view(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, sg_, bs_, ap_, mode_, 0), SL_ERR_BADARG)
/* a refusal of the geometry or of the HED arguments on every route, with and without a format and an SlParams */
#define GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, sg_, bs_, ap_, mode_) do { \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, d6, d2, ab, 0, 0, 0, sg_, bs_, ap_, mode_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, 0, 0, ab, 1, &p, &f, sg_, bs_, ap_, mode_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, d6, d2, d6, d2, 0, 0, &p, 0, sg_, bs_, ap_, mode_); \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, 0, 0, 0, 0, 0, 0, 0, &f, sg_, bs_, ap_, mode_); } while (0)
/* the same with good HED arguments */
#define GEOMOK(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_) GEOM(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, sg, bs, ap, SL_HED_SKIMAGE_018)
#define HVIEWOK(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_) \
        HVIEW(rgb_, out_, n_, h_, w_, oh_, ow_, win_, dm_, ms_, cs_, mt_, ct_, ab_, bg_, p_, f_, sg, bs, ap, SL_HED_SKIMAGE_018)

    /* required pointers */
    GEOMOK(0, out, n, h, w, oh, ow, win, 7);
    GEOMOK(rgb, 0, n, h, w, oh, ow, win, 7);
    GEOMOK(rgb, out, n, h, w, oh, ow, 0, 7);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, 0, bs, ap, SL_HED_SKIMAGE_018);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, 0, ap, SL_HED_SKIMAGE_018);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, 0, SL_HED_SKIMAGE_018);
    /* the mode: outside the range, and the three the kernel does not instantiate */
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, -1);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, SL_HED_EXPERIMENTAL_LOG10 + 1);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, 2147483647);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, -2147483647 - 1);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, SL_HED_SKIMAGE_019);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, SL_HED_SKIMAGE_017);
    GEOM(rgb, out, n, h, w, oh, ow, win, 7, sg, bs, ap, SL_HED_EXPERIMENTAL_LOG10);
    /* shapes */
    GEOMOK(rgb, out, 0, h, w, oh, ow, win, 7);
    GEOMOK(rgb, out, -1, h, w, oh, ow, win, 7);
    GEOMOK(rgb, out, n, 0, w, oh, ow, win, 7);
    GEOMOK(rgb, out, n, h, -5, oh, ow, win, 7);
    GEOMOK(rgb, out, n, 65536, 65536, oh, ow, win, 7);      /* more than 2^30 pixels */
    GEOMOK(rgb, out, n, 32768, 32769, oh, ow, win, 6);      /* just over */
    /* the output size */
    GEOMOK(rgb, out, n, h, w, 0, ow, win, 7);
    GEOMOK(rgb, out, n, h, w, oh, 0, win, 7);
    GEOMOK(rgb, out, n, h, w, -1, -1, win, 0);
    GEOMOK(rgb, out, n, h, w, h + 1, ow, win, 6);
    GEOMOK(rgb, out, n, h, w, oh, w + 1, win, 6);
    GEOMOK(rgb, out, n, h, w, 2147483647, 2147483647, win, 0);
    /* the mask */
    GEOMOK(rgb, out, n, h, w, oh, ow, win, -1);
    GEOMOK(rgb, out, n, h, w, oh, ow, win, 8);
    GEOMOK(rgb, out, n, h, w, oh, ow, win, -2147483647 - 1);
    /* quarter turns: the transposed window must fit too (64 x 48 does not fit into 64 x 48 turned) */
    GEOMOK(rgb, out, n, h, w, h, w, win, 7);
    GEOMOK(rgb, out, n, h, w, h, w, win, 1);
    GEOMOK(rgb, out, n, h, w, w + 1, w, win, 5);
    GEOMOK(rgb, out, n, w, h, oh, h, win, 3);                /* a 48 x 64 tile, 40 x 64 out: ow > h */
    /* more (tile, patch) pairs than a grid holds */
    GEOMOK(rgb, out, 1 << 22, 32768, 32768, 32768, 32768, win, 7);
    /* the statistics */
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, 0, d6, d2, ab, 0, 0, 0);         /* M_src without maxC_src */
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, d2, ab, 0, 0, 0);         /* a one-sided target */
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, 0, ab, 0, 0, &f);
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, 0, 0, 0, 0);           /* the apply route has no "no target" */
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, d2, 0, 0, 0, 0, 0, 0);            /* the source bytes: nothing else may be given */
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, d6, d2, 0, 0, 0, 0);
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, ab, 1, &p, &f);
    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, d2, d6, d2, ab, 0, 0, 0);
    /* SlParams.struct_size, two_sweep */
    {
        SlParams q = p;
        q.struct_size = 0;                         HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, &q, 0);
        q.struct_size = sizeof(SlParams) - 8;      HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, 0, 0, &q, &f);
        q.struct_size = sizeof(SlParams) + 8;      HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, &q, 0);
        q = p; q.two_sweep = 9;                    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, ab, 1, &q, 0);
        void* blk = undersized(&p);
        HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, (const SlParams*)blk, 0);
        HVIEWOK(rgb, out, n, h, w, oh, ow, win, 6, 0, 0, 0, 0, 0, 0, (const SlParams*)blk, &f);
        free(blk);
    }
    /* SlTensorFormat: struct_size, dtype, layout, std, non-finite values (the checks of sl_to_tensor) */
    {
        SlTensorFormat g = f;
        g.struct_size = 0;                               HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
        g.struct_size = sizeof(SlTensorFormat) - 8;      HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, 0, 0, &p, &g);
        g.struct_size = sizeof(SlTensorFormat) + 8;      HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
        void* blk = undersized(&f);
        HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, (const SlTensorFormat*)blk);
        HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, (const SlTensorFormat*)blk);
        free(blk);
        const int bad[] = {-1, 3, 99, -2147483647 - 1, 2147483647};
        for (unsigned i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
            g = f; g.dtype = bad[i];                     HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.layout = bad[i];                    HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
        }
        for (int c = 0; c < 3; ++c) {
            g = f; g.std[c] = 0.0;                       HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, d6, d2, ab, 0, 0, &g);
            g = f; g.std[c] = NAN;                       HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, 0, 0, 0, 0, 0, 0, 0, &g);
            g = f; g.mean[c] = -INFINITY;                HVIEWOK(rgb, out, n, h, w, oh, ow, win, 7, d6, d2, 0, 0, ab, 1, &p, &g);
        }
    }
    return report();
}
